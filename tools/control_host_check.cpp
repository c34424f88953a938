// Stand-alone check of the host twins of the control pass and the keepalive timer (rsk_control_host,
// rsk_keepalive_flush_host; rsock_amd/csrc/rsk_host.cpp) for a sanitizer build of the host code alone --
// no HIP, no Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/control_host_check.cpp rsock_amd/csrc/rsk_host.cpp -lpthread -o control_host_check
// Generated tables (client and BY_ID, 1 .. 5000 rows) and batches (DATA, control packets of every cmd with
// bodies of 0 .. 12 bytes at every alignment, CLOSE and dropped packets, unknown cmds, a miss column), each
// compared with a per-packet std::map walk; the timer against a std::map walk of OnFlush over several
// ticks.  Every column, the frame arena included, is a heap block of exactly its bytes: the arena holds
// only the bytes a body read may touch (4 or 8 per control packet, the last body on its last byte), so
// an over-read of a 4-byte body is reported; packets whose frame must not be read point far outside it.
// Exit status 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "rsk_codec.h"

static uint64_t rng_state = 0xC0471;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static uint64_t rnd64() { return ((uint64_t)rnd() << 33) ^ ((uint64_t)rnd() << 11) ^ rnd(); }

// A heap block of exactly v's bytes (at least one, so that the pointer is never NULL).
template <typename T>
static T *exact(const std::vector<T> &v) {
    T *p = (T *)malloc(v.empty() ? 1 : v.size() * sizeof(T));
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
template <typename T>
static bool same(const T *got, const std::vector<T> &want, size_t n) {
    return n == 0 || std::memcmp(got, want.data(), n * sizeof(T)) == 0;
}

typedef std::pair<uint64_t, uint64_t> Key;  // (IdBuf as a word, connKey); IdBuf 0 on a client

struct Table {
    uint32_t cap;
    bool by_id;
    std::vector<uint8_t> state, id;
    std::vector<uint64_t> key, idw;
    std::map<Key, uint32_t> map;  // the lowest LIVE row of every key
    rsk_conn_table t;
    uint8_t *e_state, *e_id;
    uint64_t *e_key;
    void *ix;
};

static void make_table(Table &T, uint32_t cap, bool by_id, const std::vector<uint64_t> &idpool) {
    T.cap = cap;
    T.by_id = by_id;
    T.state.resize(cap); T.id.resize(8ull * cap); T.key.resize(cap); T.idw.resize(cap);
    for (uint32_t r = 0; r < cap; ++r) {
        T.state[r] = (uint8_t)((rnd() % 3 ? RSK_CONN_LIVE : 0u) | (rnd() % 4 ? RSK_CONN_ALIVE : 0u) | (rnd() % 5 == 0 ? RSK_CONN_NEW : 0u));
        T.key[r] = rnd() % 8 == 0 && r ? T.key[rnd() % r]
                                       : (rnd() % 2 ? 0x10000000ull | ((uint64_t)(10001 + rnd() % 4) << 16) | (40000 + rnd() % 40) : rnd64());
        T.idw[r] = by_id ? idpool[rnd() % idpool.size()] : 0ull;
        std::memcpy(&T.id[8ull * r], &T.idw[r], 8);
        if (T.state[r] & RSK_CONN_LIVE) T.map.emplace(Key(T.idw[r], T.key[r]), r);
    }
    std::memset(&T.t, 0, sizeof T.t);
    T.t.capacity = cap;
    T.t.flags = by_id ? RSK_CONN_BY_ID : 0u;
    T.e_state = exact(T.state); T.e_id = exact(T.id); T.e_key = exact(T.key);
    T.t.state = T.e_state; T.t.conn_key = T.e_key; T.t.id = by_id ? T.e_id : nullptr;
    const uint64_t ib = rsk_conn_index_bytes(cap, T.t.flags);
    T.ix = nullptr;
    if (posix_memalign(&T.ix, 16, (size_t)ib)) exit(2);
    T.t.index = (uint32_t *)T.ix;
    if (rsk_conn_index_build_host(&T.t, nullptr, 1) != RSK_OK) exit(2);
}
static void free_table(Table &T) { free(T.e_state); free(T.e_id); free(T.e_key); free(T.ix); }

static const uint64_t kWild = 1ull << 45;  // the offset of a frame that must not be read

static int run_control(uint32_t cap, bool by_id, uint32_t n, int nthreads, bool with_tcp, bool with_miss, bool with_id) {
    std::vector<uint64_t> idpool;
    for (int k = 0; k < 4; ++k) idpool.push_back(rnd64());
    Table T;
    make_table(T, cap, by_id, idpool);
    with_id = with_id || by_id;

    std::vector<int8_t> st(n), miss(n);
    std::vector<uint8_t> cmd(n), pid(8ull * n), arena;
    std::vector<uint64_t> pkey(n), base(n), pidw(n);
    std::vector<uint16_t> inner(n), poff(n), plen(n), sp(n), dp(n);
    // the restatement's outputs
    std::vector<uint8_t> w_kind(n), w_tries(cap);
    std::vector<uint64_t> w_arg(n);
    std::vector<uint32_t> w_conn(n), w_rst(cap, 0xFFFFFFFFu);
    std::vector<uint8_t> m_cmd, m_id;
    std::vector<uint64_t> m_body, m_avoid, m_poff;
    std::vector<uint32_t> m_src;
    std::vector<uint16_t> m_plen;
    uint32_t w_nctl = 0;
    for (uint32_t r = 0; r < cap; ++r) w_tries[r] = (uint8_t)(rnd() % 3 ? rnd() % 3 : RSK_KA_NONE);
    std::vector<uint8_t> tries0 = w_tries;
    for (uint32_t k = 0; k < 300; ++k) arena.push_back((uint8_t)rnd());  // room for inner_off + pay_off in front
    uint32_t bodies = 0;
    auto put = [&](uint8_t c, uint64_t body, uint32_t i, uint64_t avoid) {
        m_poff.push_back(8ull * m_cmd.size());
        m_cmd.push_back(c); m_body.push_back(body); m_src.push_back(i); m_avoid.push_back(avoid); m_plen.push_back(8);
        for (int b = 0; b < 8; ++b) m_id.push_back(with_id ? pid[8ull * i + b] : 0);
    };
    for (uint32_t i = 0; i < n; ++i) {
        st[i] = (int8_t)(rnd() % 8 ? RSK_RECV_VALID : (rnd() % 2 ? RSK_RECV_DROP : RSK_RECV_CLOSE));
        cmd[i] = (uint8_t)(rnd() % 3 ? RSK_CMD_DATA : (rnd() % 8 ? 1 + rnd() % 4 : 5 + rnd() % 250));
        pidw[i] = by_id ? idpool[rnd() % idpool.size()] : rnd64();
        std::memcpy(&pid[8ull * i], &pidw[i], 8);
        pkey[i] = rnd64();
        inner[i] = (uint16_t)(rnd() % 80); poff[i] = (uint16_t)(31 + rnd() % 9); plen[i] = (uint16_t)(rnd() % 1400);
        sp[i] = (uint16_t)(40000 + rnd() % 40); dp[i] = (uint16_t)(10001 + rnd() % 4);
        base[i] = kWild;
        miss[i] = (int8_t)(with_miss && st[i] == RSK_RECV_VALID && rnd() % 5 == 0 ? RSK_RECV_VALID : RSK_RECV_DROP);
        uint8_t kind = RSK_CTL_NONE;
        uint64_t arg = 0;
        const bool ctl = st[i] == RSK_RECV_VALID && cmd[i] >= 1 && cmd[i] <= 4;
        if (ctl) {
            static const uint16_t lens[] = {8, 9, 8, 12, 8, 4, 8, 7, 8, 3, 8, 0, 5, 1};
            plen[i] = lens[rnd() % 14];
            const uint32_t need = cmd[i] == RSK_CMD_CONV_RST ? 4u : 8u;
            if (plen[i] < need) {
                kind = RSK_CTL_SHORT;
            } else {
                kind = cmd[i];
                // a key of the table (under this packet's IdBuf or another), or a fresh one
                uint64_t body = rnd64();
                if (rnd() % 4) {
                    const uint32_t r = rnd() % cap;
                    body = T.key[r];
                    if (by_id && rnd() % 4) { pidw[i] = T.idw[r]; std::memcpy(&pid[8ull * i], &pidw[i], 8); }
                }
                while (arena.size() % 16 != bodies % 16) arena.push_back((uint8_t)rnd());
                ++bodies;
                base[i] = arena.size() - inner[i] - poff[i];
                for (uint32_t b = 0; b < need; ++b) arena.push_back((uint8_t)(body >> (8 * b)));  // exactly the bytes read
                arg = need == 4 ? (body & 0xFFFFFFFFull) : body;
            }
        } else if (st[i] == RSK_RECV_VALID && cmd[i] > 4) {
            kind = RSK_CTL_UNKNOWN;
        } else if (st[i] == RSK_RECV_CLOSE && with_tcp && !by_id) {
            kind = RSK_CTL_TCP_CLOSE;
            arg = rsk_key_for_tcp(sp[i], dp[i]);
        }
        uint32_t row = RSK_CONN_NONE;
        if (kind >= RSK_CTL_NETCONN_RST && kind <= RSK_CTL_TCP_CLOSE) {
            const auto it = T.map.find(Key(by_id ? pidw[i] : 0ull, arg));
            if (it != T.map.end()) row = it->second;
        }
        w_kind[i] = kind; w_arg[i] = arg; w_conn[i] = row;
        w_nctl += kind != RSK_CTL_NONE;
        if (row != RSK_CONN_NONE) {
            if ((kind == RSK_CTL_NETCONN_RST || kind == RSK_CTL_TCP_CLOSE) && w_rst[row] == 0xFFFFFFFFu) w_rst[row] = i;
            if (kind == RSK_CTL_KA_RESP) w_tries[row] = RSK_KA_NONE;
        }
        if (kind == RSK_CTL_KA_REQ) put(row != RSK_CONN_NONE ? RSK_CMD_KEEP_ALIVE_RESP : RSK_CMD_NETCONN_RST, arg, i, row != RSK_CONN_NONE ? 0 : arg);
        else if (with_miss && miss[i] == RSK_RECV_VALID) put(RSK_CMD_NETCONN_RST, pkey[i], i, pkey[i]);
    }
    const uint32_t w_nmsg = (uint32_t)m_cmd.size();

    int8_t *e_st = exact(st), *e_miss = exact(miss);
    uint8_t *e_cmd = exact(cmd), *e_pid = exact(pid), *e_arena = exact(arena);
    uint64_t *e_pkey = exact(pkey), *e_base = exact(base);
    uint16_t *e_inner = exact(inner), *e_poff = exact(poff), *e_plen = exact(plen), *e_sp = exact(sp), *e_dp = exact(dp);
    rsk_control_in in = {e_st, e_cmd, with_id ? e_pid : nullptr, with_miss ? e_pkey : nullptr, e_poff, e_plen, e_arena, e_base,
                         e_inner, with_tcp ? e_sp : nullptr, with_tcp ? e_dp : nullptr, with_miss ? e_miss : nullptr};
    int bad = 0;
    for (int variant = 0; variant < 3; ++variant) {  // every output; the counts alone; nothing at all
        std::vector<uint8_t> fk(n, 0xEE), fid(8ull * n, 0xEE), fc(n, 0xEE);
        std::vector<uint64_t> fa(n, 0xEE), fb(n, 0xEE), fav(n, 0xEE), fpo(n, 0xEE);
        std::vector<uint32_t> fco(n, 0xEE), fs(n, 0xEE), frst(cap, 0xEE);
        std::vector<uint16_t> fpl(n, 0xEE);
        uint8_t *o_kind = exact(fk), *o_id = exact(fid), *o_cmd = exact(fc), *o_tries = exact(tries0);
        uint64_t *o_arg = exact(fa), *o_body = exact(fb), *o_avoid = exact(fav), *o_poff = exact(fpo);
        uint32_t *o_conn = exact(fco), *o_src = exact(fs), *o_rst = exact(frst);
        uint16_t *o_plen = exact(fpl);
        uint32_t nmsg = 0xFFFFFFFFu, nctl = 0xFFFFFFFFu;
        rsk_control_out out;
        std::memset(&out, 0, sizeof out);
        if (variant == 0) {
            out.kind = o_kind; out.arg = o_arg; out.conn = o_conn; out.rst_first = o_rst; out.ka_tries = o_tries;
            out.msgs.cmd = o_cmd; out.msgs.body = o_body; out.msgs.id = o_id; out.msgs.src = o_src;
            out.msgs.avoid_key = o_avoid; out.msgs.pay_off = o_poff; out.msgs.pay_len = o_plen;
        }
        if (variant <= 1) { out.msgs.n_msg = &nmsg; out.n_ctl = &nctl; }
        bad |= rsk_control_host(&T.t, n, &in, &out, nthreads) != RSK_OK;
        if (variant <= 1) bad |= nmsg != w_nmsg || nctl != w_nctl;
        if (variant == 0) {
            bad |= !same(o_kind, w_kind, n) || !same(o_arg, w_arg, n) || !same(o_conn, w_conn, n);
            bad |= !same(o_rst, w_rst, cap) || !same(o_tries, w_tries, cap);
            bad |= !same(o_cmd, m_cmd, w_nmsg) || !same(o_body, m_body, w_nmsg) || !same(o_id, m_id, 8ull * w_nmsg) ||
                   !same(o_src, m_src, w_nmsg) || !same(o_avoid, m_avoid, w_nmsg) || !same(o_poff, m_poff, w_nmsg) ||
                   !same(o_plen, m_plen, w_nmsg);
            for (uint32_t k = w_nmsg; k < n; ++k) bad |= o_cmd[k] != 0xEE || o_src[k] != 0xEE;  // nothing past n_msg
        }
        free(o_kind); free(o_id); free(o_cmd); free(o_tries); free(o_arg); free(o_body); free(o_avoid); free(o_poff);
        free(o_conn); free(o_src); free(o_rst); free(o_plen);
    }
    free(e_st); free(e_miss); free(e_cmd); free(e_pid); free(e_arena); free(e_pkey); free(e_base); free(e_inner);
    free(e_poff); free(e_plen); free(e_sp); free(e_dp);
    free_table(T);
    if (bad) printf("MISMATCH control cap=%u by_id=%d n=%u threads=%d tcp=%d miss=%d id=%d\n", cap, (int)by_id, n, nthreads,
                    (int)with_tcp, (int)with_miss, (int)with_id);
    return bad;
}

static int run_flush(uint32_t cap, bool by_id, uint32_t max_retry, bool online) {
    std::vector<uint64_t> idpool = {rnd64(), rnd64()};
    Table T;
    make_table(T, cap, by_id, idpool);
    const uint64_t t0 = 1ull << 40;
    const uint32_t delay = RSK_KA_REQUEST_DELAY_MS;
    std::vector<uint64_t> est(cap);
    static const int64_t edge[] = {0, -1, -1000000, 15000, 14999, 2147483647ll, 2147483648ll, 4294967296ll + 15000, 4294967296ll + 14999};
    for (uint32_t r = 0; r < cap; ++r) est[r] = rnd() % 4 ? t0 - rnd() % (2 * delay) : t0 - (uint64_t)edge[rnd() % 9];
    std::map<uint32_t, int> req;  // mReqMap, by row
    std::vector<uint8_t> tries(cap, RSK_KA_NONE);
    for (uint32_t r = 0; r < cap; ++r)
        if (rnd() % 3 == 0) { req[r] = (int)(rnd() % 3); tries[r] = (uint8_t)req[r]; }
    uint64_t *e_est = exact(est);
    uint8_t *e_tries = exact(tries);
    int bad = 0;
    for (uint32_t step = 0; step < max_retry + 2; ++step) {
        const uint64_t now = t0 + 1000ull * step;
        // OnFlush, callbacks/NetConnKeepAlive.cpp:110-145
        for (auto it = req.begin(); it != req.end();)
            it = (T.state[it->first] & RSK_CONN_LIVE) ? std::next(it) : req.erase(it);
        std::vector<uint32_t> w_sent, w_dead;
        if (online) {
            for (uint32_t r = 0; r < cap; ++r) {
                if (!(T.state[r] & RSK_CONN_LIVE) || (T.state[r] & RSK_CONN_NEW)) continue;
                if (!(now > est[r])) continue;
                // `int df = timestampMs - est`: the conversion keeps the low 32 bits
                const uint32_t low = (uint32_t)(now - est[r]);
                const int64_t df = low < 0x80000000u ? (int64_t)low : (int64_t)low - 4294967296ll;
                if (df < (int64_t)delay) continue;
                auto it = req.find(r);
                if (it != req.end()) it->second++;
                else req.emplace(r, 0);
                if (it == req.end() || it->second < (int)max_retry) w_sent.push_back(r);
            }
            for (auto it = req.begin(); it != req.end();) {
                if (it->second >= (int)max_retry) { w_dead.push_back(it->first); it = req.erase(it); }
                else ++it;
            }
        }
        std::vector<uint8_t> fc(cap, 0xEE), fid(8ull * cap, 0xEE);
        std::vector<uint64_t> f64(cap, 0xEE);
        std::vector<uint32_t> f32(cap, 0xEE);
        std::vector<uint16_t> f16(cap, 0xEE);
        uint8_t *o_cmd = exact(fc), *o_id = exact(fid);
        uint64_t *o_body = exact(f64), *o_avoid = exact(f64), *o_poff = exact(f64);
        uint32_t *o_src = exact(f32), *o_dead = exact(f32);
        uint16_t *o_plen = exact(f16);
        uint32_t nmsg = 0xFFFFFFFFu, ndead = 0xFFFFFFFFu;
        rsk_keepalive ka = {e_tries, e_est, now, delay, max_retry, online ? 1u : 0u};
        rsk_keepalive_out out = {{o_cmd, o_body, o_id, o_src, o_avoid, o_poff, o_plen, &nmsg}, o_dead, &ndead};
        bad |= rsk_keepalive_flush_host(&T.t, &ka, &out, 1) != RSK_OK;
        bad |= nmsg != w_sent.size() || ndead != w_dead.size();
        for (uint32_t k = 0; k < w_sent.size() && !bad; ++k) {
            const uint32_t r = w_sent[k];
            uint64_t w = 0;
            std::memcpy(&w, o_id + 8ull * k, 8);
            bad |= o_cmd[k] != RSK_CMD_KEEP_ALIVE_REQ || o_body[k] != T.key[r] || o_src[k] != r || o_avoid[k] != 0 ||
                   o_poff[k] != 8ull * k || o_plen[k] != 8 || w != (by_id ? T.idw[r] : 0ull);
        }
        for (uint32_t k = 0; k < w_dead.size() && !bad; ++k) bad |= o_dead[k] != w_dead[k];
        for (uint32_t r = 0; r < cap; ++r) {
            const auto it = req.find(r);
            bad |= e_tries[r] != (it == req.end() ? RSK_KA_NONE : (uint8_t)it->second);
        }
        free(o_cmd); free(o_id); free(o_body); free(o_avoid); free(o_poff); free(o_src); free(o_dead); free(o_plen);
        if (step == 1)  // a response for every second pending row
            for (auto it = req.begin(); it != req.end();) {
                e_tries[it->first] = RSK_KA_NONE;
                it = req.erase(it);
                if (it != req.end()) ++it;
            }
    }
    free(e_est); free(e_tries);
    free_table(T);
    if (bad) printf("MISMATCH flush cap=%u by_id=%d max_retry=%u online=%d\n", cap, (int)by_id, max_retry, (int)online);
    return bad;
}

int main() {
    int bad = 0, runs = 0;
    for (uint32_t cap : {1u, 2u, 65u, 1000u, 5000u})
        for (int by_id = 0; by_id < 2; ++by_id)
            for (uint32_t n : {1u, 300u, 9000u})
                for (int opt = 0; opt < 8; ++opt) {
                    if (n == 9000u && cap != 65u && cap != 5000u) continue;
                    bad |= run_control(cap, by_id != 0, n, n == 9000u ? 4 : 1, (opt & 1) != 0, (opt & 2) != 0, (opt & 4) != 0);
                    ++runs;
                }
    for (uint32_t cap : {1u, 2u, 257u, 5000u})
        for (int by_id = 0; by_id < 2; ++by_id)
            for (uint32_t mr : {1u, 3u})
                for (int online = 0; online < 2; ++online) {
                    bad |= run_flush(cap, by_id != 0, mr, online != 0);
                    ++runs;
                }
    // argument errors and the empty batch
    uint8_t st8 = RSK_CONN_LIVE, kind = 9, tries = 0;
    uint64_t k = 1, est = 0;
    alignas(16) uint32_t ix[4];
    uint32_t word = 7, rst = 7;
    int8_t s = 1;
    uint8_t c = 0, ar[8] = {0};
    uint16_t z16 = 0;
    uint64_t z64 = 0;
    rsk_conn_table t;
    std::memset(&t, 0, sizeof t);
    t.capacity = 1; t.state = &st8; t.conn_key = &k; t.index = ix;
    bad |= rsk_conn_index_build_host(&t, nullptr, 1) != RSK_OK;
    rsk_control_in in;
    std::memset(&in, 0, sizeof in);
    in.status = &s; in.cmd = &c; in.pay_off = &z16; in.pay_len = &z16; in.arena = ar; in.base_off = &z64;
    rsk_control_out out;
    std::memset(&out, 0, sizeof out);
    out.kind = &kind; out.n_ctl = &word; out.rst_first = &rst;
    bad |= rsk_control_host(&t, 1, &in, &out, 1) != RSK_OK || kind != 0 || word != 0 || rst != 0xFFFFFFFFu;
    word = rst = 7;
    rsk_control_in none;
    std::memset(&none, 0, sizeof none);
    bad |= rsk_control_host(&t, 0, &none, &out, 1) != RSK_OK || word != 0 || rst != 0xFFFFFFFFu;  // n == 0
    bad |= rsk_control_host(nullptr, 1, &in, &out, 1) != RSK_EINVAL || rsk_control_host(&t, 1, nullptr, &out, 1) != RSK_EINVAL ||
           rsk_control_host(&t, 1, &in, nullptr, 1) != RSK_EINVAL || rsk_control_host(&t, 1, &none, &out, 1) != RSK_EINVAL;
    rsk_control_in in2 = in;
    in2.tcp_sp = &z16;  // one port column alone
    bad |= rsk_control_host(&t, 1, &in2, &out, 1) != RSK_EINVAL;
    in2 = in; in2.miss = &s;  // miss without conn_key
    bad |= rsk_control_host(&t, 1, &in2, &out, 1) != RSK_EINVAL;
    rsk_control_out out2 = out;
    out2.msgs.body = &z64;  // a message array without n_msg
    bad |= rsk_control_host(&t, 1, &in, &out2, 1) != RSK_EINVAL;
    rsk_conn_table u = t;
    u.flags = RSK_CONN_BY_ID; u.id = ar;  // in->id missing with BY_ID
    bad |= rsk_control_host(&u, 1, &in, &out, 1) != RSK_EINVAL;
    rsk_keepalive ka = {&tries, &est, 1ull << 20, RSK_KA_REQUEST_DELAY_MS, RSK_KA_MAX_RETRY, 1};
    rsk_keepalive_out ko;
    std::memset(&ko, 0, sizeof ko);
    ko.msgs.n_msg = &word; ko.n_dead = &rst;
    bad |= rsk_keepalive_flush_host(&t, &ka, &ko, 1) != RSK_OK || word != 1 || rst != 0 || tries != 1;
    rsk_keepalive kb = ka;
    kb.max_retry = 0;
    bad |= rsk_keepalive_flush_host(&t, &kb, &ko, 1) != RSK_EINVAL;
    kb = ka; kb.ka_tries = nullptr;
    bad |= rsk_keepalive_flush_host(&t, &kb, &ko, 1) != RSK_EINVAL;
    rsk_keepalive_out k2 = ko;
    k2.n_dead = nullptr; k2.dead_rows = &rst;
    bad |= rsk_keepalive_flush_host(&t, &ka, &k2, 1) != RSK_EINVAL || rsk_keepalive_flush_host(nullptr, &ka, &ko, 1) != RSK_EINVAL;
    printf("%s: %d runs\n", bad ? "FAILED" : "ok", runs);
    return bad;
}
