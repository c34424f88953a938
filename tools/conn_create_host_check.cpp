// Stand-alone check of rsk_conn_create_host (rsock_amd/csrc/rsk_host.cpp), the host twin of
// rsk_conn_create_batch, for a sanitizer build of the host code alone -- no HIP, no Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/conn_create_host_check.cpp rsock_amd/csrc/rsk_host.cpp -lpthread -o conn_create_host_check
// A few hundred generated tables, each taking several calls in a row on one conn index and one pick index: client
// and BY_ID tables of 1 .. 3000 rows that are empty, sparse or full, few or many groups, the IdBuf columns at odd
// addresses; the column form (known and unknown keys, keys that share a tuple, keys without an offer, u_max below
// the missing packets) and the list form (LIVE keys, repeated keys); offers that repeat a tuple, *n_offer above and
// below m_max and 0; with and without a pick index and the lists.  Every column, the work buffer and both indexes
// are heap blocks of exactly their bytes, so an access one element outside is reported.  Each call is compared
// with a std::map walk written from INetGroup::Input / SNetGroup::CreateNetConn (conn/INetGroup.cpp:57-83,
// server/SNetGroup.cpp:20-46): the rows, the lists, conn / hit / miss, the lookup of every row's key on the conn
// index as the call left it and the pick of every group at every candidate number on the pick index as the call
// left it.  A last pass runs calls on conn and pick indexes filled with garbage: whatever rows come out, nothing
// outside the buffers may be touched.  Exit status 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <tuple>
#include <utility>
#include <vector>

#include "rsk_codec.h"

static uint64_t rng_state = 0xC0221C2EA7Eull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static uint64_t rnd64() { return ((uint64_t)rnd() << 33) ^ ((uint64_t)rnd() << 11) ^ rnd(); }

template <typename T>
static T *exact(const std::vector<T> &v, size_t shift = 0) {
    uint8_t *p = (uint8_t *)malloc(shift + (v.empty() ? 1 : v.size() * sizeof(T)));
    if (!v.empty()) std::memcpy(p + shift, v.data(), v.size() * sizeof(T));
    return (T *)(p + shift);
}
static void *aligned(size_t bytes, int fill) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, bytes)) abort();
    std::memset(p, fill, bytes);
    return p;
}

typedef std::pair<uint64_t, uint64_t> Key;                    // (IdBuf word, connKey); the word 0 without BY_ID
typedef std::tuple<uint32_t, uint16_t, uint32_t, uint16_t> Tup;  // src, sp, dst, dp: TcpCmpFn's order
static const uint32_t kSent = 0x6E6E6E6Eu;
static const uint8_t kUp = RSK_CONN_LIVE | RSK_CONN_ALIVE, kBorn = RSK_CONN_LIVE | RSK_CONN_ALIVE | RSK_CONN_NEW;

struct Conn {  // a conn the table does not know
    Key k;
    uint32_t src, dst, ack;
    uint16_t sp, dp;
    uint8_t flag;
};

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf(" (cap %u by_id %d call %d)\n", cap, (int)by_id, call); return 1; } while (0)

static int run(uint32_t cap, bool by_id, int fill, uint32_t groups, bool with_pick, bool garbage) {
    int call = -1;
    std::vector<uint8_t> state(cap), id(8ull * cap), flag(cap), ka(cap);
    std::vector<uint64_t> key(cap), idw(cap), est(cap);
    std::vector<uint32_t> src(cap), dst(cap), seq(cap), ack(cap);
    std::vector<uint16_t> sp(cap), dp(cap);
    const uint64_t i0 = rnd64();
    for (uint32_t r = 0; r < cap; ++r) {
        const uint32_t v = rnd() % 8;
        state[r] = fill == 0 ? (uint8_t)(rnd() % 2 ? RSK_CONN_ALIVE : 0x80u)
                 : fill == 2 ? kUp : (uint8_t)(v < 4 ? kUp : v == 4 ? RSK_CONN_LIVE : v == 5 ? RSK_CONN_ALIVE : 0u);
        key[r] = rnd64() | 1u;
        idw[r] = i0 + 0x9E3779B97F4A7C15ull * (rnd() % groups);
        std::memcpy(&id[8ull * r], &idw[r], 8);
        src[r] = rnd(); dst[r] = rnd(); seq[r] = rnd(); ack[r] = rnd(); sp[r] = (uint16_t)rnd(); dp[r] = (uint16_t)rnd();
        flag[r] = (uint8_t)rnd(); ka[r] = (uint8_t)(rnd() % 4); est[r] = rnd64();
    }
    rsk_conn_table t;
    std::memset(&t, 0, sizeof t);
    t.capacity = cap;
    t.flags = by_id ? RSK_CONN_BY_ID : 0u;
    const size_t shift = rnd() % 2 ? 3 : 0;  // the IdBuf columns at an odd address
    uint8_t *e_state = exact(state), *e_id = exact(id, shift), *e_flag = exact(flag), *e_ka = exact(ka);
    uint64_t *e_key = exact(key), *e_est = exact(est);
    uint32_t *e_src = exact(src), *e_dst = exact(dst), *e_seq = exact(seq), *e_ack = exact(ack);
    uint16_t *e_sp = exact(sp), *e_dp = exact(dp);
    t.state = e_state; t.conn_key = e_key; t.id = by_id ? e_id : nullptr; t.src = e_src; t.dst = e_dst; t.sp = e_sp;
    t.dp = e_dp; t.seq = e_seq; t.ack = e_ack; t.flag = e_flag;
    const uint64_t ibytes = rsk_conn_index_bytes(cap, t.flags), pbytes = rsk_conn_pick_bytes(cap, t.flags);
    t.index = (uint32_t *)aligned((size_t)ibytes, 0x5A);
    uint32_t *pick = (uint32_t *)aligned((size_t)pbytes, 0x5A);
    uint32_t counts[2];
    if (!garbage) {
        if (rsk_conn_index_build_host(&t, nullptr, 1) != RSK_OK || rsk_conn_pick_build_host(&t, pick, counts, 1) != RSK_OK)
            FAIL("build failed");
    } else {
        for (uint64_t q = 0; q < ibytes / 4; ++q) t.index[q] = rnd() % 3 ? rnd() % (2 * cap + 2) : rnd();
        for (uint64_t q = 0; q < pbytes / 4; ++q) pick[q] = rnd() % 3 ? rnd() % (2 * cap + 2) : rnd();
    }
    rsk_conn_create_rows rows = {e_state, e_key, by_id ? e_id : nullptr, e_src, e_dst, e_sp, e_dp, e_seq, e_ack, e_flag};

    for (call = 0; call < 4; ++call) {
        const bool list = rnd() % 3 == 0;
        // the new conns of the call; some share a tuple with the one before (a forged packet / a repeated offer)
        const uint32_t nconn = rnd() % (cap / 2 + 4);
        std::vector<Conn> nc(nconn);
        for (uint32_t c = 0; c < nconn; ++c) {
            nc[c].k = Key(by_id ? (rnd() % 4 ? idw[rnd() % cap] : rnd64()) : 0ull, (rnd64() & ~1ull) + 2 * (uint64_t)call);
            nc[c].src = 0x0A000000u + c; nc[c].dst = 0xC0A80001u; nc[c].sp = (uint16_t)(1024 + c % 60000); nc[c].dp = (uint16_t)(443 + call);
            nc[c].ack = rnd() % 8 ? rnd() : 0xFFFFFFFFu - rnd() % 2;
            nc[c].flag = (uint8_t)rnd();
            if (c && rnd() % 16 == 0) { nc[c].src = nc[c - 1].src; nc[c].sp = nc[c - 1].sp; }
            if (list && c && rnd() % 16 == 0) nc[c].k = nc[c - 1].k;
        }
        // the offers: a random subset in random order (list form: all, some naming LIVE keys)
        std::vector<uint32_t> o_src, o_dst, o_ack;
        std::vector<uint16_t> o_sp, o_dp;
        std::vector<uint8_t> o_flag, o_id;
        std::vector<uint64_t> o_key;
        for (uint32_t c = 0; c < nconn; ++c) {
            if (!list && rnd() % 4 == 0) continue;
            Conn x = nc[c];
            if (list && rnd() % 8 == 0) { const uint32_t r = rnd() % cap; x.k = Key(by_id ? idw[r] : 0ull, key[r]); }
            o_src.push_back(x.src); o_dst.push_back(x.dst); o_sp.push_back(x.sp); o_dp.push_back(x.dp);
            o_ack.push_back(x.ack); o_flag.push_back(x.flag); o_key.push_back(x.k.second);
            uint8_t b[8];
            std::memcpy(b, &x.k.first, 8);
            o_id.insert(o_id.end(), b, b + 8);
        }
        const uint32_t have = (uint32_t)o_src.size();
        const uint32_t m_max = rnd() % 4 ? have + 1 : 1 + rnd() % (have + 1);
        const uint32_t n_offer = rnd() % 6 == 0 ? 0u : rnd() % 2 ? have : rnd() % 2 ? have + 7 : rnd() % (have + 1);
        while (o_src.size() < m_max) {  // the columns hold m_max entries
            o_src.push_back(rnd()); o_dst.push_back(1); o_sp.push_back(1); o_dp.push_back(1); o_ack.push_back(0);
            o_flag.push_back(0); o_key.push_back(rnd64() | 1u);
            o_id.insert(o_id.end(), 8, (uint8_t)0xEE);
        }
        const uint32_t no = n_offer < m_max ? n_offer : m_max;
        // the batch
        const uint32_t n = list ? 0u : rnd() % 3 ? rnd() % 3000 : rnd() % 40;
        std::vector<uint64_t> b_key(n);
        std::vector<uint8_t> b_id(8ull * n), hit(n);
        std::vector<uint32_t> b_src(n), b_dst(n), conn(n);
        std::vector<uint16_t> b_sp(n), b_dp(n);
        std::vector<int8_t> miss(n);
        std::map<Key, uint32_t> lowest;
        for (uint32_t r = 0; r < cap; ++r)
            if (e_state[r] & RSK_CONN_LIVE) lowest.insert({Key(by_id ? idw[r] : 0ull, key[r]), r});
        for (uint32_t i = 0; i < n; ++i) {
            Key k;
            if (nconn && rnd() % 2) {
                const Conn &x = nc[rnd() % nconn];
                k = x.k; b_src[i] = x.src; b_dst[i] = x.dst; b_sp[i] = x.sp; b_dp[i] = x.dp;
            } else {
                const uint32_t r = rnd() % cap;
                k = Key(by_id ? idw[r] : 0ull, key[r]);
                b_src[i] = src[r]; b_dst[i] = dst[r]; b_sp[i] = sp[r]; b_dp[i] = dp[r];
            }
            b_key[i] = k.second;
            std::memcpy(&b_id[8ull * i], &k.first, 8);
            auto it = lowest.find(k);
            const bool dropped = rnd() % 16 == 0;  // a packet the resolve did not look up
            conn[i] = it == lowest.end() || dropped ? RSK_CONN_NONE : it->second;
            hit[i] = conn[i] != RSK_CONN_NONE;
            miss[i] = it == lowest.end() && !dropped ? RSK_RECV_VALID : RSK_RECV_DROP;
        }
        const uint32_t u_max = list ? 0u : rnd() % 3 ? n + 1 : 1 + rnd() % (n + 1);
        // the walk
        std::vector<uint8_t> w_state(e_state, e_state + cap), w_flag(e_flag, e_flag + cap), w_ka(e_ka, e_ka + cap), w_id(e_id, e_id + 8ull * cap);
        std::vector<uint64_t> w_key(e_key, e_key + cap), w_est(e_est, e_est + cap);
        std::vector<uint32_t> w_src(e_src, e_src + cap), w_dst(e_dst, e_dst + cap), w_seq(e_seq, e_seq + cap), w_ack(e_ack, e_ack + cap);
        std::vector<uint16_t> w_sp(e_sp, e_sp + cap), w_dp(e_dp, e_dp + cap);
        std::vector<uint32_t> w_conn(conn), w_rows, w_first, w_offer, w_offer_row(no, RSK_CONN_NONE);
        std::vector<uint8_t> w_hit(hit);
        std::vector<int8_t> w_miss(miss);
        uint32_t w_full = 0, w_refused = 0, vac = 0;
        const uint64_t now = rnd64();
        auto make = [&](const Key &k, uint32_t o, uint32_t first) {
            while (vac < cap && (w_state[vac] & RSK_CONN_LIVE)) ++vac;
            if (vac == cap) { ++w_full; return; }
            w_key[vac] = k.second; std::memcpy(&w_id[8ull * vac], &k.first, 8);
            w_src[vac] = o_src[o]; w_dst[vac] = o_dst[o]; w_sp[vac] = o_sp[o]; w_dp[vac] = o_dp[o]; w_flag[vac] = o_flag[o];
            w_seq[vac] = o_ack[o] + 1u; w_ack[vac] = o_ack[o] + 2u; w_est[vac] = now; w_ka[vac] = RSK_KA_NONE;
            w_state[vac] = kBorn;
            lowest.insert({k, vac});
            w_rows.push_back(vac); w_first.push_back(first); w_offer.push_back(o); w_offer_row[o] = vac;
            ++vac;
        };
        if (list) {
            std::set<Key> seen;
            for (uint32_t o = 0; o < no; ++o) {
                Key k(0, o_key[o]);
                if (by_id) std::memcpy(&k.first, &o_id[8ull * o], 8);
                if (lowest.count(k) || !seen.insert(k).second) { ++w_refused; continue; }
                make(k, o, 0);
            }
        } else {
            std::map<Tup, uint32_t> pool;  // mPool / mInfoPool: one entry per tuple, the first
            for (uint32_t o = 0; o < no; ++o) pool.insert({Tup(o_src[o], o_sp[o], o_dst[o], o_dp[o]), o});
            std::set<Key> decided;
            std::set<uint32_t> taken;
            uint32_t seen = 0;
            for (uint32_t i = 0; i < n && seen < u_max; ++i) {
                if (miss[i] != RSK_RECV_VALID) continue;
                ++seen;
                Key k(0, b_key[i]);
                if (by_id) std::memcpy(&k.first, &b_id[8ull * i], 8);
                if (!decided.insert(k).second) continue;
                auto it = pool.find(Tup(b_src[i], b_sp[i], b_dst[i], b_dp[i]));
                if (it == pool.end() || !taken.insert(it->second).second) { ++w_refused; continue; }
                make(k, it->second, i);
            }
            for (uint32_t i = 0; i < n; ++i) {
                if (miss[i] != RSK_RECV_VALID) continue;
                Key k(0, b_key[i]);
                if (by_id) std::memcpy(&k.first, &b_id[8ull * i], 8);
                auto it = lowest.find(k);
                if (it == lowest.end()) continue;
                w_conn[i] = it->second; w_hit[i] = 1; w_miss[i] = RSK_RECV_DROP;
            }
        }
        // the call
        const size_t bshift = rnd() % 2 ? 5 : 0;
        uint32_t *x_src = exact(o_src), *x_dst = exact(o_dst), *x_ack = exact(o_ack), *x_no = exact(std::vector<uint32_t>{n_offer});
        uint16_t *x_sp = exact(o_sp), *x_dp = exact(o_dp);
        uint8_t *x_flag = exact(o_flag), *x_id = exact(o_id, bshift), *p_id = exact(b_id, bshift), *p_hit = exact(hit);
        uint64_t *x_key = exact(o_key), *p_key = exact(b_key);
        uint32_t *p_src = exact(b_src), *p_dst = exact(b_dst), *p_conn = exact(conn);
        uint16_t *p_sp = exact(b_sp), *p_dp = exact(b_dp);
        int8_t *p_miss = exact(miss);
        const uint32_t m = m_max < cap ? m_max : cap;
        const bool lists = rnd() % 4 != 0, with_hit = rnd() % 4 != 0;
        uint32_t *o_rows = exact(std::vector<uint32_t>(m, kSent)), *o_first = exact(std::vector<uint32_t>(m, kSent));
        uint32_t *o_offer = exact(std::vector<uint32_t>(m, kSent)), *o_orow = exact(std::vector<uint32_t>(m_max, kSent));
        uint32_t n_new = kSent, n_full = kSent, n_refused = kSent, n_miss = kSent, pc[2] = {kSent, kSent};
        const uint64_t wbytes = rsk_conn_create_bytes(u_max, m_max, cap, t.flags);
        if (!wbytes) FAIL("rsk_conn_create_bytes");
        void *work = aligned((size_t)wbytes, 0xA5);
        uint32_t *index0 = (uint32_t *)aligned((size_t)ibytes, 0), *pick0 = (uint32_t *)aligned((size_t)pbytes, 0);
        std::memcpy(index0, t.index, (size_t)ibytes);
        std::memcpy(pick0, pick, (size_t)pbytes);
        rsk_conn_create_in in;
        std::memset(&in, 0, sizeof in);
        in.id = by_id ? p_id : nullptr; in.conn_key = p_key; in.src = p_src; in.dst = p_dst; in.sp = p_sp; in.dp = p_dp;
        in.offers = rsk_conn_offers{x_src, x_dst, x_sp, x_dp, x_ack, x_flag, list ? x_key : nullptr, list && by_id ? x_id : nullptr, x_no, m_max};
        in.u_max = u_max; in.flags = list ? RSK_CONN_CREATE_LIST : 0u; in.now_ms = now; in.established_ms = e_est; in.ka_tries = e_ka;
        in.work = work;
        rsk_conn_create_out out = {p_conn, with_hit ? p_hit : nullptr, p_miss, &n_miss, lists ? o_rows : nullptr,
                                   lists && !list ? o_first : nullptr, lists ? o_offer : nullptr, o_orow, &n_new, &n_full,
                                   &n_refused, with_pick ? pick : nullptr, with_pick ? pc : nullptr};
        if (rsk_conn_create_host(&t, &rows, n, &in, &out, 1) != RSK_OK) FAIL("create failed");
        if (!garbage) {
            if (n_new != w_rows.size() || n_full != w_full || n_refused != w_refused)
                FAIL("counts %u %u %u, want %zu %u %u", n_new, n_full, n_refused, w_rows.size(), w_full, w_refused);
            for (uint32_t j = 0; lists && j < m; ++j) {
                if (o_rows[j] != (j < n_new ? w_rows[j] : kSent)) FAIL("new_rows[%u]", j);
                if (o_offer[j] != (j < n_new ? w_offer[j] : kSent)) FAIL("new_offer[%u]", j);
                if (o_first[j] != (j < n_new && !list ? w_first[j] : kSent)) FAIL("new_first[%u]", j);
            }
            for (uint32_t o = 0; o < m_max; ++o)
                if (o_orow[o] != (o < no ? w_offer_row[o] : kSent)) FAIL("offer_row[%u]", o);
            if (std::memcmp(e_state, w_state.data(), cap) || std::memcmp(e_key, w_key.data(), 8ull * cap) ||
                (by_id && std::memcmp(e_id, w_id.data(), 8ull * cap)) || std::memcmp(e_src, w_src.data(), 4ull * cap) ||
                std::memcmp(e_dst, w_dst.data(), 4ull * cap) || std::memcmp(e_sp, w_sp.data(), 2ull * cap) ||
                std::memcmp(e_dp, w_dp.data(), 2ull * cap) || std::memcmp(e_seq, w_seq.data(), 4ull * cap) ||
                std::memcmp(e_ack, w_ack.data(), 4ull * cap) || std::memcmp(e_flag, w_flag.data(), cap) ||
                std::memcmp(e_est, w_est.data(), 8ull * cap) || std::memcmp(e_ka, w_ka.data(), cap))
                FAIL("a table column");
            if (!list) {
                uint32_t left = 0;
                for (uint32_t i = 0; i < n; ++i) {
                    left += w_miss[i] == RSK_RECV_VALID;
                    if (p_conn[i] != w_conn[i] || p_miss[i] != w_miss[i] || (with_hit && p_hit[i] != w_hit[i])) FAIL("packet %u", i);
                }
                if (n_miss != left) FAIL("n_miss %u, want %u", n_miss, left);
            } else if (n_miss != kSent) FAIL("n_miss written in list form");
            if (!n_new && std::memcmp(index0, t.index, (size_t)ibytes)) FAIL("index written though nothing was created");
            if ((!n_new || !with_pick) && std::memcmp(pick0, pick, (size_t)pbytes)) FAIL("pick written though nothing changed");
            // keep the image
            key = w_key; id = w_id; src = w_src; dst = w_dst; sp = w_sp; dp = w_dp;
            for (uint32_t r = 0; r < cap; ++r) std::memcpy(&idw[r], &id[8ull * r], 8);
            // lookups on the index as the call left it
            std::vector<int8_t> st(cap, (int8_t)RSK_RECV_VALID);
            std::vector<uint32_t> got(cap, kSent);
            int8_t *e_st = exact(st);
            uint32_t *e_got = exact(got);
            rsk_conn_resolve_in rin = {e_st, nullptr, by_id ? e_id : nullptr, e_key};
            rsk_conn_resolve_out rout = {e_got, nullptr, nullptr, nullptr};
            if (rsk_conn_resolve_host(&t, cap, &rin, &rout, 1) != RSK_OK) FAIL("resolve failed");
            for (uint32_t r = 0; r < cap; ++r) {
                auto it = lowest.find(Key(by_id ? idw[r] : 0ull, key[r]));
                if (e_got[r] != (it == lowest.end() ? RSK_CONN_NONE : it->second)) FAIL("lookup %u", r);
            }
            free(e_st); free(e_got);
            if (!with_pick && n_new && rsk_conn_pick_build_host(&t, pick, counts, 1) != RSK_OK) FAIL("pick rebuild");
            // picks: every group at every candidate number on the pick index as the call left it
            std::map<uint64_t, std::vector<uint32_t>> cand;
            for (uint32_t r = 0; r < cap; ++r)
                if ((e_state[r] & kUp) == kUp) cand[by_id ? idw[r] : 0ull].push_back(r);
            uint32_t total = 0;
            for (auto &g : cand) total += (uint32_t)g.second.size();
            if (pick[0] != total || pick[1] != cand.size()) FAIL("pick header %u %u", pick[0], pick[1]);
            if (with_pick && (pc[0] != cand.size() || pc[1] != total)) FAIL("pick counts");
            std::vector<uint8_t> qi;
            std::vector<uint32_t> dr, wantc;
            for (auto &g : cand) {
                const uint32_t gm = (uint32_t)g.second.size();
                for (uint32_t d = 0; d < (gm < 70 ? gm + 1 : 71); ++d) {
                    uint8_t b[8];
                    std::memcpy(b, &g.first, 8);
                    qi.insert(qi.end(), b, b + 8);
                    const uint32_t dd = d < 64 ? d : rnd();
                    dr.push_back(dd);
                    wantc.push_back(g.second[dd % gm]);
                }
            }
            const uint32_t pn = (uint32_t)dr.size();
            uint8_t *e_qi = exact(qi);
            uint32_t *e_dr = exact(dr), *e_pc = exact(std::vector<uint32_t>(pn, kSent));
            rsk_conn_pick_in pin = {nullptr, by_id ? e_qi : nullptr, nullptr, e_dr, 0};
            rsk_conn_pick_out pout = {e_pc, nullptr, nullptr};
            if (rsk_conn_pick_host(&t, pick, pn, &pin, &pout, 1) != RSK_OK) FAIL("pick failed");
            for (uint32_t j = 0; j < pn; ++j)
                if (e_pc[j] != wantc[j]) FAIL("pick %u: %u, want %u", j, e_pc[j], wantc[j]);
            free(e_qi); free(e_dr); free(e_pc);
            // now and then rows die and leave, the close's way
            if (rnd() % 2 == 0) {
                std::vector<uint32_t> lst;
                for (uint32_t r = 0; r < cap; ++r)
                    if (rnd() % 3 == 0) lst.push_back(r);
                uint32_t ncl = (uint32_t)lst.size(), *e_lst = exact(lst);
                void *cwork = aligned((size_t)rsk_conn_close_bytes(cap, t.flags), 0xA5);
                rsk_conn_rows crow = {e_state};
                rsk_conn_close_in cin = {e_lst, &ncl, ncl, nullptr, cwork, RSK_CONN_CLOSE_REMOVE};
                rsk_conn_close_out cout = {nullptr, nullptr, nullptr, nullptr, pick, nullptr};
                if (rsk_conn_close_host(&t, &crow, &cin, &cout, 1) != RSK_OK) FAIL("close failed");
                free(e_lst); free(cwork);
            }
        }
        free(x_src); free(x_dst); free(x_ack); free(x_no); free(x_sp); free(x_dp); free(x_flag); free(x_id - bshift);
        free(p_id - bshift); free(p_hit); free(x_key); free(p_key); free(p_src); free(p_dst); free(p_conn); free(p_sp);
        free(p_dp); free(p_miss); free(o_rows); free(o_first); free(o_offer); free(o_orow); free(work); free(index0); free(pick0);
    }
    free(e_state); free(e_id - shift); free(e_flag); free(e_ka); free(e_key); free(e_est); free(e_src); free(e_dst);
    free(e_seq); free(e_ack); free(e_sp); free(e_dp); free(t.index); free(pick);
    return 0;
}

int main() {
    const uint32_t caps[] = {1, 2, 3, 15, 16, 17, 257, 1023, 1024, 1025, 2049, 3000};
    int bad = 0, runs = 0;
    for (int garbage = 0; garbage < 2; ++garbage)
        for (uint32_t cap : caps)
            for (int by_id = 0; by_id < 2; ++by_id)
                for (int fill = 0; fill < 3; ++fill)
                    for (uint32_t groups : {1u, 3u, cap < 64 ? cap : 64u, cap})
                        for (int with_pick = 0; with_pick < 2; ++with_pick) {
                            if (!by_id && groups != 1u) continue;
                            if (cap > 1100 && groups == cap && fill != 1) continue;
                            if (garbage && (fill != 1 || !with_pick)) continue;
                            bad += run(cap, by_id != 0, fill, groups, with_pick != 0, garbage != 0);
                            ++runs;
                        }
    std::printf("conn_create_host_check: %d tables, %d failed\n", runs, bad);
    return bad ? 1 : 0;
}
