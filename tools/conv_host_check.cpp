// Stand-alone check of the conv table's host twins (rsk_conv_index_build_host, rsk_conv_resolve_host,
// rsk_conv_send_host, rsk_conv_flush_host; rsock_amd/csrc/rsk_host.cpp) for a sanitizer build of the host
// code alone -- no HIP, no Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/conv_host_check.cpp rsock_amd/csrc/rsk_host.cpp -lpthread -o conv_host_check
// A few hundred generated tables and batches per run: every flag combination, tables of 1 .. 5000 rows,
// empty, sparse, every row LIVE, every row LIVE with few distinct keys (duplicates), all of a batch on one
// row, keys that differ in one bit of dst / conv / IdBuf, CONV_RST packets with their ctl pair, control
// and dropped packets, an IdBuf column at an odd address.  Every column, the index included, is a heap
// block of exactly its bytes, so an access one element outside is reported.  Compares with a std::map
// restatement; exit status 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "rsk_codec.h"

static uint64_t rng_state = 0xC0117;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static uint64_t rnd64() { return ((uint64_t)rnd() << 33) ^ ((uint64_t)rnd() << 11) ^ rnd(); }

// A heap block of exactly v's bytes plus `shift` in front (at least one byte, so never NULL).
template <typename T>
static T *exact(const std::vector<T> &v, size_t shift = 0) {
    uint8_t *p = (uint8_t *)malloc(shift + (v.empty() ? 1 : v.size() * sizeof(T)));
    if (!v.empty()) std::memcpy(p + shift, v.data(), v.size() * sizeof(T));
    return (T *)(p + shift);
}

typedef std::tuple<uint64_t, uint32_t, uint32_t> Key;  // (IdBuf word, dst, conv); unused parts 0

struct Pools {
    std::vector<uint32_t> conv, dst;
    std::vector<uint64_t> id;
};
static Pools make_pools() {
    Pools p;
    const uint32_t c0 = rnd(), d0 = rnd();
    const uint64_t i0 = rnd64();
    p.conv = {0u, 0xFFFFFFFFu, c0, c0 ^ (1u << rnd() % 32), c0 ^ 0x80000000u, c0 ^ 1u, rnd(), rnd()};
    p.dst = {0u, 0xFFFFFFFFu, d0, d0 ^ (1u << rnd() % 32), rnd()};
    p.id = {0ull, ~0ull, i0, i0 ^ (1ull << rnd() % 64), rnd64()};
    return p;
}

static int run(uint32_t cap, uint32_t flags, int fill, uint32_t n, int nthreads) {
    // fill: 0 empty, 1 about a third LIVE, 2 every row LIVE, 3 every row LIVE with few distinct keys
    const bool by_dst = flags & RSK_CONV_BY_DST, by_id = flags & RSK_CONV_BY_ID;
    const Pools p = make_pools();
    std::vector<uint8_t> state(cap), alive(cap), id(8ull * cap);
    std::vector<uint32_t> conv(cap), dst(cap), ci(cap), co(cap), pi(cap), po(cap);
    std::vector<uint64_t> idw(cap);
    for (uint32_t r = 0; r < cap; ++r) {
        const bool live = fill >= 2 || (fill == 1 && rnd() % 3 == 0);
        state[r] = (uint8_t)((live ? RSK_CONN_LIVE : 0u) | (rnd() % 4 ? 0u : 0x82u));
        conv[r] = fill == 3 || rnd() % 3 == 0 ? p.conv[rnd() % p.conv.size()] : rnd();
        dst[r] = p.dst[rnd() % p.dst.size()];
        idw[r] = p.id[rnd() % p.id.size()];
        std::memcpy(&id[8ull * r], &idw[r], 8);
        alive[r] = (uint8_t)(rnd() % 4 ? 1 + rnd() % 2 : 0);
        ci[r] = rnd() % 2 ? 0xFFFFFFF0u + rnd() % 16 : rnd();
        co[r] = rnd();
        pi[r] = rnd() % 3 ? ci[r] : rnd();
        po[r] = rnd() % 3 ? co[r] : rnd();
    }
    auto row_key = [&](uint32_t r) { return Key(by_id ? idw[r] : 0ull, by_dst ? dst[r] : 0u, conv[r]); };
    std::map<Key, uint32_t> want_map;
    uint32_t want_dup = 0;
    for (uint32_t r = 0; r < cap; ++r)
        if (state[r] & RSK_CONN_LIVE) want_dup += !want_map.emplace(row_key(r), r).second;

    const uint64_t ibytes = rsk_conn_index_bytes(cap, 0);
    int bad = ibytes == 0 || ibytes % 16 != 0;
    rsk_conv_table t;
    std::memset(&t, 0, sizeof t);
    t.capacity = cap;
    t.flags = flags;
    const size_t shift = rnd() % 2 ? 3 : 0;  // the table's IdBuf column at an odd address
    uint8_t *e_state = exact(state), *e_alive = exact(alive), *e_id = exact(id, shift);
    uint32_t *e_conv = exact(conv), *e_dst = exact(dst), *e_ci = exact(ci), *e_co = exact(co), *e_pi = exact(pi), *e_po = exact(po);
    t.state = e_state; t.conv = e_conv; t.dst = by_dst ? e_dst : nullptr; t.id = by_id ? e_id : nullptr;
    t.cur_in = e_ci; t.cur_out = e_co; t.prev_in = e_pi; t.prev_out = e_po; t.alive = e_alive;
    void *ix = nullptr;
    if (posix_memalign(&ix, 16, (size_t)ibytes)) return 1;
    std::memset(ix, 0x5A, (size_t)ibytes);
    t.index = (uint32_t *)ix;
    uint32_t ndup = 0xFFFFFFFFu;
    bad |= rsk_conv_index_build_host(&t, &ndup, nthreads) != RSK_OK || ndup != want_dup;
    bad |= rsk_conv_index_build_host(&t, nullptr, nthreads) != RSK_OK;

    // a receive batch; with `one` every DATA packet names one row's key
    const bool one = cap && rnd() % 4 == 0;
    const uint32_t one_row = cap ? rnd() % cap : 0;
    std::vector<int8_t> st(n), want_unk(n);
    std::vector<uint8_t> cmd(n), hit(n), kind(n), pid(8ull * n);
    std::vector<uint32_t> pconv(n), pdst(n), want_row(n), want_first(cap, 0xFFFFFFFFu), want_ci(ci);
    std::vector<uint64_t> arg(n), want_body;
    std::vector<uint32_t> want_src;
    for (uint32_t i = 0; i < n; ++i) {
        st[i] = (int8_t)(rnd() % 8 ? RSK_RECV_VALID : (rnd() % 2 ? RSK_RECV_DROP : RSK_RECV_CLOSE));
        cmd[i] = (uint8_t)(rnd() % 6 ? RSK_CMD_DATA : 1 + rnd() % 5);
        hit[i] = rnd() % 10 != 0;
        uint32_t cv, d;
        uint64_t w;
        if (cap && (one || rnd() % 2)) {
            const uint32_t r = one ? one_row : rnd() % cap;
            cv = conv[r]; d = dst[r]; w = idw[r];
            if (!one && rnd() % 4 == 0) {  // one bit off in one part
                switch (rnd() % 3) {
                    case 0: cv ^= 1u << rnd() % 32; break;
                    case 1: d ^= 1u << rnd() % 32; break;
                    default: w ^= 1ull << rnd() % 64;
                }
            }
        } else {
            cv = p.conv[rnd() % p.conv.size()]; d = p.dst[rnd() % p.dst.size()]; w = p.id[rnd() % p.id.size()];
        }
        const bool rst_pkt = st[i] == RSK_RECV_VALID && cmd[i] == RSK_CMD_CONV_RST;
        kind[i] = (uint8_t)(st[i] != RSK_RECV_VALID ? RSK_CTL_NONE : cmd[i] > 4 ? RSK_CTL_UNKNOWN : cmd[i]);
        if (rst_pkt && rnd() % 8 == 0) kind[i] = RSK_CTL_SHORT;
        arg[i] = kind[i] == RSK_CTL_CONV_RST ? ((uint64_t)(rnd() % 2) << 37) | cv : rnd64();
        pconv[i] = kind[i] == RSK_CTL_CONV_RST ? rnd() : cv;  // a reset's own conv field is not its key
        pdst[i] = d;
        std::memcpy(&pid[8ull * i], &w, 8);
        const bool ex = st[i] == RSK_RECV_VALID && cmd[i] == RSK_CMD_DATA && hit[i];
        const bool rst = !ex && by_dst && kind[i] == RSK_CTL_CONV_RST;
        want_row[i] = RSK_CONN_NONE;
        if (ex || rst) {
            const auto it = want_map.find(Key(by_id ? w : 0ull, by_dst ? d : 0u, ex ? pconv[i] : cv));
            if (it != want_map.end()) want_row[i] = it->second;
        }
        const bool unk = ex && want_row[i] == RSK_CONN_NONE;
        want_unk[i] = unk ? RSK_RECV_VALID : RSK_RECV_DROP;
        if (unk) { want_body.push_back(pconv[i]); want_src.push_back(i); }
        if (ex && !unk) ++want_ci[want_row[i]];
        if (rst && want_row[i] != RSK_CONN_NONE && want_first[want_row[i]] == 0xFFFFFFFFu) want_first[want_row[i]] = i;
    }
    int8_t *e_st = exact(st);
    uint8_t *e_cmd = exact(cmd), *e_hit = exact(hit), *e_kind = exact(kind), *e_pid = exact(pid, 5);
    uint32_t *e_pconv = exact(pconv), *e_pdst = exact(pdst);
    uint64_t *e_arg = exact(arg);
    for (int variant = 0; variant < 2; ++variant) {  // every optional output, then none (and no counting)
        std::vector<uint32_t> row(n, 0xEEEEEEEEu), first(cap, 0xEEEEEEEEu), src(n, 0xEEEEEEEEu);
        std::vector<int8_t> unk(n, 0x55);
        std::vector<uint64_t> body(n, 0xEE), avoid(n, 0xEE), off(n, 0xEE);
        std::vector<uint16_t> len(n, 0xEEEE);
        std::vector<uint8_t> mc(n, 0xEE), mid(8ull * n, 0xEE);
        uint32_t nunk = 0xFFFFFFFFu, nmsg = 0xFFFFFFFFu;
        rsk_conv_resolve_in in = {e_st, e_cmd, e_hit, by_id || rnd() % 2 ? e_pid : nullptr, e_pconv, by_dst ? e_pdst : nullptr,
                                  e_kind, e_arg};
        rsk_conv_resolve_out out;
        std::memset(&out, 0, sizeof out);
        out.conv_row = row.data();
        if (!variant) {
            out.unknown = unk.data(); out.n_unknown = &nunk; out.rst_first = first.data();
            out.msgs.cmd = mc.data(); out.msgs.body = body.data(); out.msgs.id = mid.data(); out.msgs.src = src.data();
            out.msgs.avoid_key = avoid.data(); out.msgs.pay_off = off.data(); out.msgs.pay_len = len.data();
            out.msgs.n_msg = &nmsg;
        }
        rsk_conv_table tv = t;
        if (variant) tv.cur_in = nullptr;
        bad |= rsk_conv_resolve_host(&tv, n, &in, &out, nthreads) != RSK_OK || row != want_row;
        if (!variant) {
            bad |= unk != want_unk || nunk != want_src.size() || nmsg != want_src.size() || first != want_first;
            for (uint32_t k = 0; k < want_src.size(); ++k) {
                uint64_t w = 0, pw = 0;
                std::memcpy(&w, &mid[8ull * k], 8);
                if (in.id) std::memcpy(&pw, &pid[8ull * want_src[k]], 8);
                bad |= mc[k] != RSK_CMD_CONV_RST || body[k] != want_body[k] || src[k] != want_src[k] || avoid[k] != 0 ||
                       off[k] != 8ull * k || len[k] != 4 || w != pw;
            }
            for (uint32_t k = (uint32_t)want_src.size(); k < n; ++k) bad |= src[k] != 0xEEEEEEEEu || len[k] != 0xEEEE;
            bad |= std::memcmp(e_ci, want_ci.data(), 4ull * cap) != 0;
        }
    }
    bad |= std::memcmp(e_ci, want_ci.data(), 4ull * cap) != 0;  // the second variant counted nothing
    ci = want_ci;

    // a send batch: rows of every kind, rows past the capacity, NONE; counted where sent > 0
    std::vector<uint32_t> pick(n);
    std::vector<int32_t> sent(n);
    std::vector<uint32_t> want_co(co);
    uint32_t want_nbad = 0;
    for (uint32_t i = 0; i < n; ++i) {
        pick[i] = rnd() % 8 == 0 ? (rnd() % 2 ? RSK_CONN_NONE : cap + rnd() % 3) : (one ? one_row : rnd() % cap);
        sent[i] = rnd() % 4 == 0 ? (rnd() % 2 ? 0 : -1) : 31 + (int32_t)(rnd() % 1400);
    }
    uint32_t *e_pick = exact(pick);
    int32_t *e_sent = exact(sent);
    std::vector<uint32_t> o_conv(n, 0xEE), o_dst(n, 0xEE);
    std::vector<uint8_t> o_ok(n, 0xEE), o_id(8ull * n, 0xEE);
    uint32_t nbad = 0xFFFFFFFFu;
    rsk_conv_send_out so = {o_conv.data(), by_dst ? o_dst.data() : nullptr, by_id ? o_id.data() : nullptr, o_ok.data(), &nbad};
    bad |= rsk_conv_send_host(&t, n, e_pick, nullptr, &so, nthreads) != RSK_OK;  // expand: no counting
    bad |= std::memcmp(e_co, want_co.data(), 4ull * cap) != 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t r = pick[i];
        const bool ok = r < cap && (state[r] & RSK_CONN_LIVE);
        want_nbad += !ok;
        uint64_t w = 0;
        if (by_id) std::memcpy(&w, &o_id[8ull * i], 8);
        bad |= o_ok[i] != (ok ? 1 : 0) || o_conv[i] != (ok ? conv[r] : 0u) || (by_dst && o_dst[i] != (ok ? dst[r] : 0u)) ||
               (by_id && w != (ok ? idw[r] : 0ull));
        if (ok && sent[i] > 0) ++want_co[r];
    }
    bad |= nbad != want_nbad;
    rsk_conv_send_out none;
    std::memset(&none, 0, sizeof none);
    bad |= rsk_conv_send_host(&t, n, e_pick, e_sent, &none, nthreads) != RSK_OK;  // count: no output columns
    bad |= std::memcmp(e_co, want_co.data(), 4ull * cap) != 0;
    co = want_co;

    // two flushes: what the first marks, the second lists
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<uint32_t> want_dead;
        uint32_t want_alive = 0;
        for (uint32_t r = 0; r < cap; ++r) {
            if (!(state[r] & RSK_CONN_LIVE)) continue;
            if (!alive[r]) { want_dead.push_back(r); continue; }
            const bool a = pi[r] != ci[r] && po[r] != co[r];
            if (!a) alive[r] = 0;
            pi[r] = ci[r]; po[r] = co[r];
            want_alive += a;
        }
        std::vector<uint32_t> dead(cap, 0xEEEEEEEEu);
        uint32_t nd = 0xFFFFFFFFu, na = 0xFFFFFFFFu;
        rsk_conv_flush_out fo = {pass ? nullptr : dead.data(), pass && rnd() % 2 ? nullptr : &nd, &na};
        bad |= rsk_conv_flush_host(&t, &fo, nthreads) != RSK_OK || na != want_alive;
        if (fo.n_dead) bad |= nd != want_dead.size();
        if (fo.dead_rows)
            for (uint32_t k = 0; k < cap; ++k) bad |= dead[k] != (k < want_dead.size() ? want_dead[k] : 0xEEEEEEEEu);
        bad |= std::memcmp(e_alive, alive.data(), cap) != 0 || std::memcmp(e_pi, pi.data(), 4ull * cap) != 0 ||
               std::memcmp(e_po, po.data(), 4ull * cap) != 0 || std::memcmp(e_ci, ci.data(), 4ull * cap) != 0 ||
               std::memcmp(e_co, co.data(), 4ull * cap) != 0;
    }

    free(e_state); free(e_alive); free((uint8_t *)e_id - shift); free(e_conv); free(e_dst); free(e_ci); free(e_co); free(e_pi);
    free(e_po); free(ix); free(e_st); free(e_cmd); free(e_hit); free(e_kind); free(e_pid - 5); free(e_pconv); free(e_pdst);
    free(e_arg); free(e_pick); free(e_sent);
    if (bad) printf("MISMATCH cap=%u flags=%u fill=%d n=%u threads=%d\n", cap, flags, fill, n, nthreads);
    return bad;
}

int main() {
    int bad = 0, runs = 0;
    for (uint32_t cap : {1u, 2u, 3u, 64u, 65u, 1000u, 5000u})
        for (uint32_t flags = 0; flags < 4; ++flags)
            for (int fill = 0; fill < 4; ++fill)
                for (uint32_t n : {1u, 300u, 9000u})
                    for (int th : {1, 4}) {
                        if (n == 9000u && cap != 64u && cap != 5000u) continue;
                        if (th == 4 && n != 9000u) continue;
                        bad |= run(cap, flags, fill, n, th);
                        ++runs;
                    }
    // argument errors and the empty batch
    uint8_t st8 = RSK_CONN_LIVE, al = 1, idb[8] = {0};
    uint32_t cv = 5, ds = 6, c4[4] = {0, 0, 0, 0};
    alignas(16) uint32_t ix[4];
    uint32_t word = 7, row = 9;
    int8_t s = 1;
    rsk_conv_table t;
    std::memset(&t, 0, sizeof t);
    t.capacity = 1; t.state = &st8; t.conv = &cv; t.index = ix; t.alive = &al;
    t.cur_in = &c4[0]; t.cur_out = &c4[1]; t.prev_in = &c4[2]; t.prev_out = &c4[3];
    bad |= rsk_conv_index_build_host(&t, &word, 1) != RSK_OK || word != 0;
    rsk_conv_resolve_in in;
    std::memset(&in, 0, sizeof in);
    in.status = &s; in.conv = &cv;
    rsk_conv_resolve_out out;
    std::memset(&out, 0, sizeof out);
    out.conv_row = &row; out.n_unknown = &word;
    bad |= rsk_conv_resolve_host(&t, 1, &in, &out, 1) != RSK_OK || row != 0 || word != 0 || c4[0] != 1;
    word = 7;
    bad |= rsk_conv_resolve_host(&t, 0, &in, &out, 1) != RSK_OK || word != 0;  // n == 0 zeroes n_unknown
    rsk_conv_table u = t;
    u.flags = RSK_CONV_BY_DST;  // dst missing with its flag: in the table, then in the batch
    bad |= rsk_conv_index_build_host(&u, nullptr, 1) != RSK_EINVAL || rsk_conv_resolve_host(&u, 1, &in, &out, 1) != RSK_EINVAL;
    u.dst = &ds;
    bad |= rsk_conv_index_build_host(&u, nullptr, 1) != RSK_OK || rsk_conv_resolve_host(&u, 1, &in, &out, 1) != RSK_EINVAL;
    u = t; u.flags = RSK_CONV_BY_ID;
    bad |= rsk_conv_index_build_host(&u, nullptr, 1) != RSK_EINVAL;
    u.id = idb;
    bad |= rsk_conv_resolve_host(&u, 1, &in, &out, 1) != RSK_EINVAL;
    u = t; u.flags = 4;
    bad |= rsk_conv_index_build_host(&u, nullptr, 1) != RSK_EINVAL || rsk_conv_resolve_host(&u, 1, &in, &out, 1) != RSK_EINVAL;
    u = t; u.capacity = 0;
    bad |= rsk_conv_index_build_host(&u, nullptr, 1) != RSK_EINVAL || rsk_conv_resolve_host(&u, 1, &in, &out, 1) != RSK_EINVAL;
    u = t; u.index = ix + 1;
    bad |= rsk_conv_index_build_host(&u, nullptr, 1) != RSK_EINVAL;
    rsk_conv_resolve_in in2 = in;
    uint8_t kd = 0;
    in2.ctl_kind = &kd;  // the ctl pair half set
    bad |= rsk_conv_resolve_host(&t, 1, &in2, &out, 1) != RSK_EINVAL;
    rsk_conv_resolve_out out2 = out;
    uint64_t body = 0;
    out2.msgs.body = &body;  // a message array without n_msg
    bad |= rsk_conv_resolve_host(&t, 1, &in, &out2, 1) != RSK_EINVAL;
    rsk_conv_flush_out fo = {&row, nullptr, nullptr};  // dead_rows without n_dead
    bad |= rsk_conv_flush_host(&t, &fo, 1) != RSK_EINVAL;
    u = t; u.alive = nullptr;
    fo.dead_rows = nullptr;
    bad |= rsk_conv_flush_host(&u, &fo, 1) != RSK_EINVAL || rsk_conv_flush_host(&t, &fo, 1) != RSK_OK;
    rsk_conv_send_out so;
    std::memset(&so, 0, sizeof so);
    so.dst = &ds;  // an output column the table does not have
    row = 0;
    bad |= rsk_conv_send_host(&t, 1, &row, nullptr, &so, 1) != RSK_EINVAL || rsk_conv_send_host(&t, 1, nullptr, nullptr, &so, 1) != RSK_EINVAL;
    printf("%s: %d runs\n", bad ? "FAILED" : "ok", runs);
    return bad;
}
