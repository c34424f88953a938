// Stand-alone check of the connection table's host twins (rsk_conn_index_build_host,
// rsk_conn_resolve_host, rsk_conn_expand_host; rsock_amd/csrc/rsk_host.cpp) for a sanitizer build of
// the host code alone -- no HIP, no Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/conn_host_check.cpp rsock_amd/csrc/rsk_host.cpp -lpthread -o conn_host_check
// A few hundred generated tables and batches per run: client and BY_ID tables of 1 .. 5000 rows, empty,
// sparse and with every row LIVE, duplicate keys, keys 0 and 2^64 - 1, keys and IdBufs that differ in
// one bit, batches of present and absent keys with control and dropped packets.  Every column, the
// index included, is a heap block of exactly its bytes, so an access one element outside is reported.
// Compares with a std::map restatement; exit status 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "rsk_codec.h"

static uint64_t rng_state = 0xC0221;
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

typedef std::pair<uint64_t, uint64_t> Key;  // (IdBuf as a word, connKey); IdBuf 0 on a client

static uint64_t pick_key(const std::vector<uint64_t> &pool) {
    switch (rnd() % 8) {
        case 0: return 0;
        case 1: return ~0ull;
        case 2: return pool.empty() ? 1 : pool[rnd() % pool.size()] ^ (1ull << (32 + rnd() % 32));  // high word only
        case 3: return pool.empty() ? 2 : pool[rnd() % pool.size()] ^ (1ull << rnd() % 64);
        default: return 0x10000000ull | ((uint64_t)(10001 + rnd() % 10) << 16) | (32768 + rnd() % 2000);  // KeyForTcp
    }
}

static int run(uint32_t cap, bool by_id, int fill, uint32_t n, int nthreads) {
    // fill: 0 empty, 1 about a third LIVE, 2 every row LIVE, 3 every row LIVE with few distinct keys
    std::vector<uint8_t> state(cap), flag(cap), id(8ull * cap);
    std::vector<uint64_t> key(cap), idw(cap);
    std::vector<uint32_t> src(cap), dst(cap), seq(cap), ack(cap);
    std::vector<uint16_t> sp(cap), dp(cap);
    std::vector<uint64_t> pool, idpool;
    for (int k = 0; k < 4; ++k) idpool.push_back(rnd64());
    idpool.push_back(idpool[0] ^ (1ull << (8 * (rnd() % 8) + rnd() % 8)));  // one IdBuf byte differs
    for (uint32_t r = 0; r < cap; ++r) {
        const bool live = fill >= 2 || (fill == 1 && rnd() % 3 == 0);
        state[r] = (uint8_t)((live ? RSK_CONN_LIVE : 0u) | (rnd() % 4 ? RSK_CONN_ALIVE : 0u) | (rnd() % 8 == 0 ? 0x80u : 0u));
        key[r] = fill == 3 ? (pool.size() < 5 ? pick_key(pool) : pool[rnd() % pool.size()])
                           : (rnd() % 6 == 0 && !pool.empty() ? pool[rnd() % pool.size()] : (rnd() % 2 ? pick_key(pool) : rnd64()));
        pool.push_back(key[r]);
        idw[r] = by_id ? idpool[rnd() % idpool.size()] : 0ull;
        std::memcpy(&id[8ull * r], &idw[r], 8);
        src[r] = rnd(); dst[r] = rnd(); seq[r] = rnd(); ack[r] = rnd();
        sp[r] = (uint16_t)rnd(); dp[r] = (uint16_t)rnd(); flag[r] = (uint8_t)rnd();
    }
    // the restatement: the lowest LIVE row of every key
    std::map<Key, uint32_t> want_map;
    uint32_t want_dup = 0;
    for (uint32_t r = 0; r < cap; ++r)
        if (state[r] & RSK_CONN_LIVE) want_dup += !want_map.emplace(Key(idw[r], key[r]), r).second;

    const uint32_t tflags = by_id ? RSK_CONN_BY_ID : 0u;
    const uint64_t ibytes = rsk_conn_index_bytes(cap, tflags);
    int bad = ibytes == 0 || ibytes % 16 != 0;
    rsk_conn_table t;
    std::memset(&t, 0, sizeof t);
    t.capacity = cap;
    t.flags = tflags;
    uint8_t *e_state = exact(state), *e_flag = exact(flag), *e_id = exact(id);
    uint64_t *e_key = exact(key);
    uint32_t *e_src = exact(src), *e_dst = exact(dst), *e_seq = exact(seq), *e_ack = exact(ack);
    uint16_t *e_sp = exact(sp), *e_dp = exact(dp);
    t.state = e_state; t.conn_key = e_key; t.id = by_id ? e_id : nullptr;
    t.src = e_src; t.dst = e_dst; t.sp = e_sp; t.dp = e_dp; t.seq = e_seq; t.ack = e_ack; t.flag = e_flag;
    void *ix = nullptr;
    if (posix_memalign(&ix, 16, (size_t)ibytes)) return 1;  // exactly the index's bytes
    std::memset(ix, 0x5A, (size_t)ibytes);                  // the build must not depend on what was there
    t.index = (uint32_t *)ix;
    uint32_t ndup = 0xFFFFFFFFu;
    bad |= rsk_conn_index_build_host(&t, &ndup, nthreads) != RSK_OK || ndup != want_dup;
    bad |= rsk_conn_index_build_host(&t, nullptr, nthreads) != RSK_OK;  // a rebuild over a built index

    // a receive batch: present keys, absent keys, control packets, packets that are not VALID
    std::vector<int8_t> st(n);
    std::vector<uint8_t> cmd(n), pid(8ull * n);
    std::vector<uint64_t> pkey(n);
    std::vector<uint32_t> want_conn(n);
    std::vector<uint8_t> want_hit(n);
    std::vector<int8_t> want_miss(n);
    uint32_t want_nmiss = 0;
    for (uint32_t i = 0; i < n; ++i) {
        st[i] = (int8_t)(rnd() % 8 ? RSK_RECV_VALID : (rnd() % 2 ? RSK_RECV_DROP : RSK_RECV_CLOSE));
        cmd[i] = (uint8_t)(rnd() % 10 ? RSK_CMD_DATA : 1 + rnd() % 6);
        uint64_t w = by_id ? idpool[rnd() % idpool.size()] : rnd64();  // a client ignores the IdBuf
        if (cap && rnd() % 2) {
            const uint32_t r = rnd() % cap;
            pkey[i] = key[r];
            if (by_id && rnd() % 4) w = idw[r];
        } else {
            pkey[i] = rnd() % 2 ? pick_key(pool) : rnd64();
        }
        std::memcpy(&pid[8ull * i], &w, 8);
        const bool look = st[i] == RSK_RECV_VALID && cmd[i] == RSK_CMD_DATA;
        const auto it = look ? want_map.find(Key(by_id ? w : 0ull, pkey[i])) : want_map.end();
        want_conn[i] = it == want_map.end() ? RSK_CONN_NONE : it->second;
        want_hit[i] = want_conn[i] != RSK_CONN_NONE;
        want_miss[i] = look && !want_hit[i] ? RSK_RECV_VALID : RSK_RECV_DROP;
        want_nmiss += look && !want_hit[i];
    }
    int8_t *e_st = exact(st);
    uint8_t *e_cmd = exact(cmd), *e_pid = exact(pid);
    uint64_t *e_pkey = exact(pkey);
    for (int variant = 0; variant < 2; ++variant) {  // every optional output, then none of them
        std::vector<uint32_t> conn(n, 0xEEEEEEEEu);
        std::vector<uint8_t> hit(n, 0xEE);
        std::vector<int8_t> miss(n, 0x55);
        uint32_t nmiss = 0xFFFFFFFFu;
        rsk_conn_resolve_in in = {e_st, e_cmd, by_id ? e_pid : nullptr, e_pkey};
        rsk_conn_resolve_out out = {conn.data(), variant ? nullptr : hit.data(), variant ? nullptr : miss.data(),
                                    variant ? nullptr : &nmiss};
        bad |= rsk_conn_resolve_host(&t, n, &in, &out, nthreads) != RSK_OK || conn != want_conn;
        if (!variant) bad |= hit != want_hit || miss != want_miss || nmiss != want_nmiss;
    }
    {   // cmd == NULL: every VALID packet is DATA
        std::vector<uint32_t> conn(n, 0xEEEEEEEEu);
        rsk_conn_resolve_in in = {e_st, nullptr, by_id ? e_pid : nullptr, e_pkey};
        rsk_conn_resolve_out out = {conn.data(), nullptr, nullptr, nullptr};
        bad |= rsk_conn_resolve_host(&t, n, &in, &out, nthreads) != RSK_OK;
        for (uint32_t i = 0; i < n; ++i) {
            uint64_t w;
            std::memcpy(&w, &pid[8ull * i], 8);
            const auto it = st[i] == RSK_RECV_VALID ? want_map.find(Key(by_id ? w : 0ull, pkey[i])) : want_map.end();
            bad |= conn[i] != (it == want_map.end() ? RSK_CONN_NONE : it->second);
        }
    }

    // a send batch: rows of every kind, rows past the capacity, NONE
    std::vector<uint32_t> pick(n);
    for (uint32_t i = 0; i < n; ++i)
        pick[i] = rnd() % 8 == 0 ? (rnd() % 2 ? RSK_CONN_NONE : cap + rnd() % 3) : rnd() % cap;
    uint32_t *e_pick = exact(pick);
    std::vector<uint32_t> o_src(n, 0xEE), o_dst(n, 0xEE), o_ack(n, 0xEE);
    std::vector<uint16_t> o_sp(n, 0xEE), o_dp(n, 0xEE);
    std::vector<uint8_t> o_flag(n, 0xEE), o_ok(n, 0xEE), o_id(8ull * n, 0xEE);
    std::vector<uint64_t> o_key(n, 0xEE);
    uint32_t nbad = 0xFFFFFFFFu, want_nbad = 0;
    rsk_conn_expand_out eo = {o_src.data(), o_dst.data(), o_sp.data(), o_dp.data(), o_ack.data(), o_flag.data(),
                              o_key.data(), by_id ? o_id.data() : nullptr, o_ok.data(), &nbad};
    bad |= rsk_conn_expand_host(&t, n, e_pick, &eo, nthreads) != RSK_OK;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t r = pick[i];
        const bool ok = r < cap && (state[r] & 3u) == 3u;
        want_nbad += !ok;
        uint64_t w = 0;
        if (by_id) std::memcpy(&w, &o_id[8ull * i], 8);
        bad |= o_ok[i] != (ok ? 1 : 0) || o_src[i] != (ok ? src[r] : 0u) || o_dst[i] != (ok ? dst[r] : 0u) ||
               o_sp[i] != (ok ? sp[r] : 0) || o_dp[i] != (ok ? dp[r] : 0) || o_ack[i] != (ok ? ack[r] : 0u) ||
               o_flag[i] != (ok ? flag[r] : 0) || o_key[i] != (ok ? key[r] : 0ull) || (by_id && w != (ok ? idw[r] : 0ull));
    }
    bad |= nbad != want_nbad;
    rsk_conn_expand_out only_ok = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, o_ok.data(), nullptr};
    bad |= rsk_conn_expand_host(&t, n, e_pick, &only_ok, nthreads) != RSK_OK;

    free(e_state); free(e_flag); free(e_id); free(e_key); free(e_src); free(e_dst); free(e_seq); free(e_ack);
    free(e_sp); free(e_dp); free(ix); free(e_st); free(e_cmd); free(e_pid); free(e_pkey); free(e_pick);
    if (bad) printf("MISMATCH cap=%u by_id=%d fill=%d n=%u threads=%d\n", cap, (int)by_id, fill, n, nthreads);
    return bad;
}

int main() {
    int bad = 0, runs = 0;
    for (uint32_t cap : {1u, 2u, 3u, 64u, 65u, 1000u, 5000u})
        for (int by_id = 0; by_id < 2; ++by_id)
            for (int fill = 0; fill < 4; ++fill)
                for (uint32_t n : {1u, 300u, 9000u})
                    for (int th : {1, 4}) {
                        if (n == 9000u && cap != 64u && cap != 5000u) continue;
                        bad |= run(cap, by_id != 0, fill, n, th);
                        ++runs;
                    }
    // argument errors and the empty batch
    uint8_t st8 = 3, idb[8] = {0};
    uint64_t k = 1;
    alignas(16) uint32_t ix[4];
    uint32_t word = 7, cn = 0;
    int8_t s = 1;
    rsk_conn_table t;
    std::memset(&t, 0, sizeof t);
    t.capacity = 1; t.state = &st8; t.conn_key = &k; t.index = ix;
    bad |= rsk_conn_index_bytes(0, 0) != 0 || rsk_conn_index_bytes(RSK_CONN_MAX_ROWS + 1u, 0) != 0 ||
           rsk_conn_index_bytes(1, 2) != 0 || rsk_conn_index_bytes(1, 0) != 16 ||
           rsk_conn_index_bytes(RSK_CONN_MAX_ROWS, RSK_CONN_BY_ID) != 8ull * RSK_CONN_MAX_ROWS;
    bad |= rsk_conn_index_build_host(&t, &word, 1) != RSK_OK || word != 0;
    rsk_conn_resolve_in in = {&s, nullptr, nullptr, &k};
    rsk_conn_resolve_out out = {&cn, nullptr, nullptr, &word};
    bad |= rsk_conn_resolve_host(&t, 1, &in, &out, 1) != RSK_OK || cn != 0 || word != 0;
    word = 7;
    bad |= rsk_conn_resolve_host(&t, 0, &in, &out, 1) != RSK_OK || word != 0;  // n == 0 zeroes n_miss
    rsk_conn_table u = t;
    u.flags = RSK_CONN_BY_ID;  // id missing with BY_ID
    bad |= rsk_conn_index_build_host(&u, nullptr, 1) != RSK_EINVAL || rsk_conn_resolve_host(&u, 1, &in, &out, 1) != RSK_EINVAL;
    u.id = idb;                // in->id missing with BY_ID
    bad |= rsk_conn_resolve_host(&u, 1, &in, &out, 1) != RSK_EINVAL;
    u = t; u.flags = 2;
    bad |= rsk_conn_index_build_host(&u, nullptr, 1) != RSK_EINVAL || rsk_conn_resolve_host(&u, 1, &in, &out, 1) != RSK_EINVAL;
    u = t; u.capacity = 0;
    bad |= rsk_conn_index_build_host(&u, nullptr, 1) != RSK_EINVAL || rsk_conn_resolve_host(&u, 1, &in, &out, 1) != RSK_EINVAL;
    u = t; u.index = nullptr;
    bad |= rsk_conn_index_build_host(&u, nullptr, 1) != RSK_EINVAL || rsk_conn_resolve_host(&u, 1, &in, &out, 1) != RSK_EINVAL;
    u = t; u.index = ix + 1;   // not 16-B aligned
    bad |= rsk_conn_index_build_host(&u, nullptr, 1) != RSK_EINVAL;
    rsk_conn_resolve_in in2 = in;
    in2.status = nullptr;
    bad |= rsk_conn_resolve_host(&t, 1, &in2, &out, 1) != RSK_EINVAL || rsk_conn_resolve_host(&t, 1, nullptr, &out, 1) != RSK_EINVAL;
    uint8_t ok = 9;
    uint32_t o32 = 9;
    rsk_conn_expand_out eo;
    std::memset(&eo, 0, sizeof eo);
    eo.ok = &ok; eo.n_bad = &word;
    bad |= rsk_conn_expand_host(&t, 1, &cn, &eo, 1) != RSK_OK || ok != 1 || word != 0;
    eo.src = &o32;             // an output column the table does not have
    bad |= rsk_conn_expand_host(&t, 1, &cn, &eo, 1) != RSK_EINVAL;
    eo.src = nullptr; eo.ok = nullptr;
    bad |= rsk_conn_expand_host(&t, 1, &cn, &eo, 1) != RSK_EINVAL;
    word = 7;
    bad |= rsk_conn_expand_host(&t, 0, nullptr, &eo, 1) != RSK_OK || word != 0;
    printf("%s: %d runs\n", bad ? "FAILED" : "ok", runs);
    return bad;
}
