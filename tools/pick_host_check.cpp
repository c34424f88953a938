// Stand-alone check of the send pick's host twins (rsk_conn_pick_build_host, rsk_conn_pick_host;
// rsock_amd/csrc/rsk_host.cpp) for a sanitizer build of the host code alone -- no HIP, no Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/pick_host_check.cpp rsock_amd/csrc/rsk_host.cpp -lpthread -o pick_host_check
// A few hundred generated tables and batches per run: both flag values, tables of 1 .. 5000 rows, no
// candidate, some, every row one, few or many IdBufs (the all-zero one among them), avoid keys of candidates,
// of dead rows and of no row, len <= 0, IdBuf columns at odd addresses, draws from a column and from the
// seed.  Then the same batches over a pick index that is stale (state changed, no rebuild) and over ones
// that were never built (words from rows and offsets inside and outside their ranges): every conn must be
// NONE or a row of the table.  Every column, the conn index and the pick index included, is a heap block
// of exactly its bytes, so an access one element outside is reported.  Compares with a std::map
// restatement of the header's rule; exit status 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "rsk_codec.h"

static uint64_t rng_state = 0x91C4;
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

static uint64_t splitmix64_at(uint64_t seed, uint64_t i) {
    uint64_t z = seed + (i + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int run(uint32_t cap, bool by_id, int fill, uint32_t n_ids, uint32_t n, int nthreads) {
    // fill: 0 no candidate, 1 about a third, 2 every row
    constexpr uint8_t kUp = RSK_CONN_LIVE | RSK_CONN_ALIVE;
    std::vector<uint64_t> pool(n_ids + 2);
    for (auto &w : pool) w = rnd64();
    pool[0] = 0;  // an ordinary id; the last two are given to no row
    std::vector<uint8_t> state(cap), id(8ull * cap);
    std::vector<uint64_t> key(cap), idw(cap);
    for (uint32_t r = 0; r < cap; ++r) {
        state[r] = (uint8_t)(fill == 2 ? kUp : fill == 1 ? rnd() % 8 : rnd() % 2 ? RSK_CONN_LIVE : RSK_CONN_ALIVE);
        key[r] = rnd() % 8 ? 1 + rnd64() % 50 : rnd64();  // duplicates: the lowest LIVE row is the key's
        idw[r] = pool[rnd() % n_ids];
        std::memcpy(&id[8ull * r], &idw[r], 8);
    }
    std::map<uint64_t, std::vector<uint32_t>> groups;
    std::map<std::pair<uint64_t, uint64_t>, uint32_t> by_key;
    uint32_t want_cand = 0;
    for (uint32_t r = 0; r < cap; ++r) {
        if ((state[r] & kUp) == kUp) { groups[by_id ? idw[r] : 0].push_back(r); ++want_cand; }
        if (state[r] & RSK_CONN_LIVE) by_key.emplace(std::make_pair(by_id ? idw[r] : 0ull, key[r]), r);
    }

    const uint32_t flags = by_id ? RSK_CONN_BY_ID : 0;
    const uint64_t ibytes = rsk_conn_index_bytes(cap, flags), pbytes = rsk_conn_pick_bytes(cap, flags);
    int bad = ibytes == 0 || pbytes == 0 || pbytes % 16 != 0;
    rsk_conn_table t;
    std::memset(&t, 0, sizeof t);
    t.capacity = cap;
    t.flags = flags;
    const size_t shift = rnd() % 2 ? 3 : 0;  // the table's IdBuf column at an odd address
    uint8_t *e_state = exact(state), *e_id = exact(id, shift);
    uint64_t *e_key = exact(key);
    t.state = e_state; t.conn_key = e_key; t.id = by_id || rnd() % 2 ? e_id : nullptr;
    void *ix = nullptr, *px = nullptr;
    if (posix_memalign(&ix, 16, (size_t)ibytes) || posix_memalign(&px, 16, (size_t)pbytes)) return 1;
    std::memset(ix, 0x5A, (size_t)ibytes);
    std::memset(px, 0x5A, (size_t)pbytes);
    t.index = (uint32_t *)ix;
    uint32_t *pick = (uint32_t *)px;
    uint32_t counts[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    bad |= rsk_conn_index_build_host(&t, nullptr, 1) != RSK_OK;
    bad |= rsk_conn_pick_build_host(&t, pick, counts, nthreads) != RSK_OK || counts[0] != groups.size() || counts[1] != want_cand;
    bad |= rsk_conn_pick_build_host(&t, pick, nullptr, nthreads) != RSK_OK;

    std::vector<int32_t> len(n);
    std::vector<uint8_t> pid(8ull * n);
    std::vector<uint64_t> avoid(n), pw(n);
    std::vector<uint32_t> draw(n);
    for (uint32_t i = 0; i < n; ++i) {
        len[i] = rnd() % 8 ? 1 + (int32_t)(rnd() % 1400) : -(int32_t)(rnd() % 3);
        const uint32_t r = rnd() % cap;
        pw[i] = rnd() % 4 ? idw[r] : pool[rnd() % pool.size()];
        std::memcpy(&pid[8ull * i], &pw[i], 8);
        avoid[i] = rnd() % 2 ? 0 : rnd() % 8 ? key[r] : rnd64();
        draw[i] = rnd() % 16 ? (rnd() << 1) ^ rnd() : (rnd() % 2 ? 0xFFFFFFFFu : 0u);
    }
    int32_t *e_len = exact(len);
    uint8_t *e_pid = exact(pid, 5);
    uint64_t *e_avoid = exact(avoid);
    uint32_t *e_draw = exact(draw);
    const uint64_t seed = rnd64();
    for (int variant = 0; variant < 3; ++variant) {  // every column; no len / avoid / used; the seed's draws
        rsk_conn_pick_in in = {variant == 1 ? nullptr : e_len, by_id || rnd() % 2 ? e_pid : nullptr,
                               variant == 1 ? nullptr : e_avoid, variant == 2 ? nullptr : e_draw, seed};
        std::vector<uint32_t> conn(n, 0xEEEEEEEEu), want(n, RSK_CONN_NONE);
        std::vector<uint8_t> used(cap, 0), want_used(cap, 0);
        uint32_t nn = 0xFFFFFFFFu, want_nn = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (in.len && len[i] <= 0) continue;
            const uint64_t w = by_id ? pw[i] : 0;
            const auto g = groups.find(w);
            if (g == groups.end()) { ++want_nn; continue; }
            const std::vector<uint32_t> &c = g->second;
            const uint32_t m = (uint32_t)c.size(), d = in.draw ? draw[i] : (uint32_t)(splitmix64_at(seed, i) >> 32);
            uint32_t p = 0xFFFFFFFFu;
            if (in.avoid_key && avoid[i]) {
                const auto it = by_key.find(std::make_pair(w, avoid[i]));
                if (it != by_key.end())
                    for (uint32_t k = 0; k < m; ++k)
                        if (c[k] == it->second) p = k;
            }
            uint32_t k;
            if (p == 0xFFFFFFFFu) k = d % m;
            else if (m == 1) { ++want_nn; continue; }
            else { k = d % (m - 1); k += k >= p; }
            want[i] = c[k];
            want_used[c[k]] = 1;
        }
        rsk_conn_pick_out out = {conn.data(), variant == 1 ? nullptr : &nn, variant == 1 ? nullptr : used.data()};
        bad |= rsk_conn_pick_host(&t, pick, n, &in, &out, nthreads) != RSK_OK || conn != want;
        if (variant != 1) bad |= nn != want_nn || used != want_used;
    }

    // the index gone stale, then never built: only the bounds are promised
    auto bounded = [&](const uint32_t *pk) {
        std::vector<uint32_t> conn(n, 0xEEEEEEEEu);
        std::vector<uint8_t> used(cap, 0);
        uint32_t nn = 0;
        rsk_conn_pick_in in = {e_len, e_pid, e_avoid, e_draw, seed};
        rsk_conn_pick_out out = {conn.data(), &nn, used.data()};
        int b = rsk_conn_pick_host(&t, pk, n, &in, &out, nthreads) != RSK_OK;
        for (uint32_t i = 0; i < n; ++i) b |= conn[i] != RSK_CONN_NONE && conn[i] >= cap;
        return b;
    };
    for (uint32_t r = 0; r < cap; ++r) e_state[r] = (uint8_t)(rnd() % 4);
    bad |= bounded(pick);
    const uint32_t words = (uint32_t)(pbytes / 4);
    const uint32_t menu[] = {0u, 1u, 2u, cap - 1u, cap, cap + 1u, 2u * cap, words, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (int g = 0; g < 4; ++g) {
        std::vector<uint32_t> junk(words);
        for (uint32_t k = 0; k < words; ++k) junk[k] = rnd() % 2 ? menu[rnd() % 12] : rnd() % (2u * cap + 2u);
        if (by_id && g % 2) {  // group entries under ids the packets carry, so the probe finds them
            const uint32_t c4 = (cap + 3u) & ~3u, slots = (words - 4u - 2u * c4) / 5u;
            for (uint32_t s = 0; s < slots; ++s) std::memcpy(&junk[words - 4u * slots + 4u * s], &pool[rnd() % pool.size()], 8);
        }
        void *jx = nullptr;
        if (posix_memalign(&jx, 16, (size_t)pbytes)) return 1;
        std::memcpy(jx, junk.data(), (size_t)pbytes);
        bad |= bounded((const uint32_t *)jx);
        free(jx);
    }

    free(e_state); free(e_id - shift); free(e_key); free(ix); free(px); free(e_len); free(e_pid - 5); free(e_avoid); free(e_draw);
    if (bad) printf("MISMATCH cap=%u by_id=%d fill=%d ids=%u n=%u threads=%d\n", cap, (int)by_id, fill, n_ids, n, nthreads);
    return bad;
}

int main() {
    int bad = 0, runs = 0;
    for (uint32_t cap : {1u, 2u, 3u, 64u, 65u, 1000u, 5000u})
        for (int by_id = 0; by_id < 2; ++by_id)
            for (int fill = 0; fill < 3; ++fill)
                for (uint32_t n_ids : {1u, 3u, 400u})
                    for (uint32_t n : {1u, 300u, 9000u})
                        for (int th : {1, 4}) {
                            if (n == 9000u && cap != 64u && cap != 5000u) continue;
                            if (th == 4 && n != 9000u) continue;
                            if (!by_id && n_ids != 3u) continue;
                            bad |= run(cap, by_id != 0, fill, n_ids, n, th);
                            ++runs;
                        }
    // argument errors and the empty batch
    uint8_t st8 = RSK_CONN_LIVE | RSK_CONN_ALIVE, idb[8] = {0};
    uint64_t key = 5, av = 5;
    alignas(16) uint32_t ix[4], pk[16];
    uint32_t row = 9, word = 7;
    rsk_conn_table t;
    std::memset(&t, 0, sizeof t);
    t.capacity = 1; t.state = &st8; t.conn_key = &key; t.index = ix;
    bad |= rsk_conn_index_build_host(&t, nullptr, 1) != RSK_OK || rsk_conn_pick_build_host(&t, pk, nullptr, 1) != RSK_OK;
    rsk_conn_pick_in in;
    std::memset(&in, 0, sizeof in);
    rsk_conn_pick_out out = {&row, &word, nullptr};
    bad |= rsk_conn_pick_host(&t, pk, 1, &in, &out, 1) != RSK_OK || row != 0 || word != 0;
    in.avoid_key = &av;  // the only candidate is the one to avoid
    bad |= rsk_conn_pick_host(&t, pk, 1, &in, &out, 1) != RSK_OK || row != RSK_CONN_NONE || word != 1;
    bad |= rsk_conn_pick_host(&t, pk, 0, &in, &out, 1) != RSK_OK || word != 0;  // n == 0 zeroes n_none
    rsk_conn_table u = t;
    u.index = nullptr;
    bad |= rsk_conn_pick_host(&u, pk, 1, &in, &out, 1) != RSK_EINVAL;
    u = t; u.conn_key = nullptr;
    bad |= rsk_conn_pick_host(&u, pk, 1, &in, &out, 1) != RSK_EINVAL;
    in.avoid_key = nullptr;
    bad |= rsk_conn_pick_host(&u, pk, 1, &in, &out, 1) != RSK_OK;
    u = t; u.flags = RSK_CONN_BY_ID;  // id missing with BY_ID: in the table, then in the batch
    bad |= rsk_conn_pick_build_host(&u, pk, nullptr, 1) != RSK_EINVAL || rsk_conn_pick_host(&u, pk, 1, &in, &out, 1) != RSK_EINVAL;
    u.id = idb;
    bad |= rsk_conn_pick_host(&u, pk, 1, &in, &out, 1) != RSK_EINVAL;
    u = t; u.flags = 2;
    bad |= rsk_conn_pick_build_host(&u, pk, nullptr, 1) != RSK_EINVAL || rsk_conn_pick_host(&u, pk, 1, &in, &out, 1) != RSK_EINVAL;
    u = t; u.capacity = 0;
    bad |= rsk_conn_pick_build_host(&u, pk, nullptr, 1) != RSK_EINVAL || rsk_conn_pick_host(&u, pk, 1, &in, &out, 1) != RSK_EINVAL;
    u = t; u.state = nullptr;
    bad |= rsk_conn_pick_build_host(&u, pk, nullptr, 1) != RSK_EINVAL;
    bad |= rsk_conn_pick_build_host(&t, pk + 1, nullptr, 1) != RSK_EINVAL || rsk_conn_pick_host(&t, pk + 1, 1, &in, &out, 1) != RSK_EINVAL;
    bad |= rsk_conn_pick_build_host(&t, nullptr, nullptr, 1) != RSK_EINVAL || rsk_conn_pick_host(&t, nullptr, 1, &in, &out, 1) != RSK_EINVAL;
    bad |= rsk_conn_pick_host(&t, pk, 1, nullptr, &out, 1) != RSK_EINVAL || rsk_conn_pick_host(&t, pk, 1, &in, nullptr, 1) != RSK_EINVAL;
    rsk_conn_pick_out no_conn = {nullptr, &word, nullptr};
    bad |= rsk_conn_pick_host(&t, pk, 1, &in, &no_conn, 1) != RSK_EINVAL;
    bad |= rsk_conn_pick_bytes(0, 0) != 0 || rsk_conn_pick_bytes(1, 2) != 0 || rsk_conn_pick_bytes(RSK_CONN_MAX_ROWS + 1u, 0) != 0;
    printf("%s: %d runs\n", bad ? "FAILED" : "ok", runs);
    return bad;
}
