// Stand-alone check of rsk_conn_close_host (rsock_amd/csrc/rsk_host.cpp), the host twin of
// rsk_conn_close_batch, for a sanitizer build of the host code alone -- no HIP, no Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/conn_close_host_check.cpp rsock_amd/csrc/rsk_host.cpp -lpthread -o conn_close_host_check
// A few hundred generated tables, each closed several times in a row on one pick index: client and BY_ID tables
// of 1 .. 3000 rows that are empty, sparse or full, few or many groups, duplicate keys, an IdBuf column at an odd
// address; the list form with repeats, rows >= capacity, rows that are not LIVE, *n_close above and below m_max
// and 0; the column form; no marks with SWEEP; every flag combination; with and without a pick index and lists.
// Every column, the work buffer and both indexes are heap blocks of exactly their bytes, so an access one element
// outside is reported.  Each call is compared with a std::map / std::set walk: state and every list, the lookup
// of every row's key on the conn index as the close left it, and the pick of every group at every candidate
// number, with and without an avoided conn, on the pick index as the close left it.  Exit status 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "rsk_codec.h"

static uint64_t rng_state = 0xC0221C105Eull;
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
static void *aligned(size_t bytes, int fill) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, bytes)) abort();
    std::memset(p, fill, bytes);
    return p;
}

typedef std::pair<uint64_t, uint64_t> Key;  // (IdBuf word, connKey); the word 0 without BY_ID
static const uint32_t kSent = 0x6E6E6E6Eu, kNoRst = 0xFFFFFFFFu;
static const uint8_t kUp = RSK_CONN_LIVE | RSK_CONN_ALIVE;

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf(" (cap %u by_id %d call %d)\n", cap, (int)by_id, call); return 1; } while (0)

// fill: 0 empty, 1 mixed, 2 every row LIVE | ALIVE.  groups: how many IdBuf words the rows spread over.
static int run(uint32_t cap, bool by_id, int fill, uint32_t groups, bool with_pick) {
    int call = -1;
    std::vector<uint8_t> state(cap), id(8ull * cap);
    std::vector<uint64_t> key(cap), idw(cap);
    const uint64_t k0 = rnd64(), i0 = rnd64();
    for (uint32_t r = 0; r < cap; ++r) {
        const uint32_t v = rnd() % 8;
        state[r] = fill == 0 ? (uint8_t)(rnd() % 2 ? RSK_CONN_ALIVE : 0x80u)
                 : fill == 2 ? kUp : (uint8_t)((v < 5 ? kUp : v == 5 ? RSK_CONN_LIVE : v == 6 ? RSK_CONN_ALIVE : 0u) |
                                               (rnd() % 4 ? 0u : RSK_CONN_NEW) | (rnd() % 8 ? 0u : 0x80u));
        key[r] = rnd() % 8 ? rnd64() | 1u : k0 ^ (1ull << rnd() % 64);  // some duplicate keys among the rows
        idw[r] = i0 + 0x9E3779B97F4A7C15ull * (rnd() % groups);
        std::memcpy(&id[8ull * r], &idw[r], 8);
    }
    rsk_conn_table t;
    std::memset(&t, 0, sizeof t);
    t.capacity = cap;
    t.flags = by_id ? RSK_CONN_BY_ID : 0u;
    const size_t shift = rnd() % 2 ? 3 : 0;  // the table's IdBuf column at an odd address
    uint8_t *e_state = exact(state), *e_id = exact(id, shift);
    uint64_t *e_key = exact(key);
    t.state = e_state;
    t.conn_key = e_key;
    t.id = by_id ? e_id : nullptr;
    const uint64_t ibytes = rsk_conn_index_bytes(cap, t.flags), pbytes = rsk_conn_pick_bytes(cap, t.flags);
    const uint64_t wbytes = rsk_conn_close_bytes(cap, t.flags);
    t.index = (uint32_t *)aligned((size_t)ibytes, 0x5A);
    uint32_t *pick = (uint32_t *)aligned((size_t)pbytes, 0x5A);
    void *work = aligned((size_t)wbytes, 0xA5);
    uint32_t counts[2];
    if (rsk_conn_index_build_host(&t, nullptr, 1) != RSK_OK || rsk_conn_pick_build_host(&t, pick, counts, 1) != RSK_OK)
        FAIL("build failed");
    rsk_conn_rows rows = {e_state};

    int bad = 0;
    for (call = 0; call < 4 && !bad; ++call) {
        const int form = (int)(rnd() % 3);  // 0 list, 1 column, 2 none (SWEEP alone)
        uint32_t flags = rnd() % 4;
        if (form == 2) flags |= RSK_CONN_CLOSE_SWEEP;
        const bool remove = flags & RSK_CONN_CLOSE_REMOVE, sweep = flags & RSK_CONN_CLOSE_SWEEP;
        std::vector<uint32_t> lst, rst(cap, kNoRst);
        uint32_t n_close = 0, m_max = 0;
        std::vector<uint8_t> mark(cap, 0);
        if (form == 0) {
            const uint32_t m = rnd() % (2 * cap + 6);
            for (uint32_t j = 0; j < m; ++j) {
                const uint32_t v = rnd() % 16;
                lst.push_back(v == 0 ? cap : v == 1 ? cap + 1 : v == 2 ? 0x80000000u : v == 3 ? 0xFFFFFFFFu : rnd() % cap);
            }
            m_max = rnd() % 4 ? m : rnd() % (m + 1);
            n_close = rnd() % 4 == 0 ? 0u : rnd() % 2 ? m + rnd() % 100 : rnd() % (m + 1);
            for (uint32_t j = 0; j < (n_close < m_max ? n_close : m_max); ++j)
                if (lst[j] < cap) mark[lst[j]] = 1;
        } else if (form == 1) {
            const uint32_t dens = rnd() % 5;
            for (uint32_t r = 0; r < cap; ++r)
                if (dens == 4 || (dens && rnd() % (1u << (2 * dens)) == 0)) { rst[r] = rnd() % 3 ? rnd() : 0u; mark[r] = 1; }
        }
        // the walk: the rows in order
        std::vector<uint8_t> want(cap);
        std::vector<uint32_t> want_marked, want_closed;
        for (uint32_t r = 0; r < cap; ++r) {
            uint8_t st = e_state[r];
            if (st & RSK_CONN_LIVE) {
                if (mark[r] && (st & RSK_CONN_ALIVE)) want_marked.push_back(r);
                if (mark[r]) st &= (uint8_t)~RSK_CONN_ALIVE;
                if ((remove && mark[r]) || (sweep && !(st & RSK_CONN_ALIVE))) {
                    st &= (uint8_t)~(RSK_CONN_LIVE | RSK_CONN_ALIVE | RSK_CONN_NEW);
                    want_closed.push_back(r);
                }
            }
            want[r] = st;
        }
        uint32_t *e_lst = exact(lst), *e_rst = exact(rst), *e_ncl = exact(std::vector<uint32_t>{n_close});
        const bool lists = rnd() % 4 != 0;
        uint32_t *o_marked = exact(std::vector<uint32_t>(cap, kSent)), *o_closed = exact(std::vector<uint32_t>(cap, kSent));
        uint32_t n_marked = kSent, n_closed = kSent, pc[2] = {kSent, kSent};
        uint32_t *index0 = (uint32_t *)aligned((size_t)ibytes, 0), *pick0 = (uint32_t *)aligned((size_t)pbytes, 0);
        std::memcpy(index0, t.index, (size_t)ibytes);
        std::memcpy(pick0, pick, (size_t)pbytes);
        rsk_conn_close_in in = {form == 0 ? e_lst : nullptr, form == 0 ? e_ncl : nullptr, m_max,
                                form == 1 ? e_rst : nullptr, work, flags};
        rsk_conn_close_out out = {lists ? o_marked : nullptr, &n_marked, lists ? o_closed : nullptr, &n_closed,
                                  with_pick ? pick : nullptr, with_pick ? pc : nullptr};
        if (rsk_conn_close_host(&t, &rows, &in, &out, 1) != RSK_OK) FAIL("close failed");
        if (n_marked != want_marked.size() || n_closed != want_closed.size()) FAIL("counts %u %u", n_marked, n_closed);
        for (uint32_t j = 0; lists && j < cap; ++j) {
            if (o_marked[j] != (j < n_marked ? want_marked[j] : kSent)) FAIL("marked_rows[%u]", j);
            if (o_closed[j] != (j < n_closed ? want_closed[j] : kSent)) FAIL("closed_rows[%u]", j);
        }
        if (std::memcmp(e_state, want.data(), cap)) FAIL("state");
        if (std::memcmp(e_key, key.data(), 8ull * cap) || std::memcmp(e_id, id.data(), 8ull * cap)) FAIL("a key column changed");
        if (!n_closed && std::memcmp(index0, t.index, (size_t)ibytes)) FAIL("index written though nothing was removed");
        if (!n_closed && !n_marked && std::memcmp(pick0, pick, (size_t)pbytes)) FAIL("pick written though nothing changed");
        // lookups: every row's key, and a few absent ones, on the index as the close left it
        std::map<Key, uint32_t> lowest;
        std::map<uint64_t, std::vector<uint32_t>> cand;
        for (uint32_t r = 0; r < cap; ++r) {
            const uint64_t w = by_id ? idw[r] : 0ull;
            if (e_state[r] & RSK_CONN_LIVE) lowest.insert({Key(w, key[r]), r});
            if ((e_state[r] & kUp) == kUp) cand[w].push_back(r);
        }
        {
            std::vector<int8_t> st(cap + 4, (int8_t)RSK_RECV_VALID);
            std::vector<uint64_t> qk(key);
            std::vector<uint8_t> qi(id);
            for (int j = 0; j < 4; ++j) {
                qk.push_back(rnd64() & ~1ull);
                qi.insert(qi.end(), id.begin(), id.begin() + 8);
            }
            std::vector<uint32_t> conn(cap + 4, kSent);
            int8_t *e_st = exact(st);
            uint64_t *e_qk = exact(qk);
            uint8_t *e_qi = exact(qi);
            uint32_t *e_conn = exact(conn);
            rsk_conn_resolve_in rin = {e_st, nullptr, by_id ? e_qi : nullptr, e_qk};
            rsk_conn_resolve_out rout = {e_conn, nullptr, nullptr, nullptr};
            if (rsk_conn_resolve_host(&t, cap + 4, &rin, &rout, 1) != RSK_OK) FAIL("resolve failed");
            for (uint32_t j = 0; j < cap + 4; ++j) {
                uint64_t w = 0;
                if (by_id) std::memcpy(&w, &qi[8ull * j], 8);
                auto it = lowest.find(Key(w, qk[j]));
                if (e_conn[j] != (it == lowest.end() ? RSK_CONN_NONE : it->second)) FAIL("lookup %u", j);
            }
            free(e_st); free(e_qk); free(e_qi); free(e_conn);
        }
        // picks: every group (and the ids that lost theirs) at every candidate number, plain and with an avoid key
        if (with_pick) {
            uint32_t total = 0, ngroups = 0;
            for (auto &g : cand) { total += (uint32_t)g.second.size(); ++ngroups; }
            if (pc[0] != ngroups || pc[1] != total || pick[0] != total || pick[1] != ngroups) FAIL("pick counts");
            std::set<uint64_t> ids;
            for (uint32_t r = 0; r < cap; ++r) ids.insert(by_id ? idw[r] : 0ull);
            if (by_id) ids.insert(i0 ^ 0x5555ull);  // an id no row has
            std::vector<uint8_t> qi;
            std::vector<uint64_t> av;
            std::vector<uint32_t> dr, wantc;
            for (uint64_t w : ids) {
                const std::vector<uint32_t> *g = cand.count(w) ? &cand[w] : nullptr;
                const uint32_t m = g ? (uint32_t)g->size() : 0u;
                for (uint32_t d = 0; d < (m < 40 ? m + 2 : 42); ++d) {
                    for (int mode = 0; mode < 2; ++mode) {
                        uint64_t a = 0;
                        uint32_t p = 0xFFFFFFFFu;
                        if (mode && m) {  // avoid a candidate that the index names for its key
                            const uint32_t ar = (*g)[rnd() % m];
                            a = key[ar];
                            auto it = lowest.find(Key(w, a));
                            for (uint32_t q = 0; q < m; ++q)
                                if ((*g)[q] == it->second) p = q;
                            if (a == 0) p = 0xFFFFFFFFu;
                        }
                        uint32_t row = RSK_CONN_NONE;
                        if (m && p == 0xFFFFFFFFu) row = (*g)[d % m];
                        else if (m > 1) { uint32_t k = d % (m - 1); k += k >= p; row = (*g)[k]; }
                        uint8_t b[8];
                        std::memcpy(b, &w, 8);
                        qi.insert(qi.end(), b, b + 8);
                        av.push_back(a);
                        dr.push_back(d);
                        wantc.push_back(row);
                    }
                }
            }
            const uint32_t n = (uint32_t)dr.size();
            std::vector<uint32_t> conn(n, kSent);
            uint8_t *e_qi = exact(qi);
            uint64_t *e_av = exact(av);
            uint32_t *e_dr = exact(dr), *e_conn = exact(conn);
            rsk_conn_pick_in pin = {nullptr, by_id ? e_qi : nullptr, e_av, e_dr, 0};
            rsk_conn_pick_out pout = {e_conn, nullptr, nullptr};
            if (rsk_conn_pick_host(&t, pick, n, &pin, &pout, 1) != RSK_OK) FAIL("pick failed");
            for (uint32_t j = 0; j < n; ++j)
                if (e_conn[j] != wantc[j]) FAIL("pick %u: %u, want %u", j, e_conn[j], wantc[j]);
            free(e_qi); free(e_av); free(e_dr); free(e_conn);
        }
        free(e_lst); free(e_rst); free(e_ncl); free(o_marked); free(o_closed); free(index0); free(pick0);
        // now and then the host revives rows and rebuilds both indexes, and the closes go on
        if (rnd() % 3 == 0) {
            for (uint32_t r = 0; r < cap; ++r)
                if (rnd() % 4 == 0) e_state[r] |= kUp;
            if (rsk_conn_index_build_host(&t, nullptr, 1) != RSK_OK || rsk_conn_pick_build_host(&t, pick, counts, 1) != RSK_OK)
                FAIL("rebuild failed");
        }
    }
    free(e_state); free(e_id - shift); free(e_key); free(t.index); free(pick); free(work);
    return bad;
}

int main() {
    const uint32_t caps[] = {1, 2, 3, 15, 16, 17, 257, 1023, 1024, 1025, 2049, 3000};
    int bad = 0, runs = 0;
    for (uint32_t cap : caps)
        for (int by_id = 0; by_id < 2; ++by_id)
            for (int fill = 0; fill < 3; ++fill)
                for (uint32_t groups : {1u, 3u, cap < 64 ? cap : 64u, cap})
                    for (int with_pick = 0; with_pick < 2; ++with_pick) {
                        if (!by_id && groups != 1u) continue;
                        if (cap > 1100 && groups == cap && fill != 1) continue;
                        bad += run(cap, by_id != 0, fill, groups ? groups : 1u, with_pick != 0);
                        ++runs;
                    }
    std::printf("conn_close_host_check: %d tables, %d failed\n", runs, bad);
    return bad ? 1 : 0;
}
