// Stand-alone check of the tuple pool's host twins (rsock_amd/csrc/rsk_host.cpp: rsk_pool_index_build_host,
// rsk_pool_add_host, rsk_pool_offers_host, rsk_pool_settle_host, rsk_pool_flush_host) for a sanitizer build of the
// host code alone -- no HIP, no Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/pool_host_check.cpp rsock_amd/csrc/rsk_host.cpp -lpthread -o pool_host_check
// A few hundred generated servers, each an ack pool and a socket pool of 1 .. 3000 rows that take rounds of harvest
// (parse_status, zero ports, repeated handshakes, u_max below the rows), accept (list form), offers (m_max above and
// below the matches, with and without conn_key and the row lists), settle (some offers taken, missing packets of
// every kind, new_max 0) and flush.  Every column, work buffer, output list and index is a heap block of exactly its
// bytes, so an access one element outside is reported.  Each call is compared with a walk over two std::maps keyed
// as TcpCmpFn keys the reference's (src, sp, dst, dp), written from TcpAckPool::AddInfoFromPeer / Wait2TransferInfo /
// OnFlush (net/TcpAckPool.cpp) and ServerNetManager::add2Pool / GetTcp / OnFlush (server/ServerNetManager.cpp): the
// counts, the lists, the LIVE rows of both pools as maps, and the lookup of every LIVE tuple on the index as the call
// left it.  A last pass runs the calls on indexes filled with garbage: whatever comes out, nothing outside the
// buffers may be touched.  Exit status 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "rsk_codec.h"

static uint64_t rng_state = 0x9001C0FFEEull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

template <typename T>
static T *block(size_t n, uint32_t fill = 0x6E6E6E6Eu) {  // exactly n elements (one byte for none)
    T *p = (T *)malloc(n ? n * sizeof(T) : 1);
    for (size_t i = 0; i < n; ++i) p[i] = (T)fill;
    return p;
}
static void *aligned(size_t bytes, int fill) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 16)) abort();
    std::memset(p, fill, bytes);
    return p;
}

typedef std::tuple<uint32_t, uint16_t, uint32_t, uint16_t> Tup;  // src, sp, dst, dp: TcpCmpFn's order
struct Rec { uint32_t seq, ack; uint64_t expiry; };
typedef std::map<Tup, Rec> Model;
static const uint32_t kSent = 0x6E6E6E6Eu;

struct Pool {
    rsk_pool p;
    uint32_t cap;
    bool vals;
    void make(uint32_t capacity, bool with_vals, bool garbage) {
        cap = capacity; vals = with_vals;
        std::memset(&p, 0, sizeof p);
        p.capacity = cap;
        p.state = block<uint8_t>(cap); p.src = block<uint32_t>(cap); p.dst = block<uint32_t>(cap);
        p.sp = block<uint16_t>(cap); p.dp = block<uint16_t>(cap);
        p.seq = vals ? block<uint32_t>(cap) : nullptr; p.ack = vals ? block<uint32_t>(cap) : nullptr;
        p.expiry = block<uint64_t>(cap);
        for (uint32_t r = 0; r < cap; ++r) {
            p.state[r] = (uint8_t)(rnd() & 0xFE);  // no LIVE row, every other bit random
            p.src[r] = rnd(); p.dst[r] = rnd(); p.sp[r] = (uint16_t)rnd(); p.dp[r] = (uint16_t)rnd(); p.expiry[r] = rnd();
        }
        const uint64_t ib = rsk_conn_index_bytes(cap, RSK_CONN_BY_ID);
        p.index = (uint32_t *)aligned((size_t)ib, 0x5A);
        if (garbage) for (uint64_t q = 0; q < ib / 4; ++q) p.index[q] = rnd() % 3 ? rnd() % (2 * cap + 2) : rnd();
    }
    void release() {
        free(p.state); free(p.src); free(p.dst); free(p.sp); free(p.dp); free(p.seq); free(p.ack); free(p.expiry); free(p.index);
    }
    Model live() const {
        Model m;
        for (uint32_t r = 0; r < cap; ++r)
            if (p.state[r] & RSK_POOL_LIVE)
                m.emplace(Tup(p.src[r], p.sp[r], p.dst[r], p.dp[r]), Rec{vals ? p.seq[r] : 0u, vals ? p.ack[r] : 0u, p.expiry[r]});
        return m;
    }
    uint32_t n_live() const {
        uint32_t k = 0;
        for (uint32_t r = 0; r < cap; ++r) k += p.state[r] & RSK_POOL_LIVE;
        return k;
    }
};

static bool same(const Model &a, const Model &b, bool vals) {
    if (a.size() != b.size()) return false;
    for (auto ia = a.begin(), ib = b.begin(); ia != a.end(); ++ia, ++ib) {
        if (ia->first != ib->first || ia->second.expiry != ib->second.expiry) return false;
        if (vals && (ia->second.seq != ib->second.seq || ia->second.ack != ib->second.ack)) return false;
    }
    return true;
}

struct Rows {  // tuple columns of exactly n rows
    uint32_t n;
    uint32_t *src, *dst, *seq, *ack;
    uint16_t *sp, *dp;
    explicit Rows(uint32_t k) : n(k) {
        src = block<uint32_t>(k); dst = block<uint32_t>(k); seq = block<uint32_t>(k); ack = block<uint32_t>(k);
        sp = block<uint16_t>(k); dp = block<uint16_t>(k);
    }
    ~Rows() { free(src); free(dst); free(seq); free(ack); free(sp); free(dp); }
    void set(uint32_t i, const Tup &t) { src[i] = std::get<0>(t); sp[i] = std::get<1>(t); dst[i] = std::get<2>(t); dp[i] = std::get<3>(t); }
    Tup at(uint32_t i) const { return Tup(src[i], sp[i], dst[i], dp[i]); }
};

// a tuple of a small universe, so that handshakes, sockets and packets meet
static Tup some_tuple(uint32_t universe) {
    const uint32_t k = rnd() % universe;
    return Tup(0x0A000000u + k, (uint16_t)(1024 + k % 50000), 0xC0A80001u + k / 50000, (uint16_t)443);
}

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf(" (cap %u / %u round %d garbage %d)\n", cap_a, cap_s, round, (int)garbage); return 1; } while (0)

// Every LIVE tuple resolves to its row on the index as the last call left it: an add without TOUCH of exactly the
// LIVE tuples adds nothing, moves nothing and names each tuple's row.
static bool lookups_ok(Pool &pl) {
    const uint32_t k = pl.n_live();
    if (!k) return true;
    Rows in(k);
    std::vector<uint32_t> want;
    for (uint32_t r = 0, j = 0; r < pl.cap; ++r)
        if (pl.p.state[r] & RSK_POOL_LIVE) { in.set(j++, Tup(pl.p.src[r], pl.p.sp[r], pl.p.dst[r], pl.p.dp[r])); want.push_back(r); }
    uint32_t *row = block<uint32_t>(k), cnt[3];
    void *work = aligned((size_t)rsk_pool_add_bytes(k, pl.cap), 0x33);
    rsk_pool_add_in ai = {in.src, in.dst, in.sp, in.dp, in.seq, in.ack, nullptr, 1, k, 0, work};
    rsk_pool_add_out ao = {row, nullptr, nullptr, &cnt[0], &cnt[1], &cnt[2], nullptr};
    const Model before = pl.live();
    bool ok = rsk_pool_add_host(&pl.p, k, &ai, &ao, 1) == RSK_OK && cnt[0] == 0 && cnt[1] == k && cnt[2] == 0;
    for (uint32_t j = 0; ok && j < k; ++j) ok = row[j] == want[j];
    ok = ok && same(before, pl.live(), pl.vals);
    free(row); free(work);
    return ok;
}

static int run(uint32_t cap_a, uint32_t cap_s, uint32_t universe, bool garbage) {
    int round = -1;
    Pool pa, ps;
    pa.make(cap_a, true, garbage);
    ps.make(cap_s, false, garbage);
    if (!garbage && (rsk_pool_index_build_host(&pa.p, nullptr, 1) != RSK_OK || rsk_pool_index_build_host(&ps.p, nullptr, 1) != RSK_OK))
        FAIL("build failed");
    Model ma, ms;
    uint64_t now = 1000;
    void *swork = aligned((size_t)rsk_pool_settle_bytes(cap_a, cap_s), 0x77);
    for (round = 0; round < 5; ++round, now += 400) {
        // ---- harvest: AddInfoFromPeer per SYN row with both ports, the first u_max of them
        {
            const uint32_t n = rnd() % (cap_a + cap_a / 2 + 3);
            Rows in(n);
            int8_t *status = block<int8_t>(n);
            uint32_t considered = 0;
            for (uint32_t i = 0; i < n; ++i) {
                in.set(i, some_tuple(universe));
                in.seq[i] = rnd(); in.ack[i] = rnd();
                if (rnd() % 16 == 0) in.sp[i] = 0;
                if (rnd() % 16 == 0) in.dp[i] = 0;
                status[i] = (int8_t)(rnd() % 8 ? RSK_PARSE_SYN : rnd() % 4);
                considered += status[i] == RSK_PARSE_SYN && in.sp[i] && in.dp[i];
            }
            const uint32_t u_max = rnd() % 4 == 0 && considered > 1 ? considered / 2 : (n ? n : 1);
            const uint32_t m = u_max < cap_a ? u_max : cap_a;
            uint32_t *row = block<uint32_t>(n), *new_rows = block<uint32_t>(m), *new_first = block<uint32_t>(m), cnt[4];
            void *work = aligned((size_t)rsk_pool_add_bytes(u_max, cap_a), 0x33);
            rsk_pool_add_in ai = {in.src, in.dst, in.sp, in.dp, in.seq, in.ack, status, now + 1000, u_max, RSK_POOL_TOUCH, work};
            rsk_pool_add_out ao = {row, new_rows, new_first, &cnt[0], &cnt[1], &cnt[2], &cnt[3]};
            const uint32_t vacant = cap_a - pa.n_live();
            if (rsk_pool_add_host(&pa.p, n, &ai, &ao, 1) != RSK_OK) FAIL("harvest failed");
            if (!garbage) {
                uint32_t taken = 0, w_new = 0, w_again = 0, w_zero = 0;
                std::set<Tup> refused;
                for (uint32_t i = 0; i < n; ++i) {
                    if (status[i] != RSK_PARSE_SYN) continue;
                    if (!in.sp[i] || !in.dp[i]) { ++w_zero; continue; }
                    if (taken == u_max) continue;
                    ++taken;
                    auto it = ma.find(in.at(i));
                    if (it != ma.end()) { it->second.expiry = now + 1000; ++w_again; continue; }  // mInfoPool[info] = expiry
                    if (w_new == vacant) { if (!refused.insert(in.at(i)).second) ++w_again; continue; }
                    ma.emplace(in.at(i), Rec{in.seq[i], in.ack[i], now + 1000});
                    if (new_first[w_new] != i) FAIL("harvest: new_first[%u] = %u, want %u", w_new, new_first[w_new], i);
                    ++w_new;
                }
                if (cnt[0] != w_new || cnt[1] != w_again || cnt[2] != refused.size() || cnt[3] != w_zero)
                    FAIL("harvest counts %u %u %u %u, want %u %u %zu %u", cnt[0], cnt[1], cnt[2], cnt[3], w_new, w_again, refused.size(), w_zero);
                for (uint32_t j = 0; j < w_new; ++j)
                    if (new_rows[j] >= cap_a || Tup(pa.p.src[new_rows[j]], pa.p.sp[new_rows[j]], pa.p.dst[new_rows[j]], pa.p.dp[new_rows[j]]) != in.at(new_first[j]))
                        FAIL("harvest: new_rows[%u]", j);
                for (uint32_t j = w_new; j < m; ++j)
                    if (new_rows[j] != kSent || new_first[j] != kSent) FAIL("harvest: written behind the lists' end");
                for (uint32_t i = 0; i < n; ++i) {
                    const bool cons = status[i] == RSK_PARSE_SYN && in.sp[i] && in.dp[i];
                    const bool have = cons && ma.count(in.at(i));
                    if (have != (row[i] != RSK_CONN_NONE) || (have && (row[i] >= cap_a || !(pa.p.state[row[i]] & RSK_POOL_LIVE))))
                        FAIL("harvest: row[%u]", i);
                }
                if (!same(ma, pa.live(), true)) FAIL("harvest: the ack pool differs");
                if (!lookups_ok(pa)) FAIL("harvest: a LIVE tuple does not resolve");
            }
            free(row); free(new_rows); free(new_first); free(status); free(work);
        }
        // ---- accept: add2Pool's emplace per tuple (list form)
        {
            const uint32_t n = rnd() % (cap_s + 3);
            Rows in(n);
            for (uint32_t i = 0; i < n; ++i) in.set(i, some_tuple(universe));
            const uint32_t u_max = n ? n : 1;
            uint32_t cnt[4];
            void *work = aligned((size_t)rsk_pool_add_bytes(u_max, cap_s), 0x33);
            rsk_pool_add_in ai = {in.src, in.dst, in.sp, in.dp, nullptr, nullptr, nullptr, now + 1000, u_max, 0, work};
            rsk_pool_add_out ao = {nullptr, nullptr, nullptr, &cnt[0], &cnt[1], &cnt[2], &cnt[3]};
            const uint32_t vacant = cap_s - ps.n_live();
            if (rsk_pool_add_host(&ps.p, n, &ai, &ao, 1) != RSK_OK) FAIL("accept failed");
            if (!garbage) {
                uint32_t w_new = 0;
                for (uint32_t i = 0; i < n; ++i)
                    if (!ms.count(in.at(i)) && w_new < vacant) { ms.emplace(in.at(i), Rec{0, 0, now + 1000}); ++w_new; }
                if (cnt[0] != w_new || cnt[3] != 0) FAIL("accept counts %u, want %u", cnt[0], w_new);
                if (!same(ms, ps.live(), false)) FAIL("accept: the socket pool differs");
                if (!lookups_ok(ps)) FAIL("accept: a LIVE tuple does not resolve");
            }
            free(work);
        }
        // ---- offers: the tuples both maps hold, with the record's ack and TH_ACK
        uint32_t matches = 0;
        for (auto &kv : ma) matches += (uint32_t)ms.count(kv.first);
        const uint32_t m_max = rnd() % 3 == 0 && matches > 1 ? matches / 2 : matches + 1 + rnd() % 3;
        const bool lists = garbage || rnd() % 4 != 0;
        uint32_t *o_src = block<uint32_t>(m_max), *o_dst = block<uint32_t>(m_max), *o_ack = block<uint32_t>(m_max);
        uint16_t *o_sp = block<uint16_t>(m_max), *o_dp = block<uint16_t>(m_max);
        uint8_t *o_flag = block<uint8_t>(m_max);
        uint64_t *o_key = rnd() % 2 ? (uint64_t *)aligned(8ull * m_max, 0x6E) : nullptr;
        uint32_t *o_ar = block<uint32_t>(m_max), *o_sr = block<uint32_t>(m_max), n_offer = kSent, n_over = kSent;
        {
            rsk_pool_offers_out oo = {o_src, o_dst, o_sp, o_dp, o_ack, o_flag, o_key, &n_offer, lists ? o_ar : nullptr,
                                      lists ? o_sr : nullptr, &n_over, m_max};
            if (rsk_pool_offers_host(&pa.p, &ps.p, &oo, 1) != RSK_OK) FAIL("offers failed");
            if (n_offer > m_max) FAIL("offers: n_offer %u above m_max %u", n_offer, m_max);
            if (!garbage) {
                if (n_offer != (matches < m_max ? matches : m_max) || n_over != matches - n_offer)
                    FAIL("offers: %u + %u, want %u of %u", n_offer, n_over, m_max, matches);
                for (uint32_t o = 0; o < n_offer; ++o) {
                    const Tup t(o_src[o], o_sp[o], o_dst[o], o_dp[o]);
                    auto it = ma.find(t);
                    if (it == ma.end() || !ms.count(t) || o_ack[o] != it->second.ack || o_flag[o] != RSK_TH_ACK) FAIL("offers: offer %u", o);
                    if (o_key && o_key[o] != rsk_key_for_tcp(o_sp[o], o_dp[o])) FAIL("offers: conn_key %u", o);
                    if (lists && (o_ar[o] >= cap_a || o_sr[o] >= cap_s || (o && o_ar[o] <= o_ar[o - 1]))) FAIL("offers: rows of offer %u", o);
                }
                for (uint32_t o = n_offer; o < m_max; ++o)
                    if (o_src[o] != kSent || o_ack[o] != kSent || o_flag[o] != (uint8_t)kSent || o_ar[o] != kSent) FAIL("offers: written behind the list's end");
            }
        }
        // ---- settle: some offers became conns; the packets still missing empty what one pool alone holds
        {
            const uint32_t new_max = lists && rnd() % 4 ? n_offer : 0;
            uint32_t *new_offer = block<uint32_t>(new_max), n_new = 0;
            for (uint32_t o = 0; o < new_max; ++o)
                if (rnd() % 2) new_offer[n_new++] = o;
            if (garbage && new_max) { new_offer[0] = rnd(); n_new = new_max + rnd() % 3; }
            const uint32_t n = rnd() % (cap_a + 3);
            Rows pk(n);
            int8_t *miss = block<int8_t>(n);
            for (uint32_t i = 0; i < n; ++i) { pk.set(i, some_tuple(universe)); miss[i] = (int8_t)(rnd() % 2 ? RSK_RECV_VALID : RSK_RECV_DROP); }
            uint32_t *taken = block<uint32_t>(new_max), *closed = block<uint32_t>(cap_s), cnt[2];
            rsk_pool_settle_in si = {new_max ? new_offer : nullptr, new_max ? &n_new : nullptr, o_ar, o_sr, new_max, m_max, miss,
                                     pk.src, pk.dst, pk.sp, pk.dp, swork};
            rsk_pool_settle_out so = {taken, closed, &cnt[0], &cnt[1]};
            if (rsk_pool_settle_host(&pa.p, &ps.p, n, &si, &so, 1) != RSK_OK) FAIL("settle failed");
            if (!garbage) {
                for (uint32_t j = 0; j < n_new; ++j) {  // Wait2TransferInfo erases the record, GetTcp the socket
                    const uint32_t o = new_offer[j];
                    const Tup t(o_src[o], o_sp[o], o_dst[o], o_dp[o]);
                    ma.erase(t); ms.erase(t);
                    if (taken[j] != o_sr[o]) FAIL("settle: taken_sock_rows[%u]", j);
                }
                uint32_t w_closed = 0, w_purged = 0;
                for (uint32_t i = 0; i < n; ++i) {
                    if (miss[i] != RSK_RECV_VALID) continue;
                    const Tup t = pk.at(i);
                    if (ma.count(t) && ms.count(t)) continue;  // a whole offer this call did not consume
                    w_purged += (uint32_t)ma.erase(t);         // RemoveInfo
                    w_closed += (uint32_t)ms.erase(t);         // GetTcp: erase, then closeTcp
                }
                if (cnt[0] != w_closed || cnt[1] != w_purged) FAIL("settle counts %u %u, want %u %u", cnt[0], cnt[1], w_closed, w_purged);
                for (uint32_t j = 0; j < cap_s; ++j)
                    if (j < w_closed ? (closed[j] >= cap_s || (j && closed[j] <= closed[j - 1])) : closed[j] != kSent) FAIL("settle: closed_sock_rows[%u]", j);
                for (uint32_t j = n_new; j < new_max; ++j)
                    if (taken[j] != kSent) FAIL("settle: written behind taken_sock_rows' end");
                if (!same(ma, pa.live(), true) || !same(ms, ps.live(), false)) FAIL("settle: a pool differs");
                if (!lookups_ok(pa) || !lookups_ok(ps)) FAIL("settle: a LIVE tuple does not resolve");
            }
            free(new_offer); free(miss); free(taken); free(closed);
        }
        free(o_src); free(o_dst); free(o_ack); free(o_sp); free(o_dp); free(o_flag); free(o_key); free(o_ar); free(o_sr);
        // ---- flush: expiry <= now, in both
        for (int which = 0; which < 2; ++which) {
            Pool &pl = which ? ps : pa;
            Model &m = which ? ms : ma;
            uint32_t *dead = block<uint32_t>(pl.cap), n_dead = kSent;
            rsk_pool_flush_out fo = {rnd() % 4 ? dead : nullptr, &n_dead};
            const uint64_t at = now + (rnd() % 2 ? 1000 : 600);  // the expiry of this round's entries, or between two rounds'
            if (rsk_pool_flush_host(&pl.p, at, &fo, 1) != RSK_OK) FAIL("flush failed");
            if (!garbage) {
                uint32_t w = 0;
                for (auto it = m.begin(); it != m.end();)
                    if (it->second.expiry <= at) { it = m.erase(it); ++w; } else ++it;
                if (n_dead != w) FAIL("flush %d: n_dead %u, want %u", which, n_dead, w);
                for (uint32_t j = 0; fo.dead_rows && j < pl.cap; ++j)
                    if (j < w ? (dead[j] >= pl.cap || (j && dead[j] <= dead[j - 1])) : dead[j] != kSent) FAIL("flush %d: dead_rows[%u]", which, j);
                if (!same(m, pl.live(), pl.vals)) FAIL("flush %d: the pool differs", which);
                if (!lookups_ok(pl)) FAIL("flush %d: a LIVE tuple does not resolve", which);
            }
            free(dead);
        }
    }
    free(swork);
    pa.release();
    ps.release();
    return 0;
}

int main() {
    static const uint32_t caps[] = {1, 2, 3, 5, 64, 67, 255, 1025, 3000};
    int runs = 0;
    for (int garbage = 0; garbage < 2; ++garbage)
        for (uint32_t ca : caps)
            for (uint32_t cs : caps) {
                if (ca > 300 && cs > 300 && ca != cs) continue;
                for (int rep = 0; rep < (ca * cs < 10000 ? 4 : 1); ++rep, ++runs) {
                    const uint32_t big = ca > cs ? ca : cs;
                    const uint32_t universe = rep % 2 ? big + big / 2 + 2 : big / 2 + 2;  // the pools fill up, or never do
                    if (run(ca, cs, universe, garbage != 0)) return 1;
                }
            }
    std::printf("pool_host_check: %d servers, all equal\n", runs);
    return 0;
}
