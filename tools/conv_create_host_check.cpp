// Stand-alone check of rsk_conv_create_host (rsock_amd/csrc/rsk_host.cpp), the host twin of
// rsk_conv_create_batch, for a sanitizer build of the host code alone -- no HIP, no Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/conv_create_host_check.cpp rsock_amd/csrc/rsk_host.cpp -lpthread -o conv_create_host_check
// A few hundred generated tables and batches per run: every flag combination, tables of 1 .. 3000 rows that
// are empty, sparse or full (no vacant row), u_max of 1, below and above the unknown packets, one key for all
// packets, every packet another key, keys that differ in one bit of dst / conv / IdBuf, an IdBuf column at an
// odd address.  Every column, the work buffer and the index is a heap block of exactly its bytes, so an access
// one element outside is reported.  Each case resolves, creates (again while the header says to), and
// compares with a std::map walk; then every key of the table is looked up on the index as the create left it.
// Exit status 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "rsk_codec.h"

static uint64_t rng_state = 0xC0117C4EA7Eull;
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

typedef std::tuple<uint64_t, uint32_t, uint32_t> Key;  // (IdBuf word, dst, conv); unused parts 0

// fill: 0 empty, 1 about half LIVE, 2 every row LIVE.  keys: 0 = every packet another key, else the number of
// distinct new keys the packets draw from.
static int run(uint32_t cap, uint32_t flags, int fill, uint32_t n, uint32_t keys, uint32_t u_max) {
    const bool by_dst = flags & RSK_CONV_BY_DST, by_id = flags & RSK_CONV_BY_ID;
    std::vector<uint8_t> state(cap), alive(cap), id(8ull * cap);
    std::vector<uint32_t> conv(cap), dst(cap), ci(cap), co(cap), pi(cap), po(cap);
    std::vector<uint64_t> idw(cap);
    const uint32_t c0 = rnd() | 1u, d0 = rnd();
    const uint64_t i0 = rnd64();
    for (uint32_t r = 0; r < cap; ++r) {
        const bool live = fill == 2 || (fill == 1 && rnd() % 2);
        state[r] = (uint8_t)((live ? RSK_CONN_LIVE : 0u) | (rnd() % 4 ? 0u : 0x82u));
        conv[r] = (rnd() % 3 ? c0 ^ (2u << rnd() % 31) : rnd()) | 1u;  // odd: the known keys
        dst[r] = rnd() % 2 ? d0 : d0 ^ (1u << rnd() % 32);
        idw[r] = rnd() % 2 ? i0 : i0 ^ (1ull << rnd() % 64);
        std::memcpy(&id[8ull * r], &idw[r], 8);
        alive[r] = (uint8_t)(rnd() % 3);
        ci[r] = rnd(); co[r] = rnd(); pi[r] = rnd(); po[r] = rnd();
    }
    auto row_key = [&](uint32_t r) { return Key(by_id ? idw[r] : 0ull, by_dst ? dst[r] : 0u, conv[r]); };

    rsk_conv_table t;
    std::memset(&t, 0, sizeof t);
    t.capacity = cap;
    t.flags = flags;
    const size_t shift = rnd() % 2 ? 3 : 0;  // the table's IdBuf column at an odd address
    uint8_t *e_state = exact(state), *e_alive = exact(alive), *e_id = exact(id, shift);
    uint32_t *e_conv = exact(conv), *e_dst = exact(dst), *e_ci = exact(ci), *e_co = exact(co), *e_pi = exact(pi), *e_po = exact(po);
    const bool counters = rnd() % 4 != 0;
    t.state = e_state; t.conv = e_conv; t.dst = by_dst ? e_dst : nullptr; t.id = by_id ? e_id : nullptr;
    if (counters) { t.cur_in = e_ci; t.cur_out = e_co; t.prev_in = e_pi; t.prev_out = e_po; t.alive = e_alive; }
    const uint64_t ibytes = rsk_conn_index_bytes(cap, 0);
    t.index = (uint32_t *)aligned((size_t)ibytes, 0x5A);
    int bad = rsk_conv_index_build_host(&t, nullptr, 1) != RSK_OK;
    rsk_conv_rows rows = {e_state, e_conv, by_dst ? e_dst : nullptr, by_id ? e_id : nullptr};

    // the batch: DATA packets for rows of the table (known) and for new keys (even conv), dropped ones between
    std::vector<int8_t> st(n);
    std::vector<uint8_t> pid(8ull * n);
    std::vector<uint32_t> pconv(n), pdst(n);
    std::vector<uint64_t> pidw(n);
    std::vector<Key> pool(keys);
    for (uint32_t k = 0; k < keys; ++k)  // neighbours differ in one bit of one part
        pool[k] = Key(k % 3 == 2 ? i0 ^ (1ull << k % 64) : i0, k % 3 == 1 ? d0 ^ (1u << k % 32) : d0, (k / 3u) << 1);
    for (uint32_t i = 0; i < n; ++i) {
        st[i] = (int8_t)(rnd() % 8 ? RSK_RECV_VALID : RSK_RECV_DROP);
        if (keys == 0) {
            pidw[i] = i0; pdst[i] = d0; pconv[i] = i << 1;
        } else if (cap && rnd() % 3 == 0) {
            const uint32_t r = rnd() % cap;
            pidw[i] = idw[r]; pdst[i] = dst[r]; pconv[i] = conv[r];
        } else {
            const Key &k = pool[rnd() % keys];
            pidw[i] = std::get<0>(k); pdst[i] = std::get<1>(k); pconv[i] = std::get<2>(k);
        }
        std::memcpy(&pid[8ull * i], &pidw[i], 8);
    }
    auto pkt_key = [&](uint32_t i) { return Key(by_id ? pidw[i] : 0ull, by_dst ? pdst[i] : 0u, pconv[i]); };
    int8_t *e_st = exact(st);
    const size_t pshift = rnd() % 2 ? 5 : 0;  // the batch's IdBuf column at an odd address
    uint8_t *e_pid = exact(pid, pshift);
    uint32_t *e_pconv = exact(pconv), *e_pdst = exact(pdst);
    uint32_t *conv_row = exact(std::vector<uint32_t>(n, 0x6E6E6E6Eu));
    int8_t *unknown = exact(std::vector<int8_t>(n, 0x6E));
    rsk_conv_resolve_in rin;
    std::memset(&rin, 0, sizeof rin);
    rin.status = e_st; rin.conv = e_pconv; rin.dst = by_dst ? e_pdst : nullptr; rin.id = by_id ? e_pid : nullptr;
    rsk_conv_resolve_out rout;
    std::memset(&rout, 0, sizeof rout);
    rout.conv_row = conv_row; rout.unknown = unknown;
    bad |= rsk_conv_resolve_host(&t, n, &rin, &rout, 1) != RSK_OK;

    // the std::map walk: the table as it is, then per unknown packet in order what SubGroup::OnRecv does
    std::map<Key, uint32_t> m;
    for (uint32_t r = 0; r < cap; ++r)
        if (state[r] & RSK_CONN_LIVE) m.emplace(row_key(r), r);
    std::vector<uint32_t> want_row(n), want_ci(ci), want_new_rows, want_new_first;
    std::vector<int8_t> want_unk(n);
    std::vector<uint8_t> want_state(state);
    uint32_t vac = 0, full = 0, left = 0;
    std::map<Key, int> refused;
    for (uint32_t i = 0; i < n; ++i) {
        want_row[i] = RSK_CONN_NONE;
        want_unk[i] = RSK_RECV_DROP;
        if (st[i] != RSK_RECV_VALID) continue;
        auto it = m.find(pkt_key(i));
        if (it == m.end()) {
            while (vac < cap && (want_state[vac] & RSK_CONN_LIVE)) ++vac;
            if (vac < cap) {
                want_state[vac] = RSK_CONN_LIVE;
                conv[vac] = pconv[i]; dst[vac] = pdst[i]; idw[vac] = pidw[i];
                co[vac] = pi[vac] = po[vac] = 0; want_ci[vac] = 0; alive[vac] = 1;
                want_new_rows.push_back(vac);
                want_new_first.push_back(i);
                it = m.emplace(pkt_key(i), vac).first;
            } else if (refused.emplace(pkt_key(i), 1).second) {
                ++full;
            }
        }
        if (it == m.end()) { want_unk[i] = RSK_RECV_VALID; ++left; continue; }
        want_row[i] = it->second;
        ++want_ci[it->second];
    }
    // what the resolve already counted is in e_ci; the walk above counted every found packet: subtract nothing,
    // the table's cur_in after resolve + create must equal want_ci (a new row starts at 0)

    // create, again while the header says to
    const uint32_t mlist = u_max < cap ? u_max : cap;
    const uint64_t wbytes = rsk_conv_create_bytes(u_max, cap);
    bad |= wbytes == 0 || wbytes % 16 != 0;
    void *work = aligned((size_t)wbytes, 0xA5);
    rsk_conv_create_in cin;
    cin.id = by_id ? e_pid : nullptr; cin.conv = e_pconv; cin.dst = by_dst ? e_pdst : nullptr; cin.u_max = u_max; cin.work = work;
    std::vector<uint32_t> got_new_rows, got_new_first;
    uint32_t n_unknown = 0, n_full = 0, calls = 0;
    for (;;) {
        uint32_t *nr = exact(std::vector<uint32_t>(mlist, 0x6E6E6E6Eu)), *nf = exact(std::vector<uint32_t>(mlist, 0x6E6E6E6Eu));
        uint32_t n_new = 0xFFFFFFFFu;
        rsk_conv_create_out cout_ = {conv_row, unknown, &n_unknown, nr, nf, &n_new, &n_full};
        bad |= rsk_conv_create_host(&t, &rows, n, &cin, &cout_, 1) != RSK_OK;
        bad |= n_new > mlist;
        for (uint32_t j = 0; j < n_new && j < mlist; ++j) { got_new_rows.push_back(nr[j]); got_new_first.push_back(nf[j]); }
        for (uint32_t j = n_new; j < mlist; ++j) bad |= nr[j] != 0x6E6E6E6Eu || nf[j] != 0x6E6E6E6Eu;
        free(nr); free(nf);
        if (++calls > n + 1u) { bad = 1; break; }
        if (!(n_unknown > 0 && n_full == 0)) break;
    }
    bad |= got_new_rows != want_new_rows || got_new_first != want_new_first || n_unknown != left;
    // the last call's n_full counts the distinct refused keys among the packets it considered
    bad |= (full == 0) != (n_full == 0) || n_full > full || (u_max >= n && n_full != full);
    for (uint32_t i = 0; i < n; ++i) bad |= conv_row[i] != want_row[i] || unknown[i] != want_unk[i];
    for (uint32_t r = 0; r < cap; ++r) {
        const bool made = (want_state[r] & RSK_CONN_LIVE) && !(state[r] & RSK_CONN_LIVE);
        bad |= e_state[r] != (made ? (uint8_t)RSK_CONN_LIVE : state[r]) || e_conv[r] != conv[r];
        if (by_dst) bad |= e_dst[r] != dst[r];
        if (by_id) bad |= std::memcmp(e_id + 8ull * r, &idw[r], 8) != 0;
        if (counters) bad |= e_ci[r] != want_ci[r] || e_co[r] != co[r] || e_pi[r] != pi[r] || e_po[r] != po[r] || e_alive[r] != alive[r];
    }
    // every key of the table, on the index as the create left it, then on a rebuilt one
    for (int rebuilt = 0; rebuilt < 2; ++rebuilt) {
        if (rebuilt) bad |= rsk_conv_index_build_host(&t, nullptr, 1) != RSK_OK;
        std::vector<int8_t> ones(cap, RSK_RECV_VALID);
        uint32_t *look = exact(std::vector<uint32_t>(cap, 0u));
        int8_t *e_ones = exact(ones);
        rsk_conv_table tl = t;
        tl.cur_in = nullptr;
        rsk_conv_resolve_in lin;
        std::memset(&lin, 0, sizeof lin);
        lin.status = e_ones; lin.conv = e_conv; lin.dst = tl.dst; lin.id = tl.id;
        rsk_conv_resolve_out lout;
        std::memset(&lout, 0, sizeof lout);
        lout.conv_row = look;
        bad |= rsk_conv_resolve_host(&tl, cap, &lin, &lout, 1) != RSK_OK;
        for (uint32_t r = 0; r < cap; ++r) {
            auto it = m.find(row_key(r));  // conv / dst / idw hold the table as the walk left it
            bad |= look[r] != (it == m.end() ? RSK_CONN_NONE : it->second);
        }
        free(look); free(e_ones);
    }
    if (bad) fprintf(stderr, "MISMATCH cap=%u flags=%u fill=%d n=%u keys=%u u_max=%u\n", cap, flags, fill, n, keys, u_max);
    free(e_state); free(e_alive); free(e_id - shift); free(e_conv); free(e_dst); free(e_ci); free(e_co); free(e_pi); free(e_po);
    free(t.index); free(work); free(e_st); free(e_pid - pshift); free(e_pconv); free(e_pdst); free(conv_row); free(unknown);
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    const uint32_t caps[] = {1, 2, 7, 64, 257, 3000};
    const uint32_t ns[] = {0, 1, 65, 700, 4100};
    for (uint32_t flags = 0; flags < 4; ++flags)
        for (uint32_t cap : caps)
            for (int fill = 0; fill < 3; ++fill)
                for (uint32_t n : ns) {
                    const uint32_t key_counts[] = {0u, 1u, 40u, 900u}, u_maxes[] = {1u, 64u, n + 1u, 1u << 16};
                    const uint32_t keys = key_counts[rnd() % 4], u_max = u_maxes[rnd() % 4];
                    if (u_max == 1u && n > 700u) continue;  // one key per call: keep the run short
                    bad |= run(cap, flags, fill, n, keys, u_max);
                    ++cases;
                }
    // the argument checks a caller can trip without a table
    bad |= rsk_conv_create_bytes(0, 4) != 0 || rsk_conv_create_bytes((1u << 24) + 1u, 4) != 0 || rsk_conv_create_bytes(4, 0) != 0;
    bad |= rsk_conv_create_host(nullptr, nullptr, 0, nullptr, nullptr, 1) != RSK_EINVAL;
    printf("%d cases, %s\n", cases, bad ? "MISMATCH" : "all equal");
    return bad ? 1 : 0;
}
