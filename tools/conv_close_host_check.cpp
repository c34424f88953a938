// Stand-alone check of rsk_conv_close_host (rsock_amd/csrc/rsk_host.cpp), the host twin of
// rsk_conv_close_batch, for a sanitizer build of the host code alone -- no HIP, no Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/conv_close_host_check.cpp rsock_amd/csrc/rsk_host.cpp -lpthread -o conv_close_host_check
// A few hundred generated tables and calls per run, in both forms: every flag combination, tables of 1 .. 3000
// rows that are empty, sparse or full, duplicate keys among the rows, an IdBuf column at an odd address; timer
// lists with repeats, rows >= capacity, rows that are not LIVE, *n_close above and below m_max and 0; receive
// batches of 0 .. 4100 packets with resets that hit, miss and hit twice, with and without HOLD.  Every column,
// the work buffer and the index is a heap block of exactly its bytes, so an access one element outside is
// reported.  Each case is compared with a std::map walk over the rows that stay: every output, every column
// bytewise, and the lookup of every row's key on the index as the close left it.  Exit status 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "rsk_codec.h"

static uint64_t rng_state = 0xC105EC4EA7Eull;
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
static const uint32_t kSent = 0x6E6E6E6Eu, kNoRst = 0xFFFFFFFFu;

// fill: 0 empty, 1 about half LIVE, 2 every row LIVE.  form: 0 timer, 1 receive, 2 receive with HOLD.
static int run(uint32_t cap, uint32_t flags, int fill, int form, uint32_t n) {
    const bool by_dst = flags & RSK_CONV_BY_DST, by_id = flags & RSK_CONV_BY_ID, hold = form == 2;
    std::vector<uint8_t> state(cap), alive(cap), id(8ull * cap);
    std::vector<uint32_t> conv(cap), dst(cap), ci(cap), co(cap), pi(cap), po(cap);
    std::vector<uint64_t> idw(cap);
    const uint32_t c0 = rnd(), d0 = rnd();
    const uint64_t i0 = rnd64();
    for (uint32_t r = 0; r < cap; ++r) {
        const bool live = fill == 2 || (fill == 1 && rnd() % 2);
        state[r] = (uint8_t)((live ? RSK_CONN_LIVE : 0u) | (rnd() % 4 ? 0u : 0x82u));
        conv[r] = rnd() % 3 ? c0 ^ (1u << rnd() % 32) : rnd();  // few values: duplicate keys among the rows
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
    uint32_t *index0 = (uint32_t *)aligned((size_t)ibytes, 0);
    std::memcpy(index0, t.index, (size_t)ibytes);
    rsk_conv_rows rows = {e_state, e_conv, by_dst ? e_dst : nullptr, by_id ? e_id : nullptr};
    std::map<Key, uint32_t> m;  // the table as indexed: the lowest LIVE row of a key
    for (uint32_t r = 0; r < cap; ++r)
        if (state[r] & RSK_CONN_LIVE) m.emplace(row_key(r), r);

    rsk_conv_close_in cin;
    std::memset(&cin, 0, sizeof cin);
    cin.flags = hold ? RSK_CONV_CLOSE_HOLD : 0u;
    std::vector<uint8_t> marked(cap, 0);
    std::vector<uint32_t> at(cap, kNoRst), want_row;
    std::vector<int8_t> want_unk;
    uint32_t want_re = 0, want_again = 0, n_unknown = rnd() % 1000u, want_unknown = n_unknown;
    uint32_t *e_list = nullptr, *e_ncl = nullptr, *e_rst = nullptr, *conv_row = nullptr;
    uint8_t *e_kind = nullptr;
    int8_t *unknown = nullptr;
    void *work = nullptr;
    if (form == 0) {
        n = 0;
        const uint32_t m_max = rnd() % (2u * cap + 2u);
        std::vector<uint32_t> list(m_max);
        for (auto &x : list) x = rnd() % 8 ? rnd() % cap : (rnd() % 2 ? cap + rnd() % 3 : rnd());  // repeats, rows outside
        const uint32_t n_close = rnd() % 4 == 0 ? 0u : rnd() % 3 == 0 ? m_max + 1u + rnd() % 100u : rnd() % (m_max + 1u);
        for (uint32_t j = 0; j < m_max && j < n_close; ++j)
            if (list[j] < cap) marked[list[j]] = 1;
        e_list = exact(list);
        e_ncl = exact(std::vector<uint32_t>(1, n_close));
        const uint64_t wbytes = rsk_conv_close_bytes(cap);
        bad |= wbytes < cap || wbytes % 16 != 0;
        work = aligned((size_t)wbytes, 0xA5);
        cin.close_rows = e_list; cin.n_close = e_ncl; cin.m_max = m_max; cin.work = work;
    } else {
        // the resolve's outputs, synthesized: conv_row names LIVE rows (a DATA packet or a reset that hit), NONE or
        // a row outside; rst_first = the first reset packet of a row; later resets of the row: rst again
        std::vector<uint32_t> crow(n, RSK_CONN_NONE);
        std::vector<uint8_t> kind(n, RSK_CTL_NONE);
        std::vector<int8_t> unk(n, RSK_RECV_DROP);
        std::vector<uint32_t> live_rows;
        for (uint32_t r = 0; r < cap; ++r)
            if (state[r] & RSK_CONN_LIVE) live_rows.push_back(r);
        const uint32_t span = 1u + rnd() % 40u;  // packets concentrate on a few rows
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t pick = rnd() % 16;
            if (pick == 0) { unk[i] = RSK_RECV_VALID; kind[i] = (uint8_t)(rnd() % 8); continue; }  // an unknown DATA packet
            if (pick == 1) { crow[i] = cap + rnd() % 2; kind[i] = RSK_CTL_CONV_RST; continue; }  // a row outside the table
            if (pick == 2 || live_rows.empty()) { kind[i] = (uint8_t)(rnd() % 8); continue; }   // routed nowhere
            const uint32_t r = live_rows[rnd() % span % live_rows.size()];
            crow[i] = r;
            if (rnd() % 6 == 0) {
                kind[i] = RSK_CTL_CONV_RST;
                if (at[r] == kNoRst) at[r] = i;
            }
        }
        for (uint32_t r = 0; r < cap; ++r) {
            if (!(state[r] & RSK_CONN_LIVE) && rnd() % 8 == 0) at[r] = rnd() % (n + 1u);  // a mark on a row that is not LIVE
            marked[r] = at[r] != kNoRst;
        }
        want_row = crow;
        want_unk = unk;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t r = crow[i];
            if (r >= cap || !(state[r] & RSK_CONN_LIVE) || at[r] == kNoRst || i <= at[r]) continue;
            want_row[i] = RSK_CONN_NONE;
            if (kind[i] == RSK_CTL_CONV_RST) { ++want_again; continue; }
            want_unk[i] = RSK_RECV_VALID;
            ++want_re;
        }
        want_unknown += want_re;
        // what the call must not read: ctl_kind of a packet whose conv_row is no closing row
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t r = crow[i];
            if (r >= cap || !(state[r] & RSK_CONN_LIVE) || at[r] == kNoRst) kind[i] = (uint8_t)(rnd() % 2 ? RSK_CTL_CONV_RST : 0xFF);
        }
        e_rst = exact(at);
        e_kind = exact(kind);
        conv_row = exact(crow);
        unknown = exact(unk);
        cin.rst_first = e_rst;
        cin.ctl_kind = n ? e_kind : nullptr;
    }
    std::vector<uint32_t> want_rows, want_at;
    std::vector<uint8_t> stays(state);
    for (uint32_t r = 0; r < cap; ++r)
        if ((state[r] & RSK_CONN_LIVE) && marked[r]) {
            want_rows.push_back(r);
            want_at.push_back(at[r]);
            stays[r] = (uint8_t)(state[r] & ~RSK_CONN_LIVE);
        }
    std::map<Key, uint32_t> after;
    for (uint32_t r = 0; r < cap; ++r)
        if (stays[r] & RSK_CONN_LIVE) after.emplace(row_key(r), r);

    const int outs = (int)(rnd() % 4);  // which optional outputs are given
    uint32_t *cl_rows = exact(std::vector<uint32_t>(cap, kSent)), *cl_at = exact(std::vector<uint32_t>(cap, kSent));
    uint32_t n_closed = kSent, n_re = kSent, n_again = kSent;
    rsk_conv_close_out cout_;
    std::memset(&cout_, 0, sizeof cout_);
    cout_.conv_row = n ? conv_row : nullptr;
    cout_.unknown = form && outs != 1 ? unknown : nullptr;
    cout_.n_unknown = form && outs != 2 ? &n_unknown : nullptr;
    cout_.closed_rows = outs != 3 ? cl_rows : nullptr;
    cout_.closed_at = outs != 2 ? cl_at : nullptr;
    cout_.n_closed = &n_closed;
    cout_.n_reopened = outs != 1 ? &n_re : nullptr;
    cout_.n_rst_again = outs != 3 ? &n_again : nullptr;
    bad |= rsk_conv_close_host(&t, &rows, n, &cin, &cout_, 1) != RSK_OK;

    bad |= n_closed != want_rows.size();
    for (uint32_t j = 0; j < cap; ++j) {
        const bool in = j < want_rows.size();
        if (cout_.closed_rows) bad |= cl_rows[j] != (in ? want_rows[j] : kSent);
        if (cout_.closed_at) bad |= cl_at[j] != (in ? want_at[j] : kSent);
    }
    if (cout_.n_reopened) bad |= n_re != want_re;
    if (cout_.n_rst_again) bad |= n_again != want_again;
    if (cout_.n_unknown) bad |= n_unknown != want_unknown;
    for (uint32_t i = 0; i < n; ++i) {
        bad |= conv_row[i] != want_row[i];
        if (cout_.unknown) bad |= unknown[i] != want_unk[i];
    }
    for (uint32_t r = 0; r < cap; ++r) {
        bad |= e_state[r] != (hold ? state[r] : stays[r]) || e_conv[r] != conv[r] || e_dst[r] != dst[r];
        bad |= std::memcmp(e_id + 8ull * r, &idw[r], 8) != 0;
        bad |= e_ci[r] != ci[r] || e_co[r] != co[r] || e_pi[r] != pi[r] || e_po[r] != po[r] || e_alive[r] != alive[r];
    }
    if (want_rows.empty()) bad |= std::memcmp(index0, t.index, (size_t)ibytes) != 0;  // nothing closed: not a byte written
    // every row's key, on the index as the close left it, then (without HOLD) on a rebuilt one
    for (int rebuilt = 0; rebuilt < (hold ? 1 : 2); ++rebuilt) {
        if (rebuilt) bad |= rsk_conv_index_build_host(&t, nullptr, 1) != RSK_OK;
        uint32_t *look = exact(std::vector<uint32_t>(cap, 0u));
        int8_t *e_ones = exact(std::vector<int8_t>(cap, RSK_RECV_VALID));
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
            auto it = after.find(row_key(r));
            bad |= look[r] != (it == after.end() ? RSK_CONN_NONE : it->second);
        }
        free(look); free(e_ones);
    }
    if (bad) fprintf(stderr, "MISMATCH cap=%u flags=%u fill=%d form=%d n=%u\n", cap, flags, fill, form, n);
    free(e_state); free(e_alive); free(e_id - shift); free(e_conv); free(e_dst); free(e_ci); free(e_co); free(e_pi); free(e_po);
    free(t.index); free(index0); free(work); free(e_list); free(e_ncl); free(e_rst); free(e_kind); free(conv_row); free(unknown);
    free(cl_rows); free(cl_at);
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    const uint32_t caps[] = {1, 2, 7, 64, 1025, 3000};
    const uint32_t ns[] = {0, 1, 65, 2049, 4100};
    for (uint32_t flags = 0; flags < 4; ++flags)
        for (uint32_t cap : caps)
            for (int fill = 0; fill < 3; ++fill)
                for (int form = 0; form < 3; ++form)
                    for (uint32_t n : ns) {
                        if (form == 0 && n > 65u) continue;  // the timer form has no packets: three lists per table
                        bad |= run(cap, flags, fill, form, n);
                        ++cases;
                    }
    // the argument checks a caller can trip without a table
    bad |= rsk_conv_close_bytes(0) != 0 || rsk_conv_close_bytes(RSK_CONN_MAX_ROWS + 1u) != 0 || rsk_conv_close_bytes(17) != 32;
    bad |= rsk_conv_close_host(nullptr, nullptr, 0, nullptr, nullptr, 1) != RSK_EINVAL;
    printf("%d cases, %s\n", cases, bad ? "MISMATCH" : "all equal");
    return bad ? 1 : 0;
}
