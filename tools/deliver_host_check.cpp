// Stand-alone check of rsk_deliver_host (rsock_amd/csrc/rsk_host.cpp) for a sanitizer build of the host
// code alone -- no HIP, no Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/deliver_host_check.cpp rsock_amd/csrc/rsk_host.cpp -lpthread -o deliver_host_check
// Shapes follow tests/golden/onrecv.npz (428 frames, lengths 1..1453, every source alignment, about
// half VALID) and a 5000-packet batch; every buffer is sized exactly, so an access one byte outside
// is reported.  Compares against a byte-by-byte restatement; exit status 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rsk_codec.h"

static uint64_t rng_state = 0x5EED;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static int run(uint32_t n, uint32_t align, int order_kind, int nthreads, bool cut) {
    if (n == 0 && order_kind) return 0;  // an empty vector's data() may be NULL: order / n_order would disagree
    std::vector<uint64_t> base(n);
    std::vector<uint16_t> inner(n), poff(n), plen(n);
    std::vector<int8_t> st(n);
    std::vector<uint32_t> order(n, 0xFFFFFFFFu);
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        base[i] = pos;
        inner[i] = (uint16_t)(rnd() % 3 ? 0 : 21);
        poff[i] = (uint16_t)(8 + 23 + (rnd() % 8 == 0 ? rnd() % 9 : 0));
        plen[i] = (uint16_t)(rnd() % 4 == 0 ? 1 + rnd() % 16 : 1 + rnd() % 1453);
        st[i] = (int8_t)(rnd() % 2 ? 1 : (rnd() % 2 ? 0 : -1));
        pos += (uint64_t)inner[i] + poff[i] + plen[i];  // frames back to back: every alignment
    }
    std::vector<uint8_t> arena(pos);  // exactly the bytes the payloads end in
    for (auto &b : arena) b = (uint8_t)rnd();
    uint32_t cnt = n;
    if (order_kind == 1) {  // the VALID indices
        cnt = 0;
        for (uint32_t i = 0; i < n; ++i)
            if (st[i] == 1) order[cnt++] = i;
    } else if (order_kind == 2) {  // a shuffled subset with stray entries and a poisoned count
        for (uint32_t i = 0; i < n; ++i) order[i] = i;
        for (uint32_t i = n; i > 1; --i) std::swap(order[i - 1], order[rnd() % i]);
        for (uint32_t i = 0; i < n; i += 9) order[i] = n + rnd() % 7;
        cnt = 0xFFFFFFFFu;
    }
    const uint32_t m = order_kind ? (cnt < n ? cnt : n) : n;
    // restatement
    std::vector<uint64_t> want_off(n + 1);
    std::vector<uint8_t> want;
    for (uint32_t k = 0; k <= n; ++k) {
        want_off[k] = want.size();
        if (k >= m) continue;
        const uint32_t i = order_kind ? order[k] : k;
        if (i >= n || st[i] != 1) continue;
        const uint8_t *s = arena.data() + base[i] + inner[i] + poff[i];
        want.insert(want.end(), s, s + plen[i]);
        while (want.size() % align) want.push_back(0);
    }
    const uint64_t total = want.size();
    uint64_t cap = total;
    if (cut && total > 3) cap = total / 2 + 1;
    rsk_deliver_in in = {arena.data(), base.data(), inner.data(), poff.data(), plen.data(), st.data(),
                         order_kind ? order.data() : nullptr, order_kind ? &cnt : nullptr};
    uint8_t *out = (uint8_t *)aligned_alloc(16, (cap + 15) / 16 * 16 + 16);
    std::memset(out, 0xA5, (cap + 15) / 16 * 16 + 16);
    std::vector<uint64_t> off(n + 1, 7);
    uint64_t tot = 7;
    rsk_deliver_out o = {out, cap, off.data(), &tot, align};
    int bad = rsk_deliver_host(n, &in, &o, nthreads) != RSK_OK;
    bad |= tot != total || off != want_off;
    for (uint32_t k = 0; k < n && !bad; ++k) {
        const uint64_t a = want_off[k], b = want_off[k + 1];
        if (b <= cap) bad |= b > a && std::memcmp(out + a, want.data() + a, b - a) != 0;
        else
            for (uint64_t x = a; x < cap && x < b; ++x) bad |= out[x] != 0xA5;  // a cut payload is not written
    }
    for (uint64_t x = cap; x < (cap + 15) / 16 * 16 + 16; ++x) bad |= out[x] != 0xA5;
    // plan only
    std::vector<uint64_t> off2(n + 1, 7);
    rsk_deliver_out p = {nullptr, 0, off2.data(), nullptr, align};
    bad |= rsk_deliver_host(n, &in, &p, nthreads) != RSK_OK || off2 != want_off;
    free(out);
    if (bad) printf("MISMATCH n=%u align=%u order=%d threads=%d cut=%d\n", n, align, order_kind, nthreads, (int)cut);
    return bad;
}

int main() {
    int bad = 0, runs = 0;
    const uint32_t ns[] = {0, 1, 428, 5000};
    const uint32_t aligns[] = {1, 16, 128};
    for (uint32_t n : ns)
        for (uint32_t al : aligns)
            for (int ok = 0; ok < 3; ++ok)
                for (int th : {1, 4})
                    for (int cut = 0; cut < 2; ++cut, ++runs) bad |= run(n, al, ok, th, cut != 0);
    printf("%s: %d runs\n", bad ? "FAILED" : "ok", runs);
    return bad;
}
