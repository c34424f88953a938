// Stand-alone check of rsk_verify_wire_host (rsock_amd/csrc/rsk_host.cpp) for a sanitizer build of the
// host code alone -- no HIP, no Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/verify_host_check.cpp rsock_amd/csrc/rsk_host.cpp -lpthread -o verify_host_check
// A few hundred generated IPv4/TCP packets per run (every datalink, IP and TCP options, odd lengths,
// about a third with a flipped bit, some cut short by cap_len, some gated out by the status column),
// packed back to back in an arena that ends exactly at the last packet's last captured byte, so an
// access one byte outside is reported.  Compares with a byte-loop RFC 1071 restatement; exit status
// 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rsk_codec.h"

static uint64_t rng_state = 0xC5EED;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// RFC 1071, byte by byte: big-endian halfwords, an odd last byte as the high byte
static uint32_t sum_bytes(const uint8_t *p, size_t n, uint32_t s) {
    for (size_t i = 0; i < n; ++i) {
        s += (i & 1) ? p[i] : (uint32_t)p[i] << 8;
        s = (s & 0xffffu) + (s >> 16);
    }
    return s;
}

static uint32_t want_one(const uint8_t *p, uint32_t c, uint32_t L) {
    if (L == 14 && (c < 14 || p[12] != 8 || p[13] != 0)) return 0;
    if (L == 4 && (c < 4 || p[0] != 2 || p[1] || p[2] || p[3])) return 0;
    if (c < L + 20 || (p[L] >> 4) != 4 || (p[L] & 15) < 5 || c < L + 4u * (p[L] & 15)) return 0;
    const uint32_t H = 4u * (p[L] & 15), tot = p[L + 2] * 256u + p[L + 3];
    uint32_t f = RSK_CSUM_IP_CHECKED | (sum_bytes(p + L, H, 0) == 0xffffu ? RSK_CSUM_IP_OK : 0u);
    if (p[L + 9] != 6 || ((p[L + 6] * 256u + p[L + 7]) & 0x3fffu) || tot < H + 20) return f;
    if (L + tot > c) return f | RSK_CSUM_TCP_TRUNC;
    uint32_t s = sum_bytes(p + L + 12, 8, 0);
    s = sum_bytes(p + L + H, tot - H, s);
    s += 6 + (tot - H);
    while (s >> 16) s = (s & 0xffffu) + (s >> 16);
    return f | RSK_CSUM_TCP_CHECKED | (s == 0xffffu ? RSK_CSUM_TCP_OK : 0u);
}

static void put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 8); p[1] = (uint8_t)v; }

// One packet with correct checksums appended to `a`; returns its length.
static uint32_t make_packet(std::vector<uint8_t> &a, uint32_t L) {
    const uint32_t ihl = rnd() % 4 ? 5 : 5 + rnd() % 11, thl = rnd() % 4 ? 5 : 5 + rnd() % 11;
    const uint32_t pay = rnd() % 5 == 0 ? 1400 + rnd() % 81 : rnd() % 200;
    const uint32_t H = 4 * ihl, tot = H + 4 * thl + pay;
    const size_t at = a.size();
    a.resize(at + L + tot);
    uint8_t *p = a.data() + at;
    for (uint32_t k = 0; k < L + tot; ++k) p[k] = (uint8_t)rnd();
    if (L == 14) { p[12] = 8; p[13] = 0; }
    if (L == 4) { p[0] = 2; p[1] = p[2] = p[3] = 0; }
    uint8_t *ip = p + L, *tcp = ip + H;
    ip[0] = (uint8_t)(0x40 | ihl);
    put16(ip + 2, tot);
    put16(ip + 6, rnd() % 2 ? 0x4000 : 0);
    ip[9] = 6;
    put16(ip + 10, 0);
    put16(ip + 10, ~sum_bytes(ip, H, 0) & 0xffffu);
    tcp[12] = (uint8_t)(thl << 4);
    put16(tcp + 16, 0);
    uint32_t s = sum_bytes(tcp, tot - H, sum_bytes(ip + 12, 8, 0)) + 6 + (tot - H);
    while (s >> 16) s = (s & 0xffffu) + (s >> 16);
    put16(tcp + 16, ~s & 0xffffu);
    return L + tot;
}

static int run(uint32_t n, int datalink, int nthreads, bool gated) {
    const uint32_t L = datalink == RSK_DLT_EN10MB ? 14u : datalink == RSK_DLT_NULL ? 4u : 0u;
    std::vector<uint8_t> arena;
    std::vector<uint64_t> off(n);
    std::vector<uint32_t> cap(n);
    std::vector<int8_t> st(n), want_st(n);
    for (uint32_t i = 0; i < n; ++i) {
        off[i] = arena.size();
        const uint32_t len = make_packet(arena, L);
        cap[i] = len;
        uint8_t *p = arena.data() + off[i];
        const uint32_t kind = rnd() % 12;
        if (kind < 4) p[L + rnd() % (len - L)] ^= (uint8_t)(1u << rnd() % 8);   // a flipped bit
        else if (kind == 4) p[rnd() % len] = (uint8_t)rnd();                     // any byte, link header included
        else if (kind == 5) {                                                    // cut by the snap length
            cap[i] = rnd() % (len + 1);
            arena.resize(off[i] + cap[i]);
        }
        st[i] = (int8_t)(rnd() % 4 ? 1 : (rnd() % 2 ? 0 : -1));
    }
    // a gated-out packet is never read: point it far outside the arena
    std::vector<uint64_t> off_in(off);
    if (gated)
        for (uint32_t i = 0; i < n; ++i)
            if (st[i] != 1) off_in[i] = 1ull << 46;
    std::vector<uint8_t> want(n);
    uint32_t want_bad = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t f = gated && st[i] != 1 ? 0u : want_one(arena.data() + off[i], cap[i], L);
        const bool bad = ((f & RSK_CSUM_IP_CHECKED) && !(f & RSK_CSUM_IP_OK)) ||
                         ((f & RSK_CSUM_TCP_CHECKED) && !(f & RSK_CSUM_TCP_OK));
        want[i] = (uint8_t)f;
        want_st[i] = bad ? (int8_t)RSK_RECV_DROP : st[i];
        want_bad += bad;
    }
    // a heap block of exactly the arena's bytes: a read one byte past the last packet is reported
    uint8_t *exact = (uint8_t *)malloc(arena.size() ? arena.size() : 1);
    std::memcpy(exact, arena.data(), arena.size());
    std::vector<uint8_t> csum(n, 0xEE);
    std::vector<int8_t> sout(n, 0x55);
    uint32_t nbad = 0xFFFFFFFFu;
    rsk_verify_in in = {exact, off_in.data(), cap.data(), gated ? st.data() : nullptr};
    rsk_verify_out out = {csum.data(), gated ? sout.data() : nullptr, &nbad};
    int bad = rsk_verify_wire_host(n, &in, datalink, &out, nthreads) != RSK_OK;
    bad |= nbad != want_bad || csum != want || (gated && sout != want_st);
    if (gated) {  // status_out may be the status column itself
        std::vector<int8_t> inplace(st);
        rsk_verify_in in2 = {exact, off_in.data(), cap.data(), inplace.data()};
        rsk_verify_out out2 = {csum.data(), inplace.data(), nullptr};
        bad |= rsk_verify_wire_host(n, &in2, datalink, &out2, nthreads) != RSK_OK || inplace != want_st || csum != want;
    }
    free(exact);
    if (bad) printf("MISMATCH n=%u datalink=%d threads=%d gated=%d\n", n, datalink, nthreads, (int)gated);
    return bad;
}

int main() {
    int bad = 0, runs = 0;
    for (uint32_t n : {1u, 300u, 5000u})
        for (int dl : {RSK_DLT_EN10MB, RSK_DLT_NULL, RSK_DLT_RAW})
            for (int th : {1, 4})
                for (int gated = 0; gated < 2; ++gated, ++runs) bad |= run(n, dl, th, gated != 0);
    // argument errors and the empty batch
    uint8_t b = 0;
    uint64_t o = 0;
    uint32_t c = 0, nb = 7;
    int8_t s = 1;
    rsk_verify_in in = {&b, &o, &c, nullptr};
    rsk_verify_out out = {&b, &s, &nb};
    bad |= rsk_verify_wire_host(1, &in, RSK_DLT_RAW, &out, 1) != RSK_EINVAL;      // status_out without status
    out.status_out = nullptr;
    bad |= rsk_verify_wire_host(1, &in, 2, &out, 1) != RSK_EINVAL;                // datalink
    bad |= rsk_verify_wire_host(1, nullptr, RSK_DLT_RAW, &out, 1) != RSK_EINVAL;
    rsk_verify_in none = {nullptr, nullptr, nullptr, nullptr};
    bad |= rsk_verify_wire_host(1, &none, RSK_DLT_RAW, &out, 1) != RSK_EINVAL;
    bad |= rsk_verify_wire_host(0, &none, RSK_DLT_RAW, &out, 1) != RSK_OK || nb != 0;
    printf("%s: %d runs\n", bad ? "FAILED" : "ok", runs);
    return bad;
}
