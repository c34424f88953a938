// rsk_verify.hip — IPv4 header and TCP checksum verification of captured packets
// (rsk_verify_wire_batch, include/rsk_codec.h): the check the kernel's TCP input path makes before a
// segment reaches a socket, which a pcap-fed receiver (RawTcp::RawInput, conn/RawTcp.cpp:138-237)
// never gets, and the other half of rsk_encode_wire_batch's checksum fill.
//
// One launch, k_verify: a group of kGroupLanes = 8 lanes per packet, 8 packets per wave.  A group
// walks its packet in steps of 8 aligned 16-B chunks (one 128-B line per step), lane l taking chunk
// l of each step; every lane sums the aligned 32-bit words of its chunks, masked to the summed byte
// range, into 64 bits, and the group adds its lanes' folded sums with three DPP steps.  The link
// and IPv4 header fields, the IPv4 header sum and the pseudo-header addresses all come from the
// first step's chunks.
#include <hip/hip_runtime.h>

#include "rsk_ctx.h"
#include "rsk_device.h"

namespace {

using rsk::gptr;

constexpr unsigned kBlock = 256;      // threads per block
constexpr unsigned kGroupLanes = 8;   // lanes per packet
constexpr unsigned kPerBlock = kBlock / kGroupLanes;  // packets per block
static_assert((uint64_t)((RSK_VERIFY_MAX_BATCH + kPerBlock - 1u) / kPerBlock) * kBlock <= 0xFFFFFFFFull,
              "the grid of RSK_VERIFY_MAX_BATCH packets must be a legal launch");

struct VfArgs {
    const uint8_t *arena;
    const uint64_t *cap_off;
    const uint32_t *cap_len;
    const int8_t *status;
    uint8_t *csum;
    int8_t *status_out;
    uint32_t *n_bad;
    uint32_t n;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld16(const uint8_t *p) {
    const u32x4 v = *reinterpret_cast<const RSK_GLOBAL u32x4 *>(gptr(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// low k bytes set, k in [0, 4]
__device__ __forceinline__ uint32_t low_bytes(int k) { return (uint32_t)((1ull << (8 * k)) - 1ull); }
__device__ __forceinline__ int clamp4(int k) { return k < 0 ? 0 : (k > 4 ? 4 : k); }

// Sum of the four 32-bit words of chunk v with every byte outside [lo, hi) cleared (byte offsets
// inside the chunk; any integers, an empty or outside range gives 0).
__device__ __forceinline__ uint64_t sum_range(const uint4 &v, int lo, int hi) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint64_t s = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d)
        s += w[d] & low_bytes(clamp4(hi - 4 * d)) & ~low_bytes(clamp4(lo - 4 * d));
    return s;
}

// As sum_range with lo <= 0: the chunks past the first step are cut by the range's end only.
__device__ __forceinline__ uint64_t sum_lim(const uint4 &v, int hi) {
    if (hi >= 16) return (uint64_t)v.x + v.y + v.z + v.w;
    return sum_range(v, 0, hi);
}

// A sum of 32-bit words folded with end-around carry to at most 17 bits (the value mod 0xFFFF is
// kept, and so is whether it is zero).
__device__ __forceinline__ uint32_t fold17(uint64_t s) {
    s = (s & 0xffffffffull) + (s >> 32);
    s = (s & 0xffffffffull) + (s >> 32);
    const uint32_t t = (uint32_t)s;
    return (t & 0xffffu) + (t >> 16);
}
// ... to 16 bits: 0xFFFF for every nonzero multiple of 0xFFFF, 0 only for 0
__device__ __forceinline__ uint32_t fold16(uint32_t t) {
    t = (t & 0xffffu) + (t >> 16);
    t = (t & 0xffffu) + (t >> 16);
    return (t & 0xffffu) + (t >> 16);
}

// Sum of x over the 8 lanes of a group, in every lane: lane ^ 1, lane ^ 2 inside the quad, then the
// mirrored lane of the 8 (row_half_mirror), whose quad holds the other half's sum.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t group_sum(uint32_t x) {
    x += dpp<0xB1>(x);   // quad_perm [1, 0, 3, 2]
    x += dpp<0x4E>(x);   // quad_perm [2, 3, 0, 1]
    x += dpp<0x141>(x);  // row_half_mirror
    return x;
}

// L: bytes of the link header (14 EN10MB, 4 NULL, 0 RAW).  The rule is include/rsk_codec.h's.
template <int L>
__global__ __launch_bounds__(kBlock) void k_verify(VfArgs a) {
    const uint32_t l = threadIdx.x & (kGroupLanes - 1u);
    const uint32_t i = blockIdx.x * kPerBlock + threadIdx.x / kGroupLanes;
    const bool live = i < a.n;
    int8_t st = RSK_RECV_VALID;
    if (live && a.status) st = gptr(a.status)[i];
    const bool examine = live && st == RSK_RECV_VALID;  // uniform over the group
    uint32_t c = 0, r = 0;
    const uint8_t *A0 = a.arena;
    if (examine) {
        c = gptr(a.cap_len)[i];
        const uint8_t *p = a.arena + gptr(a.cap_off)[i];
        r = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
        A0 = p - r;
    }
    // Chunk k is the 16 bytes at A0 + 16 k; the packet's bytes lie at window offsets [r, r + c), in
    // chunks [0, nchunk): only those are ever loaded.
    const uint32_t nchunk = c ? (uint32_t)(((uint64_t)r + c + 15u) >> 4) : 0u;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (l < nchunk) v = ld16(A0 + 16u * l);

    // The 16 bytes from the ethertype (EN10MB) or from the packet's first byte, in every lane: five
    // window dwords from the lanes that hold them, then the byte funnel.
    constexpr int kSkip = L == 14 ? 12 : 0;
    const uint32_t s0 = r + kSkip, d0 = s0 >> 2;
    uint32_t e[5];
#pragma unroll
    for (uint32_t j = 0; j < 5; ++j)
        e[j] = (uint32_t)__shfl((int)rsk::word_at(v, (d0 + j) & 3u), (int)((d0 + j) >> 2), (int)kGroupLanes);
    uint32_t u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = rsk::funnel(e[j + 1], e[j], s0 & 3u);
    auto byte = [&u](int k) -> uint32_t { return (u[k >> 2] >> (8 * (k & 3))) & 0xffu; };
    constexpr int kIp = L - kSkip;  // the IPv4 header's first byte in u
    const uint32_t ihl = byte(kIp) & 15u, H = 4u * ihl;
    const uint32_t tot = (byte(kIp + 2) << 8) | byte(kIp + 3);
    const uint32_t frag = (byte(kIp + 6) << 8) | byte(kIp + 7);

    bool ok = examine;
    if (L == 14) ok = ok && c >= 14u && (u[0] & 0xffffu) == 0x0008u;  // 08 00
    if (L == 4) ok = ok && c >= 4u && u[0] == 2u;                     // AF_INET, little-endian
    ok = ok && c >= (uint32_t)L + 20u && (byte(kIp) >> 4) == 4u && ihl >= 5u && c >= (uint32_t)L + H;
    const bool tcp_try = ok && byte(kIp + 9) == 6u && (frag & 0x3fffu) == 0u && tot >= H + 20u;
    const bool trunc = tcp_try && (uint32_t)L + tot > c;
    const bool tcp_chk = tcp_try && !trunc;

    // Window offsets of the summed ranges: the IPv4 header, the addresses of the pseudo-header
    // (inside it) and the segment.  The segment ends at or before r + c, so its chunks are loadable.
    const int ip_lo = (int)r + L, ip_hi = ip_lo + (int)H;
    const int seg_hi = tcp_chk ? ip_lo + (int)tot : ip_hi;
    const int own = 16 * (int)l;
    uint64_t acc_ip = sum_range(v, ip_lo - own, ip_hi - own);
    uint64_t acc = sum_range(v, ip_lo + 12 - own, ip_lo + 20 - own) + sum_range(v, ip_hi - own, seg_hi - own);
    // the later steps, four chunks per lane and trip: the loads are independent, and a trip's chunks
    // past the segment's last re-read that last chunk (masked to nothing) instead of branching
    const uint32_t nseg = tcp_chk ? (uint32_t)(seg_hi + 15) >> 4 : 0u;
    for (uint32_t k = l + kGroupLanes; k < nseg; k += 4u * kGroupLanes) {
        uint4 q[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t kj = k + j * kGroupLanes;
            q[j] = ld16(A0 + 16ull * (kj < nseg ? kj : nseg - 1u));
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t kj = k + j * kGroupLanes;
            acc += sum_lim(q[j], kj < nseg ? seg_hi - 16 * (int)kj : 0);
        }
    }
    const uint32_t m_ip = fold16(group_sum(fold17(acc_ip)));
    uint32_t m = fold16(group_sum(fold17(acc)));
    // m sums little-endian halfwords at even addresses.  A range that starts at an even address has
    // the packet's halfwords byte-swapped in it, one that starts at an odd address has them as they
    // are (RFC 1071 §2(B)); then the pseudo-header's protocol and length.
    if (!(ip_lo & 1)) m = rsk::bswap16(m);
    const bool tcp_ok = fold16(m + 6u + (tot - H)) == 0xffffu;
    const bool ip_ok = m_ip == 0xffffu;

    uint32_t f = 0;
    if (ok) f |= RSK_CSUM_IP_CHECKED | (ip_ok ? RSK_CSUM_IP_OK : 0u);
    if (trunc) f |= RSK_CSUM_TCP_TRUNC;
    if (tcp_chk) f |= RSK_CSUM_TCP_CHECKED | (tcp_ok ? RSK_CSUM_TCP_OK : 0u);
    const bool bad = (ok && !ip_ok) || (tcp_chk && !tcp_ok);
    const bool writer = live && l == 0u;
    if (writer) {
        gptr(a.csum)[i] = (uint8_t)f;
        if (a.status_out) gptr(a.status_out)[i] = bad ? (int8_t)RSK_RECV_DROP : st;
    }
    if (a.n_bad) {  // the word was zeroed on the stream ahead of this launch
        const uint32_t cnt = (uint32_t)__popcll(__ballot(writer && bad));
        if (cnt && (threadIdx.x & 63u) == 0u) atomicAdd(a.n_bad, cnt);
    }
}

}  // namespace

extern "C" int rsk_verify_wire_batch(rsk_ctx *c, uint32_t n, const rsk_verify_in *in, int datalink,
                                     const rsk_verify_out *out, void *stream) {
    if (!c || !in || !out) return RSK_EINVAL;
    if (datalink != RSK_DLT_NULL && datalink != RSK_DLT_EN10MB && datalink != RSK_DLT_RAW) return RSK_EINVAL;
    if (out->status_out && !in->status) return RSK_EINVAL;
    if (n && (!in->cap_arena || !in->cap_off || !in->cap_len || !out->csum)) return RSK_EINVAL;
    if (n > RSK_VERIFY_MAX_BATCH) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (out->n_bad) {
        hipError_t e = hipMemsetAsync(out->n_bad, 0, 4, s);
        if (e != hipSuccess) { rsk::set_error("hipMemsetAsync", e); return RSK_EDEVICE; }
    }
    if (n == 0) return RSK_OK;
    VfArgs a;
    a.arena = in->cap_arena;
    a.cap_off = in->cap_off;
    a.cap_len = in->cap_len;
    a.status = in->status;
    a.csum = out->csum;
    a.status_out = out->status_out;
    a.n_bad = out->n_bad;
    a.n = n;
    const dim3 grid((n + kPerBlock - 1u) / kPerBlock), block(kBlock);
    if (datalink == RSK_DLT_EN10MB) hipLaunchKernelGGL(k_verify<14>, grid, block, 0, s, a);
    else if (datalink == RSK_DLT_NULL) hipLaunchKernelGGL(k_verify<4>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_verify<0>, grid, block, 0, s, a);
    return rsk::launch_check("k_verify");
}
