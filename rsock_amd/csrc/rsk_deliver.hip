// rsk_deliver.hip — payload delivery (rsk_deliver_batch, include/rsk_codec.h): the copy the
// reference's consumers make per packet (SConn::OnRecv, server/SConn.cpp:77-89; ClientGroup::send2Origin,
// client/ClientGroup.cpp:82-96: malloc + memcpy(base, rbuf.base, nread) of the pointer RConn::OnRecv
// computed, conn/RConn.cpp:64-85), batched: the VALID payloads gathered into one dense arena in delivery
// order, with the byte offset of every payload.
//
// Offsets: reduce-then-scan over tiles of kTile positions -- k_dl_sum (64-bit tile sums of the rounded
// lengths), k_dl_scan (one block scans the tile sums in place), k_dl_offsets (per-tile scan, writes
// out_off).  No block waits on another one.  Copy: k_dl_copy, one wave per 64 consecutive positions on a
// flat list of (payload, 16-B destination chunk) items.
#include <hip/hip_runtime.h>

#include "rsk_ctx.h"
#include "rsk_device.h"

namespace {

using rsk::funnel;
using rsk::gptr;

constexpr unsigned kBlock = 256;   // threads per block of every kernel here
constexpr unsigned kPer = 4;       // positions per thread of the offset kernels
constexpr unsigned kTile = kBlock * kPer;  // positions per tile: rsk::kDeliverTile
static_assert(kTile == rsk::kDeliverTile, "scratch size (rsk_ctx.h) and tile size must agree");
constexpr unsigned kScanBlock = 1024;  // threads of the one block that scans the tile sums
constexpr unsigned kGroup = 64;    // positions per copy wave (one per lane)

struct DlIn {
    const uint8_t *arena;
    const uint64_t *base_off;
    const uint16_t *inner_off;
    const uint16_t *pay_off;
    const uint16_t *pay_len;
    const int8_t *status;
    const uint32_t *order;
    const uint32_t *n_order;
    uint32_t n;
    uint32_t amask;  // align - 1
};

// Positions that carry an index: n without an order, else min(*n_order, n) (a poisoned count of
// 0xFFFFFFFF is clamped; its stray indices are skipped by dl_index).
__device__ __forceinline__ uint32_t dl_m(const DlIn &a) {
    if (!a.order) return a.n;
    const uint32_t c = *gptr(a.n_order);
    return c < a.n ? c : a.n;
}

// Packet index of position k < m, or 0xFFFFFFFF when it carries no bytes (a stray index or a packet
// that is not VALID): such a position is never dereferenced past its status byte.
__device__ __forceinline__ uint32_t dl_index(const DlIn &a, uint32_t k, uint32_t m) {
    if (k >= m) return ~0u;
    const uint32_t i = a.order ? gptr(a.order)[k] : k;
    if (i >= a.n) return ~0u;
    return gptr(a.status)[i] == RSK_RECV_VALID ? i : ~0u;
}

// L_k of position k (0 when it carries no bytes)
__device__ __forceinline__ uint32_t dl_len(const DlIn &a, uint32_t k, uint32_t m) {
    const uint32_t i = dl_index(a, k, m);
    return i == ~0u ? 0u : (uint32_t)gptr(a.pay_len)[i];
}

__device__ __forceinline__ uint32_t dl_round(uint32_t len, uint32_t amask) { return (len + amask) & ~amask; }

// Sum of v over the block's threads in every thread (kBlock threads; red: kBlock / 64 words of LDS).
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *red) {
    for (int off = 32; off; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (unsigned w = 0; w < kBlock / 64u; ++w) s += red[w];
    return s;
}

// Pass 1: tile_sum[t] = sum of the rounded lengths of tile t's positions.  A tile sums to at most
// 1024 * 65664 < 2^27, so 32 bits carry it; the sums are stored as 64-bit words for the scan.
__global__ __launch_bounds__(kBlock) void k_dl_sum(DlIn a, uint64_t *tile_sum) {
    __shared__ uint32_t red[kBlock / 64u];
    const uint32_t m = dl_m(a);
    const uint32_t k0 = blockIdx.x * kTile + threadIdx.x * kPer;
    uint32_t s = 0;
#pragma unroll
    for (unsigned u = 0; u < kPer; ++u)
        if (k0 + u < a.n) s += dl_round(dl_len(a, k0 + u, m), a.amask);
    s = block_sum(s, red);
    if (threadIdx.x == 0u) gptr(tile_sum)[blockIdx.x] = s;
}

// Pass 2, one block: exclusive scan of tile_sum[0, nt) in place; the total goes to tile_sum[nt],
// out_off[n] and *total.  Each thread owns ceil(nt / kScanBlock) consecutive tiles.
__global__ __launch_bounds__(kScanBlock) void k_dl_scan(uint64_t *tile_sum, uint32_t nt, uint64_t *out_off_n,
                                                        uint64_t *total) {
    __shared__ uint64_t part[kScanBlock];
    const uint32_t per = (nt + kScanBlock - 1u) / kScanBlock;
    const uint32_t lo = threadIdx.x * per < nt ? threadIdx.x * per : nt;
    const uint32_t hi = lo + per < nt ? lo + per : nt;
    RSK_GLOBAL uint64_t *ts = gptr(tile_sum);
    uint64_t s = 0;
    for (uint32_t t = lo; t < hi; ++t) s += ts[t];
    part[threadIdx.x] = s;
    __syncthreads();
    // Hillis-Steele inclusive scan of the per-thread sums
    for (unsigned d = 1; d < kScanBlock; d <<= 1) {
        const uint64_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0ull;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = part[threadIdx.x] - s;  // exclusive prefix of this thread's first tile
    for (uint32_t t = lo; t < hi; ++t) {
        const uint64_t v = ts[t];
        ts[t] = run;
        run += v;
    }
    if (threadIdx.x == kScanBlock - 1u) {
        const uint64_t tot = part[kScanBlock - 1u];
        ts[nt] = tot;
        *gptr(out_off_n) = tot;
        if (total) *gptr(total) = tot;
    }
}

// Pass 3: out_off[k] = tile base + exclusive scan of the rounded lengths inside the tile (k < n).
// Positions from m on have length 0, so their entries equal the total.
__global__ __launch_bounds__(kBlock) void k_dl_offsets(DlIn a, const uint64_t *tile_sum, uint64_t *out_off) {
    __shared__ uint32_t wsum[kBlock / 64u];
    const uint32_t m = dl_m(a);
    const uint32_t k0 = blockIdx.x * kTile + threadIdx.x * kPer;
    uint32_t len[kPer];
    uint32_t s = 0;
#pragma unroll
    for (unsigned u = 0; u < kPer; ++u) {
        len[u] = k0 + u < a.n ? dl_round(dl_len(a, k0 + u, m), a.amask) : 0u;
        s += len[u];
    }
    // inclusive scan of s over the wave, then over the block's waves
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t inc = s;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, off);
        if (lane >= (uint32_t)off) inc += v;
    }
    if (lane == 63u) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t wbase = 0;
#pragma unroll
    for (unsigned w = 0; w < kBlock / 64u; ++w)
        if (w < (threadIdx.x >> 6)) wbase += wsum[w];
    uint64_t o = gptr(tile_sum)[blockIdx.x] + wbase + (inc - s);
    RSK_GLOBAL uint64_t *oo = gptr(out_off);
#pragma unroll
    for (unsigned u = 0; u < kPer; ++u) {
        if (k0 + u < a.n) oo[k0 + u] = o;
        o += len[u];
    }
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld16(const uint8_t *p) {
    const u32x4 v = *reinterpret_cast<const RSK_GLOBAL u32x4 *>(gptr(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st16_nt(uint8_t *p, const uint4 &v) {
    const u32x4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<RSK_GLOBAL u32x4 *>(gptr(p)));
}

// rsk::funnel16 with a per-lane shift: 16 bytes from byte sh (0..15) of A||B.  Selects, not a switch:
// neighbouring lanes of the flat list belong to different payloads.
__device__ __forceinline__ uint4 funnel16_lane(const uint4 &A, const uint4 &B, uint32_t sh) {
    const uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    const uint32_t q = sh >> 2, r = sh & 3u;
    uint32_t e[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) e[i] = q == 0u ? w[i] : q == 1u ? w[i + 1] : q == 2u ? w[i + 2] : w[i + 3];
    return make_uint4(funnel(e[1], e[0], r), funnel(e[2], e[1], r), funnel(e[3], e[2], r), funnel(e[4], e[3], r));
}

// v with bytes [lim, 16) cleared, any lim
__device__ __forceinline__ uint4 keep_lim(const uint4 &v, int lim) {
    if (lim >= 16) return v;
    if (lim <= 0) return make_uint4(0u, 0u, 0u, 0u);
    return rsk::keep_bytes16(v, lim);
}

// The copy.  Wave w of the grid owns positions [64 w, 64 w + 64), one per lane: lane j reads its
// payload's destination range [out_off[k], out_off[k + 1]) and source, and the number of 16-B aligned
// destination chunks that range touches.  A wave scan of those counts makes the wave's flat item list;
// lane l then takes items l, l + 64, ...: it finds the item's payload by binary search in the scanned
// counts (LDS), builds the chunk from two aligned 16-B source loads through the funnel and stores it --
// whole (one nontemporal 16-B store) when the payload owns the chunk, else only the bytes
// [lo, hi) the payload owns, with store_range16's narrower stores: a chunk shared by up to 16 payloads
// (align < 16) is written by up to 16 items, each its own bytes, so no byte is written twice.  Bytes of
// the rounded length past L_k are zeros.  A source chunk is loaded only when it holds a payload byte,
// so no load leaves the pages the payloads lie in.
struct DlWave {
    uint32_t pre[kGroup + 1];  // exclusive scan of the chunk counts; pre[64] = items of the wave
    uint32_t len[kGroup];      // L_k
    uint32_t rlen[kGroup];     // rounded length
    uint64_t dst[kGroup];      // out_off[k]
    uint64_t src[kGroup];      // byte offset of the payload in the arena
};

// One item of a wave's flat list: the 16-B destination chunk `dp`, of which the item's payload owns the
// bytes [lo, hi); A, B the aligned source chunks around the bytes that land there, shf the funnel shift,
// lim the number of leading chunk bytes that are payload (the rest of the rounded length is zeros).
struct DlItem {
    uint4 A, B;
    uint8_t *dp;
    uint32_t shf, lo, hi;
    int32_t lim;
};

__device__ __forceinline__ void dl_load(const DlIn &a, const DlWave &W, uint8_t *out_arena, uint32_t t, DlItem &it) {
    // the payload j with pre[j] <= t < pre[j + 1]: the last j with pre[j] <= t (payloads without
    // chunks repeat their successor's pre and are skipped by taking the last one)
    uint32_t j = 0;
#pragma unroll
    for (uint32_t step = kGroup / 2u; step; step >>= 1)
        if (W.pre[j + step] <= t) j += step;
    const uint32_t c = t - W.pre[j];
    const uint64_t dj = W.dst[j];
    const uint32_t r0 = (uint32_t)(dj & 15u);
    const int32_t rel = (int32_t)(16u * c) - (int32_t)r0;  // payload byte at the chunk's byte 0
    const int32_t Lj = (int32_t)W.len[j], Rj = (int32_t)W.rlen[j];
    it.lo = c == 0u ? r0 : 0u;
    it.hi = Rj - rel < 16 ? (uint32_t)(Rj - rel) : 16u;
    it.lim = Lj - rel;
    // source bytes [x, x + 16) hold payload bytes [rel, rel + 16); the aligned chunks around them
    const uint8_t *x = a.arena + W.src[j] + (int64_t)rel;
    it.shf = (uint32_t)(reinterpret_cast<uintptr_t>(x) & 15u);
    const uint8_t *xa = x - it.shf;
    const int32_t relA = rel - (int32_t)it.shf;  // payload byte at xa[0]
    it.A = make_uint4(0u, 0u, 0u, 0u);
    it.B = it.A;
    if (relA + 16 > 0 && relA < Lj) it.A = ld16(xa);
    if (relA + 32 > 0 && relA + 16 < Lj) it.B = ld16(xa + 16);
    it.dp = out_arena + (dj - r0) + 16ull * c;
}

__device__ __forceinline__ void dl_store(const DlItem &it) {
    const uint4 v = keep_lim(funnel16_lane(it.A, it.B, it.shf), it.lim);
    if (it.lo == 0u && it.hi == 16u) st16_nt(it.dp, v);
    else rsk::store_range16(it.dp, v, it.lo, it.hi);
}

__global__ __launch_bounds__(kBlock) void k_dl_copy(DlIn a, const uint64_t *out_off, uint8_t *out_arena,
                                                    uint64_t out_cap) {
    __shared__ DlWave sh[kBlock / 64u];
    DlWave &W = sh[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t m = dl_m(a);
    const uint32_t k = (blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6)) * kGroup + lane;
    uint32_t L = 0, R = 0, nc = 0;
    uint64_t d = 0, s = 0;
    const uint32_t i = k < a.n ? dl_index(a, k, m) : ~0u;
    if (i != ~0u) {
        L = gptr(a.pay_len)[i];
        R = dl_round(L, a.amask);
        d = gptr(out_off)[k];
        if (L != 0u && d + R <= out_cap) {  // a payload cut by out_cap is not written at all
            s = gptr(a.base_off)[i] + (a.inner_off ? (uint64_t)gptr(a.inner_off)[i] : 0ull) + gptr(a.pay_off)[i];
            nc = (uint32_t)(((d & 15u) + R + 15u) >> 4);
        }
    }
    uint32_t inc = nc;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, off);
        if (lane >= (uint32_t)off) inc += v;
    }
    W.pre[lane] = inc - nc;
    if (lane == 63u) W.pre[kGroup] = inc;
    W.len[lane] = L;
    W.rlen[lane] = R;
    W.dst[lane] = d;
    W.src[lane] = s;
    __syncthreads();
    const uint32_t items = W.pre[kGroup];
    // two items per trip: both items' loads are issued before the first store waits for its own
    for (uint32_t t = lane; t < items; t += 128u) {
        const bool two = t + 64u < items;
        DlItem i0, i1;
        dl_load(a, W, out_arena, t, i0);
        if (two) dl_load(a, W, out_arena, t + 64u, i1);
        dl_store(i0);
        if (two) dl_store(i1);
    }
}

}  // namespace

extern "C" int rsk_deliver_batch(rsk_ctx *c, uint32_t n, const rsk_deliver_in *in, const rsk_deliver_out *out,
                                 void *stream) {
    if (!c || !in || !out || !out->out_off) return RSK_EINVAL;
    if (out->align == 0u || out->align > 128u || (out->align & (out->align - 1u))) return RSK_EINVAL;
    if (reinterpret_cast<uintptr_t>(out->out_arena) & 15u) return RSK_EINVAL;
    if ((in->order == nullptr) != (in->n_order == nullptr)) return RSK_EINVAL;
    if (n && (!in->base_off || !in->pay_off || !in->pay_len || !in->status)) return RSK_EINVAL;
    if (n && out->out_arena && !in->arena) return RSK_EINVAL;
    if (n > (1u << 30)) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        hipError_t e = hipMemsetAsync(out->out_off, 0, 8, s);
        if (e == hipSuccess && out->total) e = hipMemsetAsync(out->total, 0, 8, s);
        if (e != hipSuccess) { rsk::set_error("hipMemsetAsync", e); return RSK_EDEVICE; }
        return RSK_OK;
    }
    void *wsp = nullptr;
    int r = rsk::stream_ws(c, s, rsk::WS_DELIVER, rsk::deliver_ws_bytes(n), &wsp);
    if (r) return r;
    uint64_t *tile_sum = static_cast<uint64_t *>(wsp);
    DlIn a;
    a.arena = in->arena;
    a.base_off = in->base_off;
    a.inner_off = in->inner_off;
    a.pay_off = in->pay_off;
    a.pay_len = in->pay_len;
    a.status = in->status;
    a.order = in->order;
    a.n_order = in->n_order;
    a.n = n;
    a.amask = out->align - 1u;
    const uint32_t nt = (n + kTile - 1u) / kTile;
    hipLaunchKernelGGL(k_dl_sum, dim3(nt), dim3(kBlock), 0, s, a, tile_sum);
    if ((r = rsk::launch_check("k_dl_sum"))) return r;
    hipLaunchKernelGGL(k_dl_scan, dim3(1), dim3(kScanBlock), 0, s, tile_sum, nt, out->out_off + n, out->total);
    if ((r = rsk::launch_check("k_dl_scan"))) return r;
    hipLaunchKernelGGL(k_dl_offsets, dim3(nt), dim3(kBlock), 0, s, a, tile_sum, out->out_off);
    if ((r = rsk::launch_check("k_dl_offsets"))) return r;
    if (!out->out_arena) return RSK_OK;  // plan only
    const uint32_t nw = (n + kGroup - 1u) / kGroup, per_block = kBlock / 64u;
    hipLaunchKernelGGL(k_dl_copy, dim3((nw + per_block - 1u) / per_block), dim3(kBlock), 0, s, a, out->out_off,
                       out->out_arena, out->out_cap);
    return rsk::launch_check("k_dl_copy");
}
