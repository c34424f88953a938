// rsk_tile_dev.h — what the passes over tiles of packets or rows share (rsk_control.hip: control packets
// and the keepalive timer; rsk_conv.hip: conv routing, activity counts and flush): the message columns,
// the order-stable list positions of a tile's flagged items, the one-block scan of the tile counts, and
// the on-chip combining of a tile's per-row counts.  Internal (not installed).
#pragma once
#include <hip/hip_runtime.h>

#include "rsk_conn_dev.h"

namespace rsk {

constexpr unsigned kTileBlock = 256;  // threads per block of every tile pass
constexpr unsigned kTileWaves = kTileBlock / 64u;
constexpr unsigned kScanBlock = 1024;  // threads of the one block that scans the tile counts

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));  // a tile's two counts
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The message columns as the kernels write them (rsk_ctl_msgs; id as one word per entry).
struct MsgOut {
    uint8_t *cmd;
    uint64_t *body;
    uint64_t *id;
    uint32_t *src;
    uint64_t *avoid;
    uint64_t *pay_off;
    uint16_t *pay_len;
};

// Entry k of the list; its body takes 8 bytes of the body column whatever `len` says (pay_off = 8k).
__device__ __forceinline__ void put_msg(const MsgOut &m, uint32_t k, uint32_t cmd, uint64_t body, uint64_t id,
                                        uint32_t src, uint64_t avoid, uint32_t len) {
    if (m.cmd) gptr(m.cmd)[k] = (uint8_t)cmd;
    if (m.body) gptr(m.body)[k] = body;
    if (m.id) gptr(m.id)[k] = id;
    if (m.src) gptr(m.src)[k] = src;
    if (m.avoid) gptr(m.avoid)[k] = avoid;
    if (m.pay_off) gptr(m.pay_off)[k] = 8ull * k;
    if (m.pay_len) gptr(m.pay_len)[k] = (uint16_t)len;
}

// List positions of a tile's flagged items in item order: item (k, t) of the tile is its k * 256 + t-th.
// pos[k] = base + the number of flagged items before (k, this thread); cnt: PER * kTileWaves words of LDS.
// Returns the tile's number of flagged items.  Every thread of the block must call it.
template <unsigned PER>
__device__ __forceinline__ uint32_t tile_positions(const bool (&flag)[PER], uint32_t base, uint32_t (*cnt)[kTileWaves],
                                                   uint32_t (&pos)[PER]) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t below[PER];
#pragma unroll
    for (unsigned k = 0; k < PER; ++k) {
        const uint64_t b = __ballot(flag[k]);
        below[k] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0u) cnt[k][wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    uint32_t run = 0;
#pragma unroll
    for (unsigned k = 0; k < PER; ++k) {
#pragma unroll
        for (unsigned w = 0; w < kTileWaves; ++w) {
            if (w == wave) pos[k] = base + run + below[k];
            run += cnt[k][w];
        }
    }
    return run;
}

// A tile's two counts (each wave-uniform) summed over the block's waves and stored to tile[blockIdx.x]:
// one plain store per block, no atomics.  red: 2 * kTileWaves words of LDS.
__device__ __forceinline__ void tile_store_counts(u32x2 *tile, uint32_t x, uint32_t y, uint32_t (*red)[kTileWaves]) {
    if ((threadIdx.x & 63u) == 0u) {
        red[0][threadIdx.x >> 6] = x;
        red[1][threadIdx.x >> 6] = y;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        u32x2 s = u32x2{0u, 0u};
#pragma unroll
        for (unsigned w = 0; w < kTileWaves; ++w) {
            s.x += red[0][w];
            s.y += red[1][w];
        }
        gptr(tile)[blockIdx.x] = s;
    }
}

// Exclusive scan of the nt tile counts (both components) in place, one block; the totals go to
// tile[nt] and to *tot_x / *tot_y (each may be NULL).  Each thread owns ceil(nt / kScanBlock)
// consecutive tiles.  A component's total is at most the number of items (< 2^32).
static __global__ __launch_bounds__(kScanBlock) void k_tile_scan(u32x2 *tile, uint32_t nt, uint32_t *tot_x, uint32_t *tot_y) {
    __shared__ u32x2 part[kScanBlock];
    const uint32_t per = (nt + kScanBlock - 1u) / kScanBlock;
    const uint32_t lo = threadIdx.x * per < nt ? threadIdx.x * per : nt;
    const uint32_t hi = lo + per < nt ? lo + per : nt;
    RSK_GLOBAL u32x2 *ts = gptr(tile);
    u32x2 s = u32x2{0u, 0u};
    for (uint32_t t = lo; t < hi; ++t) {
        const u32x2 v = ts[t];
        s.x += v.x;
        s.y += v.y;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (unsigned d = 1; d < kScanBlock; d <<= 1) {  // Hillis-Steele inclusive scan of the per-thread sums
        const u32x2 v = threadIdx.x >= d ? part[threadIdx.x - d] : u32x2{0u, 0u};
        __syncthreads();
        part[threadIdx.x].x += v.x;
        part[threadIdx.x].y += v.y;
        __syncthreads();
    }
    u32x2 run = u32x2{part[threadIdx.x].x - s.x, part[threadIdx.x].y - s.y};
    for (uint32_t t = lo; t < hi; ++t) {
        const u32x2 v = ts[t];
        ts[t] = run;
        run.x += v.x;
        run.y += v.y;
    }
    if (threadIdx.x == kScanBlock - 1u) {
        const u32x2 tot = part[kScanBlock - 1u];
        ts[nt] = tot;
        if (tot_x) *gptr(tot_x) = tot.x;
        if (tot_y) *gptr(tot_y) = tot.y;
    }
}

// ---- a tile's per-row counts, combined on chip ---------------------------------------------------------
// Every item of a tile (PER per thread) names a row below 2^20 or RSK_CONN_NONE; counter[row] is to grow
// by the number of items that name it.  Equal rows are combined before anything leaves the CU:
//   1. per wave and step, kLeaderRounds rounds take the row of the first lane still uncounted
//      (readfirstlane), ballot the lanes that hold it and let one lane carry their number: a wave whose
//      packets share one or two convs -- a burst -- is done after them with one or two LDS operations;
//   2. what is carried goes into an open-addressing table in LDS (kAggSlots entries, twice a tile's items,
//      so at least half of it stays free): claim the row's entry by compare-and-swap, add to its count;
//   3. after a barrier every taken entry becomes ONE no-return atomic add to the counter column.
// So a tile issues one global atomic per distinct row, whatever the skew: 1 when all of its packets are one
// conv's, at most PER * 256 when every packet is another's.  Integer adds commute: the column's final
// value does not depend on the order anything ran in.
constexpr unsigned kLeaderRounds = 2;

template <unsigned PER>
struct RowAgg {
    static constexpr unsigned kSlots = 2u * PER * kTileBlock;
    uint32_t row[kSlots];
    uint32_t cnt[kSlots];
};

// Every thread of the block must call it (two barriers).  agg needs no initialisation.
template <unsigned PER>
__device__ __forceinline__ void tile_count_rows(const uint32_t (&row)[PER], uint32_t *counter, uint32_t capacity,
                                                RowAgg<PER> &agg) {
    constexpr unsigned kSlots = RowAgg<PER>::kSlots;
    static_assert((kSlots & (kSlots - 1u)) == 0u && kSlots % (4u * kTileBlock) == 0u, "a power of two, cleared by 16-B stores");
    {
        const u32x4 none = {RSK_CONN_NONE, RSK_CONN_NONE, RSK_CONN_NONE, RSK_CONN_NONE}, zero = {0u, 0u, 0u, 0u};
        u32x4 *r4 = reinterpret_cast<u32x4 *>(agg.row), *c4 = reinterpret_cast<u32x4 *>(agg.cnt);
#pragma unroll
        for (unsigned q = 0; q < kSlots / (4u * kTileBlock); ++q) {
            r4[q * kTileBlock + threadIdx.x] = none;
            c4[q * kTileBlock + threadIdx.x] = zero;
        }
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (unsigned k = 0; k < PER; ++k) {
        bool todo = row[k] != RSK_CONN_NONE;  // not yet part of a group some lane carries
        uint32_t carry = 0;                   // the items this lane puts into the table for row[k]
#pragma unroll
        for (unsigned round = 0; round < kLeaderRounds; ++round) {
            const uint64_t left = __ballot(todo);
            if (left == 0ull) break;  // wave-uniform
            const uint32_t first = (uint32_t)__builtin_ctzll(left);
            const uint32_t lead = (uint32_t)__builtin_amdgcn_readlane((int)row[k], (int)first);
            const bool mine = todo && row[k] == lead;
            const uint64_t same = __ballot(mine);
            if (mine) {
                todo = false;
                if (lane == first) carry = (uint32_t)__popcll(same);
            }
        }
        if (todo) carry = 1u;  // a row that no leader round took
        if (carry != 0u) {
            // at most PER * 256 distinct rows in kSlots = twice as many entries: a free one is met; the
            // bound only keeps a corrupted launch from spinning
            uint32_t s = (row[k] * 0x9E3779B1u) >> (32u - (unsigned)__builtin_ctz(kSlots));
            for (unsigned step = 0; step < kSlots; ++step, s = (s + 1u) & (kSlots - 1u)) {
                const uint32_t e = atomicCAS(&agg.row[s], RSK_CONN_NONE, row[k]);
                if (e == RSK_CONN_NONE || e == row[k]) {
                    atomicAdd(&agg.cnt[s], carry);
                    break;
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (unsigned q = 0; q < kSlots / kTileBlock; ++q) {
        const uint32_t s = q * kTileBlock + threadIdx.x;
        const uint32_t r = agg.row[s];
        // r is a row some item named (the callers only name rows below the capacity); the bound keeps a
        // corrupted conv_row column from writing outside the counter column
        if (r < capacity) atomicAdd(counter + r, agg.cnt[s]);
    }
}

inline bool msgs_any(const rsk_ctl_msgs &m) {
    return m.cmd || m.body || m.id || m.src || m.avoid_key || m.pay_off || m.pay_len;
}
inline MsgOut msg_out(const rsk_ctl_msgs &m) {
    return MsgOut{m.cmd, m.body, reinterpret_cast<uint64_t *>(m.id), m.src, m.avoid_key, m.pay_off, m.pay_len};
}
inline bool misaligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

// words 32-bit words at p = v, by a kernel: one thread per word.  What a captured chain fills and reads again
// (the resolve's rst_first, the close's marks) is filled this way and not by a memset node: replays of a graph
// were seen to run a byte-pattern memset node of some KB with a stale pattern once other fills had run between
// them (tests/test_gpu_conv_close.py, the captured chains).
static __global__ __launch_bounds__(kTileBlock) void k_fill_words(uint32_t *p, uint32_t words, uint32_t v) {
    const uint32_t g = blockIdx.x * kTileBlock + threadIdx.x;
    if (g < words) gptr(p)[g] = v;
}
inline int fill_words_async(uint32_t *p, uint32_t words, uint32_t v, hipStream_t s) {
    if (words == 0u) return RSK_OK;
    hipLaunchKernelGGL(k_fill_words, dim3((words + kTileBlock - 1u) / kTileBlock), dim3(kTileBlock), 0, s, p, words, v);
    return launch_check("k_fill_words");
}

inline int memset_async(void *p, int v, size_t bytes, hipStream_t s) {
    hipError_t e = hipMemsetAsync(p, v, bytes, s);
    if (e != hipSuccess) { set_error("hipMemsetAsync", e); return RSK_EDEVICE; }
    return RSK_OK;
}

}  // namespace rsk
