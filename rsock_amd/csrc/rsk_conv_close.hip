// rsk_conv_close.hip — rsk_conv_close_batch (include/rsk_codec.h): convs closed on the device table, in the
// two places the reference closes one: IGroup::Flush -> CloseConn for the convs that went quiet
// (conn/IGroup.cpp:81-107, :126-137; the timer form, behind rsk_conv_flush's dead_rows) and
// ConnReset::OnRecvConvRst -> CloseConn inside the packet walk (callbacks/ConnReset.cpp:67-77; the receive form,
// behind the resolve's rst_first), after which a DATA packet of the same key gets a new SConn
// (server/SubGroup.cpp:31-68): here its conv_row goes back to NONE / unknown for the next create.
//
// The index is open addressing without tombstones, so a row leaves it by a rebuild over the rows that stay; both
// sources of the rows to close already cost a pass over the capacity.
//
// A linear chain on the stream; the per-tile counts and the closed total in the control path's scratch:
//   k_fill_words    timer form: the mark in `work` (0); a kernel, not a memset node (rsk_tile_dev.h)
//   k_cl_scatter    timer form: mark[close_rows[j]] = 1, j < min(*n_close, m_max): plain stores of one value
//   k_cl_count      per 1024-row tile, the rows that are LIVE and marked; n_reopened, n_rst_again = 0
//   k_tile_scan     their exclusive scan; the total -> n_closed and tile[tiles]
//   k_cl_main       three passes that need the total and nothing of each other, in one launch by block range:
//                   receive form, per 2048-packet tile: the packets behind their row's reset go back to NONE (the
//                   rst_first gather is the only scattered read of a packet that is not in such a tail); per
//                   1024-row tile: closed_rows / closed_at in row order; the index cleared
//   k_cl_insert     per row: one that closes loses LIVE (unless HOLD), every other LIVE row is inserted,
//                   k_index_build's rule
// The two kernels behind the scan leave at once when the total is 0: a batch without a hitting reset, or a tick
// without a dead conv, pays the row count and two empty launches, and no byte of the index is written.
// No block waits on another and nothing spins; the probe loop is bounded by the index's size.
#include <hip/hip_runtime.h>

#include "rsk_tile_dev.h"

namespace {

using rsk::gptr;
using rsk::k_tile_scan;
using rsk::kConnEmpty;
using rsk::kScanBlock;
using rsk::misaligned8;
using rsk::tile_positions;
using rsk::u32x2;

constexpr unsigned kBlock = rsk::kTileBlock;
constexpr unsigned kWaves = rsk::kTileWaves;
constexpr unsigned kPer = 8;     // packets per thread: the resolve's tile
constexpr unsigned kRowPer = 4;  // rows per thread: the flush's tile
static_assert(kBlock * kPer == rsk::kControlTile && kBlock * kRowPer == rsk::kFlushTile,
              "scratch size (rsk_ctx.h) and tile sizes must agree");
constexpr uint32_t kFlags = RSK_CONV_BY_DST | RSK_CONV_BY_ID;
constexpr uint32_t kNoRst = 0xFFFFFFFFu;
constexpr uint32_t kScatterBlocks = 1024;  // grid-stride over close_rows

// The table as k_cl_insert reads a row's key (rsk_conv.hip's accessor).
struct DevConvTab {
    const uint32_t *conv;
    const uint32_t *dst;
    const uint64_t *ids;
    bool by_dst;
    __device__ __forceinline__ uint64_t key(uint32_t row) const {
        const uint64_t c = gptr(conv)[row];
        return by_dst ? ((uint64_t)gptr(dst)[row] << 32) | c : c;
    }
    __device__ __forceinline__ uint64_t id(uint32_t row) const { return gptr(ids)[row]; }
};

struct CloseArgs {
    DevConvTab t;
    uint8_t *state;
    uint32_t *index;
    uint8_t *mark;              // timer form: [capacity] in work; NULL in the receive form
    const uint32_t *rst_first;  // receive form: [capacity]; NULL in the timer form
    const uint32_t *close_rows, *n_close;
    const uint8_t *ctl_kind;
    uint32_t *conv_row;
    int8_t *unknown;
    uint32_t *n_unknown, *closed_rows, *closed_at, *n_reopened, *n_rst_again;
    u32x2 *tile;  // [row tiles + 1]; the last entry holds the closed total behind the scan
    uint32_t row_tiles, pkt_tiles;  // pkt_tiles: 0 in the timer form
    uint32_t n, capacity, slots, m_max;
    bool by_id, hold;
};

// Row r (r < capacity) closes: LIVE and marked.
__device__ __forceinline__ bool closes(const CloseArgs &a, uint32_t r) {
    if (!(gptr(a.state)[r] & RSK_CONN_LIVE)) return false;
    return a.mark ? gptr(a.mark)[r] != 0u : gptr(a.rst_first)[r] != kNoRst;
}
__device__ __forceinline__ uint32_t closed_total(const CloseArgs &a) { return gptr(a.tile)[a.row_tiles].x; }

__global__ __launch_bounds__(kBlock) void k_cl_scatter(CloseArgs a) {
    const uint32_t nc = *gptr(a.n_close), m = nc < a.m_max ? nc : a.m_max;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < m; j += gridDim.x * kBlock) {
        const uint32_t r = gptr(a.close_rows)[j];
        if (r < a.capacity) gptr(a.mark)[r] = (uint8_t)1;  // repeats store the same byte
    }
}

__global__ __launch_bounds__(kBlock) void k_cl_count(CloseArgs a) {
    __shared__ uint32_t red[2][kWaves];
    if (blockIdx.x == 0u && threadIdx.x == 0u) {  // written, not accumulated: k_cl_main, a later launch, adds
        if (a.n_reopened) *gptr(a.n_reopened) = 0u;
        if (a.n_rst_again) *gptr(a.n_rst_again) = 0u;
    }
    uint32_t c = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kRowPer; ++k) {
        const uint32_t r = blockIdx.x * rsk::kFlushTile + k * kBlock + threadIdx.x;
        c += (uint32_t)__popcll(__ballot(r < a.capacity && closes(a, r)));
    }
    rsk::tile_store_counts(a.tile, c, c, red);
}

// The packets of tile b: those behind their row's reset go back to NONE.  Every thread of the block calls it.
__device__ __forceinline__ void cl_packets(const CloseArgs &a, uint32_t b, uint32_t (*red)[kWaves]) {
    const uint64_t base = (uint64_t)b * rsk::kControlTile + threadIdx.x;
    uint32_t r[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        r[k] = i < a.n ? gptr(a.conv_row)[i] : (uint32_t)RSK_CONN_NONE;
    }
    uint32_t at[kPer];  // the gathers, independent loads
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) at[k] = r[k] < a.capacity ? gptr(a.rst_first)[r[k]] : kNoRst;
    uint32_t n_re = 0, n_again = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        // behind its row's reset, and the row closes (k_cl_insert, which clears LIVE, is a later launch)
        const bool tail = at[k] != kNoRst && i > at[k] && (gptr(a.state)[r[k]] & RSK_CONN_LIVE);
        bool rst = false;
        if (tail) {
            rst = gptr(a.ctl_kind)[i] == RSK_CTL_CONV_RST;
            gptr(a.conv_row)[i] = RSK_CONN_NONE;
            if (!rst && a.unknown) gptr(a.unknown)[i] = (int8_t)RSK_RECV_VALID;
        }
        n_re += (uint32_t)__popcll(__ballot(tail && !rst));
        n_again += (uint32_t)__popcll(__ballot(tail && rst));
    }
    if ((threadIdx.x & 63u) == 0u) {
        red[0][threadIdx.x >> 6] = n_re;
        red[1][threadIdx.x >> 6] = n_again;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {  // k_cl_count zeroed the two counts (n_unknown is the caller's); atomics per block
        uint32_t re = 0, again = 0;
#pragma unroll
        for (unsigned w = 0; w < kWaves; ++w) {
            re += red[0][w];
            again += red[1][w];
        }
        if (re && a.n_reopened) atomicAdd(a.n_reopened, re);
        if (re && a.n_unknown) atomicAdd(a.n_unknown, re);
        if (again && a.n_rst_again) atomicAdd(a.n_rst_again, again);
    }
}

// The closing rows of row tile b into closed_rows / closed_at, order-stable.  Every thread of the block calls it.
__device__ __forceinline__ void cl_rows(const CloseArgs &a, uint32_t b, uint32_t (*cnt)[kWaves]) {
    bool cl[kRowPer];
#pragma unroll
    for (unsigned k = 0; k < kRowPer; ++k) {
        const uint32_t r = b * rsk::kFlushTile + k * kBlock + threadIdx.x;
        cl[k] = r < a.capacity && closes(a, r);
    }
    uint32_t pos[kRowPer];
    if (tile_positions<kRowPer>(cl, gptr(a.tile)[b].x, cnt, pos) == 0u) return;
#pragma unroll
    for (unsigned k = 0; k < kRowPer; ++k) {
        const uint32_t r = b * rsk::kFlushTile + k * kBlock + threadIdx.x;
        // a row makes one entry at most, so a position is below the capacity
        if (!cl[k] || pos[k] >= a.capacity) continue;
        if (a.closed_rows) gptr(a.closed_rows)[pos[k]] = r;
        if (a.closed_at) gptr(a.closed_at)[pos[k]] = a.mark ? kNoRst : gptr(a.rst_first)[r];
    }
}

// One launch for the three passes that need the closed total and nothing of each other: blocks [0, pkt_tiles)
// take the packet tiles, the next row_tiles blocks the row tiles, the rest clear the index (kClearPer 16-B stores
// per thread; slots is a multiple of 4 and the index 16-B aligned).  None of them writes state.
constexpr unsigned kClearPer = 4;
__global__ __launch_bounds__(kBlock) void k_cl_main(CloseArgs a) {
    __shared__ uint32_t lds[kRowPer][kWaves];
    static_assert(kRowPer >= 2, "cl_packets takes two rows of it");
    if (closed_total(a) == 0u) return;  // uniform over the grid
    uint32_t b = blockIdx.x;
    if (b < a.pkt_tiles) return cl_packets(a, b, lds);
    b -= a.pkt_tiles;
    if (b < a.row_tiles) return cl_rows(a, b, lds);
    b -= a.row_tiles;
    const rsk::u32x4 empty = {kConnEmpty, kConnEmpty, kConnEmpty, kConnEmpty};
#pragma unroll
    for (unsigned k = 0; k < kClearPer; ++k) {
        const uint32_t q = (b * kClearPer + k) * kBlock + threadIdx.x;
        if (q < a.slots / 4u) reinterpret_cast<RSK_GLOBAL rsk::u32x4 *>(gptr(a.index))[q] = empty;
    }
}

// rsk_conn_dev.h's k_index_build<1> with the closed total in front: a row that closes loses LIVE (unless HOLD)
// and stays out; every other LIVE row is inserted.
__global__ __launch_bounds__(kBlock) void k_cl_insert(CloseArgs a) {
    if (closed_total(a) == 0u) return;  // uniform over the grid
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= a.capacity) return;
    const uint8_t st = gptr(a.state)[g];
    if (!(st & RSK_CONN_LIVE)) return;
    if (a.mark ? gptr(a.mark)[g] != 0u : gptr(a.rst_first)[g] != kNoRst) {
        if (!a.hold) gptr(a.state)[g] = (uint8_t)(st & ~RSK_CONN_LIVE);  // HOLD: LIVE in state, gone from the index
        return;
    }
    const uint64_t key = a.t.key(g), id = a.by_id ? a.t.id(g) : 0ull;
    uint32_t s = rsk::conn_home(key, id, a.slots);
    // at most `capacity` entries are ever taken and slots >= 2 capacity: a free entry is met within `slots`
    // steps; the bound only keeps a corrupted launch from spinning
    for (uint32_t step = 0; step < a.slots; ++step, s = rsk::conn_next(s, a.slots)) {
        const uint32_t e = atomicCAS(a.index + s, kConnEmpty, g);
        if (e == kConnEmpty) break;
        if (e < a.capacity && a.t.key(e) == key && (!a.by_id || a.t.id(e) == id)) {
            atomicMin(a.index + s, g);  // the lowest row of a key wins
            break;
        }
    }
}

bool ctab_lookup_ok(const rsk_conv_table *t) {
    return t && !(t->flags & ~kFlags) && t->capacity >= 1u && t->capacity <= RSK_CONN_MAX_ROWS && t->state && t->conv &&
           t->index && (!(t->flags & RSK_CONV_BY_DST) || t->dst) && (!(t->flags & RSK_CONV_BY_ID) || t->id);
}

}  // namespace

extern "C" int rsk_conv_close_batch(rsk_ctx *c, const rsk_conv_table *t, const rsk_conv_rows *rows, uint32_t n,
                                    const rsk_conv_close_in *in, const rsk_conv_close_out *out, void *stream) {
    if (!c || !rows || !in || !out || !ctab_lookup_ok(t)) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONV_BY_ID) != 0, by_dst = (t->flags & RSK_CONV_BY_DST) != 0;
    if (rows->state != t->state || rows->conv != t->conv || (by_dst && rows->dst != t->dst) || (by_id && rows->id != t->id))
        return RSK_EINVAL;
    const bool timer = in->close_rows != nullptr, recv = in->rst_first != nullptr;
    if (timer == recv || (in->flags & ~RSK_CONV_CLOSE_HOLD)) return RSK_EINVAL;
    const bool hold = (in->flags & RSK_CONV_CLOSE_HOLD) != 0;
    if (timer && (!in->n_close || !in->work || n != 0u || hold || in->ctl_kind)) return RSK_EINVAL;
    if (recv && (in->n_close || (n && (!in->ctl_kind || !out->conv_row)))) return RSK_EINVAL;
    if ((out->closed_rows || out->closed_at) && !out->n_closed) return RSK_EINVAL;
    if ((reinterpret_cast<uintptr_t>(t->index) & 15u) || (by_id && misaligned8(t->id))) return RSK_EINVAL;
    if (timer && (reinterpret_cast<uintptr_t>(in->work) & 15u)) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    int r;
    CloseArgs a;
    a.t = DevConvTab{t->conv, t->dst, reinterpret_cast<const uint64_t *>(t->id), by_dst};
    a.state = rows->state;
    a.index = t->index;
    a.mark = timer ? static_cast<uint8_t *>(in->work) : nullptr;
    a.rst_first = in->rst_first;
    a.close_rows = in->close_rows;
    a.n_close = in->n_close;
    a.ctl_kind = in->ctl_kind;
    a.conv_row = out->conv_row;
    a.unknown = out->unknown;
    a.n_unknown = out->n_unknown;
    a.closed_rows = out->closed_rows;
    a.closed_at = out->closed_at;
    a.n_reopened = out->n_reopened;
    a.n_rst_again = out->n_rst_again;
    a.row_tiles = (t->capacity + rsk::kFlushTile - 1u) / rsk::kFlushTile;
    a.pkt_tiles = recv ? (uint32_t)(((uint64_t)n + rsk::kControlTile - 1u) / rsk::kControlTile) : 0u;
    a.n = n;
    a.capacity = t->capacity;
    a.slots = rsk::conn_slots(t->capacity);
    a.m_max = in->m_max;
    a.by_id = by_id;
    a.hold = hold;
    void *wsp = nullptr;  // the row tiles fit the scratch of any batch size (control_ws_bytes)
    if ((r = rsk::stream_ws(c, s, rsk::WS_CONTROL, rsk::control_ws_bytes(n), &wsp))) return r;
    a.tile = static_cast<u32x2 *>(wsp);
    const dim3 blk(kBlock);
    if (timer) {
        if ((r = rsk::fill_words_async(static_cast<uint32_t *>(in->work), ((t->capacity + 15u) & ~15u) / 4u, 0u, s))) return r;
        if (in->m_max) {
            const uint32_t nb = (uint32_t)(((uint64_t)in->m_max + kBlock - 1u) / kBlock);
            hipLaunchKernelGGL(k_cl_scatter, dim3(nb < kScatterBlocks ? nb : kScatterBlocks), blk, 0, s, a);
            if ((r = rsk::launch_check("k_cl_scatter"))) return r;
        }
    }
    hipLaunchKernelGGL(k_cl_count, dim3(a.row_tiles), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cl_count"))) return r;
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile, a.row_tiles, out->n_closed,
                       static_cast<uint32_t *>(nullptr));
    if ((r = rsk::launch_check("k_tile_scan"))) return r;
    const uint32_t clear_blocks = (a.slots / 4u + kClearPer * kBlock - 1u) / (kClearPer * kBlock);
    // at most 2^21 packet tiles, 2^10 row tiles and 2^9 clear blocks
    hipLaunchKernelGGL(k_cl_main, dim3(a.pkt_tiles + a.row_tiles + clear_blocks), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cl_main"))) return r;
    hipLaunchKernelGGL(k_cl_insert, dim3((a.capacity + kBlock - 1u) / kBlock), blk, 0, s, a);
    return rsk::launch_check("k_cl_insert");
}
