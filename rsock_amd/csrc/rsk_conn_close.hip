// rsk_conn_close.hip — rsk_conn_close_batch (include/rsk_codec.h): fake-TCP conns killed and removed on the
// device connection table, the two steps of the reference: INetConn::NotifyErr clears mAlive
// (conn/INetConn.cpp:49-52) and leaves the conn in mConnMap; INetGroup::RemoveConn erases it
// (conn/INetGroup.cpp:94-101, :138-146), from IGroup::Flush for every conn that is not alive
// (conn/IGroup.cpp:81-111) or from doSend for the one it drew.  The conn index leaves a removed row by a rebuild
// over the rows that stay (rsk_conv_close.hip's route); the pick index is kept current by an order-stable
// compaction of its candidates (rsk_pick.h: the work layout and the arithmetic).
//
// A linear chain on the stream; two arrays of per-tile counts and their totals in the control path's scratch:
//   k_fill_words    list form: the marks in `work` (0); a kernel, not a memset node (rsk_tile_dev.h)
//   k_cc_scatter    list form: mark[close_rows[j]] = 1, j < min(*n_close, m_max): plain stores of one value
//   k_cc_count      per 1024-row tile: the rows that lose ALIVE and those that lose LIVE (tile A); with a pick
//                   index the entries of the same 1024 of cand whose row stays a candidate (tile B);
//                   pick_counts as the index has them
//   k_tile_scan x2  their exclusive scans; the totals -> n_marked, n_closed, pick_counts[1] and the last entries
//   k_cc_main       by block range, passes that need the totals and nothing of each other: per row tile
//                   marked_rows / closed_rows in row order; the conn index cleared (something was removed); per
//                   cand tile K, the staying candidates and their groups' old offsets into work, kConnEmpty to
//                   pos of the candidates that go (a row lost ALIVE).  State and both indexes' cand / group
//                   are only read.
//   k_cc_apply      by block range: per row the new state byte, and (something was removed) the insertion of
//                   the rows that stay, k_index_build's rule; per 1024 new positions cand and pos from work;
//                   per group entry {K[off], K[off + cnt] - K[off]} or kPickGone; the header.  work is only read.
// The two last launches leave at once when no row lost ALIVE or LIVE.  No block waits on another, nothing spins,
// no block reads a region of an index that another block of its launch writes; the probe loop is bounded by the
// index's size; no launch walks the rows on one block.
#include <hip/hip_runtime.h>

#include "rsk_pick.h"
#include "rsk_tile_dev.h"

namespace {

using rsk::gptr;
using rsk::k_tile_scan;
using rsk::kConnEmpty;
using rsk::kScanBlock;
using rsk::misaligned8;
using rsk::tile_positions;
using rsk::u32x2;
using rsk::u32x4;

constexpr unsigned kBlock = rsk::kTileBlock;
constexpr unsigned kWaves = rsk::kTileWaves;
constexpr unsigned kRowPer = 4;  // rows, or entries of cand, per thread
static_assert(kBlock * kRowPer == rsk::kFlushTile && rsk::kFlushTile == rsk::kPickTile,
              "scratch size (rsk_ctx.h), work layout (rsk_pick.h) and tile size must agree");
constexpr uint32_t kNoRst = 0xFFFFFFFFu;
constexpr uint32_t kScatterBlocks = 1024;  // grid-stride over close_rows
constexpr uint32_t kAllFlags = RSK_CONN_CLOSE_REMOVE | RSK_CONN_CLOSE_SWEEP;
constexpr uint8_t kUp = RSK_CONN_LIVE | RSK_CONN_ALIVE;
constexpr uint8_t kGone = RSK_CONN_LIVE | RSK_CONN_ALIVE | RSK_CONN_NEW;  // what a removed row loses

struct CloseArgs {
    rsk::DevConnTab t;
    uint8_t *state;
    uint32_t *index;
    const uint8_t *mark;        // list form: [capacity] in work; else NULL
    const uint32_t *rst_first;  // column form: [capacity]; else NULL
    const uint32_t *close_rows, *n_close;
    uint32_t *marked_rows, *closed_rows;
    uint32_t *pick;  // NULL: no pick index
    uint32_t *pick_counts;
    uint32_t *work;
    rsk::PickLayout pl;
    rsk::CloseLayout wl;
    u32x2 *tile_a;  // [tiles + 1] {lose ALIVE, lose LIVE}; the last entry holds the totals behind the scan
    u32x2 *tile_b;  // [tiles + 1] {candidates that stay, 0}
    uint32_t tiles, clear_blocks, row_blocks, slot_blocks;
    uint32_t capacity, slots, c4, m_max;
    bool by_id, remove, sweep;
};

__device__ __forceinline__ bool marked(const CloseArgs &a, uint32_t r) {
    return a.mark ? gptr(a.mark)[r] != 0u : a.rst_first ? gptr(a.rst_first)[r] != kNoRst : false;
}
// The state byte of row r (r < capacity) behind the call, from the one it has.
__device__ __forceinline__ uint8_t next_state(const CloseArgs &a, uint32_t r, uint8_t st) {
    if (!(st & RSK_CONN_LIVE)) return st;
    const bool m = marked(a, r);
    if (m) st = (uint8_t)(st & ~RSK_CONN_ALIVE);
    if ((a.remove && m) || (a.sweep && !(st & RSK_CONN_ALIVE))) st = (uint8_t)(st & ~kGone);
    return st;
}
__device__ __forceinline__ u32x2 totals(const CloseArgs &a) { return gptr(a.tile_a)[a.tiles]; }
// The candidates of the whole table as the index has them, bounded.
__device__ __forceinline__ uint32_t old_total(const CloseArgs &a) {
    const uint32_t t = gptr(a.pick)[0];
    return t < a.capacity ? t : a.capacity;
}
// Entry j of cand (j < the tile range) stays: it is one, and its row is a candidate behind the call.  row = its
// row when that is one of the table, else kConnEmpty.
__device__ __forceinline__ bool entry_stays(const CloseArgs &a, uint32_t j, uint32_t tot0, uint32_t &row) {
    row = kConnEmpty;
    if (j >= tot0) return false;
    const uint32_t r = gptr(a.pick)[a.pl.cand + j];  // j < capacity <= C4
    if (r >= a.capacity) return false;
    row = r;
    return (gptr(a.state)[r] & kUp) == kUp && !marked(a, r);
}

__global__ __launch_bounds__(kBlock) void k_cc_scatter(CloseArgs a, uint8_t *mark) {
    const uint32_t nc = *gptr(a.n_close), m = nc < a.m_max ? nc : a.m_max;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < m; j += gridDim.x * kBlock) {
        const uint32_t r = gptr(a.close_rows)[j];
        if (r < a.capacity) gptr(mark)[r] = (uint8_t)1;  // repeats store the same byte
    }
}

__global__ __launch_bounds__(kBlock) void k_cc_count(CloseArgs a) {
    __shared__ uint32_t red[3][kWaves];
    const uint32_t tot0 = a.pick ? old_total(a) : 0u;
    if (blockIdx.x == 0u && threadIdx.x == 0u && a.pick && a.pick_counts) {
        // what a call that changes nothing reports; k_tile_scan and k_cc_apply, later launches, write over it
        gptr(a.pick_counts)[0] = gptr(a.pick)[1];
        gptr(a.pick_counts)[1] = gptr(a.pick)[0];
    }
    uint32_t na = 0, nl = 0, nk = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kRowPer; ++k) {
        const uint32_t r = blockIdx.x * rsk::kFlushTile + k * kBlock + threadIdx.x;
        uint8_t st = 0, ns = 0;
        if (r < a.capacity) {
            st = gptr(a.state)[r];
            ns = next_state(a, r, st);
        }
        na += (uint32_t)__popcll(__ballot((st ^ ns) & RSK_CONN_ALIVE));
        nl += (uint32_t)__popcll(__ballot((st ^ ns) & RSK_CONN_LIVE));
        uint32_t row;
        nk += (uint32_t)__popcll(__ballot(a.pick && r < a.capacity && entry_stays(a, r, tot0, row)));
    }
    if ((threadIdx.x & 63u) == 0u) {
        red[0][threadIdx.x >> 6] = na;
        red[1][threadIdx.x >> 6] = nl;
        red[2][threadIdx.x >> 6] = nk;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        u32x2 sa = u32x2{0u, 0u}, sb = u32x2{0u, 0u};
#pragma unroll
        for (unsigned w = 0; w < kWaves; ++w) {
            sa.x += red[0][w];
            sa.y += red[1][w];
            sb.x += red[2][w];
        }
        gptr(a.tile_a)[blockIdx.x] = sa;
        gptr(a.tile_b)[blockIdx.x] = sb;
    }
}

// marked_rows / closed_rows of row tile b, order-stable.  Every thread of the block calls it.
__device__ __forceinline__ void cc_lists(const CloseArgs &a, uint32_t b, uint32_t (*cnt)[kWaves]) {
    bool fa[kRowPer], fl[kRowPer];
#pragma unroll
    for (unsigned k = 0; k < kRowPer; ++k) {
        const uint32_t r = b * rsk::kFlushTile + k * kBlock + threadIdx.x;
        uint8_t st = 0, ns = 0;
        if (r < a.capacity) {
            st = gptr(a.state)[r];
            ns = next_state(a, r, st);
        }
        fa[k] = ((st ^ ns) & RSK_CONN_ALIVE) != 0;  // only a marked LIVE row that had the bit loses it
        fl[k] = ((st ^ ns) & RSK_CONN_LIVE) != 0;
    }
    const u32x2 base = gptr(a.tile_a)[b];
    uint32_t pa[kRowPer], pl[kRowPer];
    tile_positions<kRowPer>(fa, base.x, cnt, pa);
    tile_positions<kRowPer>(fl, base.y, cnt + kRowPer, pl);
#pragma unroll
    for (unsigned k = 0; k < kRowPer; ++k) {
        const uint32_t r = b * rsk::kFlushTile + k * kBlock + threadIdx.x;
        // a row makes one entry at most in a list, so a position is below the capacity
        if (fa[k] && a.marked_rows && pa[k] < a.capacity) gptr(a.marked_rows)[pa[k]] = r;
        if (fl[k] && a.closed_rows && pl[k] < a.capacity) gptr(a.closed_rows)[pl[k]] = r;
    }
}

// Tile b of cand: K for its 1024 entries; an entry that stays goes to work at its new position with its group's
// old offset, one that goes gives its row's pos kConnEmpty.  Reads cand and pos, writes pos of the rows whose
// entries it owns, and work.  Every thread of the block calls it.
__device__ __forceinline__ void cc_compact(const CloseArgs &a, uint32_t b, uint32_t (*cnt)[kWaves]) {
    const uint32_t tot0 = old_total(a);
    bool keep[kRowPer];
    uint32_t row[kRowPer];
#pragma unroll
    for (unsigned k = 0; k < kRowPer; ++k) {
        const uint32_t j = b * rsk::kPickTile + k * kBlock + threadIdx.x;
        keep[k] = entry_stays(a, j, tot0, row[k]);
    }
    uint32_t np[kRowPer];
    tile_positions<kRowPer>(keep, gptr(a.tile_b)[b].x, cnt, np);
#pragma unroll
    for (unsigned k = 0; k < kRowPer; ++k) {
        const uint32_t j = b * rsk::kPickTile + k * kBlock + threadIdx.x;  // j < tiles * kPickTile
        gptr(a.work)[a.wl.k + j] = np[k];
        if (row[k] == kConnEmpty) continue;
        if (!keep[k]) {
            gptr(a.pick)[a.pl.pos + row[k]] = kConnEmpty;
        } else if (np[k] < a.c4) {  // at most one kept entry per entry: np <= j
            gptr(a.work)[a.wl.cand + np[k]] = row[k];
            if (a.by_id) {
                const uint32_t p = gptr(a.pick)[a.pl.pos + row[k]];
                gptr(a.work)[a.wl.goff + np[k]] = p <= j ? j - p : kConnEmpty;
            }
        }
    }
}

constexpr unsigned kClearPer = 4;
__global__ __launch_bounds__(kBlock) void k_cc_main(CloseArgs a) {
    __shared__ uint32_t lds[2 * kRowPer][kWaves];
    const u32x2 tot = totals(a);
    if (tot.x == 0u && tot.y == 0u) return;  // uniform over the grid
    uint32_t b = blockIdx.x;
    if (b < a.tiles) return cc_lists(a, b, lds);
    b -= a.tiles;
    if (b < a.clear_blocks) {
        if (tot.y == 0u) return;  // nothing was removed: no byte of the conn index is written
        const u32x4 empty = {kConnEmpty, kConnEmpty, kConnEmpty, kConnEmpty};
#pragma unroll
        for (unsigned k = 0; k < kClearPer; ++k) {
            const uint32_t q = (b * kClearPer + k) * kBlock + threadIdx.x;
            if (q < a.slots / 4u) reinterpret_cast<RSK_GLOBAL u32x4 *>(gptr(a.index))[q] = empty;
        }
        return;
    }
    b -= a.clear_blocks;
    if (tot.x == 0u) return;  // no row lost ALIVE: the candidates are the same
    cc_compact(a, b, lds);    // only launched with a pick index
}

// K[j] for j up to the tiles' end, where it is the total.
__device__ __forceinline__ uint32_t k_at(const CloseArgs &a, uint32_t j, uint32_t total) {
    return j < a.tiles * rsk::kPickTile ? gptr(a.work)[a.wl.k + j] : total;
}

__global__ __launch_bounds__(kBlock) void k_cc_apply(CloseArgs a) {
    const u32x2 tot = totals(a);
    if (tot.x == 0u && tot.y == 0u) return;  // uniform over the grid
    uint32_t b = blockIdx.x;
    if (b < a.row_blocks) {  // rsk_conn_dev.h's k_index_build<1> behind the row's new state
        const uint32_t g = b * kBlock + threadIdx.x;
        if (g >= a.capacity) return;
        const uint8_t st = gptr(a.state)[g], ns = next_state(a, g, st);
        if (ns != st) gptr(a.state)[g] = ns;
        if (tot.y == 0u || !(ns & RSK_CONN_LIVE)) return;
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
        return;
    }
    b -= a.row_blocks;
    if (tot.x == 0u) return;  // the pick index stays as it is; only launched with one from here on
    const uint32_t total = gptr(a.tile_b)[a.tiles].x;  // <= capacity: one per kept entry
    if (b < a.tiles) {
        if (b == 0u && threadIdx.x == 0u) {
            gptr(a.pick)[0] = total;
            if (!a.by_id) {  // with BY_ID the groups that emptied take themselves off below
                gptr(a.pick)[1] = total != 0u;
                if (a.pick_counts) gptr(a.pick_counts)[0] = total != 0u;
            }
        }
#pragma unroll
        for (unsigned k = 0; k < kRowPer; ++k) {
            const uint32_t p = b * rsk::kPickTile + k * kBlock + threadIdx.x;
            if (p >= a.c4) continue;
            uint32_t r = kConnEmpty;
            if (p < total) r = gptr(a.work)[a.wl.cand + p];
            gptr(a.pick)[a.pl.cand + p] = r;
            if (r >= a.capacity) continue;
            uint32_t at = p;
            if (a.by_id) {
                const uint32_t o = gptr(a.work)[a.wl.goff + p];
                const uint32_t ko = o < a.capacity ? k_at(a, o, total) : kConnEmpty;
                at = ko <= p ? p - ko : kConnEmpty;
            }
            gptr(a.pick)[a.pl.pos + r] = at;
        }
        return;
    }
    b -= a.tiles;
    const uint32_t s = b * kBlock + threadIdx.x;  // by_id
    if (s >= a.slots) return;
    RSK_GLOBAL u32x4 *ge = reinterpret_cast<RSK_GLOBAL u32x4 *>(gptr(a.pick + a.pl.group)) + s;
    u32x4 q = *ge;
    // a free entry, one that emptied before, or garbage: left as it is
    if (q.w == 0u || q.z >= a.capacity || q.w > a.capacity - q.z) return;
    const uint32_t k0 = k_at(a, q.z, total), k1 = k_at(a, q.z + q.w, total);
    if (k1 > k0) {
        q.z = k0;
        q.w = k1 - k0;
    } else {
        q.z = rsk::kPickGoneOff;
        q.w = rsk::kPickGoneCnt;
        atomicSub(a.pick + 1, 1u);  // integer adds commute: the word does not depend on the order
        if (a.pick_counts) atomicSub(a.pick_counts, 1u);
    }
    *ge = q;
}

}  // namespace

extern "C" int rsk_conn_close_batch(rsk_ctx *c, const rsk_conn_table *t, const rsk_conn_rows *rows,
                                    const rsk_conn_close_in *in, const rsk_conn_close_out *out, void *stream) {
    if (!c || !rows || !in || !out || !rsk::tab_lookup_ok(t) || !t->state) return RSK_EINVAL;
    if (rows->state != t->state || !in->work) return RSK_EINVAL;
    const bool list = in->close_rows != nullptr, col = in->rst_first != nullptr;
    if ((in->flags & ~kAllFlags) || (list && col) || (!list && !col && !(in->flags & RSK_CONN_CLOSE_SWEEP))) return RSK_EINVAL;
    if (list && !in->n_close) return RSK_EINVAL;
    if ((out->marked_rows && !out->n_marked) || (out->closed_rows && !out->n_closed)) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0;
    if ((reinterpret_cast<uintptr_t>(t->index) | reinterpret_cast<uintptr_t>(in->work) | reinterpret_cast<uintptr_t>(out->pick)) & 15u)
        return RSK_EINVAL;
    if (by_id && misaligned8(t->id)) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    int r;
    CloseArgs a;
    a.t = rsk::dev_tab(t);
    a.state = rows->state;
    a.index = t->index;
    a.mark = list ? static_cast<const uint8_t *>(in->work) : nullptr;
    a.rst_first = in->rst_first;
    a.close_rows = in->close_rows;
    a.n_close = in->n_close;
    a.marked_rows = out->marked_rows;
    a.closed_rows = out->closed_rows;
    a.pick = out->pick;
    a.pick_counts = out->pick ? out->pick_counts : nullptr;
    a.work = static_cast<uint32_t *>(in->work);
    a.pl = rsk::pick_layout(t->capacity, by_id);
    a.wl = rsk::close_layout(t->capacity, by_id);
    a.tiles = a.wl.tiles;
    a.capacity = t->capacity;
    a.slots = rsk::conn_slots(t->capacity);
    a.c4 = (t->capacity + 3u) & ~3u;
    a.m_max = in->m_max;
    a.by_id = by_id;
    a.remove = (in->flags & RSK_CONN_CLOSE_REMOVE) != 0;
    a.sweep = (in->flags & RSK_CONN_CLOSE_SWEEP) != 0;
    a.clear_blocks = (a.slots / 4u + kClearPer * kBlock - 1u) / (kClearPer * kBlock);
    a.row_blocks = (a.capacity + kBlock - 1u) / kBlock;
    a.slot_blocks = a.pick && by_id ? (a.slots + kBlock - 1u) / kBlock : 0u;
    void *wsp = nullptr;  // both arrays fit the scratch of any batch size (control_ws_bytes)
    if ((r = rsk::stream_ws(c, s, rsk::WS_CONTROL, rsk::control_ws_bytes(0), &wsp))) return r;
    a.tile_a = static_cast<u32x2 *>(wsp);
    a.tile_b = a.tile_a + a.tiles + 1u;
    const dim3 blk(kBlock);
    if (list) {
        if ((r = rsk::fill_words_async(a.work, a.wl.k, 0u, s))) return r;
        if (in->m_max) {
            const uint32_t nb = (uint32_t)(((uint64_t)in->m_max + kBlock - 1u) / kBlock);
            hipLaunchKernelGGL(k_cc_scatter, dim3(nb < kScatterBlocks ? nb : kScatterBlocks), blk, 0, s, a,
                               static_cast<uint8_t *>(in->work));
            if ((r = rsk::launch_check("k_cc_scatter"))) return r;
        }
    }
    hipLaunchKernelGGL(k_cc_count, dim3(a.tiles), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cc_count"))) return r;
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile_a, a.tiles, out->n_marked, out->n_closed);
    if ((r = rsk::launch_check("k_tile_scan"))) return r;
    if (a.pick) {
        hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile_b, a.tiles,
                           a.pick_counts ? a.pick_counts + 1 : static_cast<uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr));
        if ((r = rsk::launch_check("k_tile_scan"))) return r;
    }
    // at most 2^10 tiles, 2^9 clear blocks, 2^12 row blocks and 2^13 slot blocks
    hipLaunchKernelGGL(k_cc_main, dim3(a.tiles + a.clear_blocks + (a.pick ? a.tiles : 0u)), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cc_main"))) return r;
    hipLaunchKernelGGL(k_cc_apply, dim3(a.row_blocks + (a.pick ? a.tiles : 0u) + a.slot_blocks), blk, 0, s, a);
    return rsk::launch_check("k_cc_apply");
}
