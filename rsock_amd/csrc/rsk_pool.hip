// rsk_pool.hip — the tuple pool (include/rsk_codec.h): TcpAckPool::mInfoPool and ServerNetManager::mPool kept on
// the device, and the four calls that take the host out of the chain parse -> add -> offers -> resolve ->
// conn_create -> recv_ack -> settle and out of the timer's flush.  The index is rsk_conn.h's, keyed by the 4-tuple
// as the create's offers are (rsk_conn_create.h: tuple_key, tuple_ports); open addressing without tombstones, so
// rows arrive by compare-and-swap in place and leave by a rebuild over the rows that stay.
//
// Each call is a linear chain on the stream; per-tile counts in the control path's scratch.
// rsk_pool_add_batch, rsk_conv_create_batch's shape on the same work layout (rsk_conv_create.h):
//   k_pa_count      per 2048-row tile: the considered rows with both ports, and those with a zero port
//   k_tile_scan     their exclusive scans; the totals -> hdr[unknown], hdr[zero port] / *n_zero_port
//   k_pa_list       list[p] = the p-th considered row, p < min(u_max, n); the dedup table cleared
//   k_pa_dedup      a row whose tuple is LIVE in the pool is done (TOUCH: its expiry moves); the others go into
//                   the dedup table, atomicMin leaves the lowest position of a tuple; the candidates' ballots -> mask
//   k_pa_count2     tile b: (first arrivals in list tile b, vacant rows in row tile b); the ballots -> mask
//   k_tile_scan     both scans; the totals -> hdr[keys], hdr[vacant]
//   k_pa_rank       first[j], vacant[j]
//   k_pa_rows       the row columns, new_rows / new_first, the counts
//   k_pa_insert     the new rows into the index: a launch of its own, so the columns are complete before an entry
//                   names them
//   k_pa_assign     row[i], when asked for
// rsk_pool_offers:       k_po_count (per 1024-row tile of the ack pool, the rows that match) -> k_tile_scan -> k_po_emit
// rsk_pool_settle_batch: k_fill_words (the marks) -> k_ps_take (a) -> k_ps_purge (b) -> k_pl_count -> k_tile_scan
//                        per pool -> k_pl_main (closed_sock_rows, the indexes cleared) -> k_pl_insert
// rsk_pool_flush:        k_pl_count -> k_tile_scan -> k_pl_main (dead_rows, the index cleared) -> k_pl_insert
// The k_pl_* kernels serve one or two pools by block range; a pool that loses no row has its blocks leave at once
// and no byte of its index written.  No block waits on another and nothing spins.
#include <hip/hip_runtime.h>

#include "rsk_pool.h"
#include "rsk_tile_dev.h"

namespace {

using rsk::gptr;
using rsk::k_tile_scan;
using rsk::kConnEmpty;
using rsk::kScanBlock;
using rsk::tile_positions;
using rsk::u32x2;

constexpr unsigned kBlock = rsk::kTileBlock;
constexpr unsigned kWaves = rsk::kTileWaves;
constexpr unsigned kPer = 8;     // packets per thread: the resolve's tile
constexpr unsigned kRowPer = 4;  // rows per thread: the flush's tile
constexpr uint32_t kTile = kBlock * kPer;
static_assert(kTile == rsk::kControlTile && kBlock * kRowPer == rsk::kFlushTile, "scratch size (rsk_ctx.h) and tile sizes must agree");
static_assert(2u * (RSK_CONN_MAX_ROWS / rsk::kFlushTile + 1u) <= rsk::control_ws_bytes(0) / sizeof(u32x2),
              "two pools' row tiles and totals fit the control scratch of any batch size");
constexpr uint32_t kGridStride = 1024;  // blocks of a grid-stride pass over a list

// The pool as rsk_conn.h's conn_lookup takes it, and its columns.
struct DevPool {
    uint8_t *state;
    uint32_t *src, *dst;
    uint16_t *sp, *dp;
    uint32_t *seq, *ack;
    uint64_t *expiry;
    uint32_t *index;
    uint32_t capacity, slots;
    __device__ __forceinline__ uint32_t entry(uint32_t s) const { return gptr(index)[s]; }
    __device__ __forceinline__ uint64_t key(uint32_t row) const { return rsk::tuple_key(gptr(src)[row], gptr(dst)[row]); }
    __device__ __forceinline__ uint64_t id(uint32_t row) const { return rsk::tuple_ports(gptr(sp)[row], gptr(dp)[row]); }
    __device__ __forceinline__ bool live(uint32_t row) const { return (gptr(state)[row] & RSK_POOL_LIVE) != 0; }
};

DevPool dev_pool(const rsk_pool *p) {
    return DevPool{p->state, p->src, p->dst, p->sp, p->dp, p->seq, p->ack, p->expiry, p->index, p->capacity,
                   rsk::conn_slots(p->capacity)};
}

// The LIVE row of a tuple, or RSK_CONN_NONE.  An index that was never built may name a row that is not LIVE.
__device__ __forceinline__ uint32_t pool_find(const DevPool &p, uint64_t key, uint64_t ports) {
    const uint32_t r = rsk::conn_lookup(p, p.capacity, true, key, ports);
    return r < p.capacity && p.live(r) ? r : (uint32_t)RSK_CONN_NONE;
}

// k_index_build<1>'s rule for row g of pool p (the entry was free, or holds the lowest row of the tuple).
__device__ __forceinline__ void pool_insert(const DevPool &p, uint32_t g) {
    const uint64_t key = p.key(g), id = p.id(g);
    uint32_t s = rsk::conn_home(key, id, p.slots);
    // at most `capacity` entries are ever taken and slots >= 2 capacity: a free entry is met within `slots` steps;
    // the bound only keeps a corrupted launch from spinning
    for (uint32_t step = 0; step < p.slots; ++step, s = rsk::conn_next(s, p.slots)) {
        const uint32_t e = atomicCAS(p.index + s, kConnEmpty, g);
        if (e == kConnEmpty) break;
        if (e < p.capacity && p.key(e) == key && p.id(e) == id) {
            atomicMin(p.index + s, g);  // the lowest row of a tuple wins
            break;
        }
    }
}

// ---- add ---------------------------------------------------------------------------------------------------
struct AddArgs {
    DevPool p;
    const uint32_t *src, *dst;
    const uint16_t *sp, *dp;
    const uint32_t *seq, *ack;
    const int8_t *status;
    uint64_t expiry;
    uint32_t *row, *new_rows, *new_first, *n_new, *n_again, *n_full;
    uint32_t *hdr, *dedup, *list, *first, *vacant;  // work
    uint64_t *mask;                                 // work
    u32x2 *tile;
    uint32_t n;
    uint32_t u;  // min(u_max, n): entries of list
    uint32_t m;  // min(u_max, capacity): entries of first, vacant, new_rows, new_first
    bool touch;
};

__device__ __forceinline__ bool considered_row(const AddArgs &a, uint64_t i) {
    return i < a.n && (!a.status || gptr(a.status)[i] == (int8_t)RSK_PARSE_SYN);
}
__device__ __forceinline__ bool ports_ok(const AddArgs &a, uint64_t i) { return gptr(a.sp)[i] != 0u && gptr(a.dp)[i] != 0u; }
__device__ __forceinline__ uint64_t in_key(const AddArgs &a, uint64_t i) { return rsk::tuple_key(gptr(a.src)[i], gptr(a.dst)[i]); }
__device__ __forceinline__ uint64_t in_ports(const AddArgs &a, uint64_t i) { return rsk::tuple_ports(gptr(a.sp)[i], gptr(a.dp)[i]); }
// entries of list in use: hdr[unknown] was written by the scan before this launch
__device__ __forceinline__ uint32_t list_len(const AddArgs &a) {
    const uint32_t c = gptr(a.hdr)[rsk::kCreateUnknown];
    return c < a.u ? c : a.u;
}
// entries of the dedup table in use: create_slots (rsk_conv_create.h) of the listed rows, mcons >= 1
__device__ __forceinline__ uint32_t dedup_slots(uint32_t mcons) { return rsk::create_slots(mcons); }

__global__ __launch_bounds__(kBlock) void k_pa_count(AddArgs a) {
    __shared__ uint32_t red[2][kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    uint32_t c = 0, z = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        const bool cons = considered_row(a, i);
        const bool ok = cons && ports_ok(a, i);
        c += (uint32_t)__popcll(__ballot(ok));
        z += (uint32_t)__popcll(__ballot(cons && !ok));
    }
    rsk::tile_store_counts(a.tile, c, z, red);
}

__global__ __launch_bounds__(kBlock) void k_pa_list(AddArgs a) {
    __shared__ uint32_t cnt[kPer][kWaves];
    const uint32_t mcons = list_len(a);
    if (mcons == 0u) return;  // uniform over the grid
    {  // this block's share of the clear: 16-B stores, grid-stride (dedup is 16-B aligned, the slots a multiple of 4)
        const rsk::u32x4 empty = {kConnEmpty, kConnEmpty, kConnEmpty, kConnEmpty};
        const uint32_t quads = dedup_slots(mcons) / 4u;
        for (uint32_t q = blockIdx.x * kBlock + threadIdx.x; q < quads; q += gridDim.x * kBlock)
            reinterpret_cast<RSK_GLOBAL rsk::u32x4 *>(gptr(a.dedup))[q] = empty;
    }
    const uint32_t tbase = gptr(a.tile)[blockIdx.x].x;
    if (tbase >= a.u) return;  // uniform over the block: nothing of this tile is listed
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    bool sel[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        sel[k] = considered_row(a, i) && ports_ok(a, i);
    }
    uint32_t pos[kPer];
    if (tile_positions<kPer>(sel, tbase, cnt, pos) == 0u) return;
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k)
        if (sel[k] && pos[k] < a.u) gptr(a.list)[pos[k]] = (uint32_t)(base + k * kBlock);
}

// The entry of a tuple in the dedup table after k_pa_dedup: the lowest list position of the tuple among the rows
// that went in, or kConnEmpty.
__device__ __forceinline__ uint32_t dedup_find(const AddArgs &a, uint32_t mcons, uint64_t key, uint64_t ports) {
    const uint32_t dslots = dedup_slots(mcons);
    uint32_t s = rsk::conn_home(key, ports, dslots);
    for (uint32_t step = 0; step < dslots; ++step, s = rsk::conn_next(s, dslots)) {
        const uint32_t e = gptr(a.dedup)[s];
        if (e >= mcons) break;
        const uint32_t j = gptr(a.list)[e];
        if (j < a.n && in_key(a, j) == key && in_ports(a, j) == ports) return e;
    }
    return kConnEmpty;
}

__global__ __launch_bounds__(kBlock) void k_pa_dedup(AddArgs a) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x, mcons = list_len(a);
    const uint32_t i = p < mcons ? gptr(a.list)[p] : (uint32_t)RSK_CONN_NONE;
    bool cand = false;  // p held its tuple's entry at some time: only such a position can be the first arrival
    if (i < a.n) {      // list[p] is a row of the input: k_pa_list wrote it
        const uint64_t key = in_key(a, i), ports = in_ports(a, i);
        const uint32_t r = pool_find(a.p, key, ports);  // the index as it was found: k_pa_insert is a later launch
        if (r != RSK_CONN_NONE) {
            // the first handshake wins; every lane of one row stores the same value
            if (a.touch) gptr(a.p.expiry)[r] = a.expiry;
        } else {
            const uint32_t dslots = dedup_slots(mcons);
            uint32_t s = rsk::conn_home(key, ports, dslots);
            // at most mcons positions are inserted and dslots >= 2 mcons: a free entry is met; the bound only keeps
            // a corrupted launch from spinning
            for (uint32_t step = 0; step < dslots; ++step, s = rsk::conn_next(s, dslots)) {
                // a plain load first: an entry only ever falls and never changes its tuple, so a stale value is at
                // worst too high (or still free) and costs an atomic that changes nothing
                uint32_t e = gptr(a.dedup)[s];
                if (e == kConnEmpty) e = atomicCAS(a.dedup + s, kConnEmpty, p);
                if (e == kConnEmpty) {
                    cand = true;
                    break;
                }
                if (e < mcons) {
                    const uint32_t j = gptr(a.list)[e];
                    if (j < a.n && in_key(a, j) == key && in_ports(a, j) == ports) {
                        if (p < e) {
                            atomicMin(a.dedup + s, p);
                            cand = true;
                        }
                        break;
                    }
                }
            }
        }
    }
    // the wave's 64 positions are one word of the mask: the candidates, for k_pa_count2 to probe
    const uint64_t cb = __ballot(cand);
    if ((threadIdx.x & 63u) == 0u && p < mcons) gptr(a.mask)[p >> 6] = cb;
}

__device__ __forceinline__ bool is_first(const AddArgs &a, uint32_t mcons, uint64_t p) {
    if (p >= mcons) return false;
    const uint32_t i = gptr(a.list)[p];
    if (i >= a.n) return false;
    return dedup_find(a, mcons, in_key(a, i), in_ports(a, i)) == (uint32_t)p;
}
__device__ __forceinline__ bool is_vacant(const AddArgs &a, uint32_t mcons, uint64_t r) {
    return mcons != 0u && r < a.p.capacity && !a.p.live((uint32_t)r);
}

__global__ __launch_bounds__(kBlock) void k_pa_count2(AddArgs a) {
    __shared__ uint32_t red[2][kWaves];
    const uint32_t mcons = list_len(a);
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    uint32_t nf = 0, nv = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t x = base + k * kBlock;
        // the wave's 64 positions are one word of the mask, read (k_pa_dedup's candidates) and stored (the first
        // arrivals among them) by this wave alone, while it holds a listed position
        const bool held = x - (threadIdx.x & 63u) < mcons;
        const uint64_t cb = held ? gptr(a.mask)[x >> 6] : 0ull;
        const uint64_t fb = __ballot(((cb >> (threadIdx.x & 63u)) & 1ull) != 0ull && is_first(a, mcons, x));
        if ((threadIdx.x & 63u) == 0u && held) gptr(a.mask)[x >> 6] = fb;
        nf += (uint32_t)__popcll(fb);
        nv += (uint32_t)__popcll(__ballot(is_vacant(a, mcons, x)));
    }
    rsk::tile_store_counts(a.tile, nf, nv, red);
}

__global__ __launch_bounds__(kBlock) void k_pa_rank(AddArgs a) {
    __shared__ uint32_t cnt_f[kPer][kWaves], cnt_v[kPer][kWaves];
    const uint32_t mcons = list_len(a);
    if (mcons == 0u) return;  // uniform over the grid
    const u32x2 tb = gptr(a.tile)[blockIdx.x];
    if (tb.x >= a.m && tb.y >= a.m) return;  // uniform over the block: nothing of this tile is stored
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    bool f[kPer], v[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t x = base + k * kBlock;
        f[k] = x < mcons && ((gptr(a.mask)[x >> 6] >> (threadIdx.x & 63u)) & 1ull) != 0ull;
        v[k] = is_vacant(a, mcons, x);
    }
    uint32_t pf[kPer], pv[kPer];
    tile_positions<kPer>(f, tb.x, cnt_f, pf);
    tile_positions<kPer>(v, tb.y, cnt_v, pv);
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t x = base + k * kBlock;
        if (f[k] && pf[k] < a.m) gptr(a.first)[pf[k]] = gptr(a.list)[x];
        if (v[k] && pv[k] < a.m) gptr(a.vacant)[pv[k]] = (uint32_t)x;
    }
}

// keys <= listed <= u and vacant <= capacity: the minimum is at most m, the entries of first / vacant
__device__ __forceinline__ uint32_t added(const AddArgs &a) {
    const uint32_t k = gptr(a.hdr)[rsk::kCreateKeys], v = gptr(a.hdr)[rsk::kCreateVacant];
    const uint32_t c = k < v ? k : v;
    return c < a.m ? c : a.m;
}

__global__ __launch_bounds__(kBlock) void k_pa_rows(AddArgs a) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t mcons = list_len(a);
    const uint32_t nn = mcons ? added(a) : 0u;
    if (j == 0u) {
        const uint32_t keys = mcons ? gptr(a.hdr)[rsk::kCreateKeys] : 0u;
        if (a.n_new) *gptr(a.n_new) = nn;
        if (a.n_full) *gptr(a.n_full) = keys - nn;
        if (a.n_again) *gptr(a.n_again) = mcons - (keys < mcons ? keys : mcons);
    }
    if (j >= nn) return;
    const uint32_t r = gptr(a.vacant)[j], i = gptr(a.first)[j];
    if (r >= a.p.capacity || i >= a.n) return;  // k_pa_rank wrote a row and an input row
    gptr(a.p.src)[r] = gptr(a.src)[i];
    gptr(a.p.dst)[r] = gptr(a.dst)[i];
    gptr(a.p.sp)[r] = gptr(a.sp)[i];
    gptr(a.p.dp)[r] = gptr(a.dp)[i];
    if (a.p.seq) gptr(a.p.seq)[r] = gptr(a.seq)[i];
    if (a.p.ack) gptr(a.p.ack)[r] = gptr(a.ack)[i];
    gptr(a.p.expiry)[r] = a.expiry;
    gptr(a.p.state)[r] = (uint8_t)RSK_POOL_LIVE;
    if (a.new_rows) gptr(a.new_rows)[j] = r;
    if (a.new_first) gptr(a.new_first)[j] = i;
}

__global__ __launch_bounds__(kBlock) void k_pa_insert(AddArgs a) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (list_len(a) == 0u || j >= added(a)) return;
    const uint32_t r = gptr(a.vacant)[j];
    if (r >= a.p.capacity) return;
    pool_insert(a.p, r);
}

__global__ __launch_bounds__(kBlock) void k_pa_assign(AddArgs a) {
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        if (i >= a.n) continue;
        uint32_t r = RSK_CONN_NONE;
        if (considered_row(a, i) && ports_ok(a, i)) r = pool_find(a.p, in_key(a, i), in_ports(a, i));
        gptr(a.row)[i] = r;
    }
}

// ---- offers ------------------------------------------------------------------------------------------------
struct OffersArgs {
    DevPool pa, ps;
    uint32_t *src, *dst;
    uint16_t *sp, *dp;
    uint32_t *ack;
    uint8_t *flag;
    uint64_t *conn_key;
    uint32_t *n_offer, *ack_row, *sock_row, *n_over;
    u32x2 *tile;
    uint32_t row_tiles, m_max;
};

// The socket row of ack-pool row r's tuple, or RSK_CONN_NONE (also for a row that is not LIVE).
__device__ __forceinline__ uint32_t offer_match(const OffersArgs &a, uint32_t r) {
    if (r >= a.pa.capacity || !a.pa.live(r)) return RSK_CONN_NONE;
    return pool_find(a.ps, a.pa.key(r), a.pa.id(r));
}

__global__ __launch_bounds__(kBlock) void k_po_count(OffersArgs a) {
    __shared__ uint32_t red[2][kWaves];
    uint32_t c = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kRowPer; ++k) {
        const uint32_t r = blockIdx.x * rsk::kFlushTile + k * kBlock + threadIdx.x;
        c += (uint32_t)__popcll(__ballot(offer_match(a, r) != RSK_CONN_NONE));
    }
    rsk::tile_store_counts(a.tile, c, c, red);
}

__global__ __launch_bounds__(kBlock) void k_po_emit(OffersArgs a) {
    __shared__ uint32_t cnt[kRowPer][kWaves];
    const uint32_t total = gptr(a.tile)[a.row_tiles].x;
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        const uint32_t no = total < a.m_max ? total : a.m_max;
        *gptr(a.n_offer) = no;
        if (a.n_over) *gptr(a.n_over) = total - no;
    }
    const uint32_t tbase = gptr(a.tile)[blockIdx.x].x;
    if (total == 0u || tbase >= a.m_max) return;  // uniform over the block
    uint32_t sr[kRowPer];
    bool hit[kRowPer];
#pragma unroll
    for (unsigned k = 0; k < kRowPer; ++k) {
        sr[k] = offer_match(a, blockIdx.x * rsk::kFlushTile + k * kBlock + threadIdx.x);
        hit[k] = sr[k] != RSK_CONN_NONE;
    }
    uint32_t pos[kRowPer];
    if (tile_positions<kRowPer>(hit, tbase, cnt, pos) == 0u) return;
#pragma unroll
    for (unsigned k = 0; k < kRowPer; ++k) {
        const uint32_t r = blockIdx.x * rsk::kFlushTile + k * kBlock + threadIdx.x, o = pos[k];
        if (!hit[k] || o >= a.m_max) continue;
        const uint16_t sp = gptr(a.pa.sp)[r], dp = gptr(a.pa.dp)[r];
        gptr(a.src)[o] = gptr(a.pa.src)[r];
        gptr(a.dst)[o] = gptr(a.pa.dst)[r];
        gptr(a.sp)[o] = sp;
        gptr(a.dp)[o] = dp;
        gptr(a.ack)[o] = gptr(a.pa.ack)[r];   // the record's ack, never its seq
        gptr(a.flag)[o] = (uint8_t)RSK_TH_ACK;  // the flag the conn sends with, never the handshake's
        if (a.conn_key) gptr(a.conn_key)[o] = 0x10000000ull | ((uint64_t)dp << 16) | (uint64_t)sp;  // rsk_key_for_tcp
        if (a.ack_row) gptr(a.ack_row)[o] = r;
        if (a.sock_row) gptr(a.sock_row)[o] = sr[k];
    }
}

// ---- rows that leave: the settle's marked rows, the flush's expired rows ------------------------------------
struct LeavePool {
    DevPool p;
    const uint8_t *mark;  // settle: [capacity] in work; NULL in the flush
    uint64_t now;         // flush
    u32x2 *tile;          // [row_tiles + 1]: x = the rows that leave, y = the listed ones; the totals behind the scan
    uint32_t *list;       // the listed rows in row order: the flush's dead_rows, the settle's closed_sock_rows
    uint32_t row_tiles, clear_blocks;
};
struct LeaveArgs {
    LeavePool pool[2];
    uint32_t pools;
};

// Row r (r < capacity) leaves / is listed.  The settle lists the purged rows only: a taken socket is the conn's.
__device__ __forceinline__ bool leaves(const LeavePool &l, uint32_t r) {
    if (!l.p.live(r)) return false;
    return l.mark ? gptr(l.mark)[r] != rsk::kPoolStays : gptr(l.p.expiry)[r] <= l.now;
}
__device__ __forceinline__ bool listed(const LeavePool &l, uint32_t r) {
    return leaves(l, r) && (!l.mark || gptr(l.mark)[r] == rsk::kPoolPurged);
}
__device__ __forceinline__ uint32_t left_total(const LeavePool &l) { return gptr(l.tile)[l.row_tiles].x; }

__global__ __launch_bounds__(kBlock) void k_pl_count(LeaveArgs a) {
    __shared__ uint32_t red[2][kWaves];
    uint32_t b = blockIdx.x;
    const bool second = b >= a.pool[0].row_tiles;  // uniform over the block
    if (second) b -= a.pool[0].row_tiles;
    const LeavePool &l = a.pool[second ? 1 : 0];
    uint32_t x = 0, y = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kRowPer; ++k) {
        const uint32_t r = b * rsk::kFlushTile + k * kBlock + threadIdx.x;
        const bool in = r < l.p.capacity;
        x += (uint32_t)__popcll(__ballot(in && leaves(l, r)));
        y += (uint32_t)__popcll(__ballot(in && listed(l, r)));
    }
    if ((threadIdx.x & 63u) == 0u) {
        red[0][threadIdx.x >> 6] = x;
        red[1][threadIdx.x >> 6] = y;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        u32x2 s = u32x2{0u, 0u};
#pragma unroll
        for (unsigned w = 0; w < kWaves; ++w) {
            s.x += red[0][w];
            s.y += red[1][w];
        }
        gptr(l.tile)[b] = s;
    }
}

// Per pool: its row tiles list their rows, its clear blocks empty the index.  Nothing here writes state.
constexpr unsigned kClearPer = 4;
__global__ __launch_bounds__(kBlock) void k_pl_main(LeaveArgs a) {
    __shared__ uint32_t cnt[kRowPer][kWaves];
    uint32_t b = blockIdx.x;
    const uint32_t per0 = a.pool[0].row_tiles + a.pool[0].clear_blocks;
    const bool second = b >= per0;  // uniform over the block
    if (second) b -= per0;
    const LeavePool &l = a.pool[second ? 1 : 0];
    if (left_total(l) == 0u) return;  // uniform over the pool's blocks
    if (b < l.row_tiles) {
        if (!l.list) return;
        bool ls[kRowPer];
#pragma unroll
        for (unsigned k = 0; k < kRowPer; ++k) {
            const uint32_t r = b * rsk::kFlushTile + k * kBlock + threadIdx.x;
            ls[k] = r < l.p.capacity && listed(l, r);
        }
        uint32_t pos[kRowPer];
        if (tile_positions<kRowPer>(ls, gptr(l.tile)[b].y, cnt, pos) == 0u) return;
#pragma unroll
        for (unsigned k = 0; k < kRowPer; ++k) {
            const uint32_t r = b * rsk::kFlushTile + k * kBlock + threadIdx.x;
            // a row makes one entry at most, so a position is below the capacity
            if (ls[k] && pos[k] < l.p.capacity) gptr(l.list)[pos[k]] = r;
        }
        return;
    }
    b -= l.row_tiles;
    const rsk::u32x4 empty = {kConnEmpty, kConnEmpty, kConnEmpty, kConnEmpty};
#pragma unroll
    for (unsigned k = 0; k < kClearPer; ++k) {  // slots is a multiple of 4 and the index 16-B aligned
        const uint32_t q = (b * kClearPer + k) * kBlock + threadIdx.x;
        if (q < l.p.slots / 4u) reinterpret_cast<RSK_GLOBAL rsk::u32x4 *>(gptr(l.p.index))[q] = empty;
    }
}

// A row that leaves loses LIVE, by the lane that owns it; every other LIVE row is inserted.
__global__ __launch_bounds__(kBlock) void k_pl_insert(LeaveArgs a) {
    uint32_t b = blockIdx.x;
    const uint32_t per0 = (a.pool[0].p.capacity + kBlock - 1u) / kBlock;
    const bool second = b >= per0;  // uniform over the block
    if (second) b -= per0;
    const LeavePool &l = a.pool[second ? 1 : 0];
    if (left_total(l) == 0u) return;  // uniform over the pool's blocks
    const uint32_t g = b * kBlock + threadIdx.x;
    if (g >= l.p.capacity) return;
    const uint8_t st = gptr(l.p.state)[g];
    if (!(st & RSK_POOL_LIVE)) return;
    if (l.mark ? gptr(l.mark)[g] != rsk::kPoolStays : gptr(l.p.expiry)[g] <= l.now) {
        gptr(l.p.state)[g] = (uint8_t)(st & ~RSK_POOL_LIVE);
        return;
    }
    pool_insert(l.p, g);
}

// The chain behind the marks / for the expiry: count, a scan per pool, main, insert.
int leave_chain(LeaveArgs &a, uint32_t *tot_y[2], hipStream_t s) {
    int r;
    uint32_t count_blocks = 0, main_blocks = 0, insert_blocks = 0;
    for (uint32_t k = 0; k < a.pools; ++k) {
        LeavePool &l = a.pool[k];
        l.row_tiles = (l.p.capacity + rsk::kFlushTile - 1u) / rsk::kFlushTile;
        l.clear_blocks = (l.p.slots / 4u + kClearPer * kBlock - 1u) / (kClearPer * kBlock);
        count_blocks += l.row_tiles;
        main_blocks += l.row_tiles + l.clear_blocks;
        insert_blocks += (l.p.capacity + kBlock - 1u) / kBlock;
    }
    const dim3 blk(kBlock);
    hipLaunchKernelGGL(k_pl_count, dim3(count_blocks), blk, 0, s, a);
    if ((r = rsk::launch_check("k_pl_count"))) return r;
    for (uint32_t k = 0; k < a.pools; ++k) {
        hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.pool[k].tile, a.pool[k].row_tiles,
                           static_cast<uint32_t *>(nullptr), tot_y[k]);
        if ((r = rsk::launch_check("k_tile_scan"))) return r;
    }
    hipLaunchKernelGGL(k_pl_main, dim3(main_blocks), blk, 0, s, a);
    if ((r = rsk::launch_check("k_pl_main"))) return r;
    hipLaunchKernelGGL(k_pl_insert, dim3(insert_blocks), blk, 0, s, a);
    return rsk::launch_check("k_pl_insert");
}

// ---- settle ------------------------------------------------------------------------------------------------
struct SettleArgs {
    DevPool pa, ps;
    uint8_t *mark_a, *mark_s;
    const uint32_t *new_offer, *n_new, *ack_row, *sock_row;
    uint32_t new_max, m_max;
    const int8_t *miss;
    const uint32_t *src, *dst;
    const uint16_t *sp, *dp;
    uint32_t *taken;
    uint32_t n;
};

// (a): the two rows of every offer that became a conn.  Plain stores of one value; an offer is named once.
__global__ __launch_bounds__(kBlock) void k_ps_take(SettleArgs a) {
    const uint32_t nn = *gptr(a.n_new), m = nn < a.new_max ? nn : a.new_max;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < m; j += gridDim.x * kBlock) {
        const uint32_t o = gptr(a.new_offer)[j];
        uint32_t sr = RSK_CONN_NONE;
        if (o < a.m_max) {
            const uint32_t ar = gptr(a.ack_row)[o];
            sr = gptr(a.sock_row)[o];
            if (ar < a.pa.capacity) gptr(a.mark_a)[ar] = rsk::kPoolTaken;
            if (sr < a.ps.capacity) gptr(a.mark_s)[sr] = rsk::kPoolTaken;
            else sr = RSK_CONN_NONE;
        }
        if (a.taken) gptr(a.taken)[j] = sr;
    }
}

// (b): a packet still missing.  Decided from state and the marks of (a) -- kPoolTaken, which this launch never
// writes -- so the marks other lanes store meanwhile (kPoolPurged, on rows that are not taken) change nothing.
__global__ __launch_bounds__(kBlock) void k_ps_purge(SettleArgs a) {
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        if (i >= a.n || gptr(a.miss)[i] != (int8_t)RSK_RECV_VALID) continue;
        const uint64_t key = rsk::tuple_key(gptr(a.src)[i], gptr(a.dst)[i]);
        const uint64_t ports = rsk::tuple_ports(gptr(a.sp)[i], gptr(a.dp)[i]);
        const uint32_t ra = pool_find(a.pa, key, ports), rs = pool_find(a.ps, key, ports);
        const bool in_a = ra != RSK_CONN_NONE && gptr(a.mark_a)[ra] != rsk::kPoolTaken;
        const bool in_s = rs != RSK_CONN_NONE && gptr(a.mark_s)[rs] != rsk::kPoolTaken;
        if (in_a == in_s) continue;  // a whole offer stays; nothing to remove
        if (in_a) gptr(a.mark_a)[ra] = rsk::kPoolPurged;
        else gptr(a.mark_s)[rs] = rsk::kPoolPurged;
    }
}

uint32_t tiles(uint64_t items) { return (uint32_t)((items + kTile - 1u) / kTile); }

}  // namespace

extern "C" int rsk_pool_index_build(rsk_ctx *c, const rsk_pool *p, uint32_t *n_dup, void *stream) {
    if (!c || !rsk::pool_ok(p, false)) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    return rsk::index_build(dev_pool(p), p->index, p->state, p->capacity, true, n_dup, (hipStream_t)stream);
}

extern "C" int rsk_pool_add_batch(rsk_ctx *c, const rsk_pool *p, uint32_t n, const rsk_pool_add_in *in,
                                  const rsk_pool_add_out *out, void *stream) {
    if (!c || !rsk::pool_add_args_ok(p, n, in, out)) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    int r;
    if (n == 0) {  // the four counts, by a kernel each: no memset node (rsk_tile_dev.h)
        for (uint32_t *word : {out->n_new, out->n_again, out->n_full, out->n_zero_port})
            if (word && (r = rsk::fill_words_async(word, 1u, 0u, s))) return r;
        return RSK_OK;
    }
    const rsk::CreateLayout l = rsk::create_layout(in->u_max, p->capacity);
    uint32_t *w = static_cast<uint32_t *>(in->work);
    AddArgs a;
    a.p = dev_pool(p);
    a.src = in->src;
    a.dst = in->dst;
    a.sp = in->sp;
    a.dp = in->dp;
    a.seq = in->seq;
    a.ack = in->ack;
    a.status = in->parse_status;
    a.expiry = in->expiry;
    a.row = out->row;
    a.new_rows = out->new_rows;
    a.new_first = out->new_first;
    a.n_new = out->n_new;
    a.n_again = out->n_again;
    a.n_full = out->n_full;
    a.hdr = w;
    a.mask = reinterpret_cast<uint64_t *>(w + l.mask);
    a.dedup = w + l.dedup;
    a.list = w + l.list;
    a.first = w + l.first;
    a.vacant = w + l.vacant;
    a.n = n;
    a.u = in->u_max < n ? in->u_max : n;
    a.m = in->u_max < p->capacity ? in->u_max : p->capacity;
    a.touch = (in->flags & RSK_POOL_TOUCH) != 0;
    const uint32_t nt = tiles(n), nt_u = tiles(a.u), nt_c = tiles(p->capacity), nt2 = nt_u > nt_c ? nt_u : nt_c;
    // tiles(u) <= tiles(n) and tiles(capacity) is below the flush's share of the scratch
    void *wsp = nullptr;
    if ((r = rsk::stream_ws(c, s, rsk::WS_CONTROL, rsk::control_ws_bytes(n), &wsp))) return r;
    a.tile = static_cast<u32x2 *>(wsp);
    const dim3 blk(kBlock);
    hipLaunchKernelGGL(k_pa_count, dim3(nt), blk, 0, s, a);
    if ((r = rsk::launch_check("k_pa_count"))) return r;
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile, nt, a.hdr + rsk::kCreateUnknown,
                       out->n_zero_port ? out->n_zero_port : a.hdr + rsk::kPoolZeroPort);
    if ((r = rsk::launch_check("k_tile_scan"))) return r;
    hipLaunchKernelGGL(k_pa_list, dim3(nt), blk, 0, s, a);
    if ((r = rsk::launch_check("k_pa_list"))) return r;
    hipLaunchKernelGGL(k_pa_dedup, dim3((a.u + kBlock - 1u) / kBlock), blk, 0, s, a);
    if ((r = rsk::launch_check("k_pa_dedup"))) return r;
    hipLaunchKernelGGL(k_pa_count2, dim3(nt2), blk, 0, s, a);
    if ((r = rsk::launch_check("k_pa_count2"))) return r;
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile, nt2, a.hdr + rsk::kCreateKeys,
                       a.hdr + rsk::kCreateVacant);
    if ((r = rsk::launch_check("k_tile_scan"))) return r;
    hipLaunchKernelGGL(k_pa_rank, dim3(nt2), blk, 0, s, a);
    if ((r = rsk::launch_check("k_pa_rank"))) return r;
    const dim3 grid_m((a.m + kBlock - 1u) / kBlock);
    hipLaunchKernelGGL(k_pa_rows, grid_m, blk, 0, s, a);
    if ((r = rsk::launch_check("k_pa_rows"))) return r;
    hipLaunchKernelGGL(k_pa_insert, grid_m, blk, 0, s, a);
    if ((r = rsk::launch_check("k_pa_insert"))) return r;
    if (!out->row) return RSK_OK;
    hipLaunchKernelGGL(k_pa_assign, dim3(nt), blk, 0, s, a);
    return rsk::launch_check("k_pa_assign");
}

extern "C" int rsk_pool_offers(rsk_ctx *c, const rsk_pool *pa, const rsk_pool *ps, const rsk_pool_offers_out *out,
                               void *stream) {
    if (!c || !rsk::pool_offers_args_ok(pa, ps, out)) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    int r;
    OffersArgs a;
    a.pa = dev_pool(pa);
    a.ps = dev_pool(ps);
    a.src = out->src;
    a.dst = out->dst;
    a.sp = out->sp;
    a.dp = out->dp;
    a.ack = out->ack;
    a.flag = out->flag;
    a.conn_key = out->conn_key;
    a.n_offer = out->n_offer;
    a.ack_row = out->offer_ack_row;
    a.sock_row = out->offer_sock_row;
    a.n_over = out->n_over;
    a.row_tiles = (pa->capacity + rsk::kFlushTile - 1u) / rsk::kFlushTile;
    a.m_max = out->m_max;
    void *wsp = nullptr;  // the row tiles fit the scratch of any batch size (control_ws_bytes)
    if ((r = rsk::stream_ws(c, s, rsk::WS_CONTROL, rsk::control_ws_bytes(0), &wsp))) return r;
    a.tile = static_cast<u32x2 *>(wsp);
    const dim3 blk(kBlock);
    hipLaunchKernelGGL(k_po_count, dim3(a.row_tiles), blk, 0, s, a);
    if ((r = rsk::launch_check("k_po_count"))) return r;
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile, a.row_tiles, static_cast<uint32_t *>(nullptr),
                       static_cast<uint32_t *>(nullptr));
    if ((r = rsk::launch_check("k_tile_scan"))) return r;
    hipLaunchKernelGGL(k_po_emit, dim3(a.row_tiles), blk, 0, s, a);
    return rsk::launch_check("k_po_emit");
}

extern "C" int rsk_pool_settle_batch(rsk_ctx *c, const rsk_pool *pa, const rsk_pool *ps, uint32_t n,
                                     const rsk_pool_settle_in *in, const rsk_pool_settle_out *out, void *stream) {
    if (!c || !rsk::pool_settle_args_ok(pa, ps, n, in, out)) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    int r;
    SettleArgs a;
    a.pa = dev_pool(pa);
    a.ps = dev_pool(ps);
    a.mark_a = static_cast<uint8_t *>(in->work);
    a.mark_s = a.mark_a + rsk::pool_round16(pa->capacity);
    a.new_offer = in->new_offer;
    a.n_new = in->n_new;
    a.ack_row = in->offer_ack_row;
    a.sock_row = in->offer_sock_row;
    a.new_max = in->new_max;
    a.m_max = in->m_max;
    a.miss = in->miss;
    a.src = in->src;
    a.dst = in->dst;
    a.sp = in->sp;
    a.dp = in->dp;
    a.taken = out->taken_sock_rows;
    a.n = n;
    void *wsp = nullptr;  // two pools' row tiles and totals fit the scratch of any batch size (control_ws_bytes)
    if ((r = rsk::stream_ws(c, s, rsk::WS_CONTROL, rsk::control_ws_bytes(n), &wsp))) return r;
    // a kernel, not a memset node (rsk_tile_dev.h)
    if ((r = rsk::fill_words_async(static_cast<uint32_t *>(in->work), (uint32_t)(rsk::pool_settle_bytes(pa->capacity, ps->capacity) / 4u),
                                   0u, s)))
        return r;
    const dim3 blk(kBlock);
    if (in->new_max) {
        const uint32_t nb = (in->new_max + kBlock - 1u) / kBlock;
        hipLaunchKernelGGL(k_ps_take, dim3(nb < kGridStride ? nb : kGridStride), blk, 0, s, a);
        if ((r = rsk::launch_check("k_ps_take"))) return r;
    }
    if (n) {
        hipLaunchKernelGGL(k_ps_purge, dim3(tiles(n)), blk, 0, s, a);
        if ((r = rsk::launch_check("k_ps_purge"))) return r;
    }
    LeaveArgs la;
    la.pools = 2;
    la.pool[0].p = a.pa;
    la.pool[0].mark = a.mark_a;
    la.pool[0].now = 0;
    la.pool[0].tile = static_cast<u32x2 *>(wsp);
    la.pool[0].list = nullptr;
    la.pool[1].p = a.ps;
    la.pool[1].mark = a.mark_s;
    la.pool[1].now = 0;
    la.pool[1].tile = la.pool[0].tile + (pa->capacity + rsk::kFlushTile - 1u) / rsk::kFlushTile + 1u;
    la.pool[1].list = out->closed_sock_rows;
    uint32_t *tot_y[2] = {out->n_purged_ack, out->n_closed};
    return leave_chain(la, tot_y, s);
}

extern "C" int rsk_pool_flush(rsk_ctx *c, const rsk_pool *p, uint64_t now_ms, const rsk_pool_flush_out *out, void *stream) {
    if (!c || !rsk::pool_flush_args_ok(p, out)) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    void *wsp = nullptr;
    if (int r = rsk::stream_ws(c, s, rsk::WS_CONTROL, rsk::control_ws_bytes(0), &wsp)) return r;
    LeaveArgs la;
    la.pools = 1;
    la.pool[0].p = dev_pool(p);
    la.pool[0].mark = nullptr;
    la.pool[0].now = now_ms;
    la.pool[0].tile = static_cast<u32x2 *>(wsp);
    la.pool[0].list = out->dead_rows;
    la.pool[1] = la.pool[0];  // never reached: every block belongs to the first pool
    la.pool[1].row_tiles = la.pool[1].clear_blocks = 0;
    uint32_t *tot_y[2] = {out->n_dead, nullptr};
    return leave_chain(la, tot_y, s);
}
