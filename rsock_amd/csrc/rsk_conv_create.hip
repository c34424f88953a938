// rsk_conv_create.hip — rsk_conv_create_batch (include/rsk_codec.h): the convs born in a receive batch made
// on the device table, SubGroup::OnRecv -> newConn inside the packet walk (server/SubGroup.cpp:31-68), with
// a fresh IConn::DataStat per row (conn/IConn.h:80-84).  The first call that writes table rows and updates
// an index in place: the index is open addressing without tombstones, filled by compare-and-swap with an
// atomicMin tie-break (k_index_build, rsk_conn_dev.h), so an insert-only update leaves every lookup valid.
//
// A linear chain on the stream; `work` as laid out in rsk_conv_create.h, hdr = the counts between launches:
//   k_cc_count      per 2048-packet tile, the packets with unknown == VALID; *n_unknown = 0 (a store, not a
//                   memset node: rsk_tile_dev.h, k_fill_words)
//   k_tile_scan     their exclusive scan; the total -> hdr[unknown]
//   k_cc_list       list[p] = the p-th unknown packet, p < u = min(u_max, n): the considered packets; and the
//                   dedup table cleared -- as many entries as the considered packets need (create_slots), so
//                   a batch with few unknown packets clears little and one with none clears nothing
//   k_cc_dedup      k_index_build<1> over the list: key = the packet's (id, dst, conv), entry = a list
//                   position; atomicMin leaves the lowest position of a key, so
//                   entry == own position <=> first arrival.  A position that never held its entry cannot be
//                   one: the ballots of those that did go to `mask`, one 64-bit word per wave
//   k_cc_count2     tile b: (first arrivals in list tile b, vacant rows in row tile b); only mask's candidates
//                   are probed, and the first-arrival ballots replace them in `mask`, so k_cc_rank probes nothing
//   k_tile_scan     both scans; the totals -> hdr[keys], hdr[vacant]
//   k_cc_rank       first[j] = the packet of the j-th first arrival (from mask), vacant[j] = the j-th vacant
//                   row, j < min(u_max, capacity)
//   k_cc_rows       n_new = min(keys, vacant): the row columns, new_rows / new_first, n_new, n_full
//   k_cc_insert     the new rows into tab->index -- a launch of its own, so that the row columns are complete
//                   before any entry names them
//   k_cc_assign     one pass over the batch: a lookup per packet still unknown, conv_row / unknown of the
//                   found ones, cur_in by tile_count_rows, n_unknown with one atomic per block
// Every kernel but the counts leaves at once when hdr[unknown] == 0: the steady state costs the launches.
// No block waits on another and nothing spins; every probe loop is bounded by its table's size.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rsk_conv_create.h"
#include "rsk_tile_dev.h"

namespace {

using rsk::gptr;
using rsk::k_tile_scan;
using rsk::kConnEmpty;
using rsk::kScanBlock;
using rsk::misaligned8;
using rsk::RowAgg;
using rsk::tile_positions;
using rsk::u32x2;
using rsk::zero_word;

constexpr unsigned kBlock = rsk::kTileBlock;
constexpr unsigned kWaves = rsk::kTileWaves;
constexpr unsigned kPer = 8;  // items per thread: the resolve's tile
constexpr uint32_t kTile = kBlock * kPer;
static_assert(kTile == rsk::kControlTile, "scratch size (rsk_ctx.h) and tile size must agree");
static_assert(RSK_CONN_MAX_ROWS / kTile + 1u <= RSK_CONN_MAX_ROWS / rsk::kFlushTile, "the row tiles fit the control scratch");

constexpr uint32_t kFlags = RSK_CONV_BY_DST | RSK_CONV_BY_ID;

// The table as rsk_conn.h's conn_lookup takes it (rsk_conv.hip's accessor).
struct DevConvTab {
    const uint32_t *index;
    const uint32_t *conv;
    const uint32_t *dst;
    const uint64_t *ids;
    bool by_dst;
    __device__ __forceinline__ uint32_t entry(uint32_t s) const { return gptr(index)[s]; }
    __device__ __forceinline__ uint64_t key(uint32_t row) const {
        const uint64_t c = gptr(conv)[row];
        return by_dst ? ((uint64_t)gptr(dst)[row] << 32) | c : c;
    }
    __device__ __forceinline__ uint64_t id(uint32_t row) const { return gptr(ids)[row]; }
};

struct CreateArgs {
    DevConvTab t;
    // the table's columns, writable
    uint8_t *state;
    uint32_t *tconv, *tdst;
    uint64_t *tids;
    uint32_t *cur_in, *cur_out, *prev_in, *prev_out;
    uint8_t *alive;
    uint32_t *index;
    // the packets' key columns
    const uint64_t *id;
    const uint32_t *conv, *dst;
    uint32_t *conv_row;
    int8_t *unknown;
    uint32_t *n_unknown, *new_rows, *new_first, *n_new, *n_full;
    uint32_t *hdr, *dedup, *list, *first, *vacant;  // work
    uint64_t *mask;                                 // work: bit p % 64 of word p / 64 = list position p is a first arrival
    u32x2 *tile;
    uint32_t n, capacity;
    uint32_t u;       // min(u_max, n): entries of list
    uint32_t m;       // min(u_max, capacity): entries of first, vacant, new_rows, new_first
    bool by_id;
};

__device__ __forceinline__ uint64_t pkt_key(const CreateArgs &a, uint64_t i) {
    const uint64_t c = gptr(a.conv)[i];
    return a.t.by_dst ? ((uint64_t)gptr(a.dst)[i] << 32) | c : c;
}
__device__ __forceinline__ uint64_t pkt_id(const CreateArgs &a, uint64_t i) { return a.by_id ? gptr(a.id)[i] : 0ull; }
// entries of list in use: hdr[unknown] was written by the scan before this launch
__device__ __forceinline__ uint32_t considered(const CreateArgs &a) {
    const uint32_t unk = gptr(a.hdr)[rsk::kCreateUnknown];
    return unk < a.u ? unk : a.u;
}

// entries of the dedup table in use: create_slots (rsk_conv_create.h) of the considered packets, mcons >= 1
__device__ __forceinline__ uint32_t dedup_slots(uint32_t mcons) {
    const uint32_t s = 1u << (32u - (uint32_t)__builtin_clz(2u * mcons - 1u));  // the power of two >= 2 mcons
    return s < 4u ? 4u : s;
}

__global__ __launch_bounds__(kBlock) void k_cc_count(CreateArgs a) {
    __shared__ uint32_t red[2][kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    if (a.n_unknown && blockIdx.x == 0u && threadIdx.x == 0u) *gptr(a.n_unknown) = 0u;  // k_cc_assign, a later launch, adds
    uint32_t c = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        c += (uint32_t)__popcll(__ballot(i < a.n && gptr(a.unknown)[i] == (int8_t)RSK_RECV_VALID));
    }
    rsk::tile_store_counts(a.tile, c, c, red);
}

__global__ __launch_bounds__(kBlock) void k_cc_list(CreateArgs a) {
    __shared__ uint32_t cnt[kPer][kWaves];
    const uint32_t mcons = considered(a);
    if (mcons == 0u) return;  // uniform over the grid
    {  // this block's share of the clear: 16-B stores, grid-stride (dedup is 16-B aligned, the slots a multiple of 4)
        const rsk::u32x4 empty = {kConnEmpty, kConnEmpty, kConnEmpty, kConnEmpty};
        const uint32_t quads = dedup_slots(mcons) / 4u;
        for (uint32_t q = blockIdx.x * kBlock + threadIdx.x; q < quads; q += gridDim.x * kBlock)
            reinterpret_cast<RSK_GLOBAL rsk::u32x4 *>(gptr(a.dedup))[q] = empty;
    }
    const uint32_t tbase = gptr(a.tile)[blockIdx.x].x;
    if (tbase >= a.u) return;  // uniform over the block: nothing of this tile is considered
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    bool unk[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        unk[k] = i < a.n && gptr(a.unknown)[i] == (int8_t)RSK_RECV_VALID;
    }
    uint32_t pos[kPer];
    if (tile_positions<kPer>(unk, tbase, cnt, pos) == 0u) return;
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k)
        if (unk[k] && pos[k] < a.u) gptr(a.list)[pos[k]] = (uint32_t)(base + k * kBlock);
}

// The entry of list position p's key in the dedup table after k_cc_dedup: the lowest position of the key
// (p itself for a first arrival), or kConnEmpty in a table that does not hold it (never, after the insert).
__device__ __forceinline__ uint32_t dedup_find(const CreateArgs &a, uint32_t mcons, uint64_t key, uint64_t id) {
    const uint32_t dslots = dedup_slots(mcons);
    uint32_t s = rsk::conn_home(key, id, dslots);
    for (uint32_t step = 0; step < dslots; ++step, s = rsk::conn_next(s, dslots)) {
        const uint32_t e = gptr(a.dedup)[s];
        if (e >= mcons) break;
        const uint32_t j = gptr(a.list)[e];
        if (j < a.n && pkt_key(a, j) == key && pkt_id(a, j) == id) return e;
    }
    return kConnEmpty;
}

__global__ __launch_bounds__(kBlock) void k_cc_dedup(CreateArgs a) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x, mcons = considered(a);
    const uint32_t i = p < mcons ? gptr(a.list)[p] : RSK_CONN_NONE;
    bool cand = false;  // p held its key's entry at some time: only such a position can be the first arrival
    if (i < a.n) {      // list[p] is a packet of the batch: k_cc_list wrote it
        const uint64_t key = pkt_key(a, i), id = pkt_id(a, i);
        const uint32_t dslots = dedup_slots(mcons);
        uint32_t s = rsk::conn_home(key, id, dslots);
        // mcons positions are inserted and dslots >= 2 mcons: a free entry is met; the bound only keeps a
        // corrupted launch from spinning
        for (uint32_t step = 0; step < dslots; ++step, s = rsk::conn_next(s, dslots)) {
            // a plain load first: an entry only ever falls and never changes its key, so a stale value is at
            // worst too high (or still free) and costs an atomic that changes nothing -- while the packets
            // behind a key's first arrival, most of a batch of few convs, leave without one
            uint32_t e = gptr(a.dedup)[s];
            if (e == kConnEmpty) e = atomicCAS(a.dedup + s, kConnEmpty, p);
            if (e == kConnEmpty) {
                cand = true;
                break;
            }
            // an entry's key never changes once taken: only positions of one key replace each other in it
            if (e < mcons) {
                const uint32_t j = gptr(a.list)[e];
                if (j < a.n && pkt_key(a, j) == key && pkt_id(a, j) == id) {
                    if (p < e) {
                        atomicMin(a.dedup + s, p);
                        cand = true;
                    }
                    break;
                }
            }
        }
    }
    // the wave's 64 positions are one word of the mask: the candidates, for k_cc_count2 to probe
    const uint64_t cb = __ballot(cand);
    if ((threadIdx.x & 63u) == 0u && p < mcons) gptr(a.mask)[p >> 6] = cb;
}

// Is list position p (tile item) a first arrival; is row r vacant.
__device__ __forceinline__ bool is_first(const CreateArgs &a, uint32_t mcons, uint64_t p) {
    if (p >= mcons) return false;
    const uint32_t i = gptr(a.list)[p];
    if (i >= a.n) return false;
    return dedup_find(a, mcons, pkt_key(a, i), pkt_id(a, i)) == (uint32_t)p;
}
__device__ __forceinline__ bool is_vacant(const CreateArgs &a, uint32_t mcons, uint64_t r) {
    return mcons != 0u && r < a.capacity && !(gptr(a.state)[r] & RSK_CONN_LIVE);
}

__global__ __launch_bounds__(kBlock) void k_cc_count2(CreateArgs a) {
    __shared__ uint32_t red[2][kWaves];
    const uint32_t mcons = considered(a);
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    uint32_t nf = 0, nv = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t x = base + k * kBlock;
        // the wave's 64 positions are one word of the mask, read (k_cc_dedup's candidates) and stored (the first
        // arrivals among them) by this wave alone, while it holds a considered position
        const bool held = x - (threadIdx.x & 63u) < mcons;
        const uint64_t cb = held ? gptr(a.mask)[x >> 6] : 0ull;
        const uint64_t fb = __ballot(((cb >> (threadIdx.x & 63u)) & 1ull) != 0ull && is_first(a, mcons, x));
        if ((threadIdx.x & 63u) == 0u && held) gptr(a.mask)[x >> 6] = fb;
        nf += (uint32_t)__popcll(fb);
        nv += (uint32_t)__popcll(__ballot(is_vacant(a, mcons, x)));
    }
    rsk::tile_store_counts(a.tile, nf, nv, red);
}

__global__ __launch_bounds__(kBlock) void k_cc_rank(CreateArgs a) {
    __shared__ uint32_t cnt_f[kPer][kWaves], cnt_v[kPer][kWaves];
    const uint32_t mcons = considered(a);
    if (mcons == 0u) return;  // uniform over the grid
    const u32x2 tb = gptr(a.tile)[blockIdx.x];
    if (tb.x >= a.m && tb.y >= a.m) return;  // uniform over the block: nothing of this tile is stored
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    bool f[kPer], v[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t x = base + k * kBlock;
        // k_cc_count2's ballot of this wave and step (mcons <= u: the word lies in the mask)
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

// keys <= considered <= u and vacant <= capacity: the minimum is at most m, the entries of first / vacant
__device__ __forceinline__ uint32_t created(const CreateArgs &a) {
    const uint32_t k = gptr(a.hdr)[rsk::kCreateKeys], v = gptr(a.hdr)[rsk::kCreateVacant];
    const uint32_t c = k < v ? k : v;
    return c < a.m ? c : a.m;
}

__global__ __launch_bounds__(kBlock) void k_cc_rows(CreateArgs a) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const bool any = gptr(a.hdr)[rsk::kCreateUnknown] != 0u;
    const uint32_t nn = any ? created(a) : 0u;
    if (j == 0u) {
        if (a.n_new) *gptr(a.n_new) = nn;
        if (a.n_full) *gptr(a.n_full) = any ? gptr(a.hdr)[rsk::kCreateKeys] - nn : 0u;
    }
    if (j >= nn) return;
    const uint32_t r = gptr(a.vacant)[j], i = gptr(a.first)[j];
    if (r >= a.capacity || i >= a.n) return;  // k_cc_rank wrote a row and a packet
    gptr(a.tconv)[r] = gptr(a.conv)[i];
    if (a.t.by_dst) gptr(a.tdst)[r] = gptr(a.dst)[i];
    if (a.by_id) gptr(a.tids)[r] = gptr(a.id)[i];
    if (a.cur_in) gptr(a.cur_in)[r] = 0u;
    if (a.cur_out) gptr(a.cur_out)[r] = 0u;
    if (a.prev_in) gptr(a.prev_in)[r] = 0u;
    if (a.prev_out) gptr(a.prev_out)[r] = 0u;
    if (a.alive) gptr(a.alive)[r] = (uint8_t)1;
    gptr(a.state)[r] = (uint8_t)RSK_CONN_LIVE;
    if (a.new_rows) gptr(a.new_rows)[j] = r;
    if (a.new_first) gptr(a.new_first)[j] = i;
}

__global__ __launch_bounds__(kBlock) void k_cc_insert(CreateArgs a) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (gptr(a.hdr)[rsk::kCreateUnknown] == 0u || j >= created(a)) return;
    const uint32_t r = gptr(a.vacant)[j];
    if (r >= a.capacity) return;
    const uint64_t key = a.t.key(r), id = a.by_id ? a.t.id(r) : 0ull;
    const uint32_t slots = rsk::conn_slots(a.capacity);
    uint32_t s = rsk::conn_home(key, id, slots);
    // k_index_build's rule: at most `capacity` entries are ever taken and slots >= 2 capacity
    for (uint32_t step = 0; step < slots; ++step, s = rsk::conn_next(s, slots)) {
        const uint32_t e = atomicCAS(a.index + s, kConnEmpty, r);
        if (e == kConnEmpty) break;
        if (e < a.capacity && a.t.key(e) == key && (!a.by_id || a.t.id(e) == id)) {
            atomicMin(a.index + s, r);  // the lowest row of a key wins
            break;
        }
    }
}

template <bool COUNT>
__global__ __launch_bounds__(kBlock) void k_cc_assign(CreateArgs a) {
    __shared__ uint32_t wave_unk[kWaves];
    __shared__ std::conditional_t<COUNT, RowAgg<kPer>, char> agg;
    if (gptr(a.hdr)[rsk::kCreateUnknown] == 0u) return;  // uniform over the grid; k_cc_count zeroed *n_unknown
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    bool unk[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        unk[k] = i < a.n && gptr(a.unknown)[i] == (int8_t)RSK_RECV_VALID;
    }
    uint64_t key[kPer], id[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        key[k] = id[k] = 0ull;
        if (unk[k]) {
            key[k] = pkt_key(a, i);
            id[k] = pkt_id(a, i);
        }
    }
    uint32_t row[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        row[k] = RSK_CONN_NONE;
        if (unk[k]) row[k] = rsk::conn_lookup(a.t, a.capacity, a.by_id, key[k], id[k]);
    }
    uint32_t left = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        if (row[k] != RSK_CONN_NONE) {  // a row of the table: conn_lookup returns nothing else
            gptr(a.conv_row)[i] = row[k];
            gptr(a.unknown)[i] = (int8_t)RSK_RECV_DROP;
        }
        left += (uint32_t)__popcll(__ballot(unk[k] && row[k] == RSK_CONN_NONE));
    }
    if (a.n_unknown) {  // k_cc_count zeroed the word; one atomic per block
        if ((threadIdx.x & 63u) == 0u) wave_unk[threadIdx.x >> 6] = left;
        __syncthreads();
        if (threadIdx.x == 0u) {
            uint32_t total = 0;
#pragma unroll
            for (unsigned w = 0; w < kWaves; ++w) total += wave_unk[w];
            if (total) atomicAdd(a.n_unknown, total);
        }
    }
    if constexpr (COUNT) rsk::tile_count_rows<kPer>(row, a.cur_in, a.capacity, reinterpret_cast<RowAgg<kPer> &>(agg));
}

bool ctab_lookup_ok(const rsk_conv_table *t) {
    return t && !(t->flags & ~kFlags) && t->capacity >= 1u && t->capacity <= RSK_CONN_MAX_ROWS && t->state && t->conv &&
           t->index && (!(t->flags & RSK_CONV_BY_DST) || t->dst) && (!(t->flags & RSK_CONV_BY_ID) || t->id);
}

uint32_t tiles(uint64_t items) { return (uint32_t)((items + kTile - 1u) / kTile); }

}  // namespace

extern "C" int rsk_conv_create_batch(rsk_ctx *c, const rsk_conv_table *t, const rsk_conv_rows *rows, uint32_t n,
                                     const rsk_conv_create_in *in, const rsk_conv_create_out *out, void *stream) {
    if (!c || !rows || !in || !out || !ctab_lookup_ok(t) || !in->work) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONV_BY_ID) != 0, by_dst = (t->flags & RSK_CONV_BY_DST) != 0;
    if (rows->state != t->state || rows->conv != t->conv || (by_dst && rows->dst != t->dst) || (by_id && rows->id != t->id))
        return RSK_EINVAL;
    if (in->u_max == 0u || in->u_max > rsk::kCreateMaxU) return RSK_EINVAL;
    if (n && (!out->conv_row || !out->unknown || !in->conv || (by_dst && !in->dst) || (by_id && !in->id))) return RSK_EINVAL;
    if (misaligned8(in->id) || (by_id && misaligned8(t->id)) || (reinterpret_cast<uintptr_t>(in->work) & 15u)) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    int r;
    if (n == 0) {
        if ((r = zero_word(out->n_unknown, s)) || (r = zero_word(out->n_new, s))) return r;
        return zero_word(out->n_full, s);
    }
    const rsk::CreateLayout l = rsk::create_layout(in->u_max, t->capacity);
    uint32_t *w = static_cast<uint32_t *>(in->work);
    CreateArgs a;
    a.t = DevConvTab{t->index, t->conv, t->dst, reinterpret_cast<const uint64_t *>(t->id), by_dst};
    a.state = rows->state;
    a.tconv = rows->conv;
    a.tdst = by_dst ? rows->dst : nullptr;
    a.tids = by_id ? reinterpret_cast<uint64_t *>(rows->id) : nullptr;
    a.cur_in = t->cur_in;
    a.cur_out = t->cur_out;
    a.prev_in = t->prev_in;
    a.prev_out = t->prev_out;
    a.alive = t->alive;
    a.index = t->index;
    a.id = reinterpret_cast<const uint64_t *>(in->id);
    a.conv = in->conv;
    a.dst = in->dst;
    a.conv_row = out->conv_row;
    a.unknown = out->unknown;
    a.n_unknown = out->n_unknown;
    a.new_rows = out->new_rows;
    a.new_first = out->new_first;
    a.n_new = out->n_new;
    a.n_full = out->n_full;
    a.hdr = w;
    a.mask = reinterpret_cast<uint64_t *>(w + l.mask);
    a.dedup = w + l.dedup;
    a.list = w + l.list;
    a.first = w + l.first;
    a.vacant = w + l.vacant;
    a.n = n;
    a.capacity = t->capacity;
    a.u = in->u_max < n ? in->u_max : n;
    a.m = in->u_max < t->capacity ? in->u_max : t->capacity;
    a.by_id = by_id;
    const uint32_t nt = tiles(n), nt_u = tiles(a.u), nt_c = tiles(t->capacity), nt2 = nt_u > nt_c ? nt_u : nt_c;
    // tiles(u) <= tiles(n) and tiles(capacity) is below the flush's share of the scratch
    void *wsp = nullptr;
    if ((r = rsk::stream_ws(c, s, rsk::WS_CONTROL, rsk::control_ws_bytes(n), &wsp))) return r;
    a.tile = static_cast<u32x2 *>(wsp);
    const dim3 blk(kBlock);
    hipLaunchKernelGGL(k_cc_count, dim3(nt), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cc_count"))) return r;
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile, nt, a.hdr + rsk::kCreateUnknown,
                       static_cast<uint32_t *>(nullptr));
    if ((r = rsk::launch_check("k_tile_scan"))) return r;
    hipLaunchKernelGGL(k_cc_list, dim3(nt), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cc_list"))) return r;
    hipLaunchKernelGGL(k_cc_dedup, dim3((a.u + kBlock - 1u) / kBlock), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cc_dedup"))) return r;
    hipLaunchKernelGGL(k_cc_count2, dim3(nt2), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cc_count2"))) return r;
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile, nt2, a.hdr + rsk::kCreateKeys,
                       a.hdr + rsk::kCreateVacant);
    if ((r = rsk::launch_check("k_tile_scan"))) return r;
    hipLaunchKernelGGL(k_cc_rank, dim3(nt2), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cc_rank"))) return r;
    const dim3 grid_m((a.m + kBlock - 1u) / kBlock);
    hipLaunchKernelGGL(k_cc_rows, grid_m, blk, 0, s, a);
    if ((r = rsk::launch_check("k_cc_rows"))) return r;
    hipLaunchKernelGGL(k_cc_insert, grid_m, blk, 0, s, a);
    if ((r = rsk::launch_check("k_cc_insert"))) return r;
    if (t->cur_in) hipLaunchKernelGGL(k_cc_assign<true>, dim3(nt), blk, 0, s, a);
    else hipLaunchKernelGGL(k_cc_assign<false>, dim3(nt), blk, 0, s, a);
    return rsk::launch_check("k_cc_assign");
}
