// rsk_conn_create.hip — rsk_conn_create_batch (include/rsk_codec.h): the fake-TCP conns born in a receive batch,
// or dialled by a client, made on the device connection table: INetGroup::Input's miss path
// (conn/INetGroup.cpp:57-83) -> SNetGroup::CreateNetConn (server/SNetGroup.cpp:20-46) -> ServerNetManager::GetTcp
// (server/ServerNetManager.cpp:52-75) -> FakeTcp::Init -> AddNetConn.  The deduplication and the first-arrival
// ranking are rsk_conv_create.hip's; the conn index takes the new rows by k_index_build's rule; the pick index
// takes them by an order-stable merge.
//
// An ITEM is a considered packet (column form) or an offer (list form).  A linear chain on the stream; `work` as
// laid out in rsk_conn_create.h, hdr = the counts between launches:
//   k_cn_count      column form: per 2048-packet tile the packets with miss == VALID; *n_miss = 0
//   k_tile_scan     their exclusive scan; the total -> hdr[unknown]
//   k_cn_prep       list[p] = the p-th missing packet; the dedup table, the offer table, claim and orank cleared --
//                   as many entries as the items and the offers need; pick_counts as the index has them
//   k_cn_dedup      by block range: the items into the dedup table by key (entry = the lowest item of a key; the
//                   ballots of the items that ever held an entry -> mask); the offers into the offer table by
//                   4-tuple (entry = the lowest offer of a tuple)
//   k_cn_claim      per first arrival (mask, probed): its offer -- column form: the tuple's, and atomicMin of the
//                   item into claim[offer]; list form: its own unless the key is LIVE in the table
//   k_cn_count2     tile b: (items of tile b that take part: first arrival, an offer, and the offer's lowest
//                   claim; vacant rows of row tile b); the ballots -> mask
//   k_tile_scan     both scans; the totals -> hdr[offered], hdr[vacant]
//   k_cn_rank       first[j] = the j-th such item, vacant[j] = the j-th vacant row, orank[offer] = j
//   k_cn_rows       n_new = min(offered, vacant): the row columns, the lists, offer_row, the counts; the table
//                   of the new rows' IdBufs cleared
//   k_cn_insert     the new rows into tab->index -- a launch of its own, so that the row columns are complete
//                   before an entry names them; per new row its group's old {off, cnt} and entry, and its IdBuf
//                   into nlead (entry = the lowest j)
//   k_cn_lead       BY_ID + pick: key[j] = (place of the group << 32) | row, the place being the group's old
//                   offset or, for a group without candidates, the old total + its lowest j; the lowest j of
//                   such a group takes the first free or emptied (kPickGone) entry of its chain with one atomic
//                   (no id is compared in this launch: the IdBufs were looked up in the one before)
//   k_cn_sort       BY_ID + pick: skey = the keys in ascending order, each key's rank counted by its own lane
//                   over all keys through LDS (without BY_ID the rows are in order as they are)
//   k_cn_merge      pick, by block range: every old entry and every new row to its new place in work; every
//                   group entry with candidates to its new {off, cnt}
//   k_cn_apply      pick: cand and pos from work; the entries of the groups that had no candidates; the header
//   k_cn_assign     column form: a lookup per packet still missing, conn / hit / miss, n_miss
// Every kernel behind k_cn_prep leaves at once when there is no item, every kernel behind k_cn_rows when nothing
// was created.  No block waits on another and nothing spins; every probe loop is bounded by its table's size.
#include <hip/hip_runtime.h>

#include "rsk_conn_create.h"
#include "rsk_pick.h"
#include "rsk_tile_dev.h"

namespace {

using rsk::gptr;
using rsk::k_tile_scan;
using rsk::kConnEmpty;
using rsk::kScanBlock;
using rsk::tile_positions;
using rsk::u32x2;
using rsk::u32x4;

constexpr unsigned kBlock = rsk::kTileBlock;
constexpr unsigned kWaves = rsk::kTileWaves;
constexpr unsigned kPer = 8;
constexpr uint32_t kTile = kBlock * kPer;
constexpr unsigned kRowPer = 4;
static_assert(kTile == rsk::kControlTile, "scratch size (rsk_ctx.h) and tile size must agree");
static_assert(rsk::kCcMaxOffers / kTile <= 2u * (RSK_CONN_MAX_ROWS / rsk::kFlushTile), "the offer tiles fit the control scratch");
constexpr uint32_t kCcTot0 = 4;  // hdr: the candidates the pick index had

struct Args {
    rsk::DevConnTab t;
    uint8_t *state;
    uint64_t *tkey, *tids;
    uint32_t *tsrc, *tdst;
    uint16_t *tsp, *tdp;
    uint32_t *tseq, *tack;
    uint8_t *tflag;
    uint64_t *est;
    uint8_t *ka;
    uint64_t now_ms;
    uint32_t *index;
    const uint64_t *id, *key;  // the packets
    const uint32_t *src, *dst;
    const uint16_t *sp, *dp;
    uint32_t *conn;
    uint8_t *hit;
    int8_t *miss;
    uint32_t *n_miss;
    const uint32_t *osrc, *odst;  // the offers
    const uint16_t *osp, *odp;
    const uint32_t *oack;
    const uint8_t *oflag;
    const uint64_t *okey, *oid;
    const uint32_t *n_offer;
    uint32_t *new_rows, *new_first, *new_offer, *offer_row, *n_new, *n_full, *n_refused;
    uint32_t *pick, *pick_counts;
    uint32_t *hdr, *dedup, *list, *oidx, *ohash, *claim, *orank, *first, *vacant;  // work
    uint32_t *goff, *gcnt, *slot, *sj, *nlead, *wcand, *wposv;
    uint64_t *mask, *key64, *skey;
    u32x2 *tile;
    rsk::PickLayout pl;
    uint32_t n, capacity, u, m, m_max, c4, slots;
    bool by_id, list_form, repeat;
};

// the power of two >= 2 x, at least 4 (create_slots of rsk_conv_create.h), x >= 1
__device__ __forceinline__ uint32_t dslots_of(uint32_t x) {
    const uint32_t s = 1u << (32u - (uint32_t)__builtin_clz(2u * x - 1u));
    return s < 4u ? 4u : s;
}
__device__ __forceinline__ uint32_t offers(const Args &a) {
    const uint32_t no = *gptr(a.n_offer);
    return no < a.m_max ? no : a.m_max;
}
// the items of the call: hdr[unknown] was written by the scan before the launches that ask
__device__ __forceinline__ uint32_t items(const Args &a) {
    if (a.list_form) return offers(a);
    const uint32_t unk = gptr(a.hdr)[rsk::kCcUnknown];
    return unk < a.u ? unk : a.u;
}
// what item p stands for: an offer, or a packet (kConnEmpty when list[p] is none)
__device__ __forceinline__ uint32_t item_src(const Args &a, uint32_t p) {
    if (a.list_form) return p;
    const uint32_t i = gptr(a.list)[p];
    return i < a.n ? i : kConnEmpty;
}
__device__ __forceinline__ uint64_t src_key(const Args &a, uint32_t x) { return a.list_form ? gptr(a.okey)[x] : gptr(a.key)[x]; }
__device__ __forceinline__ uint64_t src_id(const Args &a, uint32_t x) {
    return !a.by_id ? 0ull : a.list_form ? gptr(a.oid)[x] : gptr(a.id)[x];
}
__device__ __forceinline__ uint64_t offer_tk(const Args &a, uint32_t o) { return rsk::tuple_key(gptr(a.osrc)[o], gptr(a.odst)[o]); }
__device__ __forceinline__ uint64_t offer_tp(const Args &a, uint32_t o) { return rsk::tuple_ports(gptr(a.osp)[o], gptr(a.odp)[o]); }
__device__ __forceinline__ uint32_t old_total(const Args &a) {
    const uint32_t t = gptr(a.pick)[0];
    return t < a.capacity ? t : a.capacity;
}
// the new conns of the call: offered <= items, vacant <= capacity, and never more than the lists hold
__device__ __forceinline__ uint32_t created(const Args &a, uint32_t it) {
    if (it == 0u) return 0u;
    const uint32_t k = gptr(a.hdr)[rsk::kCcOffered], v = gptr(a.hdr)[rsk::kCcVacant];
    const uint32_t c = k < v ? k : v;
    return c < a.m ? c : a.m;
}

__global__ __launch_bounds__(kBlock) void k_cn_count(Args a) {
    __shared__ uint32_t red[2][kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    if (a.n_miss && blockIdx.x == 0u && threadIdx.x == 0u) *gptr(a.n_miss) = 0u;  // k_cn_assign, a later launch, adds
    uint32_t c = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        c += (uint32_t)__popcll(__ballot(i < a.n && gptr(a.miss)[i] == (int8_t)RSK_RECV_VALID));
    }
    rsk::tile_store_counts(a.tile, c, 0u, red);
}

__global__ __launch_bounds__(kBlock) void k_cn_prep(Args a) {
    __shared__ uint32_t cnt[kPer][kWaves];
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        gptr(a.hdr)[rsk::kCcKeys] = 0u;  // k_cn_claim adds
        if (a.pick) {
            gptr(a.hdr)[kCcTot0] = old_total(a);
            if (a.pick_counts) {  // what a call that creates nothing reports; k_cn_apply writes over it
                gptr(a.pick_counts)[0] = gptr(a.pick)[1];
                gptr(a.pick_counts)[1] = gptr(a.pick)[0];
            }
        }
    }
    const uint32_t it = items(a);
    if (it == 0u) return;  // uniform over the grid
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x, stride = gridDim.x * kBlock, no = offers(a);
    const u32x4 empty = {kConnEmpty, kConnEmpty, kConnEmpty, kConnEmpty};
    for (uint32_t q = g; q < dslots_of(it) / 4u; q += stride) reinterpret_cast<RSK_GLOBAL u32x4 *>(gptr(a.dedup))[q] = empty;
    if (!a.list_form && no)
        for (uint32_t q = g; q < dslots_of(no) / 4u; q += stride) reinterpret_cast<RSK_GLOBAL u32x4 *>(gptr(a.ohash))[q] = empty;
    for (uint32_t o = g; o < no; o += stride) {
        gptr(a.orank)[o] = kConnEmpty;
        // claim holds 1 + an item; 0 is below every claim: the offer was consumed by an earlier call
        if (!a.list_form) gptr(a.claim)[o] = a.repeat && gptr(a.offer_row)[o] != RSK_CONN_NONE ? 0u : kConnEmpty;
    }
    if (a.list_form) return;
    const uint32_t tbase = gptr(a.tile)[blockIdx.x].x;
    if (tbase >= a.u) return;  // uniform over the block: nothing of this tile is considered
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    bool unk[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        unk[k] = i < a.n && gptr(a.miss)[i] == (int8_t)RSK_RECV_VALID;
    }
    uint32_t pos[kPer];
    if (tile_positions<kPer>(unk, tbase, cnt, pos) == 0u) return;
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k)
        if (unk[k] && pos[k] < a.u) gptr(a.list)[pos[k]] = (uint32_t)(base + k * kBlock);
}

// The entry of item p's key in the dedup table behind k_cn_dedup: the lowest item of the key.
__device__ __forceinline__ uint32_t dedup_find(const Args &a, uint32_t it, uint64_t key, uint64_t id) {
    const uint32_t ds = dslots_of(it);
    uint32_t s = rsk::conn_home(key, id, ds);
    for (uint32_t step = 0; step < ds; ++step, s = rsk::conn_next(s, ds)) {
        const uint32_t e = gptr(a.dedup)[s];
        if (e >= it) break;
        const uint32_t x = item_src(a, e);
        if (x != kConnEmpty && src_key(a, x) == key && src_id(a, x) == id) return e;
    }
    return kConnEmpty;
}

__global__ __launch_bounds__(kBlock) void k_cn_dedup(Args a, uint32_t item_blocks) {
    const uint32_t it = items(a);
    if (it == 0u) return;  // uniform over the grid
    if (blockIdx.x >= item_blocks) {  // the offers by tuple: k_index_build's rule, the lowest offer of a tuple wins
        const uint32_t o = (blockIdx.x - item_blocks) * kBlock + threadIdx.x, no = offers(a);
        if (o >= no) return;
        const uint64_t tk = offer_tk(a, o), tp = offer_tp(a, o);
        const uint32_t ds = dslots_of(no);
        uint32_t s = rsk::conn_home(tk, tp, ds);
        for (uint32_t step = 0; step < ds; ++step, s = rsk::conn_next(s, ds)) {
            const uint32_t e = atomicCAS(a.ohash + s, kConnEmpty, o);
            if (e == kConnEmpty) break;
            if (e < no && offer_tk(a, e) == tk && offer_tp(a, e) == tp) {
                atomicMin(a.ohash + s, o);
                break;
            }
        }
        return;
    }
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t x = p < it ? item_src(a, p) : kConnEmpty;
    bool cand = false;  // p held its key's entry at some time: only such an item can be the first arrival
    if (x != kConnEmpty) {
        const uint64_t key = src_key(a, x), id = src_id(a, x);
        const uint32_t ds = dslots_of(it);
        uint32_t s = rsk::conn_home(key, id, ds);
        // `it` items are inserted and ds >= 2 it: a free entry is met; the bound only keeps a corrupted launch
        // from spinning
        for (uint32_t step = 0; step < ds; ++step, s = rsk::conn_next(s, ds)) {
            uint32_t e = gptr(a.dedup)[s];  // a stale value is at worst too high or still free (rsk_conv_create.hip)
            if (e == kConnEmpty) e = atomicCAS(a.dedup + s, kConnEmpty, p);
            if (e == kConnEmpty) {
                cand = true;
                break;
            }
            if (e < it) {
                const uint32_t y = item_src(a, e);
                if (y != kConnEmpty && src_key(a, y) == key && src_id(a, y) == id) {
                    if (p < e) {
                        atomicMin(a.dedup + s, p);
                        cand = true;
                    }
                    break;
                }
            }
        }
    }
    const uint64_t cb = __ballot(cand);  // the wave's 64 items are one word of the mask
    if ((threadIdx.x & 63u) == 0u && p < it) gptr(a.mask)[p >> 6] = cb;
}

__global__ __launch_bounds__(kBlock) void k_cn_claim(Args a) {
    const uint32_t it = items(a);
    if (it == 0u) return;  // uniform over the grid
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & 63u;
    const bool held = p - lane < it;  // wave-uniform: the wave owns a word of the mask
    const uint64_t cb = held ? gptr(a.mask)[p >> 6] : 0ull;
    bool first = false;
    uint32_t x = kConnEmpty;
    uint64_t key = 0ull, id = 0ull;
    if (p < it && ((cb >> lane) & 1ull)) {
        x = item_src(a, p);
        if (x != kConnEmpty) {
            key = src_key(a, x);
            id = src_id(a, x);
            first = dedup_find(a, it, key, id) == p;
        }
    }
    const uint64_t fb = __ballot(first);
    if (lane == 0u && held) {
        gptr(a.mask)[p >> 6] = fb;
        if (fb && !a.list_form) atomicAdd(a.hdr + rsk::kCcKeys, (uint32_t)__popcll(fb));  // integer adds commute
    }
    if (!first) return;
    uint32_t o = kConnEmpty;
    if (a.list_form) {
        if (rsk::conn_lookup(a.t, a.capacity, a.by_id, key, id) == kConnEmpty) o = p;
    } else {
        const uint32_t no = offers(a);
        if (no) {
            const uint64_t tk = rsk::tuple_key(gptr(a.src)[x], gptr(a.dst)[x]), tp = rsk::tuple_ports(gptr(a.sp)[x], gptr(a.dp)[x]);
            const uint32_t ds = dslots_of(no);
            uint32_t s = rsk::conn_home(tk, tp, ds);
            for (uint32_t step = 0; step < ds; ++step, s = rsk::conn_next(s, ds)) {
                const uint32_t e = gptr(a.ohash)[s];
                if (e >= no) break;
                if (offer_tk(a, e) == tk && offer_tp(a, e) == tp) {
                    o = e;
                    break;
                }
            }
        }
        if (o != kConnEmpty) atomicMin(a.claim + o, p + 1u);  // the key with the lowest first packet takes the offer
    }
    gptr(a.oidx)[p] = o;
}

// Item p (a first arrival by the mask's bit) takes part: it has an offer, and the offer is its own.
__device__ __forceinline__ bool takes_part(const Args &a, uint32_t p, uint32_t no) {
    const uint32_t o = gptr(a.oidx)[p];
    if (o >= no) return false;
    return a.list_form || gptr(a.claim)[o] == p + 1u;
}
__device__ __forceinline__ bool is_vacant(const Args &a, uint32_t it, uint64_t r) {
    return it != 0u && r < a.capacity && !(gptr(a.state)[r] & RSK_CONN_LIVE);
}

__global__ __launch_bounds__(kBlock) void k_cn_count2(Args a) {
    __shared__ uint32_t red[2][kWaves];
    const uint32_t it = items(a), no = it ? offers(a) : 0u, lane = threadIdx.x & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    uint32_t ne = 0, nv = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t x = base + k * kBlock;
        const bool held = x - lane < it;
        const uint64_t fb = held ? gptr(a.mask)[x >> 6] : 0ull;
        const uint64_t eb = __ballot(((fb >> lane) & 1ull) != 0ull && x < it && takes_part(a, (uint32_t)x, no));
        if (lane == 0u && held) gptr(a.mask)[x >> 6] = eb;
        ne += (uint32_t)__popcll(eb);
        nv += (uint32_t)__popcll(__ballot(is_vacant(a, it, x)));
    }
    rsk::tile_store_counts(a.tile, ne, nv, red);
}

__global__ __launch_bounds__(kBlock) void k_cn_rank(Args a) {
    __shared__ uint32_t cnt_f[kPer][kWaves], cnt_v[kPer][kWaves];
    const uint32_t it = items(a);
    if (it == 0u) return;  // uniform over the grid
    const u32x2 tb = gptr(a.tile)[blockIdx.x];
    if (tb.x >= a.m && tb.y >= a.m) return;  // uniform over the block: nothing of this tile is stored
    const uint32_t no = offers(a);
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    bool f[kPer], v[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t x = base + k * kBlock;
        f[k] = x < it && ((gptr(a.mask)[x >> 6] >> (threadIdx.x & 63u)) & 1ull) != 0ull;
        v[k] = is_vacant(a, it, x);
    }
    uint32_t pf[kPer], pv[kPer];
    tile_positions<kPer>(f, tb.x, cnt_f, pf);
    tile_positions<kPer>(v, tb.y, cnt_v, pv);
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t x = base + k * kBlock;
        if (f[k] && pf[k] < a.m) {
            gptr(a.first)[pf[k]] = (uint32_t)x;
            const uint32_t o = gptr(a.oidx)[x];
            if (o < no) gptr(a.orank)[o] = pf[k];  // one item per offer takes part
        }
        if (v[k] && pv[k] < a.m) gptr(a.vacant)[pv[k]] = (uint32_t)x;
    }
}

__global__ __launch_bounds__(kBlock) void k_cn_rows(Args a) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x, stride = gridDim.x * kBlock;
    const uint32_t it = items(a), nn = created(a, it), no = offers(a);
    if (g == 0u) {
        const uint32_t off = it ? gptr(a.hdr)[rsk::kCcOffered] : 0u, keys = !it ? 0u : a.list_form ? no : gptr(a.hdr)[rsk::kCcKeys];
        if (a.n_new) *gptr(a.n_new) = nn;
        if (a.n_full) *gptr(a.n_full) = off - nn;
        if (a.n_refused) *gptr(a.n_refused) = keys >= off ? keys - off : 0u;
    }
    if (a.offer_row && g < no) {  // thread o owns offer_row[o]
        uint32_t row = RSK_CONN_NONE;
        if (nn) {
            const uint32_t j = gptr(a.orank)[g];
            if (j < nn) row = gptr(a.vacant)[j];
        }
        if (row < a.capacity || !(a.repeat && gptr(a.offer_row)[g] != RSK_CONN_NONE)) gptr(a.offer_row)[g] = row < a.capacity ? row : RSK_CONN_NONE;
    }
    if (nn == 0u) return;  // uniform over the grid
    if (a.pick && a.by_id) {
        const u32x4 empty = {kConnEmpty, kConnEmpty, kConnEmpty, kConnEmpty};
        for (uint32_t q = g; q < dslots_of(nn) / 4u; q += stride) reinterpret_cast<RSK_GLOBAL u32x4 *>(gptr(a.nlead))[q] = empty;
    }
    if (g >= nn) return;
    const uint32_t r = gptr(a.vacant)[g], p = gptr(a.first)[g];
    if (r >= a.capacity || p >= it) return;  // k_cn_rank wrote a row and an item
    const uint32_t x = item_src(a, p), o = gptr(a.oidx)[p];
    if (x == kConnEmpty || o >= no) return;
    gptr(a.tkey)[r] = src_key(a, x);
    if (a.by_id) gptr(a.tids)[r] = src_id(a, x);
    gptr(a.tsrc)[r] = gptr(a.osrc)[o];
    gptr(a.tdst)[r] = gptr(a.odst)[o];
    gptr(a.tsp)[r] = gptr(a.osp)[o];
    gptr(a.tdp)[r] = gptr(a.odp)[o];
    gptr(a.tflag)[r] = gptr(a.oflag)[o];
    const uint32_t oa = gptr(a.oack)[o];
    gptr(a.tseq)[r] = rsk::create_seq(oa);
    gptr(a.tack)[r] = rsk::create_ack(oa);
    if (a.est) gptr(a.est)[r] = a.now_ms;
    if (a.ka) gptr(a.ka)[r] = (uint8_t)RSK_KA_NONE;
    gptr(a.state)[r] = (uint8_t)(RSK_CONN_LIVE | RSK_CONN_ALIVE | RSK_CONN_NEW);
    if (a.new_rows) gptr(a.new_rows)[g] = r;
    if (a.new_first && !a.list_form) gptr(a.new_first)[g] = x;
    if (a.new_offer) gptr(a.new_offer)[g] = o;
}

// The group entry s of the pick index.
__device__ __forceinline__ u32x4 group_at(const Args &a, uint32_t s) {
    return reinterpret_cast<const RSK_GLOBAL u32x4 *>(gptr(a.pick + a.pl.group))[s];
}
__device__ __forceinline__ bool group_has(const Args &a, const u32x4 &q) {  // candidates, inside cand
    return q.w >= 1u && q.z < a.capacity && q.w <= a.capacity - q.z;
}

__global__ __launch_bounds__(kBlock) void k_cn_insert(Args a) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t it = items(a), nn = created(a, it);
    if (j >= nn) return;
    const uint32_t r = gptr(a.vacant)[j];
    if (r >= a.capacity) return;
    const uint64_t key = a.t.key(r), id = a.by_id ? a.t.id(r) : 0ull;
    uint32_t s = rsk::conn_home(key, id, a.slots);
    // k_index_build's rule: at most `capacity` entries are ever taken and slots >= 2 capacity
    for (uint32_t step = 0; step < a.slots; ++step, s = rsk::conn_next(s, a.slots)) {
        const uint32_t e = atomicCAS(a.index + s, kConnEmpty, r);
        if (e == kConnEmpty) break;
        if (e < a.capacity && a.t.key(e) == key && (!a.by_id || a.t.id(e) == id)) {
            atomicMin(a.index + s, r);  // the lowest row of a key wins
            break;
        }
    }
    if (!a.pick) return;
    if (!a.by_id) {  // one group at 0; the rows are ascending in j
        gptr(a.skey)[j] = r;
        gptr(a.sj)[j] = j;
        gptr(a.goff)[j] = 0u;
        gptr(a.gcnt)[j] = gptr(a.hdr)[kCcTot0];
        return;
    }
    uint32_t off = kConnEmpty, cnt = 0u;  // the group's candidates; none: k_cn_lead finds it an entry
    s = rsk::conn_home(0ull, id, a.slots);
    for (uint32_t step = 0; step < a.slots; ++step, s = rsk::conn_next(s, a.slots)) {
        const u32x4 q = group_at(a, s);
        if (q.w == 0u) break;  // free: the IdBuf has no entry
        if (((uint64_t)q.x | ((uint64_t)q.y << 32)) == id) {
            if (group_has(a, q)) {
                off = q.z;
                cnt = q.w;
            }
            break;
        }
    }
    gptr(a.goff)[j] = off;
    gptr(a.gcnt)[j] = cnt;
    gptr(a.slot)[j] = kConnEmpty;
    const uint32_t ds = dslots_of(nn);
    s = rsk::conn_home(0ull, id, ds);
    for (uint32_t step = 0; step < ds; ++step, s = rsk::conn_next(s, ds)) {
        const uint32_t e = atomicCAS(a.nlead + s, kConnEmpty, j);
        if (e == kConnEmpty) break;
        if (e < nn) {
            const uint32_t re = gptr(a.vacant)[e];
            if (re < a.capacity && a.t.id(re) == id) {
                atomicMin(a.nlead + s, j);
                break;
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_cn_lead(Args a) {  // BY_ID with a pick index
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t it = items(a), nn = created(a, it);
    if (j >= nn) return;
    const uint32_t r = gptr(a.vacant)[j];
    if (r >= a.capacity) {
        gptr(a.key64)[j] = ~0ull;
        return;
    }
    const uint64_t id = a.t.id(r);
    uint32_t jf = j;  // the lowest j of the IdBuf
    const uint32_t ds = dslots_of(nn);
    uint32_t s = rsk::conn_home(0ull, id, ds);
    for (uint32_t step = 0; step < ds; ++step, s = rsk::conn_next(s, ds)) {
        const uint32_t e = gptr(a.nlead)[s];
        if (e >= nn) break;
        const uint32_t re = gptr(a.vacant)[e];
        if (re < a.capacity && a.t.id(re) == id) {
            jf = e;
            break;
        }
    }
    const uint32_t off = gptr(a.goff)[j];
    const uint32_t place = off != kConnEmpty ? off : gptr(a.hdr)[kCcTot0] + jf;  // below 2^21
    gptr(a.key64)[j] = ((uint64_t)place << 32) | r;
    if (jf != j || off != kConnEmpty) return;
    // The lowest j of a group without candidates takes the first entry of its IdBuf's chain that is free (count 0)
    // or was left without candidates by a close (kPickGone): one compare-and-swap on the count word, or on the offset
    // word, to kPickTakenOff, which no other claimant takes for either.  No id is read: the claimants are
    // deduplicated, a group with candidates is never taken from, and an IdBuf whose emptied entry another group
    // takes is simply one without an entry -- what it was to every pick already.  So the entries in use never
    // exceed the groups that have candidates plus the entries no chain has reached yet, however many IdBufs a
    // table sees in its life.  (The IdBuf's own emptied entry, if it has one, lies on this walk too.)
    s = rsk::conn_home(0ull, id, a.slots);
    for (uint32_t step = 0; step < a.slots; ++step, s = rsk::conn_next(s, a.slots)) {
        uint32_t *g = a.pick + a.pl.group + 4u * s;
        const uint32_t c = __hip_atomic_load(g + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == 0u) {
            if (atomicCAS(g + 3, 0u, rsk::kPickGoneCnt) != 0u) continue;
            __hip_atomic_store(g + 2, rsk::kPickTakenOff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (c != rsk::kPickGoneCnt ||
                   atomicCAS(g + 2, rsk::kPickGoneOff, rsk::kPickTakenOff) != rsk::kPickGoneOff) {
            continue;
        }
        gptr(g)[0] = (uint32_t)id;
        gptr(g)[1] = (uint32_t)(id >> 32);
        gptr(a.slot)[j] = s;
        break;
    }
}

// skey = key64 in ascending order (the keys differ: a row is new once): lane j counts the keys below its own.
__global__ __launch_bounds__(kBlock) void k_cn_sort(Args a) {
    __shared__ uint64_t tile[kBlock];
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t it = items(a), nn = created(a, it);
    if (blockIdx.x * kBlock >= nn) return;  // uniform over the block
    const uint64_t mine = j < nn ? gptr(a.key64)[j] : 0ull;
    uint32_t rank = 0;
    for (uint32_t base = 0; base < nn; base += kBlock) {
        const uint32_t q = base + threadIdx.x;
        tile[threadIdx.x] = q < nn ? gptr(a.key64)[q] : ~0ull;
        __syncthreads();
#pragma unroll 8
        for (unsigned k = 0; k < kBlock; ++k) rank += tile[k] < mine;
        __syncthreads();
    }
    if (j < nn && rank < nn) {
        gptr(a.skey)[rank] = mine;
        gptr(a.sj)[rank] = j;
    }
}

struct SKeys {
    const uint64_t *k;
    __device__ __forceinline__ uint64_t operator()(uint32_t i) const { return gptr(k)[i]; }
};

__global__ __launch_bounds__(kBlock) void k_cn_merge(Args a, uint32_t tiles, uint32_t new_blocks) {
    const uint32_t it = items(a), nn = created(a, it);
    if (nn == 0u) return;  // uniform over the grid
    const uint32_t tot0 = gptr(a.hdr)[kCcTot0];
    const SKeys sk{a.skey};
    uint32_t b = blockIdx.x;
    if (b < tiles) {  // the old entries
#pragma unroll
        for (unsigned k = 0; k < kRowPer; ++k) {
            const uint32_t i = b * rsk::kPickTile + k * kBlock + threadIdx.x;
            if (i >= tot0) continue;
            const uint32_t r = gptr(a.pick)[a.pl.cand + i];  // i < capacity <= C4
            if (r >= a.capacity) continue;
            uint32_t p = i, o = 0u;
            if (a.by_id) {
                p = gptr(a.pick)[a.pl.pos + r];
                if (p > i) continue;  // no index a build or an update left
                o = i - p;
            }
            const uint32_t t = rsk::lower_bound_u64(sk, nn, ((uint64_t)o << 32) | r);
            const uint32_t t0 = a.by_id ? rsk::lower_bound_u64(sk, nn, (uint64_t)o << 32) : 0u;
            if (i + t < a.c4) {
                gptr(a.wcand)[i + t] = r;
                gptr(a.wposv)[i + t] = p + (t - t0);
            }
        }
        return;
    }
    b -= tiles;
    if (b < new_blocks) {  // the new rows
        const uint32_t t = b * kBlock + threadIdx.x;
        if (t >= nn) return;
        const uint64_t key = gptr(a.skey)[t];
        const uint32_t r = (uint32_t)key, j = gptr(a.sj)[t];
        if (r >= a.capacity || j >= nn) return;
        const uint32_t off = gptr(a.goff)[j], cnt = gptr(a.gcnt)[j];
        uint32_t ip = tot0, lb = 0u, t0;
        if (off != kConnEmpty && off < a.capacity && cnt <= a.capacity - off) {
            uint32_t lo = 0, hi = cnt;  // the rows of the group's old candidates below r
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (gptr(a.pick)[a.pl.cand + off + mid] < r) lo = mid + 1u;
                else hi = mid;
            }
            lb = lo;
            ip = off + lb;
            t0 = a.by_id ? rsk::lower_bound_u64(sk, nn, (uint64_t)off << 32) : 0u;
        } else {
            t0 = rsk::lower_bound_u64(sk, nn, key & 0xFFFFFFFF00000000ull);
        }
        if (ip + t < a.c4) {
            gptr(a.wcand)[ip + t] = r;
            gptr(a.wposv)[ip + t] = lb + (t - t0);
        }
        return;
    }
    b -= new_blocks;  // BY_ID: the entries of the groups that have candidates; each lane reads and writes its own
    const uint32_t s = b * kBlock + threadIdx.x;
    if (s >= a.slots) return;
    RSK_GLOBAL u32x4 *ge = reinterpret_cast<RSK_GLOBAL u32x4 *>(gptr(a.pick + a.pl.group)) + s;
    u32x4 q = *ge;
    if (!group_has(a, q)) return;
    const uint32_t t0 = rsk::lower_bound_u64(sk, nn, (uint64_t)q.z << 32), t1 = rsk::lower_bound_u64(sk, nn, ((uint64_t)q.z + 1u) << 32);
    if (t1 == 0u) return;  // no new row stands before or inside the group
    q.z += t0;
    q.w += t1 - t0;
    *ge = q;
}

__global__ __launch_bounds__(kBlock) void k_cn_apply(Args a, uint32_t tiles) {
    const uint32_t it = items(a), nn = created(a, it);
    if (nn == 0u) return;  // uniform over the grid
    const uint32_t tot0 = gptr(a.hdr)[kCcTot0];
    const uint32_t total = tot0 + nn < a.capacity ? tot0 + nn : a.capacity;  // candidates are rows: never more
    uint32_t b = blockIdx.x;
    if (b < tiles) {
        if (b == 0u && threadIdx.x == 0u) {
            gptr(a.pick)[0] = total;
            if (a.pick_counts) gptr(a.pick_counts)[1] = total;
            if (!a.by_id) {
                gptr(a.pick)[1] = 1u;
                if (a.pick_counts) gptr(a.pick_counts)[0] = 1u;
            }
        }
#pragma unroll
        for (unsigned k = 0; k < kRowPer; ++k) {
            const uint32_t p = b * rsk::kPickTile + k * kBlock + threadIdx.x;
            if (p >= total) continue;
            const uint32_t r = gptr(a.wcand)[p];
            if (r >= a.capacity) continue;  // only behind an index that was none
            gptr(a.pick)[a.pl.cand + p] = r;
            gptr(a.pick)[a.pl.pos + r] = gptr(a.wposv)[p];
        }
        return;
    }
    b -= tiles;  // BY_ID: the groups that had no candidates, by the lowest j of each
    const uint32_t j = b * kBlock + threadIdx.x;
    if (j >= nn || gptr(a.goff)[j] != kConnEmpty) return;
    const uint64_t key = gptr(a.key64)[j];
    if ((uint32_t)(key >> 32) != tot0 + j) return;
    const uint32_t s = gptr(a.slot)[j];
    if (s >= a.slots) return;
    const SKeys sk{a.skey};
    const uint64_t lo = key & 0xFFFFFFFF00000000ull;
    const uint32_t t0 = rsk::lower_bound_u64(sk, nn, lo), t1 = rsk::lower_bound_u64(sk, nn, lo + (1ull << 32));
    uint32_t *g = a.pick + a.pl.group + 4u * s;
    gptr(g)[2] = tot0 + t0;
    gptr(g)[3] = t1 - t0;  // >= 1: the lane's own row
    atomicAdd(a.pick + 1, 1u);  // integer adds commute
    if (a.pick_counts) atomicAdd(a.pick_counts, 1u);
}

__global__ __launch_bounds__(kBlock) void k_cn_assign(Args a) {
    __shared__ uint32_t wave_left[kWaves];
    const uint32_t unk0 = gptr(a.hdr)[rsk::kCcUnknown];
    if (unk0 == 0u) return;  // uniform over the grid; k_cn_count zeroed *n_miss
    const uint32_t it = items(a), nn = created(a, it);
    if (nn == 0u) {  // nothing was created: every missing packet stays missing
        if (a.n_miss && blockIdx.x == 0u && threadIdx.x == 0u) *gptr(a.n_miss) = unk0;
        return;
    }
    const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    uint32_t left = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        const bool unk = i < a.n && gptr(a.miss)[i] == (int8_t)RSK_RECV_VALID;
        uint32_t row = RSK_CONN_NONE;
        if (unk) row = rsk::conn_lookup(a.t, a.capacity, a.by_id, gptr(a.key)[i], a.by_id ? gptr(a.id)[i] : 0ull);
        if (row != RSK_CONN_NONE) {
            gptr(a.conn)[i] = row;
            if (a.hit) gptr(a.hit)[i] = (uint8_t)1;
            gptr(a.miss)[i] = (int8_t)RSK_RECV_DROP;
        }
        left += (uint32_t)__popcll(__ballot(unk && row == RSK_CONN_NONE));
    }
    if (a.n_miss) {
        if ((threadIdx.x & 63u) == 0u) wave_left[threadIdx.x >> 6] = left;
        __syncthreads();
        if (threadIdx.x == 0u) {
            uint32_t total = 0;
#pragma unroll
            for (unsigned w = 0; w < kWaves; ++w) total += wave_left[w];
            if (total) atomicAdd(a.n_miss, total);
        }
    }
}

uint32_t tiles_of(uint64_t items) { return (uint32_t)((items + kTile - 1u) / kTile); }
uint32_t blocks_of(uint64_t items) { return (uint32_t)((items + kBlock - 1u) / kBlock); }

}  // namespace

extern "C" int rsk_conn_create_batch(rsk_ctx *c, const rsk_conn_table *t, const rsk_conn_create_rows *rows, uint32_t n,
                                     const rsk_conn_create_in *in, const rsk_conn_create_out *out, void *stream) {
    if (!c || !rsk::conn_create_args_ok(t, rows, n, in, out, true)) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0, list = (in->flags & RSK_CONN_CREATE_LIST) != 0;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    int r;
    const rsk_conn_offers &of = in->offers;
    const rsk::ConnCreateLayout l = rsk::conn_create_layout(in->u_max, of.m_max, t->capacity);
    uint32_t *w = static_cast<uint32_t *>(in->work);
    Args a;
    a.t = rsk::dev_tab(t);
    a.state = rows->state;
    a.tkey = rows->conn_key;
    a.tids = by_id ? reinterpret_cast<uint64_t *>(rows->id) : nullptr;
    a.tsrc = rows->src;
    a.tdst = rows->dst;
    a.tsp = rows->sp;
    a.tdp = rows->dp;
    a.tseq = rows->seq;
    a.tack = rows->ack;
    a.tflag = rows->flag;
    a.est = in->established_ms;
    a.ka = in->ka_tries;
    a.now_ms = in->now_ms;
    a.index = t->index;
    a.id = reinterpret_cast<const uint64_t *>(in->id);
    a.key = in->conn_key;
    a.src = in->src;
    a.dst = in->dst;
    a.sp = in->sp;
    a.dp = in->dp;
    a.conn = out->conn;
    a.hit = out->hit;
    a.miss = out->miss;
    a.n_miss = list ? nullptr : out->n_miss;
    a.osrc = of.src;
    a.odst = of.dst;
    a.osp = of.sp;
    a.odp = of.dp;
    a.oack = of.ack;
    a.oflag = of.flag;
    a.okey = of.conn_key;
    a.oid = reinterpret_cast<const uint64_t *>(of.id);
    a.n_offer = of.n_offer;
    a.new_rows = out->new_rows;
    a.new_first = out->new_first;
    a.new_offer = out->new_offer;
    a.offer_row = out->offer_row;
    a.n_new = out->n_new;
    a.n_full = out->n_full;
    a.n_refused = out->n_refused;
    a.pick = out->pick;
    a.pick_counts = out->pick ? out->pick_counts : nullptr;
    a.hdr = w;
    a.mask = reinterpret_cast<uint64_t *>(w + l.mask);
    a.dedup = w + l.dedup;
    a.list = w + l.list;
    a.oidx = w + l.oidx;
    a.ohash = w + l.ohash;
    a.claim = w + l.claim;
    a.orank = w + l.orank;
    a.first = w + l.first;
    a.vacant = w + l.vacant;
    a.key64 = reinterpret_cast<uint64_t *>(w + l.key);
    a.skey = reinterpret_cast<uint64_t *>(w + l.skey);
    a.goff = w + l.goff;
    a.gcnt = w + l.gcnt;
    a.slot = w + l.slot;
    a.sj = w + l.sj;
    a.nlead = w + l.nlead;
    a.wcand = w + l.cand;
    a.wposv = w + l.posv;
    a.pl = rsk::pick_layout(t->capacity, by_id);
    a.n = n;
    a.capacity = t->capacity;
    a.u = in->u_max < n ? in->u_max : n;
    a.m_max = of.m_max;
    a.m = of.m_max < t->capacity ? of.m_max : t->capacity;
    a.c4 = (t->capacity + 3u) & ~3u;
    a.slots = rsk::conn_slots(t->capacity);
    a.by_id = by_id;
    a.list_form = list;
    a.repeat = (in->flags & RSK_CONN_CREATE_REPEAT) != 0;
    const uint32_t item_max = list ? of.m_max : a.u;  // the items a call can have
    const uint32_t nt = list ? tiles_of(of.m_max) : (n ? tiles_of(n) : 1u);
    const uint32_t nt_i = tiles_of(item_max), nt_c = tiles_of(t->capacity), nt2 = nt_i > nt_c ? (nt_i ? nt_i : 1u) : nt_c;
    void *wsp = nullptr;  // tiles(items) <= max(tiles(n), 1024) and tiles(capacity) <= 512: inside any reserve
    if ((r = rsk::stream_ws(c, s, rsk::WS_CONTROL, rsk::control_ws_bytes(n), &wsp))) return r;
    a.tile = static_cast<u32x2 *>(wsp);
    const dim3 blk(kBlock);
    if (!list) {
        hipLaunchKernelGGL(k_cn_count, dim3(nt), blk, 0, s, a);
        if ((r = rsk::launch_check("k_cn_count"))) return r;
        hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile, nt, a.hdr + rsk::kCcUnknown,
                           static_cast<uint32_t *>(nullptr));
        if ((r = rsk::launch_check("k_tile_scan"))) return r;
    }
    hipLaunchKernelGGL(k_cn_prep, dim3(nt), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cn_prep"))) return r;
    const uint32_t item_blocks = item_max ? blocks_of(item_max) : 1u;
    hipLaunchKernelGGL(k_cn_dedup, dim3(item_blocks + (list ? 0u : blocks_of(of.m_max))), blk, 0, s, a, item_blocks);
    if ((r = rsk::launch_check("k_cn_dedup"))) return r;
    hipLaunchKernelGGL(k_cn_claim, dim3(item_blocks), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cn_claim"))) return r;
    hipLaunchKernelGGL(k_cn_count2, dim3(nt2), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cn_count2"))) return r;
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile, nt2, a.hdr + rsk::kCcOffered, a.hdr + rsk::kCcVacant);
    if ((r = rsk::launch_check("k_tile_scan"))) return r;
    hipLaunchKernelGGL(k_cn_rank, dim3(nt2), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cn_rank"))) return r;
    const uint32_t new_blocks = blocks_of(a.m);
    hipLaunchKernelGGL(k_cn_rows, dim3(blocks_of(a.m > of.m_max ? a.m : of.m_max)), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cn_rows"))) return r;
    hipLaunchKernelGGL(k_cn_insert, dim3(new_blocks), blk, 0, s, a);
    if ((r = rsk::launch_check("k_cn_insert"))) return r;
    if (a.pick) {
        const uint32_t ptiles = (t->capacity + rsk::kPickTile - 1u) / rsk::kPickTile;
        if (by_id) {
            hipLaunchKernelGGL(k_cn_lead, dim3(new_blocks), blk, 0, s, a);
            if ((r = rsk::launch_check("k_cn_lead"))) return r;
            hipLaunchKernelGGL(k_cn_sort, dim3(new_blocks), blk, 0, s, a);
            if ((r = rsk::launch_check("k_cn_sort"))) return r;
        }
        // at most 2^10 tiles, 2^12 blocks of new rows and 2^13 of group entries
        hipLaunchKernelGGL(k_cn_merge, dim3(ptiles + new_blocks + (by_id ? blocks_of(a.slots) : 0u)), blk, 0, s, a, ptiles, new_blocks);
        if ((r = rsk::launch_check("k_cn_merge"))) return r;
        hipLaunchKernelGGL(k_cn_apply, dim3(ptiles + (by_id ? new_blocks : 0u)), blk, 0, s, a, ptiles);
        if ((r = rsk::launch_check("k_cn_apply"))) return r;
    }
    if (!list) {
        hipLaunchKernelGGL(k_cn_assign, dim3(nt), blk, 0, s, a);
        if ((r = rsk::launch_check("k_cn_assign"))) return r;
    }
    return RSK_OK;
}
