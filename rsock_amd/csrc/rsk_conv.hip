// rsk_conv.hip — the conv table on the device (rsk_conv_table, include/rsk_codec.h): the reference's last
// lookup before a payload reaches anybody -- SubGroup::OnRecv by BuildConvKey(dst, conv) in the SubGroup
// of the packet's IdBuf (server/SubGroup.cpp:31-50, server/ServerGroup.cpp:44-60), ClientGroup::OnRecv by
// conv (client/ClientGroup.cpp:65-80) -- with ConnReset::OnRecvConvRst / SendConvRst
// (callbacks/ConnReset.cpp:34-41, :67-77), the per-conv packet counts of IConn::DataStat
// (conn/IConn.cpp:63-79) and IGroup::Flush (conn/IGroup.cpp:81-107).
//
//   k_index_build    rsk_conn_dev.h's, over this table's accessor (key = dst:conv or conv).
//   k_conv_resolve   tile form of k_conn_resolve (rsk_conn.hip): lane t takes packets t, t + 256, ... of its
//                    2048-packet tile, whole-wave column accesses, all loads of a tile before the probes.
//                    The probe reads index, conv, dst, id -- never the counter columns, whose lines the
//                    atomics drop from the XCD's L2.  With cur_in given the tile's rows are combined on
//                    chip (tile_count_rows, rsk_tile_dev.h): one no-return atomic per distinct row and tile.
//                    With a list or a count asked for it also stores its tile's number of unknown packets.
//   k_tile_scan      rsk_tile_dev.h's: one block scans the tile counts.
//   k_conv_msgs      the CONV_RST list from the verdicts in conv_row, order-stable; no probes.
//   k_conv_send      gather of the row's conv, dst, id; cur_out counted as cur_in is.
//   k_cf_count / k_cf_main   IGroup::Flush over the rows, the launches of rsk_keepalive_flush.
// No block waits on another and nothing spins.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rsk_tile_dev.h"

namespace {

using rsk::gptr;
using rsk::k_tile_scan;
using rsk::kScanBlock;
using rsk::misaligned8;
using rsk::MsgOut;
using rsk::RowAgg;
using rsk::tile_positions;
using rsk::u32x2;
using rsk::zero_word;

constexpr unsigned kBlock = rsk::kTileBlock;
constexpr unsigned kWaves = rsk::kTileWaves;
constexpr unsigned kPer = 8;       // packets per thread: k_conn_resolve's tile
constexpr unsigned kFlushPer = 4;  // rows per thread
static_assert(kBlock * kPer == rsk::kControlTile && kBlock * kFlushPer == rsk::kFlushTile,
              "scratch size (rsk_ctx.h) and tile sizes must agree");
static_assert((uint64_t)RSK_MAX_BATCH + kBlock * kPer - 1u <= 0xFFFFFFFFull, "the block counts are computed in 32 bits");

constexpr uint32_t kFlags = RSK_CONV_BY_DST | RSK_CONV_BY_ID;

// The table as rsk_conn.h's conn_lookup and rsk_conn_dev.h's k_index_build take it.
struct DevConvTab {
    const uint32_t *index;
    const uint32_t *conv;
    const uint32_t *dst;
    const uint64_t *ids;  // the [C*8] IdBuf bytes, 8-B aligned, one word per row
    bool by_dst;
    __device__ __forceinline__ uint32_t entry(uint32_t s) const { return gptr(index)[s]; }
    __device__ __forceinline__ uint64_t key(uint32_t row) const {
        const uint64_t c = gptr(conv)[row];
        return by_dst ? ((uint64_t)gptr(dst)[row] << 32) | c : c;
    }
    __device__ __forceinline__ uint64_t id(uint32_t row) const { return gptr(ids)[row]; }
};

bool ctab_ok(const rsk_conv_table *t) {
    return t && !(t->flags & ~kFlags) && t->capacity >= 1u && t->capacity <= RSK_CONN_MAX_ROWS;
}
// what a lookup (and the build) reads
bool ctab_lookup_ok(const rsk_conv_table *t) {
    return ctab_ok(t) && t->state && t->conv && t->index && (!(t->flags & RSK_CONV_BY_DST) || t->dst) &&
           (!(t->flags & RSK_CONV_BY_ID) || t->id);
}
DevConvTab dev_ctab(const rsk_conv_table *t) {
    return DevConvTab{t->index, t->conv, t->dst, reinterpret_cast<const uint64_t *>(t->id), (t->flags & RSK_CONV_BY_DST) != 0};
}

// ---- rsk_conv_resolve_batch -----------------------------------------------------------------------------
struct ResolveArgs {
    DevConvTab t;
    const int8_t *status;
    const uint8_t *cmd, *hit;
    const uint64_t *id;  // [n] IdBuf bytes as one word each, or NULL
    const uint32_t *conv, *dst;
    const uint8_t *ctl_kind;
    const uint64_t *ctl_arg;
    uint32_t *conv_row;
    int8_t *unknown;
    uint32_t *rst_first;
    uint32_t *cur_in;
    MsgOut m;
    u32x2 *tile;  // [tiles + 1] the unknown packets per tile, twice; NULL when neither a list nor a count is asked for
    uint32_t n, capacity;
    bool by_id;
};

enum : uint32_t { kSkip = 0, kData = 1, kRst = 2 };

// What the columns that are no key fields decide for packet i (i < n).
__device__ __forceinline__ bool examined(const ResolveArgs &a, uint64_t i) {
    const bool data = gptr(a.status)[i] == RSK_RECV_VALID && (!a.cmd || gptr(a.cmd)[i] == RSK_CMD_DATA);
    return data && (!a.hit || gptr(a.hit)[i] != 0u);
}

template <bool COUNT>
__global__ __launch_bounds__(kBlock) void k_conv_resolve(ResolveArgs a) {
    __shared__ uint32_t red[2][kWaves];
    __shared__ std::conditional_t<COUNT, RowAgg<kPer>, char> agg;
    const uint64_t base = (uint64_t)blockIdx.x * rsk::kControlTile + threadIdx.x;
    // 1. the columns that decide what is looked up (independent loads)
    bool live[kPer];
    uint32_t mode[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        live[k] = i < a.n;
        mode[k] = kSkip;
        if (live[k]) {
            const bool ex = examined(a, i);
            const bool rst = a.ctl_kind && a.t.by_dst ? gptr(a.ctl_kind)[i] == RSK_CTL_CONV_RST : false;
            mode[k] = ex ? kData : rst ? kRst : kSkip;
        }
    }
    // 2. the key fields, only of the packets that are looked up
    uint64_t key[kPer], id[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        key[k] = id[k] = 0ull;
        if (mode[k] != kSkip) {
            key[k] = mode[k] == kData ? (uint64_t)gptr(a.conv)[i] : (uint64_t)(uint32_t)gptr(a.ctl_arg)[i];
            if (a.t.by_dst) key[k] |= (uint64_t)gptr(a.dst)[i] << 32;
            if (a.by_id) id[k] = gptr(a.id)[i];
        }
    }
    // 3. the probes
    uint32_t row[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        row[k] = RSK_CONN_NONE;
        if (mode[k] != kSkip) row[k] = rsk::conn_lookup(a.t, a.capacity, a.by_id, key[k], id[k]);
    }
    // 4. the per-packet outputs, the resets' rows
    uint32_t n_unk = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        const bool unk = mode[k] == kData && row[k] == RSK_CONN_NONE;
        if (live[k]) {
            gptr(a.conv_row)[i] = row[k];
            if (a.unknown) gptr(a.unknown)[i] = unk ? (int8_t)RSK_RECV_VALID : (int8_t)RSK_RECV_DROP;
            // a row of the table: conn_lookup returns nothing else
            if (a.rst_first && mode[k] == kRst && row[k] != RSK_CONN_NONE) atomicMin(a.rst_first + row[k], (uint32_t)i);
        }
        n_unk += (uint32_t)__popcll(__ballot(unk));
    }
    if (a.tile) rsk::tile_store_counts(a.tile, n_unk, n_unk, red);  // uniform over the grid
    // 5. cur_in: one atomic per distinct row of the tile
    if constexpr (COUNT) {
        uint32_t crow[kPer];
#pragma unroll
        for (unsigned k = 0; k < kPer; ++k) crow[k] = mode[k] == kData ? row[k] : RSK_CONN_NONE;
        rsk::tile_count_rows<kPer>(crow, a.cur_in, a.capacity, reinterpret_cast<RowAgg<kPer> &>(agg));
    }
}

// The list of the unknown packets: the verdict of packet i is examined(i) && conv_row[i] == NONE, as
// k_conv_resolve left it; tile[b].x = the list position of tile b's first entry.
__global__ __launch_bounds__(kBlock) void k_conv_msgs(ResolveArgs a) {
    __shared__ uint32_t cnt[kPer][kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * rsk::kControlTile + threadIdx.x;
    bool unk[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        unk[k] = i < a.n && examined(a, i) && gptr(a.conv_row)[i] == RSK_CONN_NONE;
    }
    uint32_t pos[kPer];
    const uint32_t total = tile_positions<kPer>(unk, gptr(a.tile)[blockIdx.x].x, cnt, pos);
    if (total == 0u) return;
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        // one message per packet at most, so a position is below n; the bound holds whatever the tile
        // bases are (columns changed between the passes)
        if (!unk[k] || pos[k] >= a.n) continue;
        const uint64_t i = base + k * kBlock;
        rsk::put_msg(a.m, pos[k], RSK_CMD_CONV_RST, (uint64_t)gptr(a.conv)[i], a.id ? gptr(a.id)[i] : 0ull, (uint32_t)i,
                     0ull, 4u);
    }
}

// ---- rsk_conv_send_batch ----------------------------------------------------------------------------------
struct SendArgs {
    const uint8_t *state;
    const uint32_t *tconv, *tdst;
    const uint64_t *tids;
    const uint32_t *conv_row;
    const int32_t *sent;
    uint32_t *conv, *dst;
    uint64_t *id;
    uint8_t *ok;
    uint32_t *n_bad;
    uint32_t *cur_out;
    uint32_t n, capacity;
};

template <bool COUNT>
__global__ __launch_bounds__(kBlock) void k_conv_send(SendArgs a) {
    __shared__ uint32_t wave_bad[kWaves];
    __shared__ std::conditional_t<COUNT, RowAgg<kPer>, char> agg;
    const uint64_t base = (uint64_t)blockIdx.x * rsk::kControlTile + threadIdx.x;
    bool live[kPer];
    uint32_t r[kPer];
    int32_t sn[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        live[k] = i < a.n;
        r[k] = live[k] ? gptr(a.conv_row)[i] : (uint32_t)RSK_CONN_NONE;
        sn[k] = COUNT && live[k] ? gptr(a.sent)[i] : 0;
    }
    bool ok[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) ok[k] = r[k] < a.capacity && (gptr(a.state)[r[k]] & RSK_CONN_LIVE);
    // the gathers (independent loads), then the stores, column by column
    uint32_t cv[kPer], ds[kPer];
    uint64_t idw[kPer];
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        cv[k] = ds[k] = 0u;
        idw[k] = 0ull;
        if (ok[k]) {
            if (a.conv) cv[k] = gptr(a.tconv)[r[k]];
            if (a.dst) ds[k] = gptr(a.tdst)[r[k]];
            if (a.id) idw[k] = gptr(a.tids)[r[k]];
        }
    }
    uint32_t bad = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kPer; ++k) {
        const uint64_t i = base + k * kBlock;
        if (live[k]) {
            if (a.conv) gptr(a.conv)[i] = cv[k];
            if (a.dst) gptr(a.dst)[i] = ds[k];
            if (a.id) gptr(a.id)[i] = idw[k];
            if (a.ok) gptr(a.ok)[i] = ok[k];
        }
        bad += (uint32_t)__popcll(__ballot(live[k] && !ok[k]));
    }
    if (a.n_bad) {  // the word was zeroed on the stream ahead of this launch; one atomic per block
        if ((threadIdx.x & 63u) == 0u) wave_bad[threadIdx.x >> 6] = bad;
        __syncthreads();
        if (threadIdx.x == 0u) {
            uint32_t total = 0;
#pragma unroll
            for (unsigned w = 0; w < kWaves; ++w) total += wave_bad[w];
            if (total) atomicAdd(a.n_bad, total);
        }
    }
    if constexpr (COUNT) {
        uint32_t crow[kPer];
#pragma unroll
        for (unsigned k = 0; k < kPer; ++k) crow[k] = ok[k] && sn[k] > 0 ? r[k] : (uint32_t)RSK_CONN_NONE;
        rsk::tile_count_rows<kPer>(crow, a.cur_out, a.capacity, reinterpret_cast<RowAgg<kPer> &>(agg));
    }
}

// ---- rsk_conv_flush -----------------------------------------------------------------------------------
struct FlushArgs {
    const uint8_t *state;
    uint8_t *alive;
    const uint32_t *cur_in, *cur_out;
    uint32_t *prev_in, *prev_out;
    uint32_t *dead_rows;
    u32x2 *tile;  // (dead rows, rows alive after the pass) per tile; NULL when no list and no count is asked for
    uint32_t capacity;
};

// IGroup::Flush for one row (include/rsk_codec.h, steps 1-3).  Reads state, then alive of a LIVE row, then
// the four counters of a row that is alive.
struct FlRow {
    bool dead, flush, alive;  // listed; DataStat::Flush runs; alive after the pass
    uint32_t ci, co;
};
__device__ __forceinline__ FlRow fl_row(const FlushArgs &a, uint32_t r) {
    FlRow o;
    o.dead = o.flush = o.alive = false;
    o.ci = o.co = 0u;
    if (!(gptr(a.state)[r] & RSK_CONN_LIVE)) return o;
    if (gptr(a.alive)[r] == 0u) {
        o.dead = true;
        return o;
    }
    o.flush = true;
    o.ci = gptr(a.cur_in)[r];
    o.co = gptr(a.cur_out)[r];
    o.alive = gptr(a.prev_in)[r] != o.ci && gptr(a.prev_out)[r] != o.co;
    return o;
}

__global__ __launch_bounds__(kBlock) void k_cf_count(FlushArgs a) {
    __shared__ uint32_t red[2][kWaves];
    uint32_t n_dead = 0, n_alive = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kFlushPer; ++k) {
        const uint32_t r = blockIdx.x * rsk::kFlushTile + k * kBlock + threadIdx.x;
        FlRow o;
        o.dead = o.alive = false;
        if (r < a.capacity) o = fl_row(a, r);
        n_dead += (uint32_t)__popcll(__ballot(o.dead));
        n_alive += (uint32_t)__popcll(__ballot(o.alive));
    }
    rsk::tile_store_counts(a.tile, n_dead, n_alive, red);
}

__global__ __launch_bounds__(kBlock) void k_cf_main(FlushArgs a) {
    __shared__ uint32_t cnt[kFlushPer][kWaves];
    bool dead[kFlushPer];
#pragma unroll
    for (unsigned k = 0; k < kFlushPer; ++k) {
        const uint32_t r = blockIdx.x * rsk::kFlushTile + k * kBlock + threadIdx.x;
        dead[k] = false;
        if (r < a.capacity) {
            const FlRow o = fl_row(a, r);
            dead[k] = o.dead;
            if (o.flush) {
                if (!o.alive) gptr(a.alive)[r] = (uint8_t)0;  // it was non-zero: DataStat::mAlive only ever falls here
                gptr(a.prev_in)[r] = o.ci;
                gptr(a.prev_out)[r] = o.co;
            }
        }
    }
    if (!a.tile || !a.dead_rows) return;  // uniform over the grid
    uint32_t pd[kFlushPer];
    const uint32_t nd = tile_positions<kFlushPer>(dead, gptr(a.tile)[blockIdx.x].x, cnt, pd);
    if (nd == 0u) return;
#pragma unroll
    for (unsigned k = 0; k < kFlushPer; ++k) {
        const uint32_t r = blockIdx.x * rsk::kFlushTile + k * kBlock + threadIdx.x;
        // a row makes one entry at most, so a position is below the capacity
        if (dead[k] && pd[k] < a.capacity) gptr(a.dead_rows)[pd[k]] = r;
    }
}

}  // namespace

extern "C" int rsk_conv_index_build(rsk_ctx *c, const rsk_conv_table *t, uint32_t *n_dup, void *stream) {
    if (!c || !ctab_lookup_ok(t)) return RSK_EINVAL;
    if (reinterpret_cast<uintptr_t>(t->index) & 15u) return RSK_EINVAL;
    if ((t->flags & RSK_CONV_BY_ID) && misaligned8(t->id)) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    return rsk::index_build(dev_ctab(t), t->index, t->state, t->capacity, (t->flags & RSK_CONV_BY_ID) != 0, n_dup,
                            (hipStream_t)stream);
}

extern "C" int rsk_conv_resolve_batch(rsk_ctx *c, const rsk_conv_table *t, uint32_t n, const rsk_conv_resolve_in *in,
                                      const rsk_conv_resolve_out *out, void *stream) {
    if (!c || !in || !out || !ctab_lookup_ok(t)) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONV_BY_ID) != 0, by_dst = (t->flags & RSK_CONV_BY_DST) != 0;
    if (n && (!in->status || !in->conv || !out->conv_row || (by_dst && !in->dst) || (by_id && !in->id))) return RSK_EINVAL;
    if (misaligned8(in->id) || misaligned8(out->msgs.id) || (by_id && misaligned8(t->id))) return RSK_EINVAL;
    if ((in->ctl_kind == nullptr) != (in->ctl_arg == nullptr)) return RSK_EINVAL;
    const bool list = rsk::msgs_any(out->msgs);
    if (list && !out->msgs.n_msg) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    int r;
    if (out->rst_first && (r = rsk::fill_words_async(out->rst_first, t->capacity, 0xFFFFFFFFu, s))) return r;
    if (n == 0) {
        if ((r = zero_word(out->msgs.n_msg, s))) return r;
        return zero_word(out->n_unknown, s);
    }
    ResolveArgs a;
    a.t = dev_ctab(t);
    a.status = in->status;
    a.cmd = in->cmd;
    a.hit = in->hit;
    a.id = reinterpret_cast<const uint64_t *>(in->id);
    a.conv = in->conv;
    a.dst = in->dst;
    a.ctl_kind = in->ctl_kind;
    a.ctl_arg = in->ctl_arg;
    a.conv_row = out->conv_row;
    a.unknown = out->unknown;
    a.rst_first = out->rst_first;
    a.cur_in = t->cur_in;
    a.m = rsk::msg_out(out->msgs);
    a.tile = nullptr;
    a.n = n;
    a.capacity = t->capacity;
    a.by_id = by_id;
    const uint32_t nt = (uint32_t)(((uint64_t)n + rsk::kControlTile - 1u) / rsk::kControlTile);
    const bool counts = list || out->msgs.n_msg || out->n_unknown;
    if (counts) {
        void *wsp = nullptr;
        if ((r = rsk::stream_ws(c, s, rsk::WS_CONTROL, rsk::control_ws_bytes(n), &wsp))) return r;
        a.tile = static_cast<u32x2 *>(wsp);
    }
    if (t->cur_in) hipLaunchKernelGGL(k_conv_resolve<true>, dim3(nt), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(k_conv_resolve<false>, dim3(nt), dim3(kBlock), 0, s, a);
    if ((r = rsk::launch_check("k_conv_resolve")) || !counts) return r;
    // both components of a tile's counts are its unknown packets: the two totals are n_msg and n_unknown
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile, nt, out->msgs.n_msg, out->n_unknown);
    if ((r = rsk::launch_check("k_tile_scan"))) return r;
    if (!list) return RSK_OK;
    hipLaunchKernelGGL(k_conv_msgs, dim3(nt), dim3(kBlock), 0, s, a);
    return rsk::launch_check("k_conv_msgs");
}

extern "C" int rsk_conv_send_batch(rsk_ctx *c, const rsk_conv_table *t, uint32_t n, const uint32_t *conv_row,
                                   const int32_t *sent, const rsk_conv_send_out *out, void *stream) {
    if (!c || !out || !ctab_ok(t) || !t->state) return RSK_EINVAL;
    if ((out->conv && !t->conv) || (out->dst && !t->dst) || (out->id && !t->id) || (sent && !t->cur_out)) return RSK_EINVAL;
    if (out->id && (misaligned8(out->id) || misaligned8(t->id))) return RSK_EINVAL;
    if (n && !conv_row) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (int r = zero_word(out->n_bad, s)) return r;
    if (n == 0) return RSK_OK;
    SendArgs a;
    a.state = t->state;
    a.tconv = t->conv;
    a.tdst = t->dst;
    a.tids = reinterpret_cast<const uint64_t *>(t->id);
    a.conv_row = conv_row;
    a.sent = sent;
    a.conv = out->conv;
    a.dst = out->dst;
    a.id = reinterpret_cast<uint64_t *>(out->id);
    a.ok = out->ok;
    a.n_bad = out->n_bad;
    a.cur_out = t->cur_out;
    a.n = n;
    a.capacity = t->capacity;
    const uint32_t nt = (uint32_t)(((uint64_t)n + rsk::kControlTile - 1u) / rsk::kControlTile);
    if (sent) hipLaunchKernelGGL(k_conv_send<true>, dim3(nt), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(k_conv_send<false>, dim3(nt), dim3(kBlock), 0, s, a);
    return rsk::launch_check("k_conv_send");
}

extern "C" int rsk_conv_flush(rsk_ctx *c, const rsk_conv_table *t, const rsk_conv_flush_out *out, void *stream) {
    if (!c || !out || !ctab_ok(t) || !t->state || !t->alive) return RSK_EINVAL;
    if (!t->cur_in || !t->cur_out || !t->prev_in || !t->prev_out) return RSK_EINVAL;
    if (out->dead_rows && !out->n_dead) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    FlushArgs a;
    a.state = t->state;
    a.alive = t->alive;
    a.cur_in = t->cur_in;
    a.cur_out = t->cur_out;
    a.prev_in = t->prev_in;
    a.prev_out = t->prev_out;
    a.dead_rows = out->dead_rows;
    a.tile = nullptr;
    a.capacity = t->capacity;
    const uint32_t nt = (t->capacity + rsk::kFlushTile - 1u) / rsk::kFlushTile;
    int r;
    if (out->dead_rows || out->n_dead || out->n_alive) {
        void *wsp = nullptr;
        if ((r = rsk::stream_ws(c, s, rsk::WS_CONTROL, rsk::control_ws_bytes(0), &wsp))) return r;
        a.tile = static_cast<u32x2 *>(wsp);
        hipLaunchKernelGGL(k_cf_count, dim3(nt), dim3(kBlock), 0, s, a);
        if ((r = rsk::launch_check("k_cf_count"))) return r;
        hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile, nt, out->n_dead, out->n_alive);
        if ((r = rsk::launch_check("k_tile_scan"))) return r;
    }
    hipLaunchKernelGGL(k_cf_main, dim3(nt), dim3(kBlock), 0, s, a);
    return rsk::launch_check("k_cf_main");
}
