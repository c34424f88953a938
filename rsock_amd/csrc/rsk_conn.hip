// rsk_conn.hip — the fake-TCP connection table on the device (rsk_conn_table, include/rsk_codec.h):
// INetGroup's map from connKey to INetConn (conn/INetGroup.cpp:57-83) as an open-addressing index over
// caller-owned columns, and the TcpInfo of each FakeTcp (conn/FakeTcp.cpp:14-50) as those columns.
//
//   k_index_build   (rsk_conn_dev.h, shared with the conv table through the accessor) launched twice per
//                   rebuild: clear the index, then insert the LIVE rows; the lowest row of a key wins.
//   k_conn_resolve  one lane per packet and step, 8 steps per block; the probe runs through global memory
//                   (the index and the key column of a table of rsock's size stay in L2).
//   k_conn_expand   one lane per packet; a gather from the row's columns, every output column stored
//                   by whole waves at consecutive addresses.
// The hash and the probe rule are rsk_conn.h's, shared with the host twins (rsk_host.cpp).  No scratch
// and no host state: a memset node for a given count and one kernel per call.
#include <hip/hip_runtime.h>

#include "rsk_conn_dev.h"

namespace {

using rsk::DevConnTab;
using rsk::dev_tab;
using rsk::gptr;
using rsk::tab_lookup_ok;
using rsk::tab_ok;
using rsk::wave_count;
using rsk::zero_word;

constexpr unsigned kBlock = 256;  // threads per block
static_assert((uint64_t)RSK_MAX_BATCH + 8u * kBlock - 1u <= 0xFFFFFFFFull, "the block counts are computed in 32 bits");

struct ResolveArgs {
    DevConnTab t;
    const int8_t *status;
    const uint8_t *cmd;
    const uint64_t *id;  // [n] IdBuf bytes as one word each
    const uint64_t *conn_key;
    uint32_t *conn;
    uint8_t *hit;
    int8_t *miss;
    uint32_t *n_miss;
    uint32_t n, capacity;
    bool by_id;
};

// A block takes kResolveTile consecutive packets, lane t the packets t, t + 256, ... of the tile (every
// load and store of a column is a whole wave at consecutive addresses).  The misses are counted by
// ballot per wave and step, summed over the block's waves through LDS, and added with one atomic per
// block: a batch in which every wave has a miss (a flood of unknown keys) otherwise queues n / 64
// atomics on one word, which took ten times the kernel's own time at 4M packets.
constexpr unsigned kResolvePer = 8;
constexpr unsigned kResolveTile = kBlock * kResolvePer;

__global__ __launch_bounds__(kBlock) void k_conn_resolve(ResolveArgs a) {
    __shared__ uint32_t wave_miss[kBlock / 64u];
    const uint64_t base = (uint64_t)blockIdx.x * kResolveTile + threadIdx.x;
    // the loads of every step first (independent), then the probes
    bool live[kResolvePer], look[kResolvePer];
    uint64_t key[kResolvePer], id[kResolvePer];
#pragma unroll
    for (unsigned k = 0; k < kResolvePer; ++k) {
        const uint64_t i = base + k * kBlock;
        live[k] = i < a.n;
        // status and cmd side by side (cmd is no key field): one round trip before the key's, not two
        const int8_t st = live[k] ? gptr(a.status)[i] : (int8_t)RSK_RECV_DROP;
        const uint8_t cm = live[k] && a.cmd ? gptr(a.cmd)[i] : (uint8_t)RSK_CMD_DATA;
        look[k] = st == RSK_RECV_VALID && cm == RSK_CMD_DATA;
        key[k] = id[k] = 0ull;
        if (look[k]) {  // the key fields of a packet that is not looked up are never read
            key[k] = gptr(a.conn_key)[i];
            if (a.by_id) id[k] = gptr(a.id)[i];
        }
    }
    uint32_t cnt = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kResolvePer; ++k) {
        const uint64_t i = base + k * kBlock;
        uint32_t row = RSK_CONN_NONE;
        if (look[k]) row = rsk::conn_lookup(a.t, a.capacity, a.by_id, key[k], id[k]);
        const bool miss = look[k] && row == RSK_CONN_NONE;
        if (live[k]) {
            gptr(a.conn)[i] = row;
            if (a.hit) gptr(a.hit)[i] = row != RSK_CONN_NONE;
            if (a.miss) gptr(a.miss)[i] = miss ? (int8_t)RSK_RECV_VALID : (int8_t)RSK_RECV_DROP;
        }
        cnt += (uint32_t)__popcll(__ballot(miss));
    }
    if (a.n_miss) {  // the word was zeroed on the stream ahead of this launch
        if ((threadIdx.x & 63u) == 0u) wave_miss[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0u) {
            uint32_t total = 0;
#pragma unroll
            for (unsigned w = 0; w < kBlock / 64u; ++w) total += wave_miss[w];
            if (total) atomicAdd(a.n_miss, total);
        }
    }
}

struct ExpandArgs {
    rsk_conn_table t;
    const uint32_t *conn;
    rsk_conn_expand_out o;
    uint32_t n;
};

__global__ __launch_bounds__(kBlock) void k_conn_expand(ExpandArgs a) {
    constexpr uint8_t kUp = RSK_CONN_LIVE | RSK_CONN_ALIVE;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < a.n;
    uint32_t r = 0;
    bool ok = false;
    if (live) {
        r = gptr(a.conn)[i];
        ok = r < a.t.capacity && (gptr(a.t.state)[r] & kUp) == kUp;
    }
    if (!ok) r = 0;  // a row every column has (capacity >= 1); its values are dropped below
    // the gathers first (independent loads), then the stores, column by column
    uint32_t src = 0, dst = 0, ack = 0, sp = 0, dp = 0, flag = 0;
    uint64_t key = 0, id = 0;
    if (ok) {
        if (a.o.src) src = gptr(a.t.src)[r];
        if (a.o.dst) dst = gptr(a.t.dst)[r];
        if (a.o.sp) sp = gptr(a.t.sp)[r];
        if (a.o.dp) dp = gptr(a.t.dp)[r];
        if (a.o.ack) ack = gptr((const uint32_t *)a.t.ack)[r];
        if (a.o.flag) flag = gptr(a.t.flag)[r];
        if (a.o.conn_key) key = gptr(a.t.conn_key)[r];
        if (a.o.id) id = gptr(reinterpret_cast<const uint64_t *>(a.t.id))[r];
    }
    if (live) {
        if (a.o.src) gptr(a.o.src)[i] = src;
        if (a.o.dst) gptr(a.o.dst)[i] = dst;
        if (a.o.sp) gptr(a.o.sp)[i] = (uint16_t)sp;
        if (a.o.dp) gptr(a.o.dp)[i] = (uint16_t)dp;
        if (a.o.ack) gptr(a.o.ack)[i] = ack;
        if (a.o.flag) gptr(a.o.flag)[i] = (uint8_t)flag;
        if (a.o.conn_key) gptr(a.o.conn_key)[i] = key;
        if (a.o.id) gptr(reinterpret_cast<uint64_t *>(a.o.id))[i] = id;
        gptr(a.o.ok)[i] = ok;
    }
    if (a.o.n_bad) wave_count(a.o.n_bad, live && !ok);
}

}  // namespace

extern "C" int rsk_conn_index_build(rsk_ctx *c, const rsk_conn_table *t, uint32_t *n_dup, void *stream) {
    if (!c || !tab_lookup_ok(t) || !t->state) return RSK_EINVAL;
    if (reinterpret_cast<uintptr_t>(t->index) & 15u) return RSK_EINVAL;
    if ((t->flags & RSK_CONN_BY_ID) && (reinterpret_cast<uintptr_t>(t->id) & 7u)) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    return rsk::index_build(dev_tab(t), t->index, t->state, t->capacity, (t->flags & RSK_CONN_BY_ID) != 0, n_dup,
                            (hipStream_t)stream);
}

extern "C" int rsk_conn_resolve_batch(rsk_ctx *c, const rsk_conn_table *t, uint32_t n, const rsk_conn_resolve_in *in,
                                      const rsk_conn_resolve_out *out, void *stream) {
    if (!c || !in || !out || !tab_lookup_ok(t)) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0;
    if (n && (!in->status || !in->conn_key || !out->conn || (by_id && !in->id))) return RSK_EINVAL;
    if (by_id && ((reinterpret_cast<uintptr_t>(t->id) | reinterpret_cast<uintptr_t>(in->id)) & 7u)) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (int r = zero_word(out->n_miss, s)) return r;
    if (n == 0) return RSK_OK;
    ResolveArgs a;
    a.t = dev_tab(t);
    a.status = in->status;
    a.cmd = in->cmd;
    a.id = reinterpret_cast<const uint64_t *>(in->id);
    a.conn_key = in->conn_key;
    a.conn = out->conn;
    a.hit = out->hit;
    a.miss = out->miss;
    a.n_miss = out->n_miss;
    a.n = n;
    a.capacity = t->capacity;
    a.by_id = by_id;
    hipLaunchKernelGGL(k_conn_resolve, dim3((n + kResolveTile - 1u) / kResolveTile), dim3(kBlock), 0, s, a);
    return rsk::launch_check("k_conn_resolve");
}

extern "C" int rsk_conn_expand_batch(rsk_ctx *c, const rsk_conn_table *t, uint32_t n, const uint32_t *conn,
                                     const rsk_conn_expand_out *out, void *stream) {
    if (!c || !out || !tab_ok(t) || !t->state) return RSK_EINVAL;
    if ((out->src && !t->src) || (out->dst && !t->dst) || (out->sp && !t->sp) || (out->dp && !t->dp) ||
        (out->ack && !t->ack) || (out->flag && !t->flag) || (out->conn_key && !t->conn_key) || (out->id && !t->id))
        return RSK_EINVAL;
    if (out->id && ((reinterpret_cast<uintptr_t>(t->id) | reinterpret_cast<uintptr_t>(out->id)) & 7u)) return RSK_EINVAL;
    if (n && (!conn || !out->ok)) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (int r = zero_word(out->n_bad, s)) return r;
    if (n == 0) return RSK_OK;
    ExpandArgs a;
    a.t = *t;
    a.conn = conn;
    a.o = *out;
    a.n = n;
    hipLaunchKernelGGL(k_conn_expand, dim3((n + kBlock - 1u) / kBlock), dim3(kBlock), 0, s, a);
    return rsk::launch_check("k_conn_expand");
}
