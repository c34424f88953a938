// rsk_control.hip — control packets and the keepalive timer on the device's connection table
// (rsk_control_batch, rsk_keepalive_flush; include/rsk_codec.h): what IAppGroup::Input's control branches
// (conn/IAppGroup.cpp:76-96), ConnReset::Input (callbacks/ConnReset.cpp:43-90), NetConnKeepAlive::Input
// (callbacks/NetConnKeepAlive.cpp:37-98), IAppGroup::ProcessTcpFinOrRst (conn/IAppGroup.cpp:103-116) and
// NetConnKeepAlive::OnFlush (:110-145) do per packet and per conn, as passes over a batch and over the
// table's rows, with the messages to send as an order-stable compacted list.
//
// Both entry points are reduce-then-scan over tiles, three launches in a linear chain:
//   k_ctl_count / k_ka_count   per tile, the number of list entries its items will make (through LDS, one
//                              plain store per block: no atomics);
//   k_tile_scan (rsk_tile_dev.h, shared with rsk_conv.hip)   one block: exclusive scan of the tile counts in place, the totals to the
//                              caller's count words;
//   k_ctl_main / k_ka_main     the work itself; every item's list position = its tile's base + its rank
//                              inside the tile.
// No block waits on another, there is no look-back and no spin.  A message of the control pass never
// depends on a lookup (a KA_REQ is answered whether it hits or misses), so k_ctl_count reads two bytes
// per packet and, for cmd 3 only, the payload length.  Tile form as k_conn_resolve (rsk_conn.hip): lane t
// of a block takes items t, t + 256, ... of its tile, every column access is a whole wave at consecutive
// addresses, every step's loads are issued before the probes.
#include <hip/hip_runtime.h>

#include "rsk_tile_dev.h"

namespace {

using rsk::DevConnTab;
using rsk::funnel;
using rsk::gptr;
using rsk::k_tile_scan;
using rsk::kScanBlock;
using rsk::misaligned8;
using rsk::msg_out;
using rsk::MsgOut;
using rsk::msgs_any;
using rsk::put_msg;
using rsk::tile_positions;
using rsk::u32x2;

constexpr unsigned kBlock = rsk::kTileBlock;
constexpr unsigned kWaves = rsk::kTileWaves;
constexpr unsigned kCtlPer = 8;  // packets per thread: the resolve's tile
constexpr unsigned kKaPer = 4;   // rows per thread
static_assert(kBlock * kCtlPer == rsk::kControlTile && kBlock * kKaPer == rsk::kFlushTile,
              "scratch size (rsk_ctx.h) and tile sizes must agree");

// ---- rsk_control_batch ---------------------------------------------------------------------------------
struct CtlArgs {
    DevConnTab t;
    const int8_t *status;
    const uint8_t *cmd;
    const uint64_t *id;  // [n] IdBuf bytes as one word each, or NULL
    const uint64_t *conn_key;
    const uint16_t *pay_off, *pay_len;
    const uint8_t *arena;
    const uint64_t *base_off;
    const uint16_t *inner_off;
    const uint16_t *tcp_sp, *tcp_dp;
    const int8_t *miss;
    uint8_t *kind;
    uint64_t *arg;
    uint32_t *conn;
    uint32_t *rst_first;
    uint8_t *ka_tries;
    MsgOut m;
    u32x2 *tile;  // [tiles + 1] (messages, control packets) per tile; NULL when neither a list nor a count is asked for
    uint32_t n, capacity;
    bool by_id;
    bool close_ok;  // CLOSE packets are examined: the port columns are given and the table is not BY_ID
    bool list;      // a message array is given
};

// What status and cmd alone decide: RSK_CTL_NONE, RSK_CTL_UNKNOWN, RSK_CTL_TCP_CLOSE, or for cmd 1..4 the
// kind of that number, which stands if the body is long enough (RSK_CTL_SHORT otherwise).
__device__ __forceinline__ uint32_t ctl_pre(int8_t st, uint32_t cm, bool close_ok) {
    if (st == RSK_RECV_VALID) return cm == RSK_CMD_DATA ? (uint32_t)RSK_CTL_NONE : cm <= 4u ? cm : (uint32_t)RSK_CTL_UNKNOWN;
    return st == RSK_RECV_CLOSE && close_ok ? (uint32_t)RSK_CTL_TCP_CLOSE : (uint32_t)RSK_CTL_NONE;
}
__device__ __forceinline__ uint32_t ctl_need(uint32_t pre) { return pre == RSK_CTL_CONV_RST ? 4u : 8u; }

__global__ __launch_bounds__(kBlock) void k_ctl_count(CtlArgs a) {
    __shared__ uint32_t red[2][kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * rsk::kControlTile + threadIdx.x;
    uint32_t pre[kCtlPer];
    bool live[kCtlPer], mis[kCtlPer];
#pragma unroll
    for (unsigned k = 0; k < kCtlPer; ++k) {
        const uint64_t i = base + k * kBlock;
        live[k] = i < a.n;
        const int8_t st = live[k] ? gptr(a.status)[i] : (int8_t)RSK_RECV_DROP;
        const uint32_t cm = live[k] ? gptr(a.cmd)[i] : 0u;
        mis[k] = live[k] && a.miss ? gptr(a.miss)[i] == RSK_RECV_VALID : false;
        pre[k] = ctl_pre(st, cm, a.close_ok);
    }
    uint32_t n_msg = 0, n_ctl = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kCtlPer; ++k) {
        bool msg = mis[k];
        if (pre[k] == RSK_CTL_KA_REQ) msg = gptr(a.pay_len)[base + k * kBlock] >= 8u || mis[k];
        n_msg += (uint32_t)__popcll(__ballot(msg));
        n_ctl += (uint32_t)__popcll(__ballot(pre[k] != RSK_CTL_NONE));
    }
    if ((threadIdx.x & 63u) == 0u) {
        red[0][threadIdx.x >> 6] = n_msg;
        red[1][threadIdx.x >> 6] = n_ctl;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        u32x2 s = u32x2{0u, 0u};
#pragma unroll
        for (unsigned w = 0; w < kWaves; ++w) {
            s.x += red[0][w];
            s.y += red[1][w];
        }
        gptr(a.tile)[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kBlock) void k_ctl_main(CtlArgs a) {
    __shared__ uint32_t cnt[kCtlPer][kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * rsk::kControlTile + threadIdx.x;
    bool live[kCtlPer], mis[kCtlPer];
    uint32_t kind[kCtlPer];
    // 1. status and cmd of every step (independent loads)
#pragma unroll
    for (unsigned k = 0; k < kCtlPer; ++k) {
        const uint64_t i = base + k * kBlock;
        live[k] = i < a.n;
        const int8_t st = live[k] ? gptr(a.status)[i] : (int8_t)RSK_RECV_DROP;
        const uint32_t cm = live[k] ? gptr(a.cmd)[i] : 0u;
        mis[k] = live[k] && a.miss ? gptr(a.miss)[i] == RSK_RECV_VALID : false;
        kind[k] = ctl_pre(st, cm, a.close_ok);
    }
    // 2. the columns a control packet needs: its length and the place of its body, the ports of a CLOSE
    //    packet, the IdBuf and the connKey where a lookup or a message takes them
    uint64_t arg[kCtlPer], idw[kCtlPer], ck[kCtlPer];
    const uint8_t *body[kCtlPer];
#pragma unroll
    for (unsigned k = 0; k < kCtlPer; ++k) {
        const uint64_t i = base + k * kBlock;
        arg[k] = idw[k] = ck[k] = 0ull;
        body[k] = nullptr;
        const uint32_t pre = kind[k];
        if (pre >= RSK_CTL_CONV_RST && pre <= RSK_CTL_KA_RESP) {
            if (gptr(a.pay_len)[i] < ctl_need(pre)) {
                kind[k] = RSK_CTL_SHORT;
            } else {
                body[k] = a.arena + gptr(a.base_off)[i] + (a.inner_off ? (uint64_t)gptr(a.inner_off)[i] : 0ull) +
                          gptr(a.pay_off)[i];
            }
        } else if (pre == RSK_CTL_TCP_CLOSE) {
            // rsk_key_for_tcp (KeyGenerator.cpp:16-25)
            arg[k] = 0x10000000ull | ((uint64_t)gptr(a.tcp_dp)[i] << 16) | (uint64_t)gptr(a.tcp_sp)[i];
        }
        const bool msg = mis[k] || kind[k] == RSK_CTL_KA_REQ;
        const bool look = kind[k] >= RSK_CTL_NETCONN_RST && kind[k] <= RSK_CTL_KA_RESP;
        if (a.id && ((look && a.by_id) || (msg && a.list))) idw[k] = gptr(a.id)[i];
        if (mis[k] && kind[k] != RSK_CTL_KA_REQ) ck[k] = gptr(a.conn_key)[i];
    }
    // 3. the body bytes [0, 4) / [0, 8): the aligned dwords that hold one of them, no other
#pragma unroll
    for (unsigned k = 0; k < kCtlPer; ++k) {
        if (!body[k]) continue;
        const uint32_t r = (uint32_t)(reinterpret_cast<uintptr_t>(body[k]) & 3u), need = ctl_need(kind[k]);
        const RSK_GLOBAL uint32_t *q = reinterpret_cast<const RSK_GLOBAL uint32_t *>(gptr(body[k] - r));
        const uint32_t w0 = q[0];
        const uint32_t w1 = r + need > 4u ? q[1] : 0u;
        const uint32_t w2 = r + need > 8u ? q[2] : 0u;
        const uint32_t lo = funnel(w1, w0, r);
        arg[k] = need == 4u ? (uint64_t)lo : ((uint64_t)funnel(w2, w1, r) << 32) | lo;
    }
    // 4. the probes
    uint32_t row[kCtlPer];
#pragma unroll
    for (unsigned k = 0; k < kCtlPer; ++k) {
        row[k] = RSK_CONN_NONE;
        if (kind[k] >= RSK_CTL_NETCONN_RST && kind[k] <= RSK_CTL_TCP_CLOSE)
            row[k] = rsk::conn_lookup(a.t, a.capacity, a.by_id, arg[k], idw[k]);
    }
    // 5. the per-packet outputs and the per-row effects
    bool msg[kCtlPer];
#pragma unroll
    for (unsigned k = 0; k < kCtlPer; ++k) {
        const uint64_t i = base + k * kBlock;
        msg[k] = mis[k] || kind[k] == RSK_CTL_KA_REQ;
        if (!live[k]) continue;
        if (a.kind) gptr(a.kind)[i] = (uint8_t)kind[k];
        if (a.arg) gptr(a.arg)[i] = arg[k];
        if (a.conn) gptr(a.conn)[i] = row[k];
        if (row[k] != RSK_CONN_NONE) {  // a row of the table: conn_lookup returns nothing else
            if (a.rst_first && (kind[k] == RSK_CTL_NETCONN_RST || kind[k] == RSK_CTL_TCP_CLOSE))
                atomicMin(a.rst_first + row[k], (uint32_t)i);
            if (a.ka_tries && kind[k] == RSK_CTL_KA_RESP) gptr(a.ka_tries)[row[k]] = (uint8_t)RSK_KA_NONE;
        }
    }
    // 6. the messages, in packet order
    if (!a.list) return;  // uniform over the grid
    uint32_t pos[kCtlPer];
    const uint32_t total = tile_positions<kCtlPer>(msg, gptr(a.tile)[blockIdx.x].x, cnt, pos);
    if (total == 0u) return;
#pragma unroll
    for (unsigned k = 0; k < kCtlPer; ++k) {
        // one message per packet at most, so a position is below n; the bound holds whatever the tile
        // bases are (columns changed between the passes)
        if (!msg[k] || pos[k] >= a.n) continue;
        const uint32_t i = (uint32_t)(base + k * kBlock);
        if (kind[k] == RSK_CTL_KA_REQ) {
            const bool hit = row[k] != RSK_CONN_NONE;
            put_msg(a.m, pos[k], hit ? RSK_CMD_KEEP_ALIVE_RESP : RSK_CMD_NETCONN_RST, arg[k], idw[k], i, hit ? 0ull : arg[k], 8u);
        } else {
            put_msg(a.m, pos[k], RSK_CMD_NETCONN_RST, ck[k], idw[k], i, ck[k], 8u);
        }
    }
}

// ---- rsk_keepalive_flush -------------------------------------------------------------------------------
struct KaArgs {
    const uint8_t *state;
    const uint64_t *conn_key;
    const uint64_t *ids;  // the table's IdBuf column as words, or NULL
    uint8_t *tries;
    const uint64_t *est;
    uint64_t now;
    int32_t delay;
    uint32_t max_retry;
    MsgOut m;
    uint32_t *dead_rows;
    u32x2 *tile;  // (requests, dead rows) per tile; NULL when no list and no count is asked for
    uint32_t capacity;
    bool online;
};

// OnFlush for one row (include/rsk_codec.h, steps 1-4): the row's new tries, whether a request goes out
// and whether the row timed out.  Reads the row's state and tries, and est only where step 2 needs it.
struct KaRow {
    uint32_t was, tries;
    bool emit, dead;
};
__device__ __forceinline__ KaRow ka_row(const KaArgs &a, uint32_t r) {
    KaRow o;
    const uint32_t st = gptr(a.state)[r];
    o.was = o.tries = gptr(a.tries)[r];
    o.emit = o.dead = false;
    if (!(st & RSK_CONN_LIVE)) {
        o.tries = RSK_KA_NONE;
        return o;
    }
    if (!a.online) return o;
    if (!(st & RSK_CONN_NEW)) {
        const uint64_t est = gptr(a.est)[r];
        if (a.now > est && (int32_t)(uint32_t)(a.now - est) >= a.delay) {
            const bool had = o.tries != RSK_KA_NONE;
            o.tries = had ? (o.tries + 1u) & 0xFFu : 0u;
            o.emit = !had || o.tries < a.max_retry;
        }
    }
    if (o.tries != RSK_KA_NONE && o.tries >= a.max_retry) {
        o.tries = RSK_KA_NONE;
        o.dead = true;
    }
    return o;
}

__global__ __launch_bounds__(kBlock) void k_ka_count(KaArgs a) {
    __shared__ uint32_t red[2][kWaves];
    uint32_t n_req = 0, n_dead = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kKaPer; ++k) {
        const uint32_t r = blockIdx.x * rsk::kFlushTile + k * kBlock + threadIdx.x;
        KaRow o;
        o.emit = o.dead = false;
        if (r < a.capacity) o = ka_row(a, r);
        n_req += (uint32_t)__popcll(__ballot(o.emit));
        n_dead += (uint32_t)__popcll(__ballot(o.dead));
    }
    if ((threadIdx.x & 63u) == 0u) {
        red[0][threadIdx.x >> 6] = n_req;
        red[1][threadIdx.x >> 6] = n_dead;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        u32x2 s = u32x2{0u, 0u};
#pragma unroll
        for (unsigned w = 0; w < kWaves; ++w) {
            s.x += red[0][w];
            s.y += red[1][w];
        }
        gptr(a.tile)[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kBlock) void k_ka_main(KaArgs a) {
    __shared__ uint32_t cnt[2][kKaPer][kWaves];
    bool emit[kKaPer], dead[kKaPer];
#pragma unroll
    for (unsigned k = 0; k < kKaPer; ++k) {
        const uint32_t r = blockIdx.x * rsk::kFlushTile + k * kBlock + threadIdx.x;
        emit[k] = dead[k] = false;
        if (r < a.capacity) {
            const KaRow o = ka_row(a, r);
            emit[k] = o.emit;
            dead[k] = o.dead;
            if (o.tries != o.was) gptr(a.tries)[r] = (uint8_t)o.tries;
        }
    }
    if (!a.tile) return;  // uniform over the grid: no list and no count
    const u32x2 tb = gptr(a.tile)[blockIdx.x];
    uint32_t pe[kKaPer], pd[kKaPer];
    const uint32_t ne = tile_positions<kKaPer>(emit, tb.x, cnt[0], pe);
    const uint32_t nd = tile_positions<kKaPer>(dead, tb.y, cnt[1], pd);
    if (ne == 0u && nd == 0u) return;
#pragma unroll
    for (unsigned k = 0; k < kKaPer; ++k) {
        const uint32_t r = blockIdx.x * rsk::kFlushTile + k * kBlock + threadIdx.x;
        // a row makes one entry per list at most, so a position is below the capacity
        if (emit[k] && pe[k] < a.capacity)
            put_msg(a.m, pe[k], RSK_CMD_KEEP_ALIVE_REQ, gptr(a.conn_key)[r], a.ids ? gptr(a.ids)[r] : 0ull, r, 0ull, 8u);
        if (dead[k] && a.dead_rows && pd[k] < a.capacity) gptr(a.dead_rows)[pd[k]] = r;
    }
}

}  // namespace

extern "C" int rsk_control_batch(rsk_ctx *c, const rsk_conn_table *t, uint32_t n, const rsk_control_in *in,
                                 const rsk_control_out *out, void *stream) {
    if (!c || !in || !out || !rsk::tab_lookup_ok(t)) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0;
    if (n && (!in->status || !in->cmd || !in->arena || !in->base_off || !in->pay_off || !in->pay_len || (by_id && !in->id)))
        return RSK_EINVAL;
    if ((in->tcp_sp == nullptr) != (in->tcp_dp == nullptr)) return RSK_EINVAL;
    if (in->miss && !in->conn_key) return RSK_EINVAL;
    if (misaligned8(in->id) || misaligned8(out->msgs.id) || (by_id && misaligned8(t->id))) return RSK_EINVAL;
    const bool list = msgs_any(out->msgs);
    if (list && !out->msgs.n_msg) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    int r;
    // a kernel, not a memset node: the captured chain control -> conn_close reads the column again (rsk_tile_dev.h)
    if (out->rst_first && (r = rsk::fill_words_async(out->rst_first, t->capacity, 0xFFFFFFFFu, s))) return r;
    if (n == 0) {
        if ((r = rsk::zero_word(out->msgs.n_msg, s))) return r;
        return rsk::zero_word(out->n_ctl, s);
    }
    CtlArgs a;
    a.t = rsk::dev_tab(t);
    a.status = in->status;
    a.cmd = in->cmd;
    a.id = reinterpret_cast<const uint64_t *>(in->id);
    a.conn_key = in->conn_key;
    a.pay_off = in->pay_off;
    a.pay_len = in->pay_len;
    a.arena = in->arena;
    a.base_off = in->base_off;
    a.inner_off = in->inner_off;
    a.tcp_sp = in->tcp_sp;
    a.tcp_dp = in->tcp_dp;
    a.miss = in->miss;
    a.kind = out->kind;
    a.arg = out->arg;
    a.conn = out->conn;
    a.rst_first = out->rst_first;
    a.ka_tries = out->ka_tries;
    a.m = msg_out(out->msgs);
    a.tile = nullptr;
    a.n = n;
    a.capacity = t->capacity;
    a.by_id = by_id;
    a.close_ok = in->tcp_sp && !by_id;
    a.list = list;
    const uint32_t nt = (uint32_t)(((uint64_t)n + rsk::kControlTile - 1u) / rsk::kControlTile);
    if (list || out->msgs.n_msg || out->n_ctl) {
        void *wsp = nullptr;
        if ((r = rsk::stream_ws(c, s, rsk::WS_CONTROL, rsk::control_ws_bytes(n), &wsp))) return r;
        a.tile = static_cast<u32x2 *>(wsp);
        hipLaunchKernelGGL(k_ctl_count, dim3(nt), dim3(kBlock), 0, s, a);
        if ((r = rsk::launch_check("k_ctl_count"))) return r;
        hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile, nt, out->msgs.n_msg, out->n_ctl);
        if ((r = rsk::launch_check("k_tile_scan"))) return r;
    }
    hipLaunchKernelGGL(k_ctl_main, dim3(nt), dim3(kBlock), 0, s, a);
    return rsk::launch_check("k_ctl_main");
}

extern "C" int rsk_keepalive_flush(rsk_ctx *c, const rsk_conn_table *t, const rsk_keepalive *ka,
                                   const rsk_keepalive_out *out, void *stream) {
    if (!c || !ka || !out || !rsk::tab_ok(t) || !t->state || !t->conn_key) return RSK_EINVAL;
    if (!ka->ka_tries || !ka->established_ms) return RSK_EINVAL;
    if (ka->max_retry < 1u || ka->max_retry > 254u) return RSK_EINVAL;
    const bool list = msgs_any(out->msgs);
    if ((list && !out->msgs.n_msg) || (out->dead_rows && !out->n_dead)) return RSK_EINVAL;
    if (out->msgs.id && (misaligned8(out->msgs.id) || misaligned8(t->id))) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    KaArgs a;
    a.state = t->state;
    a.conn_key = t->conn_key;
    a.ids = out->msgs.id ? reinterpret_cast<const uint64_t *>(t->id) : nullptr;
    a.tries = ka->ka_tries;
    a.est = ka->established_ms;
    a.now = ka->now_ms;
    a.delay = (int32_t)ka->request_delay_ms;
    a.max_retry = ka->max_retry;
    a.m = msg_out(out->msgs);
    a.dead_rows = out->dead_rows;
    a.tile = nullptr;
    a.capacity = t->capacity;
    a.online = ka->online != 0u;
    const uint32_t nt = (t->capacity + rsk::kFlushTile - 1u) / rsk::kFlushTile;
    int r;
    if (list || out->msgs.n_msg || out->dead_rows || out->n_dead) {
        void *wsp = nullptr;
        if ((r = rsk::stream_ws(c, s, rsk::WS_CONTROL, rsk::control_ws_bytes(0), &wsp))) return r;
        a.tile = static_cast<u32x2 *>(wsp);
        hipLaunchKernelGGL(k_ka_count, dim3(nt), dim3(kBlock), 0, s, a);
        if ((r = rsk::launch_check("k_ka_count"))) return r;
        hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanBlock), 0, s, a.tile, nt, out->msgs.n_msg, out->n_dead);
        if ((r = rsk::launch_check("k_tile_scan"))) return r;
    }
    hipLaunchKernelGGL(k_ka_main, dim3(nt), dim3(kBlock), 0, s, a);
    return rsk::launch_check("k_ka_main");
}
