// rsk_pick.hip — INetGroup::doSend's pick of a connection per outgoing packet (conn/INetGroup.cpp:111-135)
// on the device connection table (rsk_conn_pick_build, rsk_conn_pick_batch; include/rsk_codec.h).  The
// rule is the header's; the layout of the pick index and its lookup are rsk_pick.h's, shared with the host
// twins (rsk_host.cpp).
//
//   k_conn_pick     one lane per packet and step, 8 steps per block, as k_conn_resolve: the column loads
//                   of every step first, then the dependent chain (the group's 16-B entry, the candidate;
//                   with an avoid key the conn index's probe and the row's position).  No scratch, no host
//                   state: a memset node for a given count and this kernel.
//   the build       set-up rate: k_index_build (rsk_conn_dev.h) over the IdBufs of the candidate rows gives
//                   every group its lowest candidate as leader; k_pick_init, k_pick_count and the one-block
//                   k_pick_rank give the groups their entries, counts, offsets and the candidates their
//                   positions in row order.
#include <hip/hip_runtime.h>

#include "rsk_conn_dev.h"
#include "rsk_pick.h"

namespace {

using rsk::gptr;
using rsk::kConnEmpty;
using rsk::PickGroup;
using rsk::PickLayout;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned kBlock = 256;
constexpr unsigned kPickPer = 8;
constexpr unsigned kPickTile = kBlock * kPickPer;
static_assert((uint64_t)RSK_MAX_BATCH + kPickTile - 1u <= 0xFFFFFFFFull, "the block counts are computed in 32 bits");

// The pick index as rsk_pick.h's lookups take it.
struct DevPick {
    const uint32_t *w;
    PickLayout l;
    __device__ __forceinline__ uint32_t word(uint32_t i) const { return gptr(w)[i]; }
    __device__ __forceinline__ PickGroup group(uint32_t s) const {
        const u32x4 q = reinterpret_cast<const RSK_GLOBAL u32x4 *>(gptr(w + l.group))[s];
        return PickGroup{(uint64_t)q.x | ((uint64_t)q.y << 32), q.z, q.w};
    }
    __device__ __forceinline__ uint32_t cand(uint32_t i) const { return gptr(w)[l.cand + i]; }
    __device__ __forceinline__ uint32_t pos(uint32_t r) const { return gptr(w)[l.pos + r]; }
};

struct PickArgs {
    rsk::DevConnTab t;
    DevPick p;
    const int32_t *len;
    const uint64_t *id;  // [n] IdBuf bytes as one word each
    const uint64_t *avoid;
    const uint32_t *draw;
    uint64_t seed;
    uint32_t *conn;
    uint32_t *n_none;
    uint8_t *used;
    uint32_t n, capacity;
    bool by_id;
};

// The candidates of a client's one group staged in LDS (STAGE, tables without BY_ID only).
constexpr unsigned kPickLds = 1024;
struct LdsCand {
    const uint32_t *c;
    __device__ __forceinline__ uint32_t cand(uint32_t i) const { return c[i]; }
};

// A block takes kPickTile consecutive packets, lane t the packets t, t + 256, ... of the tile (every load
// and store of a column is a whole wave at consecutive addresses); the NONE count goes through LDS into
// one atomic per block.  With STAGE the block first copies the one group's candidates
// into LDS when there are at most kPickLds of them (the count is the index's, read here: no host state),
// and a packet's candidate is an LDS read; a larger group takes the loads from global memory as without.
template <bool STAGE>
__global__ __launch_bounds__(kBlock) void k_conn_pick(PickArgs a) {
    __shared__ uint32_t wave_none[kBlock / 64u];
    __shared__ uint32_t lds_cand[STAGE ? kPickLds : 1u];
    uint32_t m0 = 0;
    bool staged = false;
    if (STAGE) {
        m0 = a.p.word(0u);
        staged = m0 >= 1u && m0 <= kPickLds && m0 <= a.capacity;  // block-uniform
        if (staged)
            for (uint32_t j = threadIdx.x; j < m0; j += kBlock) lds_cand[j] = a.p.cand(j);
        __syncthreads();
    }
    const uint64_t base = (uint64_t)blockIdx.x * kPickTile + threadIdx.x;
    bool live[kPickPer], take[kPickPer];
    uint64_t id[kPickPer], av[kPickPer];
    uint32_t d[kPickPer];
#pragma unroll
    for (unsigned k = 0; k < kPickPer; ++k) {
        const uint64_t i = base + k * kBlock;
        live[k] = i < a.n;
        take[k] = live[k] && (!a.len || gptr(a.len)[i] > 0);
    }
#pragma unroll
    for (unsigned k = 0; k < kPickPer; ++k) {
        const uint64_t i = base + k * kBlock;
        id[k] = av[k] = 0ull;
        d[k] = 0u;
        if (take[k]) {  // the fields of a packet that is not taken are never read
            if (a.by_id) id[k] = gptr(a.id)[i];
            if (a.avoid) av[k] = gptr(a.avoid)[i];
            d[k] = a.draw ? gptr(a.draw)[i] : (uint32_t)(rsk::pick_splitmix64_at(a.seed, i) >> 32);
        }
    }
    uint32_t cnt = 0;  // wave-uniform
#pragma unroll
    for (unsigned k = 0; k < kPickPer; ++k) {
        const uint64_t i = base + k * kBlock;
        uint32_t row = RSK_CONN_NONE, off = 0u, m = m0;
        if (take[k] && ((STAGE && staged) || rsk::pick_group(a.p, a.capacity, a.by_id, id[k], off, m))) {
            uint32_t ap = kConnEmpty;
            if (av[k] != 0ull) {
                const uint32_t r = rsk::conn_lookup(a.t, a.capacity, a.by_id, av[k], id[k]);
                if (r != kConnEmpty) ap = a.p.pos(r);
            }
            row = STAGE && staged ? rsk::pick_row(LdsCand{lds_cand}, a.capacity, 0u, m0, d[k], ap)
                                  : rsk::pick_row(a.p, a.capacity, off, m, d[k], ap);
        }
        if (live[k]) gptr(a.conn)[i] = row;
        if (a.used && row != RSK_CONN_NONE) gptr(a.used)[row] = (uint8_t)1;  // row < capacity (pick_row)
        cnt += (uint32_t)__popcll(__ballot(take[k] && row == RSK_CONN_NONE));
    }
    if (a.n_none) {  // the word was zeroed on the stream ahead of this launch
        if ((threadIdx.x & 63u) == 0u) wave_none[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0u) {
            uint32_t total = 0;
#pragma unroll
            for (unsigned w = 0; w < kBlock / 64u; ++w) total += wave_none[w];
            if (total) atomicAdd(a.n_none, total);
        }
    }
}

__global__ void k_pick_zero(uint32_t *word) { *gptr(word) = 0u; }

// ---- the build ---------------------------------------------------------------------------------------

// The rows as k_index_build keys them for the groups: the IdBuf alone.
struct GroupTab {
    const uint64_t *ids;
    __device__ __forceinline__ uint64_t key(uint32_t) const { return 0ull; }
    __device__ __forceinline__ uint64_t id(uint32_t row) const { return gptr(ids)[row]; }
};

struct BuildArgs {
    const uint8_t *state;
    const uint64_t *ids;
    uint32_t *w;  // the pick index
    PickLayout l;
    uint32_t *counts;
    uint32_t capacity, slots;
    bool by_id;
};

constexpr uint8_t kUp = RSK_CONN_LIVE | RSK_CONN_ALIVE;

// The entry of `id` in lead (built over the candidate rows), or kConnEmpty.
__device__ __forceinline__ uint32_t group_slot(const BuildArgs &a, uint64_t id) {
    uint32_t s = rsk::conn_home(0ull, id, a.slots);
    for (uint32_t step = 0; step < a.slots; ++step, s = rsk::conn_next(s, a.slots)) {
        const uint32_t e = gptr(a.w)[a.l.lead + s];
        if (e >= a.capacity) break;
        if (gptr(a.ids)[e] == id) return s;
    }
    return kConnEmpty;
}

// The state column k_index_build inserts from: LIVE where the row is a candidate.  It stands in the pos
// area (capacity bytes of its 4 * C4), which k_pick_init fills after the insert.
__global__ __launch_bounds__(kBlock) void k_pick_derive(BuildArgs a) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r < a.capacity)
        reinterpret_cast<RSK_GLOBAL uint8_t *>(gptr(a.w + a.l.pos))[r] =
            (gptr(a.state)[r] & kUp) == kUp ? (uint8_t)RSK_CONN_LIVE : (uint8_t)0;
}

// Header zero, cand and pos kConnEmpty, and an entry {id, 0, 0} beside every taken entry of lead.
__global__ __launch_bounds__(kBlock) void k_pick_init(BuildArgs a) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g < rsk::kPickHdr) gptr(a.w)[g] = 0u;
    if (g < a.l.lead - a.l.cand) gptr(a.w)[a.l.cand + g] = kConnEmpty;
    if (a.by_id && g < a.slots) {
        const uint32_t e = gptr(a.w)[a.l.lead + g];
        uint64_t id = 0ull;
        if (e < a.capacity) id = gptr(a.ids)[e];
        const u32x4 q = {(uint32_t)id, (uint32_t)(id >> 32), 0u, 0u};
        reinterpret_cast<RSK_GLOBAL u32x4 *>(gptr(a.w + a.l.group))[g] = q;
    }
}

// BY_ID: the groups' counts.
__global__ __launch_bounds__(kBlock) void k_pick_count(BuildArgs a) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= a.capacity || (gptr(a.state)[r] & kUp) != kUp) return;
    const uint32_t s = group_slot(a, gptr(a.ids)[r]);
    if (s != kConnEmpty) atomicAdd(a.w + a.l.group + 4u * s + 3u, 1u);
}

constexpr unsigned kRankBlock = 1024;
constexpr unsigned kRankWaves = kRankBlock / 64u;

// Exclusive sums of v over the block's threads; total = the block's sum.  Every thread calls it.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *wsum, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (unsigned o = 1; o < 64u; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (unsigned w = 0; w < kRankWaves; ++w) {
        const uint32_t x = wsum[w];
        before += w < wave ? x : 0u;
        all += x;
    }
    __syncthreads();  // wsum is written again by the next call
    total = all;
    return before + inc - v;
}

// One block walks the rows in tiles of 1024, in order.  Per tile: the leaders (a group's lowest candidate)
// give their groups the next offsets, in row order, and restart the groups' counts at zero; then every
// candidate takes position (its group's count so far) + (the candidates of its group before it in the
// tile) and the counts advance.  The running counts are read and added with device-scope atomics, the
// barriers between them order the tile's steps.
__global__ __launch_bounds__(kRankBlock) void k_pick_rank(BuildArgs a) {
    __shared__ uint32_t slot_of[kRankBlock];
    __shared__ uint32_t wsum[kRankWaves];
    uint32_t total = 0, groups = 0;  // the same in every thread
    for (uint32_t tile = 0; tile < a.capacity; tile += kRankBlock) {
        const uint32_t r = tile + threadIdx.x;
        bool up = r < a.capacity && (gptr(a.state)[r] & kUp) == kUp;
        uint32_t s = 0u;
        if (up && a.by_id) {
            s = group_slot(a, gptr(a.ids)[r]);
            up = s != kConnEmpty;  // only when state changed under the build
            if (!up) s = 0u;
        }
        uint32_t *g = a.w + a.l.group + 4u * s;  // {id lo, id hi, off, cnt}; by_id only
        uint32_t p = 0, off = 0;
        if (!a.by_id) {
            uint32_t sum;
            p = total + block_scan(up ? 1u : 0u, wsum, sum);
            total += sum;
        } else {
            const bool leader = up && gptr(a.w)[a.l.lead + s] == r;
            uint32_t sum, nlead;
            const uint32_t mine = leader ? __hip_atomic_load(g + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            const uint32_t before = block_scan(mine, wsum, sum);
            (void)block_scan(leader ? 1u : 0u, wsum, nlead);
            if (leader) {
                __hip_atomic_store(g + 2, total + before, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(g + 3, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            total += sum;
            groups += nlead;
            slot_of[threadIdx.x] = up ? s : kConnEmpty;
            __threadfence();
            __syncthreads();
            uint32_t intra = 0;
            if (up) {
                const uint32_t full = threadIdx.x & ~3u;
                for (uint32_t j = 0; j < full; j += 4u) {
                    const uint4 q = *reinterpret_cast<const uint4 *>(&slot_of[j]);
                    intra += (q.x == s) + (q.y == s) + (q.z == s) + (q.w == s);
                }
                for (uint32_t j = full; j < threadIdx.x; ++j) intra += slot_of[j] == s;
                off = __hip_atomic_load(g + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                p = __hip_atomic_load(g + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + intra;
            }
            __syncthreads();  // every count was read before any is advanced
            if (up) atomicAdd(g + 3, 1u);
            __threadfence();
            __syncthreads();
        }
        // off + p < capacity: the groups' counts sum to at most the candidates, and those to the capacity
        if (up && off < a.capacity && p < a.capacity - off) {
            gptr(a.w)[a.l.pos + r] = p;
            gptr(a.w)[a.l.cand + off + p] = r;
        }
    }
    if (threadIdx.x == 0u) {
        if (!a.by_id) groups = total != 0u;
        gptr(a.w)[0] = total;
        gptr(a.w)[1] = groups;
        if (a.counts) {
            gptr(a.counts)[0] = groups;
            gptr(a.counts)[1] = total;
        }
    }
}

bool pick_tab_ok(const rsk_conn_table *t) { return rsk::tab_ok(t) && (!(t->flags & RSK_CONN_BY_ID) || t->id); }

}  // namespace

extern "C" int rsk_conn_pick_build(rsk_ctx *c, const rsk_conn_table *t, uint32_t *pick, uint32_t *counts, void *stream) {
    if (!c || !pick_tab_ok(t) || !t->state || !pick) return RSK_EINVAL;
    if (reinterpret_cast<uintptr_t>(pick) & 15u) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0;
    if (by_id && (reinterpret_cast<uintptr_t>(t->id) & 7u)) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    BuildArgs a;
    a.state = t->state;
    a.ids = reinterpret_cast<const uint64_t *>(t->id);
    a.w = pick;
    a.l = rsk::pick_layout(t->capacity, by_id);
    a.counts = counts;
    a.capacity = t->capacity;
    a.slots = rsk::conn_slots(t->capacity);
    a.by_id = by_id;
    // grids: at most 2^21 / 256 blocks (the slots of 2^20 rows), far below the 2^31 - 1 of a launch
    const uint32_t rows = (a.capacity + kBlock - 1u) / kBlock;
    const uint32_t fill = a.l.lead - a.l.cand > a.slots ? a.l.lead - a.l.cand : a.slots;
    if (by_id) {
        hipLaunchKernelGGL(k_pick_derive, dim3(rows), dim3(kBlock), 0, s, a);
        if (int r = rsk::launch_check("k_pick_derive")) return r;
        const uint8_t *dstate = reinterpret_cast<const uint8_t *>(pick + a.l.pos);
        if (int r = rsk::index_build(GroupTab{a.ids}, pick + a.l.lead, dstate, a.capacity, true, nullptr, s)) return r;
    }
    hipLaunchKernelGGL(k_pick_init, dim3((fill + kBlock - 1u) / kBlock), dim3(kBlock), 0, s, a);
    if (by_id) hipLaunchKernelGGL(k_pick_count, dim3(rows), dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL(k_pick_rank, dim3(1), dim3(kRankBlock), 0, s, a);
    return rsk::launch_check("k_pick_rank");
}

extern "C" int rsk_conn_pick_batch(rsk_ctx *c, const rsk_conn_table *t, const uint32_t *pick, uint32_t n,
                                   const rsk_conn_pick_in *in, const rsk_conn_pick_out *out, void *stream) {
    if (!c || !in || !out || !pick || !pick_tab_ok(t)) return RSK_EINVAL;
    if (reinterpret_cast<uintptr_t>(pick) & 15u) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0;
    if (in->avoid_key && (!t->conn_key || !t->index)) return RSK_EINVAL;
    if (n && (!out->conn || (by_id && !in->id))) return RSK_EINVAL;
    if (by_id && ((reinterpret_cast<uintptr_t>(t->id) | reinterpret_cast<uintptr_t>(in->id)) & 7u)) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    rsk::DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    // a kernel, not a memset node: behind rsk_conn_close_batch the call is part of captured chains, and replays of
    // a graph were seen to run a memset node with a stale pattern (rsk_tile_dev.h's k_fill_words)
    if (out->n_none) {
        hipLaunchKernelGGL(k_pick_zero, dim3(1), dim3(1), 0, s, out->n_none);
        if (int r = rsk::launch_check("k_pick_zero")) return r;
    }
    if (n == 0) return RSK_OK;
    PickArgs a;
    a.t = rsk::dev_tab(t);
    a.p = DevPick{pick, rsk::pick_layout(t->capacity, by_id)};
    a.len = in->len;
    a.id = reinterpret_cast<const uint64_t *>(in->id);
    a.avoid = in->avoid_key;
    a.draw = in->draw;
    a.seed = in->seed;
    a.conn = out->conn;
    a.n_none = out->n_none;
    a.used = out->used;
    a.n = n;
    a.capacity = t->capacity;
    a.by_id = by_id;
    const dim3 grid((n + kPickTile - 1u) / kPickTile);
    // a client table of at most kPickLds rows stages its candidates (0.92x the plain kernel at 10 conns and
    // 4M packets); a larger one would pay the count's load and the barrier for nothing
    const bool stage = !by_id && (c->pick_path == 2 || (c->pick_path == 0 && t->capacity <= kPickLds));
    if (stage) hipLaunchKernelGGL(k_conn_pick<true>, grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(k_conn_pick<false>, grid, dim3(kBlock), 0, s, a);
    return rsk::launch_check("k_conn_pick");
}

// Internal (not in the header; tools/bench_paths.py): 0 = by the table (above), 1 = every table takes its
// candidates from global memory, 2 = every table without BY_ID runs k_conn_pick<true>, which stages them
// when there are at most kPickLds.
extern "C" int rsk__set_pick_path(rsk_ctx *c, int path) {
    if (!c || path < 0 || path > 2) return RSK_EINVAL;
    c->pick_path = path;
    return RSK_OK;
}
