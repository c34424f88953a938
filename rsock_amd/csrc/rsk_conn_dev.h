// rsk_conn_dev.h — the connection table as the device kernels read it, and the host-side checks of a
// rsk_conn_table, shared by rsk_conn.hip (index, resolve, expand) and rsk_control.hip (control packets,
// keepalive timer); and the index build kernel, which rsk_conv.hip runs over its own table through the
// accessor.  Internal (not installed).
#pragma once
#include <hip/hip_runtime.h>

#include "rsk_conn.h"
#include "rsk_ctx.h"
#include "rsk_device.h"

namespace rsk {

// The table as rsk_conn.h's conn_lookup takes it.
struct DevConnTab {
    const uint32_t *index;
    const uint64_t *conn_key;
    const uint64_t *ids;  // the [C*8] IdBuf bytes, 8-B aligned, one word per row
    __device__ __forceinline__ uint32_t entry(uint32_t s) const { return gptr(index)[s]; }
    __device__ __forceinline__ uint64_t key(uint32_t row) const { return gptr(conn_key)[row]; }
    __device__ __forceinline__ uint64_t id(uint32_t row) const { return gptr(ids)[row]; }
};

inline bool tab_ok(const rsk_conn_table *t) {
    return t && !(t->flags & ~RSK_CONN_BY_ID) && t->capacity >= 1u && t->capacity <= RSK_CONN_MAX_ROWS;
}
// what a lookup reads
inline bool tab_lookup_ok(const rsk_conn_table *t) {
    return tab_ok(t) && t->conn_key && t->index && (!(t->flags & RSK_CONN_BY_ID) || t->id);
}
inline DevConnTab dev_tab(const rsk_conn_table *t) {
    return DevConnTab{t->index, t->conn_key, reinterpret_cast<const uint64_t *>(t->id)};
}

// Zero a given device count on the stream ahead of the kernel that adds to it.
inline int zero_word(uint32_t *word, hipStream_t s) {
    if (!word) return RSK_OK;
    hipError_t e = hipMemsetAsync(word, 0, 4, s);
    if (e != hipSuccess) { set_error("hipMemsetAsync", e); return RSK_EDEVICE; }
    return RSK_OK;
}

// One atomic per wave for a count of lanes (the word was zeroed on the stream ahead of the launch).
__device__ __forceinline__ void wave_count(uint32_t *word, bool mine) {
    const uint32_t cnt = (uint32_t)__popcll(__ballot(mine));
    if (cnt && (threadIdx.x & 63u) == 0u) atomicAdd(word, cnt);
}

// ---- the index build, shared by every table whose accessor T gives key(row) and id(row) ---------------
//   k_index_build   launched twice per rebuild: <0> clears the index with 16-B stores, <1> inserts the
//                   LIVE rows, one lane per row and one CAS per probe step; a row that meets an entry
//                   with its own key leaves the lower row there (atomicMin), so the lowest row of a key
//                   wins whatever order the lanes ran in, and exactly one row loses per meeting.
constexpr unsigned kBuildBlock = 256;

template <typename T>
struct IndexBuildArgs {
    T t;
    uint32_t *index;
    const uint8_t *state;
    uint32_t *n_dup;
    uint32_t capacity, slots;
    bool by_id;
};

template <int PHASE, typename T>
__global__ __launch_bounds__(kBuildBlock) void k_index_build(IndexBuildArgs<T> a) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint32_t g = blockIdx.x * kBuildBlock + threadIdx.x;
    if (PHASE == 0) {  // slots is a multiple of 4 and the index 16-B aligned
        const u32x4 empty = {kConnEmpty, kConnEmpty, kConnEmpty, kConnEmpty};
        if (g < a.slots / 4u) reinterpret_cast<RSK_GLOBAL u32x4 *>(gptr(a.index))[g] = empty;
        return;
    }
    bool dup = false;
    if (g < a.capacity && (gptr(a.state)[g] & RSK_CONN_LIVE)) {
        const uint64_t key = a.t.key(g), id = a.by_id ? a.t.id(g) : 0ull;
        uint32_t s = conn_home(key, id, a.slots);
        // at most `capacity` entries are ever taken and slots >= 2 capacity: a free entry is met within
        // `slots` steps; the bound only keeps a corrupted launch from spinning
        for (uint32_t step = 0; step < a.slots; ++step, s = conn_next(s, a.slots)) {
            const uint32_t e = atomicCAS(a.index + s, kConnEmpty, g);
            if (e == kConnEmpty) break;  // the entry was free and is now this row's
            // e is a row of this build (the clear ran before this launch), and an entry's key never
            // changes once taken: only rows of the same key replace each other in it
            if (e < a.capacity && a.t.key(e) == key && (!a.by_id || a.t.id(e) == id)) {
                atomicMin(a.index + s, g);  // one of the two rows stays: the other is the duplicate
                dup = true;
                break;
            }
        }
    }
    if (a.n_dup) wave_count(a.n_dup, dup);
}

// The two launches on s, after zeroing a given *n_dup there.
template <typename T>
inline int index_build(const T &t, uint32_t *index, const uint8_t *state, uint32_t capacity, bool by_id, uint32_t *n_dup,
                       hipStream_t s) {
    if (int r = zero_word(n_dup, s)) return r;
    IndexBuildArgs<T> a;
    a.t = t;
    a.index = index;
    a.state = state;
    a.n_dup = n_dup;
    a.capacity = capacity;
    a.slots = conn_slots(capacity);
    a.by_id = by_id;
    hipLaunchKernelGGL((k_index_build<0, T>), dim3((a.slots / 4u + kBuildBlock - 1u) / kBuildBlock), dim3(kBuildBlock), 0, s, a);
    hipLaunchKernelGGL((k_index_build<1, T>), dim3((a.capacity + kBuildBlock - 1u) / kBuildBlock), dim3(kBuildBlock), 0, s, a);
    return launch_check("k_index_build");
}

}  // namespace rsk
