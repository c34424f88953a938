// rsk_conn_dev.h — the connection table as the device kernels read it, and the host-side checks of a
// rsk_conn_table, shared by rsk_conn.hip (index, resolve, expand) and rsk_control.hip (control packets,
// keepalive timer).  Internal (not installed).
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

}  // namespace rsk
