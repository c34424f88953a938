// rsk_conn.h — the hash and the probe rule of the connection table's index (rsk_conn_table::index,
// include/rsk_codec.h), compiled for the host (rsk_host.cpp) and for the device (rsk_conn.hip): an
// index built by either side and copied to the other is valid there.
//
// The index is an open-addressing table of conn_slots(capacity) 32-bit entries, a power of two of at
// least twice the capacity, so at least half of it stays free and a probe for an absent key ends at a
// free entry even when every row is LIVE.  An entry is a row number, or kConnEmpty.  A key's entry is
// the first one from conn_home(...) on, stepping by one and wrapping, that holds a row with that key:
// no entry before it is free.  Every key has one entry, whichever order the rows were inserted in;
// which row of several with one key it names is the builder's business (the lowest).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RSK_CONN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RSK_CONN_HD inline
#endif

namespace rsk {

constexpr uint32_t kConnEmpty = 0xFFFFFFFFu;

// entries of the index of a table of `capacity` rows (capacity in [1, 2^20]): 4 .. 2^21
RSK_CONN_HD uint32_t conn_slots(uint32_t capacity) {
    uint32_t s = 4u;
    while (s < 2u * capacity) s <<= 1;
    return s;
}

// splitmix64's finaliser: every input bit reaches every output bit
RSK_CONN_HD uint64_t conn_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// First entry probed for (id, key); id = 0 for a table without RSK_CONN_BY_ID.
RSK_CONN_HD uint32_t conn_home(uint64_t key, uint64_t id, uint32_t slots) {
    return (uint32_t)(conn_mix(key ^ conn_mix(id + 0x9e3779b97f4a7c15ull)) >> 32) & (slots - 1u);
}
RSK_CONN_HD uint32_t conn_next(uint32_t slot, uint32_t slots) { return (slot + 1u) & (slots - 1u); }

// The row of (id, key), or kConnEmpty.  T gives entry(slot), key(row) and id(row) (id only with
// by_id).  An entry that is no row of the table (free, or garbage in an index that was never built)
// ends the probe, and so does a walk over every entry: the lookup reads nothing outside the table
// and always ends.
template <typename T>
RSK_CONN_HD uint32_t conn_lookup(const T &t, uint32_t capacity, bool by_id, uint64_t key, uint64_t id) {
    const uint32_t slots = conn_slots(capacity);
    uint32_t s = conn_home(key, by_id ? id : 0ull, slots);
    for (uint32_t step = 0; step < slots; ++step, s = conn_next(s, slots)) {
        const uint32_t row = t.entry(s);
        if (row >= capacity) break;
        if (t.key(row) == key && (!by_id || t.id(row) == id)) return row;
    }
    return kConnEmpty;
}

}  // namespace rsk
