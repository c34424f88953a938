// rsk_pool.h — what the device side of the tuple pool (rsk_pool.hip) and its host twins (rsk_host.cpp) share:
// the key a pooled 4-tuple is hashed and compared by, the layout of the work buffers, the marks of the settle
// and the header's RSK_EINVAL lists.  No HIP in here.  Internal (not installed).
//
// rsk_pool_add_batch's work is rsk_conv_create_batch's (rsk_conv_create.h: hdr, mask, dedup, list, first, vacant)
// for the same u_max and capacity.  rsk_pool_settle_batch's work is one mark byte per row, the ack pool's rows
// first, each part rounded up to 16 B.
#pragma once
#include <stdint.h>

#include "../../include/rsk_codec.h"
#include "rsk_conn_create.h"

namespace rsk {

// a row's mark in the settle: it leaves because its offer became a conn (a), or because a packet that is still
// missing carries its tuple and the other pool has no entry for it (b)
enum : uint8_t { kPoolStays = 0, kPoolTaken = 1, kPoolPurged = 2 };

// words of the add's hdr behind rsk_conv_create.h's three
enum : uint32_t { kPoolZeroPort = 3 };

inline uint64_t pool_round16(uint64_t b) { return (b + 15u) & ~15ull; }
inline uint64_t pool_settle_bytes(uint32_t cap_ack, uint32_t cap_sock) { return pool_round16(cap_ack) + pool_round16(cap_sock); }

inline bool pool_cap_ok(uint32_t capacity) { return capacity >= 1u && capacity <= RSK_CONN_MAX_ROWS; }

// what a lookup reads, and the index's alignment; vals: seq and ack are needed too (the ack pool)
inline bool pool_ok(const rsk_pool *p, bool vals) {
    if (!p || !pool_cap_ok(p->capacity)) return false;
    if (!p->state || !p->src || !p->dst || !p->sp || !p->dp || !p->expiry || !p->index) return false;
    if (vals && (!p->seq || !p->ack)) return false;
    return !(reinterpret_cast<uintptr_t>(p->index) & 15u) && !(reinterpret_cast<uintptr_t>(p->expiry) & 7u);
}

inline bool pool_add_args_ok(const rsk_pool *p, uint32_t n, const rsk_pool_add_in *in, const rsk_pool_add_out *out) {
    if (!in || !out || !pool_ok(p, false) || !in->work) return false;
    if (in->flags & ~RSK_POOL_TOUCH) return false;
    if (in->u_max == 0u || in->u_max > kCreateMaxU) return false;
    if (n && (!in->src || !in->dst || !in->sp || !in->dp)) return false;
    if (n && ((p->seq && !in->seq) || (p->ack && !in->ack))) return false;
    if ((out->new_rows || out->new_first) && !out->n_new) return false;
    if (reinterpret_cast<uintptr_t>(in->work) & 15u) return false;
    return n <= RSK_MAX_BATCH;
}

inline bool pool_offers_args_ok(const rsk_pool *a, const rsk_pool *s, const rsk_pool_offers_out *out) {
    if (!out || !pool_ok(a, true) || !pool_ok(s, false)) return false;
    if (out->m_max == 0u || out->m_max > kCcMaxOffers) return false;
    if (!out->src || !out->dst || !out->sp || !out->dp || !out->ack || !out->flag || !out->n_offer) return false;
    return !(reinterpret_cast<uintptr_t>(out->conn_key) & 7u);
}

inline bool pool_settle_args_ok(const rsk_pool *a, const rsk_pool *s, uint32_t n, const rsk_pool_settle_in *in,
                                const rsk_pool_settle_out *out) {
    if (!in || !out || !pool_ok(a, false) || !pool_ok(s, false) || !in->work) return false;
    if (in->m_max == 0u || in->m_max > kCcMaxOffers || in->new_max > kCcMaxOffers) return false;
    if (in->new_max && (!in->new_offer || !in->n_new || !in->offer_ack_row || !in->offer_sock_row)) return false;
    if (n && (!in->miss || !in->src || !in->dst || !in->sp || !in->dp)) return false;
    if (out->closed_sock_rows && !out->n_closed) return false;
    if (reinterpret_cast<uintptr_t>(in->work) & 15u) return false;
    return n <= RSK_MAX_BATCH;
}

inline bool pool_flush_args_ok(const rsk_pool *p, const rsk_pool_flush_out *out) {
    return out && pool_ok(p, false) && !(out->dead_rows && !out->n_dead);
}

}  // namespace rsk
