// rsk_conn_create.h — what rsk_conn_create_batch (rsk_conn_create.hip) and its host twin (rsk_host.cpp, which
// also answers rsk_conn_create_bytes) share: the layout of the caller-owned work buffer, the key an offer's
// 4-tuple is hashed and compared by, and the row's initial seq / ack.  No HIP in here.  Internal (not installed).
//
// An ITEM is what may make a conn: a considered packet (column form) or an offer (list form).  With
// UI = max(u_max, m_max) items at most, MO = m_max offers and M = min(m_max, capacity) new conns at most, the
// buffer is 32-bit words in this order, every part rounded up to 16 B:
//   hdr     [16]               the counts one launch leaves for the next (kCc* below)
//   mask    [create_mask_words(UI)]  one bit per item: dedup candidate -> first arrival -> takes a row
//   dedup   [create_slots(UI)] open-addressing table of item positions by key, hash and probe rule of rsk_conn.h
//   list    [UI]               column form: the considered packets, in packet order
//   oidx    [UI]               the offer of a first arrival (its own index in list form), kConnEmpty: none
//   ohash   [create_slots(MO)] column form: open-addressing table of offers by 4-tuple, the lowest index wins
//   claim   [MO]               column form: 1 + the lowest item that names the offer; 0 = consumed before
//   orank   [MO]               the j of the new conn the offer becomes, kConnEmpty: none
//   first   [M]                the item of the j-th new conn
//   vacant  [M]                the j-th vacant row
// and for the pick index's update:
//   key     [2 M]              64-bit: (the place of the row's group << 32) | row, per new conn j
//   skey    [2 M]              the same keys in ascending order
//   goff    [M]                per j: its group's old offset into cand, kConnEmpty for a group without candidates
//   gcnt    [M]                per j: its group's old count
//   slot    [M]                per j: the group entry of its IdBuf, kConnEmpty before it has one
//   sj      [M]                per place in skey, the j of its key
//   nlead   [create_slots(M)]  open-addressing table over the new rows' IdBufs, an entry = the lowest j
//   cand    [C4]               the candidates at their new places
//   posv    [C4]               per new place, the row's position in its group
// A call uses the head of each part only (the tables are as large as its items, offers and new conns need).
#pragma once
#include <stdint.h>

#include "../../include/rsk_codec.h"
#include "rsk_conv_create.h"

namespace rsk {

constexpr uint32_t kCcMaxOffers = 2u * 0x100000u;  // m_max: at most 1024 tiles of 2048 offers
enum : uint32_t { kCcUnknown = 0, kCcKeys = 1, kCcOffered = 2, kCcVacant = 3 };  // words of hdr

struct ConnCreateLayout {
    uint64_t mask, dedup, list, oidx, ohash, claim, orank, first, vacant;
    uint64_t key, skey, goff, gcnt, slot, sj, nlead, cand, posv, words;  // offsets and the total, in words
};

inline uint64_t cc_round4(uint64_t w) { return (w + 3u) & ~3ull; }

// u_max in [0, kCreateMaxU], m_max in [1, kCcMaxOffers], capacity in [1, 2^20]
inline ConnCreateLayout conn_create_layout(uint32_t u_max, uint32_t m_max, uint32_t capacity) {
    const uint32_t ui = u_max > m_max ? u_max : m_max, m = m_max < capacity ? m_max : capacity;
    const uint64_t c4 = (capacity + 3u) & ~3u;
    ConnCreateLayout l;
    l.mask = kCreateHdrWords;
    l.dedup = l.mask + create_mask_words(ui);
    l.list = l.dedup + create_slots(ui);
    l.oidx = l.list + cc_round4(ui);
    l.ohash = l.oidx + cc_round4(ui);
    l.claim = l.ohash + create_slots(m_max);
    l.orank = l.claim + cc_round4(m_max);
    l.first = l.orank + cc_round4(m_max);
    l.vacant = l.first + cc_round4(m);
    l.key = l.vacant + cc_round4(m);
    l.skey = l.key + cc_round4(2ull * m);
    l.goff = l.skey + cc_round4(2ull * m);
    l.gcnt = l.goff + cc_round4(m);
    l.slot = l.gcnt + cc_round4(m);
    l.sj = l.slot + cc_round4(m);
    l.nlead = l.sj + cc_round4(m);
    l.cand = l.nlead + create_slots(m);
    l.posv = l.cand + c4;
    l.words = l.posv + c4;
    return l;
}

// The header's RSK_EINVAL list but the NULL ctx; ids8: the id columns must be 8-B aligned (the device side).
inline bool conn_create_args_ok(const rsk_conn_table *t, const rsk_conn_create_rows *rows, uint32_t n,
                                const rsk_conn_create_in *in, const rsk_conn_create_out *out, bool ids8) {
    if (!t || !rows || !in || !out || !in->work) return false;
    if ((t->flags & ~RSK_CONN_BY_ID) || t->capacity < 1u || t->capacity > RSK_CONN_MAX_ROWS) return false;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0, list = (in->flags & RSK_CONN_CREATE_LIST) != 0;
    if (!t->state || !t->conn_key || !t->index || (by_id && !t->id) || !t->src || !t->dst || !t->sp || !t->dp || !t->seq ||
        !t->ack || !t->flag)
        return false;
    if (rows->state != t->state || rows->conn_key != t->conn_key || (by_id && rows->id != t->id) || rows->src != t->src ||
        rows->dst != t->dst || rows->sp != t->sp || rows->dp != t->dp || rows->seq != t->seq || rows->ack != t->ack ||
        rows->flag != t->flag)
        return false;
    if (in->flags & ~(RSK_CONN_CREATE_LIST | RSK_CONN_CREATE_REPEAT)) return false;
    const rsk_conn_offers &o = in->offers;
    if (o.m_max == 0u || o.m_max > kCcMaxOffers || in->u_max > kCreateMaxU || (!list && in->u_max == 0u)) return false;
    if (!o.src || !o.dst || !o.sp || !o.dp || !o.ack || !o.flag || !o.n_offer) return false;
    if (list && (n != 0u || !o.conn_key || (by_id && !o.id))) return false;
    if (!list && n && (!out->miss || !out->conn || !in->conn_key || !in->src || !in->dst || !in->sp || !in->dp || (by_id && !in->id)))
        return false;
    if ((out->new_rows || out->new_first || out->new_offer) && !out->n_new) return false;
    if ((in->flags & RSK_CONN_CREATE_REPEAT) && !out->offer_row) return false;
    if ((reinterpret_cast<uintptr_t>(t->index) | reinterpret_cast<uintptr_t>(in->work) | reinterpret_cast<uintptr_t>(out->pick)) & 15u)
        return false;
    if (ids8 && by_id && ((reinterpret_cast<uintptr_t>(t->id) | reinterpret_cast<uintptr_t>(in->id) | reinterpret_cast<uintptr_t>(o.id)) & 7u))
        return false;
    return n <= RSK_MAX_BATCH;
}

// An offer's 4-tuple as the (key, id) pair of rsk_conn.h's hash: TcpCmpFn compares src, sp, dst, dp.
RSK_CONN_HD uint64_t tuple_key(uint32_t src, uint32_t dst) { return ((uint64_t)src << 32) | dst; }
RSK_CONN_HD uint64_t tuple_ports(uint16_t sp, uint16_t dp) { return ((uint64_t)sp << 16) | dp; }

// FakeTcp::Init on the TcpInfo Wait2TransferInfo leaves (tests/golden/tcpstate.npz)
RSK_CONN_HD uint32_t create_seq(uint32_t offer_ack) { return offer_ack + 1u; }
RSK_CONN_HD uint32_t create_ack(uint32_t offer_ack) { return offer_ack + 2u; }

// The first index in [0, n) of the ascending 64-bit keys at k whose key is not below x.
template <typename F>
RSK_CONN_HD uint32_t lower_bound_u64(const F &at, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (at(mid) < x) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

}  // namespace rsk
