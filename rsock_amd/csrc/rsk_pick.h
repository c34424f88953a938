// rsk_pick.h — the layout and the lookup of the pick index (rsk_conn_pick_build / rsk_conn_pick_batch,
// include/rsk_codec.h), compiled for the host (rsk_host.cpp) and for the device (rsk_pick.hip): an index
// built by either side and copied to the other is valid there.
//
// The index is 32-bit words, 16-B aligned, for a table of C rows (C4 = C rounded up to a multiple of 4,
// S = conn_slots(C)):
//   [0, 4)              header: word 0 = the candidates of the whole table, word 1 = the groups that have
//                       one (1 or 0 without BY_ID), words 2-3 zero
//   [4, 4 + C4)         cand: the candidate rows, group by group (the groups in the order of their lowest
//                       candidate row), ascending inside a group; without BY_ID the one group starts at 0
//   [4 + C4, 4 + 2 C4)  pos: a row's position among its group's candidates, kConnEmpty for a row that is
//                       none
// and with BY_ID only
//   [.., + S)           lead: an open-addressing table over the IdBufs that have a candidate, keyed
//                       conn_home(0, id, S), an entry = the group's lowest candidate row (the build's own
//                       probe; the pick does not read it)
//   [.., + 4 S)         group: one 16-B entry per lead entry, {IdBuf word, offset into cand, count}; a
//                       count of 0 marks a free entry (an all-zero IdBuf is an ordinary id)
// A packet's chain is one 16-B load (its group), then one 4-B load (the candidate); the avoid key adds
// the conn index's probe and one load of pos.  Which entry of `group` an IdBuf takes depends on the order
// the build's lanes ran in; cand and pos, and so every pick, do not.
//
// Every value read from the index is bounded before it is used as an offset (a count above what is left
// of cand, an offset or a candidate outside the table give RSK_CONN_NONE), so an index that is stale or
// was never built gives an unspecified row of the table or NONE and no access outside the index or the
// table.
#pragma once
#include <stdint.h>

#include "rsk_conn.h"

namespace rsk {

constexpr uint32_t kPickHdr = 4u;  // header words

struct PickGroup {
    uint64_t id;
    uint32_t off, cnt;
};

struct PickLayout {
    uint32_t cand, pos, lead, group, words;  // word offsets, and the total
};

RSK_CONN_HD PickLayout pick_layout(uint32_t capacity, bool by_id) {
    const uint32_t c4 = (capacity + 3u) & ~3u, slots = conn_slots(capacity);
    PickLayout l;
    l.cand = kPickHdr;
    l.pos = l.cand + c4;
    l.lead = l.pos + c4;
    l.group = l.lead + (by_id ? slots : 0u);
    l.words = l.group + (by_id ? 4u * slots : 0u);
    return l;
}

// splitmix64's word i (rsk_fill_splitmix, rsock_amd/workload.splitmix64_np)
RSK_CONN_HD uint64_t pick_splitmix64_at(uint64_t seed, uint64_t i) {
    uint64_t z = seed + (i + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The group of `id`: its offset into cand and its count m >= 1, both bounded by the capacity; false for
// an id without a candidate.  P gives word(i) (a header word) and group(slot).
template <typename P>
RSK_CONN_HD bool pick_group(const P &p, uint32_t capacity, bool by_id, uint64_t id, uint32_t &off, uint32_t &m) {
    off = 0u;
    m = 0u;
    if (!by_id) {
        m = p.word(0u);
    } else {
        const uint32_t slots = conn_slots(capacity);
        uint32_t s = conn_home(0ull, id, slots);
        for (uint32_t step = 0; step < slots; ++step, s = conn_next(s, slots)) {
            const PickGroup g = p.group(s);
            if (g.cnt == 0u) break;
            if (g.id == id) {
                off = g.off;
                m = g.cnt;
                break;
            }
        }
    }
    return m >= 1u && off < capacity && m <= capacity - off;
}

// Candidate number k of the m at off, with draw d and the avoided candidate's position ap (kConnEmpty:
// none): the row, or kConnEmpty.  (off, m) as pick_group gave them; P gives cand(i).
template <typename P>
RSK_CONN_HD uint32_t pick_row(const P &p, uint32_t capacity, uint32_t off, uint32_t m, uint32_t d, uint32_t ap) {
    uint32_t k;
    if (ap < m) {
        if (m == 1u) return kConnEmpty;
        k = d % (m - 1u);
        k += k >= ap;
    } else {
        k = d % m;
    }
    const uint32_t r = p.cand(off + k);
    return r < capacity ? r : kConnEmpty;
}

// ---- rsk_conn_close_batch's work buffer and its update of the pick index (rsk_conn_close.hip, rsk_host.cpp) ----
// A close only takes candidates away, and a group's candidates are contiguous in cand: the new cand is the old
// one compacted order-stably over the entries whose row stays LIVE|ALIVE.  With K[j] = the kept entries before
// entry j, entry j moves to K[j], a group {off, cnt} becomes {K[off], K[off + cnt] - K[off]}, and a row's new
// position is K[j] - K[its group's off], where the group's old offset is j - (the row's old position): no
// group is looked up.  A group that lost every candidate keeps its entry as kPickGone, which pick_group's
// bounds turn into NONE: a count of 0 would free the entry and cut the probe chains of other ids.  lead is
// left as the build made it (only the build reads it, and it writes it first).
// work, 16-B aligned, in 32-bit words behind the marks:
//   [0, C16) bytes  mark: one byte per row (list form), C16 = C rounded up to a multiple of 16
//   K        [T]    T = the capacity rounded up to a multiple of kPickTile; all of it is written by a call
//                   that changes the pick index
//   cand     [C4]   the kept rows at their new positions
//   goff     [C4]   BY_ID only: per new position, the old offset of the entry's group (kConnEmpty: none)
constexpr uint32_t kPickTile = 1024u;                        // entries of cand per tile of the update
constexpr uint32_t kPickGoneOff = 0xFFFFFFFFu, kPickGoneCnt = 1u;  // {off, cnt} of a group without candidates
// off of an emptied or free entry that rsk_conn_create_batch is giving to a new group (between two of its launches)
constexpr uint32_t kPickTakenOff = 0xFFFFFFFEu;

struct CloseLayout {
    uint32_t k, cand, goff, words;  // word offsets into work, and the total
    uint32_t tiles;                 // tiles of kPickTile rows or entries
};

RSK_CONN_HD CloseLayout close_layout(uint32_t capacity, bool by_id) {
    const uint32_t c4 = (capacity + 3u) & ~3u, c16 = (capacity + 15u) & ~15u;
    CloseLayout l;
    l.tiles = (capacity + kPickTile - 1u) / kPickTile;
    l.k = c16 / 4u;
    l.cand = l.k + l.tiles * kPickTile;
    l.goff = l.cand + c4;
    l.words = l.goff + (by_id ? c4 : 0u);
    return l;
}

}  // namespace rsk
