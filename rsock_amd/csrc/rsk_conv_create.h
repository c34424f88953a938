// rsk_conv_create.h — the layout of rsk_conv_create_batch's caller-owned work buffer (include/rsk_codec.h),
// shared by the device side (rsk_conv_create.hip) and the host twin (rsk_host.cpp, which also answers
// rsk_conv_create_bytes).  No HIP in here.  Internal (not installed).
//
// 32-bit words, in this order:
//   hdr    [16]                 the counts one launch leaves for the next (kCreate* below)
//   mask   [create_mask_words(u_max)] one bit per list position: a first arrival (64-bit words, 8-B aligned)
//   dedup  [create_slots(u_max)] open-addressing table of list positions, hash and probe rule of rsk_conn.h
//   list   [u_max]              the considered packets, in packet order
//   first  [min(u_max, C)]      the first packet of the j-th distinct key
//   vacant [min(u_max, C)]      the j-th vacant row
// A call uses the head of each part only: its dedup table has create_slots(considered packets) entries, so a
// batch with few unknown packets clears and probes a small table whatever u_max is.
#pragma once
#include <stdint.h>

#include "rsk_conn.h"

namespace rsk {

constexpr uint32_t kCreateMaxU = 1u << 24;
constexpr uint32_t kCreateHdrWords = 16;
enum : uint32_t { kCreateUnknown = 0, kCreateKeys = 1, kCreateVacant = 2 };  // words of hdr

// entries of the dedup table for at most u considered packets (u in [1, 2^24]): 4 .. 2^25, at least 2 u
RSK_CONN_HD uint32_t create_slots(uint32_t u) {
    uint32_t s = 4u;
    while (s < 2u * u) s <<= 1;
    return s;
}

// 32-bit words of the first-arrival mask: one 64-bit word per 64 list positions, rounded up to 16 B
RSK_CONN_HD uint32_t create_mask_words(uint32_t u) { return (2u * ((u + 63u) / 64u) + 3u) & ~3u; }

struct CreateLayout {
    uint64_t mask, dedup, list, first, vacant, words;  // offsets and the total, in words
};

inline CreateLayout create_layout(uint32_t u_max, uint32_t capacity) {
    const uint64_t m = u_max < capacity ? u_max : capacity;
    CreateLayout l;
    l.mask = kCreateHdrWords;
    l.dedup = l.mask + create_mask_words(u_max);
    l.list = l.dedup + create_slots(u_max);
    l.first = l.list + u_max;
    l.vacant = l.first + m;
    l.words = (l.vacant + m + 3u) & ~3ull;
    return l;
}

}  // namespace rsk
