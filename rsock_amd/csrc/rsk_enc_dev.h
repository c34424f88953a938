// rsk_enc_dev.h — what the framing encode (rsk_kernels.hip) and the wire build (rsk_wire.hip) share: the
// call's arguments, phase 1 (one lane per packet: status, tag, header words), the batch statistic behind
// AUTO, the 16-B loads and stores, the flat copy's record, the per-set packet mapping and the per-set
// copy-path thresholds.  Internal (not installed); anonymous namespace as in rsk_codec_dev.h.
#pragma once
#include "rsk_codec_dev.h"

namespace rsk {
// The arguments of an n-packet encode call (named: rsk::enc_args, rsk_ctx.h, fills them for both units).
struct EncArgs {
    const uint8_t *payload;
    const uint64_t *pay_off;
    const uint16_t *pay_len;
    const uint8_t *cmd;
    const uint32_t *conv;
    const uint64_t *conn_key;
    const uint8_t *id;  // n*8, 8-byte aligned, or null
    uint8_t *frame;
    const uint64_t *frame_off;
    int32_t *status;
    uint32_t id_lo, id_hi;
    uint32_t n;
    uint32_t pad;  // log2 of the zero-pad granularity (4: RSK_ENC_ZERO_PAD16, 7: RSK_ENC_ZERO_PAD128), 0 = none
};
}  // namespace rsk

using rsk::EncArgs;

namespace {

// ---- phase 1: one lane per packet ---------------------------------------------------------------
// status (RConn.cpp:88-98), tag (rhash.cpp:20-41 via md5_tag), frame words 0..7 (tag + EncHead +
// payload[0]); `slow` marks a framed packet whose frame is not 16-B aligned (k_encode_wire: the
// shifted copies).
struct Lane1 {
    int32_t st;
    uint64_t po, fo;
    uint32_t H[8];
    bool slow;
};

// SADD: added to a framed packet's status (the two-pass wire build: the wire length, HL + 31 + P)
template <bool TAG = true, bool LANE = false, int SADD = 0>
__device__ __forceinline__ Lane1 encode_phase1(const EncArgs &a, const KeySched &ks, uint64_t i) {
    Lane1 L;
    L.st = 0;
    L.po = 0;
    L.fo = 0;
    L.slow = false;
#pragma unroll
    for (int q = 0; q < 8; ++q) L.H[q] = 0;
    if (i < a.n) {
        L.po = a.pay_off[i];
        const uint32_t P = a.pay_len[i];
        L.fo = a.frame_off[i];
        L.st = P == 0 ? RSK_SEND_RESET
                      : (P > RSK_MAX_PAYLOAD ? RSK_SEND_OVERSIZE : (int32_t)(RSK_HEAD_SIZE + P));
        if (L.st > 0) {
            const uint32_t b0 = TAG ? a.payload[L.po] : 0u;
            if (TAG) tag_of<LANE>(ks, b0, L.H[0], L.H[1]);
            uint32_t id0 = a.id_lo, id1 = a.id_hi;
            if (a.id) {
                const uint2 v = *reinterpret_cast<const uint2 *>(a.id + 8 * i);
                id0 = v.x;
                id1 = v.y;
            }
            head_words(a.cmd[i], id0, id1, a.conv[i], a.conn_key[i], b0, L.H);
            L.slow = (reinterpret_cast<uintptr_t>(a.frame + L.fo) & 15u) != 0;
        }
        a.status[i] = L.st > 0 ? L.st + SADD : L.st;
    }
    return L;
}

// The tag half of phase 1 for a set that skipped it (encode_phase1<false>): payload[0], MD5, and
// payload[0] into frame byte 31 (H[7]).
__device__ __forceinline__ void encode_tag(const EncArgs &a, const KeySched &ks, Lane1 &L) {
    if (L.st > 0) {
        const uint32_t b0 = a.payload[L.po];
        tag_of(ks, b0, L.H[0], L.H[1]);
        L.H[7] |= b0 << 24;
    }
}

// The batch statistic behind the next calls' choice of encode path (rsk_encode_batch, enc_path): one
// wave reads pay_len at 64 evenly spaced packets and stores their mean payload length (bit 31 set:
// valid) to a host-mapped word of the context.  k_encode_heads does it in its block 0; calls on the
// other paths launch k_enc_sample behind the encode (the per-set kernel itself carries no extra
// argument: one more pointer in its arguments cost C4 12 % through SGPR spills, gpurun_out/r04o).
constexpr uint32_t kStatValid = 0x80000000u;
constexpr uint32_t kStatPacked = 0x40000000u;  // the sampled frames lie back to back (output-stationary copy)
constexpr uint32_t kStatMean = 0xffffu;        // the sampled mean payload
// With frame_off (round 6) it also checks whether each sampled packet's frame ends where the next
// packet's begins, inside a 16-B chunk (byte-packed frames without a pad share their boundary
// chunks): three in four -> kStatPacked, which lets AUTO take the output-stationary copy
// (k_encode_os).  Frames packed at a 16-B pitch share nothing, and the packet copies are faster
// there (C4 16-B packed: 0.36 vs 0.435 ms).  A hint only: every copy writes the same bytes.
__device__ __forceinline__ void enc_sample(const uint16_t *pay_len, uint32_t n, uint32_t *stat,
                                           const uint64_t *frame_off = nullptr, uint32_t pad = 0u) {
    if (stat == nullptr || blockIdx.x != 0u || threadIdx.x >= 64u) return;  // one wave of block 0
    const uint64_t i = ((uint64_t)threadIdx.x * n) >> 6;
    const uint32_t P = pay_len[i];
    uint32_t v = P;
    bool packed = false;
    if (frame_off && pad == 0u && i + 1u < n && P != 0u && P <= (uint32_t)RSK_MAX_PAYLOAD) {
        const uint64_t e = frame_off[i] + RSK_HEAD_SIZE + P;
        packed = frame_off[i + 1] == e && (e & 15u) != 0u;  // the next frame starts inside e's 16-B chunk
    }
    const uint32_t np = (uint32_t)__popcll(__ballot(packed));
#pragma unroll
    for (int off = 32; off; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    if (threadIdx.x == 0u)
        __hip_atomic_store(stat, kStatValid | (np >= 48u ? kStatPacked : 0u) | (v >> 6), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
}

// Nontemporal loads (bit 0) and stores (bit 1) of the two-pass copies, ld16 / st16's NT (C3 -1.4 % against
// 2, and 256-thread blocks against 64 / 512 / 1024: profiles/r04r_two_pass_ab.json).
constexpr int kStream = 3;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <int NT>
__device__ __forceinline__ uint4 ld16(const uint8_t *p) {
    const RSK_GLOBAL u32x4 *g = reinterpret_cast<const RSK_GLOBAL u32x4 *>(rsk::gptr(p));
    u32x4 v;
    if constexpr (NT & 1) v = __builtin_nontemporal_load(g);
    else v = *g;
    return make_uint4(v.x, v.y, v.z, v.w);
}
template <int NT>
__device__ __forceinline__ void st16(uint8_t *p, const uint4 &v) {
    RSK_GLOBAL u32x4 *g = reinterpret_cast<RSK_GLOBAL u32x4 *>(rsk::gptr(p));
    const u32x4 w = {v.x, v.y, v.z, v.w};
    if constexpr (NT & 2) __builtin_nontemporal_store(w, g);
    else *g = w;
}
// Store chunk data v whose first `lim` bytes belong to the frame: whole chunk when lim >= 16;
// with padding, the tail (or the whole chunk, lim <= 0) is zeroed; without, only [0, lim).
template <int NT>
__device__ __forceinline__ void store_last16(uint8_t *d, const uint4 &v, int lim, bool pad) {
    if (lim >= 16) st16<NT>(d, v);
    else if (pad) st16<NT>(d, lim > 0 ? rsk::keep_bytes16(v, lim) : make_uint4(0u, 0u, 0u, 0u));
    else rsk::store_partial16(d, v, lim);
}

// Bytes written for a frame of flen bytes at d: flen, or up to the next 2^pad boundary.
__device__ __forceinline__ uint32_t padded_len(const uint8_t *d, uint32_t flen, uint32_t pad) {
    if (!pad) return flen;
    const uint32_t m = (1u << pad) - 1u;
    return flen + ((m + 1u - ((uint32_t)(reinterpret_cast<uintptr_t>(d) + flen) & m)) & m);
}

struct alignas(16) CopyRec {
    const uint8_t *src_al;  // 16-B aligned source of chunk 2 (payload + 1 - sh; wire: its own base)
    uint8_t *dst;           // 16-B aligned destination of chunk 0
    uint32_t cstart;        // first flat chunk index of this packet within the set
    uint32_t sh;            // funnel shift (bits 0-3) | frame offset r << 4 (encode)
    int32_t last_rel;       // last payload byte, relative to src_al
    uint32_t flen;          // frame length (31 + P)
};

// 16 bytes at byte offset sh (0..15, per lane) of A||B, branch-free
__device__ __forceinline__ uint4 funnel16_lane(const uint4 &A, const uint4 &B, uint32_t sh) {
    const uint32_t q = sh >> 2, r = sh & 3u;
    const uint32_t W[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    uint32_t E[5];
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        const uint32_t w0 = W[d], w1 = d + 1 < 8 ? W[d + 1] : 0u, w2 = d + 2 < 8 ? W[d + 2] : 0u,
                       w3 = d + 3 < 8 ? W[d + 3] : 0u;
        E[d] = q == 0 ? w0 : q == 1 ? w1 : q == 2 ? w2 : w3;
    }
    uint4 o;
    o.x = rsk::funnel(E[1], E[0], r);
    o.y = rsk::funnel(E[2], E[1], r);
    o.z = rsk::funnel(E[3], E[2], r);
    o.w = rsk::funnel(E[4], E[3], r);
    return o;
}

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t wave_shl1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, false);  // wave_shl:1
}

__device__ __forceinline__ uint4 rdl4(const uint4 &v, uint32_t j) {
    return make_uint4(rdl(v.x, j), rdl(v.y, j), rdl(v.z, j), rdl(v.w, j));
}

// ---- the per-set kernels (k_encode, k_encode_wire): packet mapping and store policy ---------------
// Grouped-interleave mapping.  A super-block of kSetSbw consecutive waves owns kSetSbw * 64
// consecutive packets; wave wl of it takes groups of kSetGrp consecutive packets strided by
// kSetSbw * kSetGrp (lane l: group (l / kSetGrp) * kSetSbw + wl, packet l % kSetGrp in it).  Each wave
// still frames 64 packets (descriptor loads coalesced per 8-packet group), but the resident waves copy
// one compact stretch of the arenas at a time (kSetSbw * kSetGrp packets per super-block) instead of
// each its own region 64 packets from the next wave's: C3 -3.7 %, C4 -4.1 %, C2 within 1 % against the
// tiled mapping (profiles/r02_ab_encode_mapping.json; renumbering the blocks so that each XCD's blocks
// own consecutive waves measured no gain, profiles/r01_ab_xcd_map.json).  The grid holds only waves
// that own a packet (enc_grid).
constexpr uint32_t kSetGrp = 8, kSetSbw = 1024;

// The packet of lane `lane` of the grid's wave wg (n: past the batch); false (wave-uniform) when the
// wave owns no packet.
__device__ __forceinline__ bool set_packet(uint64_t wg, uint32_t lane, uint32_t n, uint64_t &i) {
    const uint64_t sb = wg / kSetSbw, wl = wg % kSetSbw;
    if (sb * kSetSbw * 64u + wl * kSetGrp >= n) return false;  // the wave's smallest packet
    const uint64_t gi = sb * kSetSbw * 64u + ((uint64_t)(lane / kSetGrp) * kSetSbw + wl) * kSetGrp + lane % kSetGrp;
    i = gi < n ? gi : n;
    return true;
}

// The set's frames (or wire packets: `len` bytes at frame + fo; on: the lane's is written) leave gaps:
// some pair of neighbours in one group (the last packet of a group: the next lane's packet is not the
// next frame) does not lie back to back, padded end to start.  nfo / non: the next lane's offset, and
// whether it is written.
__device__ __forceinline__ bool set_gaps(const EncArgs &a, uint64_t fo, uint32_t len, bool on, uint32_t lane,
                                         uint64_t &nfo, bool &non) {
    const uint32_t fend = on ? padded_len(a.frame + fo, len, a.pad) : 0u;
    const uint64_t end = fo + fend;
    nfo = (uint64_t)(uint32_t)__shfl_down((int)(uint32_t)fo, 1) |
          ((uint64_t)(uint32_t)__shfl_down((int)(uint32_t)(fo >> 32), 1) << 32);
    non = __shfl_down((int)on, 1) != 0;
    return __ballot(on && non && lane % kSetGrp != kSetGrp - 1u && end != nfo) != 0ull;
}

// Copy-path choice for the hybrid kernel: the per-packet loop wastes lanes on short frames (a
// 95-B frame uses 6 of 64 lanes), the flat list costs a binary search + LDS table per chunk.
// Measured crossover: flat wins below a set-mean frame of ~256 B.
constexpr uint32_t kFlatBelowMeanBytes = 256;
// The tag moves into the copy loop for sets of long frames only; with short frames an iteration
// carries fewer bytes per MD5 (C4: +10 % with the tag deferred).
constexpr uint32_t kDeferTagMeanBytes = 1024;

}  // namespace
