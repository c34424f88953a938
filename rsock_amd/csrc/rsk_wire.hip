// rsk_wire.hip — encode straight to wire packets for gfx950, and rsk_encode_wire_batch.
//
// Kernels:
//   k_encode_wire   RConn::Output + RawTcp::SendRawTcp (conn/RawTcp.cpp:280-341): frames plus the
//   (_w4)           IPv4/TCP headers and checksums libnet writes, two-launch hybrid over
//                   k_encode's per-set mapping (the per-packet half held to 4 waves per SIMD).
//   k_wire_heads /  the two-pass form: header images as records, then K = 1, 2 or 4 packets per copy
//   k_wire_copy     wave.
// Phase 1, the 16-B copies and the set mapping are shared with the framing encode (rsk_enc_dev.h); the
// arguments, the grid and AUTO's statistic come from rsk_kernels.hip (rsk::enc_args .. sample_next, rsk_ctx.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/rsk_codec.h"
#include "rsk_ctx.h"
#include "rsk_enc_dev.h"

namespace {

using rsk::DeviceGuard;
using rsk::enc_args;
using rsk::enc_grid;
using rsk::enc_path;
using rsk::g_last_error;
using rsk::kTwoPassMinPackets;
using rsk::launch_check;
using rsk::sample_next;
using rsk::sampled_mean;

// ---------------------------------------------------------------------------------------------
// Encode straight to wire packets (RConn::Output + RawTcp::SendRawTcp / libnet)
// ---------------------------------------------------------------------------------------------
struct WireArgs {
    const uint32_t *src, *dst;
    const uint16_t *sp, *dp;
    const uint32_t *seq, *ack;
    const uint8_t *flag;
    const uint16_t *ip_id;
    uint32_t eth[4];  // 14 link-header bytes, LE words
};

// one's-complement sum of the little-endian 16-bit halves of w (RFC 1071 is byte-order agnostic:
// summing LE halfwords and storing ~sum little-endian gives the big-endian checksum bytes)
__device__ __forceinline__ uint32_t hsum(uint32_t w) { return (w & 0xffffu) + (w >> 16); }
// acc + the four words' 16-bit halves: one v_dot2_u32_u16 (halves x (1, 1)) per word
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t hsum4(const uint4 &v, uint32_t acc) {
    const u16x2 one = {1, 1};
    acc = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, v.x), one, acc, false);
    acc = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, v.y), one, acc, false);
    acc = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, v.z), one, acc, false);
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, v.w), one, acc, false);
}
__device__ __forceinline__ uint32_t fold16(uint32_t s) {
    s = (s & 0xffffu) + (s >> 16);
    s = (s & 0xffffu) + (s >> 16);
    return s;
}
// OR `nb` bytes of v (LE) into the byte image PW at byte offset off (all compile-time after inlining)
template <int N>
__device__ __forceinline__ void put_bytes(uint32_t (&PW)[N], int off, uint32_t v, int nb) {
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (b < nb) PW[(off + b) >> 2] |= ((v >> (8 * b)) & 0xffu) << (8 * ((off + b) & 3));
}

template <int E>  // E = link header bytes before IPv4: 0 (RAW4) or 14 (Ethernet)
struct WireGeom {
    static constexpr int HL = E + 40;                // bytes before the frame
    static constexpr int HB = HL + RSK_HEAD_SIZE;     // bytes before the payload
    static constexpr int NPRE = HB / 16 + 1;          // chunks built from the prefix image
    static constexpr int NPW = 4 * NPRE;              // prefix words (covers HB + 16 payload bytes at least... up to 16*NPRE)
    static constexpr int D0 = 16 * NPRE - HB;         // payload offset of chunk NPRE's first byte
    static constexpr int CK = E + 36;                 // TCP checksum byte offset
    static constexpr int IPC = E + 10;                // IPv4 checksum byte offset
};

// payload bytes [0, 16) of a P-byte payload as 4 LE words (bytes past P zero)
__device__ __forceinline__ void wire_payload_prefix(const uint8_t *pay, uint32_t P, uint32_t (&pw)[4]) {
    rsk::load_window<4>(pay, pay + P - 1, pw);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = (int)P - 4 * q;
        pw[q] &= k >= 4 ? 0xffffffffu : (k <= 0 ? 0u : ((1u << (8 * k)) - 1u));
    }
}

// those words into the prefix image at wire offset HB (the part that falls inside the NPRE chunks)
template <int E>
__device__ __forceinline__ void wire_put_prefix(uint32_t (&PW)[WireGeom<E>::NPW], const uint32_t (&pw)[4]) {
    using G = WireGeom<E>;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int off = G::HB + 4 * q;
        const int nb = (off + 4 <= 4 * G::NPW) ? 4 : 4 * G::NPW - off;
        if (nb > 0) put_bytes(PW, off, pw[q], nb);
    }
}

// ---- phase 1 (one lane per packet): the wire prefix image PW = link header, IPv4 header (with its
// checksum), TCP header (checksum 0), frame bytes [0, 31) and payload bytes [0, D0) (masked to P);
// sum_pre = TCP checksum contribution of the pseudo-header and PW from the TCP header on; the
// packet status becomes the wire length.
template <int E>
__device__ __forceinline__ void wire_phase1(const EncArgs &a, const WireArgs &wa, const Lane1 &L, uint64_t i,
                                            uint32_t (&PW)[WireGeom<E>::NPW], uint32_t &sum_pre, int32_t &wst,
                                            bool pre = true) {
    using G = WireGeom<E>;
#pragma unroll
    for (int q = 0; q < G::NPW; ++q) PW[q] = 0;
    sum_pre = 0;
    wst = L.st;
    if (L.st <= 0) return;
    const uint32_t flen = (uint32_t)L.st, P = flen - RSK_HEAD_SIZE;
    const uint32_t wlen = G::HL + flen;
    wst = (int32_t)wlen;
    a.status[i] = wst;
    const uint32_t src = wa.src[i], dst = wa.dst[i], sp = wa.sp[i], dp = wa.dp[i];
    const uint32_t seq = wa.seq[i], ack = wa.ack[i], fl = wa.flag[i], id = wa.ip_id[i];
    if constexpr (E > 0) {
#pragma unroll
        for (int b = 0; b < E; b += 4) put_bytes(PW, b, wa.eth[b >> 2], E - b < 4 ? E - b : 4);
    }
    // IPv4 header (libnet_build_ipv4): 45 00 | len | id | 40 00 | 40 06 | csum | src | dst
    const uint32_t tot = 40u + flen;
    put_bytes(PW, E + 0, 0x45u | (rsk::bswap16(tot) << 16), 4);
    put_bytes(PW, E + 4, rsk::bswap16(id) | (0x0040u << 16), 4);
    put_bytes(PW, E + 8, 64u | (6u << 8), 2);
    put_bytes(PW, E + 12, src, 4);
    put_bytes(PW, E + 16, dst, 4);
    const uint32_t ips = hsum(0x45u | (rsk::bswap16(tot) << 16)) + hsum(rsk::bswap16(id) | (0x0040u << 16)) +
                         hsum(64u | (6u << 8)) + hsum(src) + hsum(dst);
    put_bytes(PW, G::IPC, ~fold16(ips) & 0xffffu, 2);
    // TCP header (libnet_build_tcp): sp dp seq ack | 50 flags | ffff | csum | 0000
    const uint32_t t0 = rsk::bswap16(sp) | (rsk::bswap16(dp) << 16), t1 = rsk::bswap32(seq),
                   t2 = rsk::bswap32(ack), t3 = 0x50u | (fl << 8) | (0xffffu << 16);
    put_bytes(PW, E + 20, t0, 4);
    put_bytes(PW, E + 24, t1, 4);
    put_bytes(PW, E + 28, t2, 4);
    put_bytes(PW, E + 32, t3, 4);
    // frame bytes [0, 31) = tag + EncHead (H[7]'s top byte is payload[0], written below)
#pragma unroll
    for (int q = 0; q < 8; ++q) put_bytes(PW, G::HL + 4 * q, L.H[q], q == 7 ? 3 : 4);
    // payload bytes [0, 16) (bounded by P; bytes past P stay zero); !pre: left to the copy loop
    // (copy_wire_pkt_dpp<..., TAG = true>), which adds them with the tag
    if (pre) {
        uint32_t pw[4];
        wire_payload_prefix(a.payload + L.po, P, pw);
        wire_put_prefix<E>(PW, pw);
    }
    // pseudo-header (src, dst, 0, 6, tcp_len) + TCP header + prefix frame/payload bytes, from the
    // TCP header start (even offset E + 20) to the end of the prefix chunks
    uint32_t s = hsum(src) + hsum(dst) + (6u << 8) + rsk::bswap16(20u + flen);
#pragma unroll
    for (int q = (E + 20) / 4; q < G::NPW; ++q) s += ((E + 20) % 4 && q == (E + 20) / 4) ? (PW[q] >> 16) : hsum(PW[q]);
    sum_pre = s;
}

// Wave-wide sum of v (each lane's value < 2^26): DPP row_shr 1/2/4/8 inclusive scans within each
// 16-lane row (bound_ctrl: lanes shifted in from outside the row read 0), then the four row totals.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
    return rdl(v, 15) + rdl(v, 31) + rdl(v, 47) + rdl(v, 63);
}

// A wire packet whose first byte sits r = dst mod 16 (1..15) bytes into a chunk: destination chunk j
// (aligned base d0 = dst - r) holds wire-image bytes [16j - r, 16j - r + 16), i.e. the 16 bytes at
// offset 16 - r of image chunks j - 1 and j.  Image chunks c < NPRE are the prefix image in LDS (the
// TCP checksum ORed into its chunk), c >= NPRE the payload chunks V of the copy (lane c - NPRE, slot
// q; zero past the packet).  Lane l of slot q stores destination chunk NPRE + l + 64q with its
// predecessor from lane l - 1 by a DPP wave shift (lane 0: the last prefix chunk, or lane 63 of slot
// 0), lanes 0 .. NPRE - 1 the prefix chunks; chunk 0 from byte r on, the last up to the packet's
// (padded) end, so packets packed at any byte offset never touch their neighbours.
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);  // wave_shr:1
}
template <int E, int NT>
__device__ __forceinline__ void wire_store_shifted(const EncArgs &a, const uint32_t *img, uint32_t ck, uint8_t *dst,
                                                   uint32_t r, uint32_t wlen, const uint4 (&V)[2], uint32_t lane) {
    using G = WireGeom<E>;
    uint8_t *d0 = dst - r;
    const uint32_t nst = (r + padded_len(dst, wlen, a.pad) + 15u) >> 4;
    const int wend = (int)(r + wlen);  // packet bytes counted from d0
    const bool pad = a.pad != 0u;
    const uint32_t sh = 16u - r;
    // slot 1's lane 0 takes lane 63 of slot 0 (read in uniform flow); slot 0's lane 0 the last prefix chunk
    const uint4 l63 = make_uint4(rdl(V[0].x, 63), rdl(V[0].y, 63), rdl(V[0].z, 63), rdl(V[0].w, 63));
    const uint4 lastpre = *reinterpret_cast<const uint4 *>(img + 4 * (G::NPRE - 1));  // never the checksum chunk
    static_assert(G::CK / 16 < G::NPRE - 1, "checksum chunk below the last prefix chunk");
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        uint4 prev = make_uint4(wave_shr1(V[q].x), wave_shr1(V[q].y), wave_shr1(V[q].z), wave_shr1(V[q].w));
        if (lane == 0u) prev = q == 0 ? lastpre : l63;
        const uint32_t j = G::NPRE + lane + 64u * q;
        if (j < nst) store_last16<NT>(d0 + 16u * j, rsk::funnel16(prev, V[q], sh), wend - 16 * (int)j, pad);
    }
    if (lane < (uint32_t)G::NPRE && lane < nst) {
        uint4 c1 = *reinterpret_cast<const uint4 *>(img + 4u * lane);
        uint4 c0 = lane ? *reinterpret_cast<const uint4 *>(img + 4u * (lane - 1u)) : make_uint4(0u, 0u, 0u, 0u);
        constexpr uint32_t kc = G::CK / 16, kw = (G::CK & 15) >> 2, kb = 8 * (G::CK & 3);
        const uint32_t cw = ck << kb;
        if (lane == kc) {
            if (kw == 0) c1.x |= cw; else if (kw == 1) c1.y |= cw; else if (kw == 2) c1.z |= cw; else c1.w |= cw;
        }
        if (lane == kc + 1u) {
            if (kw == 0) c0.x |= cw; else if (kw == 1) c0.y |= cw; else if (kw == 2) c0.z |= cw; else c0.w |= cw;
        }
        const uint4 d = rsk::funnel16(c0, c1, sh);
        if (lane == 0u) rsk::store_range16(d0, d, r, 16u);
        else store_last16<NT>(d0 + 16u * lane, d, wend - 16 * (int)lane, pad);
    }
}

// ---- the same with one aligned load per chunk: the funnel partner comes from lane + 1 by DPP (as
// copy_pkt_dpp), all PU packets' loads issued before the first shift. ------------------------------
// TAG (sets of long frames, as copy_pkt_dpp_tag): phase 1 left the tag, payload[0] at frame byte
// 31 and the payload prefix bytes out of the prefix images, so that each payload's first line is read
// once, here, next to the chunk loads that fetch it anyway.  Lane p loads packet p's first 16 payload
// bytes before the chunk loads, runs the MD5 while they are in flight, ORs the missing bytes into
// the packet's LDS prefix image and hands their checksum share to the packet's checksum.
template <int E, int PU, int NT, bool TAG = false>
__device__ __forceinline__ void copy_wire_pkt_dpp(const EncArgs &a, const KeySched &ks, const Lane1 &L,
                                                  uint32_t *stage, uint32_t sum_pre, int32_t wst, uint32_t lane,
                                                  uint64_t vm) {
    using G = WireGeom<E>;
    while (vm) {
        uint32_t js[PU];
        bool on[PU];
#pragma unroll
        for (int p = 0; p < PU; ++p) {
            on[p] = vm != 0ull;
            js[p] = on[p] ? (uint32_t)__builtin_ctzll(vm) : 0u;
            if (on[p]) vm &= vm - 1ull;
        }
        uint32_t pw[4] = {0u, 0u, 0u, 0u}, myP = 0, myj = 0;  // TAG: lane p's packet
        if constexpr (TAG) {
            uint64_t mypo = 0;
#pragma unroll
            for (int p = 0; p < PU; ++p) {  // uniform readlanes, per-lane selects
                const uint32_t wl = on[p] ? rdl((uint32_t)wst, js[p]) : 0u;
                const uint64_t po = rdl64(L.po, js[p]);
                if (lane == (uint32_t)p) {
                    myP = on[p] ? wl - G::HB : 0u;
                    mypo = po;
                    myj = js[p];
                }
            }
            if (myP) wire_payload_prefix(a.payload + mypo, myP, pw);
        }
        uint4 A[PU][2];
        uint32_t wlen[PU], shp[PU];
        uint8_t *dstp[PU];
        bool ld1[PU];  // source chunk 64 holds payload bytes (slot 1 loaded; lane 63's funnel partner)
#pragma unroll
        for (int p = 0; p < PU; ++p) {
            wlen[p] = on[p] ? (uint32_t)rdl((uint32_t)wst, js[p]) : 0u;
            const uint32_t P = wlen[p] - G::HB;
            const uint8_t *pay = a.payload + rdl64(L.po, js[p]);
            dstp[p] = a.frame + rdl64(L.fo, js[p]);
            shp[p] = (uint32_t)((reinterpret_cast<uintptr_t>(pay) + G::D0) & 15u);
            const uint8_t *src_al = pay + G::D0 - shp[p];
            const int32_t last_rel = (int32_t)P - 1 - G::D0 + (int32_t)shp[p];
            // round 4: slot 1 skipped for packets that do not reach it -- RAW4 only: measured on
            // Ethernet packets it cost more (SGPR spills 392 -> 450, C4 0.421 -> 0.451 ms) than it saved
            // (RAW4 C4 0.455 -> 0.413 ms, C3 2.339 -> 2.295; profiles/r04_paths_wire.json)
            ld1[p] = E != 0 || (on[p] && last_rel >= 16 * 64);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const uint32_t m = lane + 64u * q;  // source chunk of frame chunk NPRE + m
                A[p][q] = make_uint4(0u, 0u, 0u, 0u);
                // slot 1 only for payloads reaching source chunk 64 (uniform: most C4 packets do not)
                if (q == 1 && !ld1[p]) continue;
                if (on[p] && (int32_t)(16u * m) <= last_rel) A[p][q] = ld16<0>(src_al + 16u * m);
            }
        }
        uint32_t dsum = 0;  // TAG: lane p, checksum share of the bytes it adds to packet p's prefix image
        if constexpr (TAG) {
            uint32_t t0, t1;
            tag_of(ks, pw[0] & 0xffu, t0, t1);
            uint32_t D[G::NPW];
#pragma unroll
            for (int q = 0; q < G::NPW; ++q) D[q] = 0;
            put_bytes(D, G::HL, t0, 4);
            put_bytes(D, G::HL + 4, t1, 4);
            wire_put_prefix<E>(D, pw);  // payload bytes from wire offset HB (frame byte 31 = payload[0])
            if (myP) {
#pragma unroll
                for (int q = G::HL / 4; q < G::NPW; ++q) {
                    stage[myj * G::NPW + q] |= D[q];
                    dsum += hsum(D[q]);
                }
            }
            wave_lds_sync();
        }
        uint4 v[PU][2];
        uint32_t ck[PU];
#pragma unroll
        for (int p = 0; p < PU; ++p) {
            uint4 B[2];
            B[0] = make_uint4(wave_shl1(A[p][0].x), wave_shl1(A[p][0].y), wave_shl1(A[p][0].z), wave_shl1(A[p][0].w));
            B[1] = make_uint4(0u, 0u, 0u, 0u);
            const uint32_t nch = (wlen[p] + 15u) >> 4;
            // round 4: slot 1's shifts, funnels and sums only for packets that reach it (uniform); a
            // dead slot 1 holds zeros, which is what the zero-pad stores below need
            const bool s1 = E != 0 || nch > (uint32_t)G::NPRE + 64u;  // implies ld1[p]
            if (ld1[p]) {
                const uint4 l0 = make_uint4(rdl(A[p][1].x, 0), rdl(A[p][1].y, 0), rdl(A[p][1].z, 0),
                                            rdl(A[p][1].w, 0));  // read in uniform flow (see k_encode)
                if (lane == 63u) B[0] = l0;
            }
            if (s1)
                B[1] = make_uint4(wave_shl1(A[p][1].x), wave_shl1(A[p][1].y), wave_shl1(A[p][1].z), wave_shl1(A[p][1].w));
            uint32_t part = 0;
            v[p][1] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (q == 1 && !s1) continue;  // uniform
                const uint32_t k = G::NPRE + lane + 64u * q;
                v[p][q] = rsk::funnel16(A[p][q], B[q], shp[p]);
                const int lim = (int)wlen[p] - 16 * (int)k;
                if (k < nch) {
                    if (lim < 16) v[p][q] = rsk::keep_bytes16(v[p][q], lim);
                    part = hsum4(v[p][q], part);
                }
            }
            ck[p] = part;
        }
#pragma unroll
        for (int p = 0; p < PU; ++p)
            ck[p] = ~fold16(wave_sum(ck[p]) + rdl(sum_pre, js[p]) + (TAG ? rdl(dsum, (uint32_t)p) : 0u)) & 0xffffu;
#pragma unroll
        for (int p = 0; p < PU; ++p) {
            if (!on[p]) continue;
            const uint32_t r = (uint32_t)(reinterpret_cast<uintptr_t>(dstp[p]) & 15u);  // uniform
            if (r == 0u) {
                const uint32_t nst = (padded_len(dstp[p], wlen[p], a.pad) + 15u) >> 4;
                if (lane < (uint32_t)G::NPRE && lane < nst) {
                    const uint4 sv = *reinterpret_cast<const uint4 *>(stage + js[p] * G::NPW + 4u * lane);
                    uint32_t w4[4] = {sv.x, sv.y, sv.z, sv.w};
                    if (lane == (uint32_t)(G::CK / 16)) w4[(G::CK & 15) >> 2] |= ck[p] << (8 * (G::CK & 3));
                    store_last16<NT>(dstp[p] + 16u * lane, make_uint4(w4[0], w4[1], w4[2], w4[3]),
                                    (int)wlen[p] - 16 * (int)lane, a.pad != 0u);
                }
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    if (E == 0 && q == 1 && nst <= (uint32_t)G::NPRE + 64u) continue;  // uniform
                    const uint32_t k = G::NPRE + lane + 64u * q;
                    if (k < nst) store_last16<NT>(dstp[p] + 16u * k, v[p][q], (int)wlen[p] - 16 * (int)k, a.pad != 0u);
                }
            } else {
                wire_store_shifted<E, NT>(a, stage + js[p] * G::NPW, ck[p], dstp[p], r, wlen[p], v[p], lane);
            }
        }
    }
}

// ---- flat copy for short packets, two passes over the set: (1) the payload chunks of all packets as
// one flat chunk list (as copy_flat), each lane adding its chunk's halfword sum into the packet's
// LDS slot; (2) the NPRE prefix chunks of every packet as a dense (packet, chunk) grid read from the
// LDS stage, the TCP checksum patched into chunk CK/16 — both passes store coalesced runs.
template <int E, int U>
__device__ __forceinline__ void copy_wire_flat(const EncArgs &a, const Lane1 &L, const uint32_t *stage,
                                               uint32_t sum_pre, int32_t wst, uint32_t lane, bool mine,
                                               CopyRec *recs, uint32_t *cend, uint32_t *psum) {
    using G = WireGeom<E>;
    uint32_t cc = 0;
    CopyRec r;
    r.src_al = nullptr; r.dst = nullptr; r.cstart = 0; r.sh = 0; r.last_rel = 0; r.flen = 0;
    if (mine) {
        uint8_t *dst = a.frame + L.fo;
        const uint32_t wlen = (uint32_t)wst;
        const uint32_t nst = (padded_len(dst, wlen, a.pad) + 15u) >> 4;
        cc = nst > (uint32_t)G::NPRE ? nst - G::NPRE : 0u;
        const uint8_t *pay = a.payload + L.po;
        const uint32_t sh = (uint32_t)((reinterpret_cast<uintptr_t>(pay) + G::D0) & 15u);
        r.src_al = pay + G::D0 - sh;
        r.dst = dst;
        r.sh = sh;
        r.last_rel = (int32_t)(wlen - G::HB) - 1 - G::D0 + (int32_t)sh;
        r.flen = wlen;
    }
    uint32_t inc = cc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(inc, off);
        if (lane >= (uint32_t)off) inc += v;
    }
    r.cstart = inc - cc;
    recs[lane] = r;
    cend[lane] = inc;
    psum[lane] = sum_pre;
    const uint32_t C = (uint32_t)__shfl((int)inc, 63);
    wave_lds_sync();
    for (uint32_t g0 = 0; g0 < C; g0 += 64u * U) {
        uint4 A[U], B[U];
        uint8_t *dsts[U];
        uint32_t shs[U], pk[U];
        int32_t lims[U];
        bool act[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t g = g0 + 64u * u + lane;
            act[u] = g < C;
            A[u] = make_uint4(0u, 0u, 0u, 0u);
            B[u] = make_uint4(0u, 0u, 0u, 0u);
            shs[u] = 0;
            lims[u] = 0;
            dsts[u] = nullptr;
            pk[u] = 0;
            if (act[u]) {
                uint32_t lo = 0;
#pragma unroll
                for (uint32_t st = 32; st; st >>= 1)
                    if (cend[lo + st - 1] <= g) lo += st;
                const CopyRec rr = recs[lo];
                const uint32_t ro = 16u * (g - rr.cstart);
                lims[u] = (int32_t)rr.flen - 16 * G::NPRE - (int32_t)ro;
                if (lims[u] > 0) {  // chunk holds packet bytes (else pure pad)
                    A[u] = ld16<0>(rr.src_al + ro);
                    if (rr.sh != 0u && (int32_t)(ro + 16u) <= rr.last_rel) B[u] = ld16<0>(rr.src_al + ro + 16);
                }
                shs[u] = rr.sh;
                dsts[u] = rr.dst + 16 * G::NPRE + ro;
                pk[u] = lo;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!act[u]) continue;
            uint4 v = funnel16_lane(A[u], B[u], shs[u]);
            if (lims[u] < 16) v = lims[u] > 0 ? rsk::keep_bytes16(v, lims[u]) : make_uint4(0u, 0u, 0u, 0u);
            const uint32_t s = hsum4(v, 0u);
            if (s) atomicAdd(&psum[pk[u]], s);
            store_last16<0>(dsts[u], v, lims[u], a.pad != 0u);
        }
    }
    wave_lds_sync();
    // pass 2: prefix chunk (j, c) for g = NPRE * j + c
#pragma unroll
    for (int t = 0; t < G::NPRE; ++t) {
        const uint32_t g = 64u * t + lane;
        const uint32_t j = g / G::NPRE, c = g - j * G::NPRE;
        const CopyRec rr = recs[j];
        if (rr.dst == nullptr) continue;  // not a vector-path packet
        const uint32_t nstj = (padded_len(rr.dst, rr.flen, a.pad) + 15u) >> 4;
        if (c >= nstj) continue;
        const uint4 sv = *reinterpret_cast<const uint4 *>(stage + j * G::NPW + 4u * c);
        uint32_t w4[4] = {sv.x, sv.y, sv.z, sv.w};
        if (c == (uint32_t)(G::CK / 16)) {
            const uint32_t ck = ~fold16(psum[j]) & 0xffffu;
            w4[(G::CK & 15) >> 2] |= ck << (8 * (G::CK & 3));
        }
        store_last16<0>(rr.dst + 16u * c, make_uint4(w4[0], w4[1], w4[2], w4[3]), (int)rr.flen - 16 * (int)c,
                        a.pad != 0u);
    }
}

// ---- the flat copy at any packet alignment (sets with an unaligned packet): the flat list holds
// DESTINATION chunks j >= NPRE of every packet (r = dst mod 16; chunk j holds wire-image bytes
// [16j - r, 16j - r + 16), the image chunks j - 1 and j funnelled by 16 - r).  A lane loads the
// source chunks of image chunks j - 1 and j (three aligned loads; image chunk NPRE - 1 is the last
// prefix chunk, from LDS), adds image chunk j's halfword sum to the packet's checksum (each image
// chunk once: the extra destination chunk past the image sums nothing) and stores chunk j whole;
// pass 2 stores the shifted prefix chunks (chunk 0 from byte r on) with the checksum.  Aligned
// packets (r = 0) of such a set take the same path with chunk j = image chunk j.
template <int E, int U>
__device__ __forceinline__ void copy_wire_flat_any(const EncArgs &a, const Lane1 &L, const uint32_t *stage,
                                                   uint32_t sum_pre, int32_t wst, uint32_t lane, bool mine,
                                                   CopyRec *recs, uint32_t *cend, uint32_t *psum) {
    using G = WireGeom<E>;
    uint32_t cc = 0;
    CopyRec r;
    r.src_al = nullptr; r.dst = nullptr; r.cstart = 0; r.sh = 0; r.last_rel = 0; r.flen = 0;
    if (mine) {
        uint8_t *dst = a.frame + L.fo;
        const uint32_t wlen = (uint32_t)wst;
        const uint32_t ro = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
        const uint32_t nst = (ro + padded_len(dst, wlen, a.pad) + 15u) >> 4;  // destination chunks from d0
        cc = nst > (uint32_t)G::NPRE ? nst - G::NPRE : 0u;
        const uint8_t *pay = a.payload + L.po;
        const uint32_t sh = (uint32_t)((reinterpret_cast<uintptr_t>(pay) + G::D0) & 15u);
        r.src_al = pay + G::D0 - sh;
        r.dst = dst;
        r.sh = sh | (ro << 4);
        r.last_rel = (int32_t)(wlen - G::HB) - 1 - G::D0 + (int32_t)sh;
        r.flen = wlen;
    }
    uint32_t inc = cc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(inc, off);
        if (lane >= (uint32_t)off) inc += v;
    }
    r.cstart = inc - cc;
    recs[lane] = r;
    cend[lane] = inc;
    psum[lane] = sum_pre;
    const uint32_t C = (uint32_t)__shfl((int)inc, 63);
    wave_lds_sync();
    for (uint32_t g0 = 0; g0 < C; g0 += 64u * U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t g = g0 + 64u * u + lane;
            if (g >= C) continue;
            uint32_t lo = 0;
#pragma unroll
            for (uint32_t st = 32; st; st >>= 1)
                if (cend[lo + st - 1] <= g) lo += st;
            const CopyRec rr = recs[lo];
            const uint32_t sh = rr.sh & 15u, ro = rr.sh >> 4;
            const uint32_t m = g - rr.cstart;  // image / destination chunk NPRE + m
            // image chunk NPRE + m from source chunks m, m + 1; image chunk NPRE + m - 1 from m - 1, m
            uint4 S0 = make_uint4(0u, 0u, 0u, 0u), S1 = S0, S2 = S0;
            if ((int32_t)(16u * m) <= rr.last_rel) S1 = ld16<0>(rr.src_al + 16u * m);
            if ((int32_t)(16u * m + 16u) <= rr.last_rel) S2 = ld16<0>(rr.src_al + 16u * m + 16u);
            if (ro != 0u && m != 0u) S0 = ld16<0>(rr.src_al + 16u * m - 16u);
            const int32_t limi = (int32_t)rr.flen - 16 * (G::NPRE + (int32_t)m);  // packet bytes in image chunk
            uint4 im = limi > 0 ? funnel16_lane(S1, S2, sh) : make_uint4(0u, 0u, 0u, 0u);
            if (limi > 0 && limi < 16) im = rsk::keep_bytes16(im, limi);
            const uint32_t s = hsum4(im, 0u);
            if (s) atomicAdd(&psum[lo], s);
            uint4 d = im;
            if (ro != 0u) {
                const uint4 ip = m == 0u ? *reinterpret_cast<const uint4 *>(stage + lo * G::NPW + 4 * (G::NPRE - 1))
                                         : funnel16_lane(S0, S1, sh);  // image chunk NPRE + m - 1 (full)
                d = funnel16_lane(ip, im, 16u - ro);
            }
            const uint32_t jj = G::NPRE + m;
            store_last16<0>(rr.dst - ro + 16u * jj, d, (int)(ro + rr.flen) - 16 * (int)jj, a.pad != 0u);
        }
    }
    wave_lds_sync();
    // pass 2: shifted prefix chunk (j, c) for g = NPRE * j + c
    static_assert(G::CK / 16 < G::NPRE - 1, "checksum chunk below the last prefix chunk");
#pragma unroll
    for (int t = 0; t < G::NPRE; ++t) {
        const uint32_t g = 64u * t + lane;
        const uint32_t j = g / G::NPRE, c = g - j * G::NPRE;
        const CopyRec rr = recs[j];
        if (rr.dst == nullptr) continue;  // not framed
        const uint32_t ro = rr.sh >> 4;
        const uint32_t nstj = (ro + padded_len(rr.dst, rr.flen, a.pad) + 15u) >> 4;
        if (c >= nstj) continue;
        const uint32_t ck = ~fold16(psum[j]) & 0xffffu;
        constexpr uint32_t kc = G::CK / 16, kw = (G::CK & 15) >> 2, kb = 8 * (G::CK & 3);
        uint4 c1 = *reinterpret_cast<const uint4 *>(stage + j * G::NPW + 4u * c);
        uint4 c0 = c ? *reinterpret_cast<const uint4 *>(stage + j * G::NPW + 4u * (c - 1u)) : make_uint4(0u, 0u, 0u, 0u);
        const uint32_t cw = ck << kb;
        if (c == kc) {
            if (kw == 0) c1.x |= cw; else if (kw == 1) c1.y |= cw; else if (kw == 2) c1.z |= cw; else c1.w |= cw;
        }
        if (c == kc + 1u) {
            if (kw == 0) c0.x |= cw; else if (kw == 1) c0.y |= cw; else if (kw == 2) c0.z |= cw; else c0.w |= cw;
        }
        uint8_t *d0 = rr.dst - ro;
        if (ro == 0u) store_last16<0>(d0 + 16u * c, c1, (int)rr.flen - 16 * (int)c, a.pad != 0u);
        else if (c == 0u) rsk::store_range16(d0, funnel16_lane(c0, c1, 16u - ro), ro, 16u);
        else store_last16<0>(d0 + 16u * c, funnel16_lane(c0, c1, 16u - ro), (int)(ro + rr.flen) - 16 * (int)c,
                             a.pad != 0u);
    }
}

// The per-set wire build: two launches over the same grid (k_encode's grouped-interleave mapping:
// 8-packet groups across 1024-wave super-blocks, grid by enc_grid).  Each wave derives the set's copy
// path from pay_len alone -- the flat chunk list below a set-mean wire length of kFlatBelowMeanBytes,
// else the per-packet DPP copy -- and returns unless it is its launch's path, so every set is handled
// exactly once and each launch sizes LDS (hence occupancy) for its own path only (one launch holding
// both: C3 2.75 vs 2.52 ms).  MODE 5: the per-packet half (PU packets per iteration), with the tag and
// payload prefix deferred into the copy loop for sets of long frames; MODE 4: the flat half.
template <int E, int MODE>
struct WireLds {
    static constexpr int kStage = 64 * WireGeom<E>::NPW * 4;  // prefix images (both paths)
    static constexpr bool kFlat = MODE == 4;
    static constexpr int kBytes = kStage + (kFlat ? 64 * (int)sizeof(CopyRec) + 2 * 64 * 4 : 0);
};

// Per-wave copy-path choice (identical in both launches).
__device__ __forceinline__ bool wire_flat_choice(bool vec, uint32_t wlen) {
    uint32_t fl = vec ? wlen : 0u;
#pragma unroll
    for (int off = 32; off; off >>= 1) fl += __shfl_xor(fl, off);
    return fl < kFlatBelowMeanBytes * (uint32_t)__popcll(__ballot(vec));
}

template <int E, int MODE, int PU, int U>
__device__ __forceinline__ void encode_wire_set(const EncArgs &a, const WireArgs &wa, const KeySched &ks) {
    static_assert(MODE == 4 || MODE == 5, "the flat half and the per-packet half");
    using G = WireGeom<E>;
    __shared__ uint4 lds[kWavesPerBlock][WireLds<E, MODE>::kBytes / 16];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    // set_packet's mapping, spelled out: through the helper these kernels' register allocation changes
    const uint64_t wg = (uint64_t)blockIdx.x * kWavesPerBlock + w;
    const uint64_t sb = wg / kSetSbw, wl = wg % kSetSbw;
    const uint64_t first = sb * (kSetSbw * 64u) + wl * kSetGrp;
    if (first >= a.n) return;  // wave-uniform; no block barriers below
    const uint64_t gi = sb * (kSetSbw * 64u) + ((uint64_t)(lane / kSetGrp) * kSetSbw + wl) * kSetGrp + lane % kSetGrp;
    const uint64_t i = gi < a.n ? gi : a.n;
    {  // is this set ours?
        bool v0 = false;
        uint32_t wlen = 0;
        if (i < a.n) {
            const uint32_t P = a.pay_len[i];
            v0 = P != 0u && P <= (uint32_t)RSK_MAX_PAYLOAD;  // any alignment: both copies take all
            wlen = G::HL + RSK_HEAD_SIZE + P;
        }
        if (wire_flat_choice(v0, wlen) != (MODE == 4)) return;
    }
    Lane1 L = encode_phase1<MODE != 5>(a, ks, i);
    bool defer = false;
    if constexpr (MODE == 5) {  // the set mean frame length decides (as k_encode)
        const bool v = L.st > 0;
        uint32_t fl = v ? (uint32_t)L.st : 0u;
#pragma unroll
        for (int off = 32; off; off >>= 1) fl += __shfl_xor(fl, off);
        defer = fl >= kDeferTagMeanBytes * (uint32_t)__popcll(__ballot(v));
        if (!defer) encode_tag(a, ks, L);
    }
    uint32_t PW[G::NPW];
    uint32_t sum_pre;
    int32_t wst;
    wire_phase1<E>(a, wa, L, i, PW, sum_pre, wst, !defer);
    const bool vec = L.st > 0;  // every framed packet takes a vector path, at any alignment
    const uint64_t vm = __ballot(vec);
    uint8_t *slice = reinterpret_cast<uint8_t *>(lds[w]);
    uint32_t *stage = reinterpret_cast<uint32_t *>(slice);
    if (L.st > 0) {  // every framed packet's prefix image
#pragma unroll
        for (int c = 0; c < G::NPRE; ++c)
            *reinterpret_cast<uint4 *>(stage + lane * G::NPW + 4 * c) =
                make_uint4(PW[4 * c], PW[4 * c + 1], PW[4 * c + 2], PW[4 * c + 3]);
    }
    if constexpr (MODE == 4) {
        CopyRec *recs = reinterpret_cast<CopyRec *>(slice + WireLds<E, MODE>::kStage);
        uint32_t *cend = reinterpret_cast<uint32_t *>(slice + WireLds<E, MODE>::kStage + 64 * sizeof(CopyRec));
        if (__ballot(L.st > 0 && L.slow) != 0ull)  // an unaligned packet: the any-alignment list
            copy_wire_flat_any<E, U>(a, L, stage, sum_pre, wst, lane, L.st > 0, recs, cend, cend + 64);
        else
            copy_wire_flat<E, U>(a, L, stage, sum_pre, wst, lane, vec, recs, cend, cend + 64);
    } else {
        wave_lds_sync();
        // store policy per set, as k_encode: stream the stores when the wire packets leave gaps
        uint64_t nfo;
        bool nvec;
        const bool gaps = set_gaps(a, L.fo, (uint32_t)wst, vec, lane, nfo, nvec);
        if (defer) {
            if (gaps) copy_wire_pkt_dpp<E, PU, 2, true>(a, ks, L, stage, sum_pre, wst, lane, vm);
            else copy_wire_pkt_dpp<E, PU, 0, true>(a, ks, L, stage, sum_pre, wst, lane, vm);
        } else {
            if (gaps) copy_wire_pkt_dpp<E, PU, 2>(a, ks, L, stage, sum_pre, wst, lane, vm);
            else copy_wire_pkt_dpp<E, PU, 0>(a, ks, L, stage, sum_pre, wst, lane, vm);
        }
    }
}

template <int E, int MODE, int PU, int U>
__global__ __launch_bounds__(kBlock) void k_encode_wire(EncArgs a, WireArgs wa, KeySched ks) {
    stage_tags(ks);
    encode_wire_set<E, MODE, PU, U>(a, wa, ks);
}

// The same held to 4 waves per SIMD (<= 128 VGPRs): the deferred-tag build (MODE 5) needs 131 and
// would otherwise drop to 3, which costs the sets that keep the tag in phase 1 (C4 +9 %).
template <int E, int MODE, int PU, int U>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_encode_wire_w4(
    EncArgs a, WireArgs wa, KeySched ks) {
    stage_tags(ks);
    encode_wire_set<E, MODE, PU, U>(a, wa, ks);
}

// ---- the two-pass wire build (round 6): a header pass, one lane per packet (MD5
// tags 64 to a wave), writes each packet's whole header image -- link, IPv4 with its checksum, TCP,
// the 31 frame-head bytes: wire bytes [0, HB), HB = 71 RAW4 / 85 Ethernet -- as Q + 1 = 5 / 6 16-B
// chunks of a record, with the TCP checksum's share of the pseudo-header and the image (from the TCP
// header on) in the last chunk's bytes 12..15, which the payload overwrites; the status is the wire
// length.  Then copy waves of K packets as k_encode_copy's: lane k takes IMAGE chunk k -- wire bytes
// [16k, 16k + 16): the record's chunk (one 16-B load by lanes 0..Q) for k < Q, record and payload for
// k = Q, payload beyond (one aligned load per chunk and the DPP funnel) -- sums the payload halfwords
// on the way into the TCP checksum (a wave reduction), which the lane of the checksum chunk ORs in
// before the stores.  A packet whose first byte is not 16-B aligned (r = dst mod 16) stores
// destination chunk j = image chunks j - 1 and j funnelled by 16 - r (wave_shr:1), so the checksum is
// summed in image coordinates at any alignment.
template <int E>
struct WireRec {
    static constexpr int HB = WireGeom<E>::HB, Q = HB / 16, R = HB % 16;  // RAW4 71 = 4 x 16 + 7; Eth 85 = 5 x 16 + 5
    static constexpr int NC = Q + 1;                                       // record chunks (80 / 96 B)
    static_assert(R != 0 && R <= 12 && WireGeom<E>::CK / 16 < Q, "record layout");
};

// base: the chunk's first packet (a.n = its end); chunk c of packet i at rec[c * stride + i - base]
template <int E>
__global__ __launch_bounds__(kBlock) void k_wire_heads(EncArgs a, WireArgs wa, KeySched ks, uint4 *rec,
                                                       uint32_t *stat, uint64_t base, uint64_t stride) {
    using G = WireGeom<E>;
    using W = WireRec<E>;
    constexpr int NIW = 4 * W::NC;
    stage_tags(ks);
    enc_sample(a.pay_len, a.n, stat);
    const uint64_t i = base + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const Lane1 L = encode_phase1<true, true, G::HL>(a, ks, i < a.n ? i : a.n);
    if (i >= a.n || L.st <= 0) return;
    const uint32_t flen = (uint32_t)L.st;
    uint32_t PW[NIW];
#pragma unroll
    for (int q = 0; q < NIW; ++q) PW[q] = 0u;
    const uint32_t src = wa.src[i], dst = wa.dst[i], sp = wa.sp[i], dp = wa.dp[i];
    const uint32_t seq = wa.seq[i], ack = wa.ack[i], fl = wa.flag[i], id = wa.ip_id[i];
    if constexpr (E > 0) {
#pragma unroll
        for (int b = 0; b < E; b += 4) put_bytes(PW, b, wa.eth[b >> 2], E - b < 4 ? E - b : 4);
    }
    // IPv4 header (libnet_build_ipv4): 45 00 | len | id | 40 00 | 40 06 | csum | src | dst
    const uint32_t tot = 40u + flen;
    const uint32_t ip0 = 0x45u | (rsk::bswap16(tot) << 16), ip1 = rsk::bswap16(id) | (0x0040u << 16);
    put_bytes(PW, E + 0, ip0, 4);
    put_bytes(PW, E + 4, ip1, 4);
    put_bytes(PW, E + 8, 64u | (6u << 8), 2);
    put_bytes(PW, E + 12, src, 4);
    put_bytes(PW, E + 16, dst, 4);
    const uint32_t ips = hsum(ip0) + hsum(ip1) + hsum(64u | (6u << 8)) + hsum(src) + hsum(dst);
    put_bytes(PW, G::IPC, ~fold16(ips) & 0xffffu, 2);
    // TCP header (libnet_build_tcp): sp dp seq ack | 50 flags | ffff | csum (0 here) | 0000
    put_bytes(PW, E + 20, rsk::bswap16(sp) | (rsk::bswap16(dp) << 16), 4);
    put_bytes(PW, E + 24, rsk::bswap32(seq), 4);
    put_bytes(PW, E + 28, rsk::bswap32(ack), 4);
    put_bytes(PW, E + 32, 0x50u | (fl << 8) | (0xffffu << 16), 4);
    // frame bytes [0, 31) = tag + EncHead (payload[0], H[7]'s top byte, comes with the payload)
#pragma unroll
    for (int q = 0; q < 8; ++q) put_bytes(PW, G::HL + 4 * q, L.H[q], q == 7 ? 3 : 4);
    // the checksum's share: pseudo-header (src, dst, 0, 6, tcp_len) + the image from the TCP header on
    uint32_t s = hsum(src) + hsum(dst) + (6u << 8) + rsk::bswap16(20u + flen);
#pragma unroll
    for (int q = (E + 20) / 4; q < NIW; ++q) s += ((E + 20) % 4 && q == (E + 20) / 4) ? (PW[q] >> 16) : hsum(PW[q]);
    PW[NIW - 1] = s;  // bytes 12..15 of chunk Q: payload positions, overwritten by the copy
    // chunk-major records: each store instruction of the wave writes 1 KB contiguous
#pragma unroll
    for (int c = 0; c < W::NC; ++c)
        rec[(uint64_t)c * stride + (i - base)] = make_uint4(PW[4 * c], PW[4 * c + 1], PW[4 * c + 2], PW[4 * c + 3]);
}

// base: the launch's first packet; rbase / stride: the record chunk's (k_wire_heads)
template <int E, int K>
__global__ __launch_bounds__(kBlock) void k_wire_copy(EncArgs a, const uint4 *rec, uint64_t base, uint64_t rbase,
                                                      uint64_t stride) {
    using G = WireGeom<E>;
    using W = WireRec<E>;
    constexpr int HB = W::HB, Q = W::Q, R = W::R;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t i0 = base + ((uint64_t)blockIdx.x * kWavesPerBlock + w) * K;
    if (i0 >= a.n) return;
    // descriptors, lanes 0..K-1 (one round trip)
    uint32_t dP = 0;
    uint64_t dpo = 0, dfo = 0;
    {
        const uint64_t il = i0 + lane;
        if (lane < (uint32_t)K && il < a.n) {
            dP = a.pay_len[il];
            dpo = a.pay_off[il];
            dfo = a.frame_off[il];
        }
    }
    uint4 A[K][2], H[K];
    uint32_t Pp[K], shp[K];
#pragma unroll
    for (int p = 0; p < K; ++p) {
        const uint32_t P = rdl(dP, (uint32_t)p);
        const bool on = i0 + p < a.n && P != 0u && P <= (uint32_t)RSK_MAX_PAYLOAD;  // uniform
        Pp[p] = on ? P : 0u;
        // the record chunk of lane k <= Q
        H[p] = on && lane <= (uint32_t)Q ? rec[(uint64_t)lane * stride + (i0 + p - rbase)] : make_uint4(0u, 0u, 0u, 0u);
        const uint8_t *src = a.payload + rdl64(dpo, (uint32_t)p);
        shp[p] = (uint32_t)((reinterpret_cast<uintptr_t>(src) - (uint32_t)R) & 15u);
        const uint8_t *srcp = src - R - shp[p];  // aligned: image chunk k <- source chunks k - Q, k - Q + 1
        const int32_t first_rel = R + (int32_t)shp[p], last_rel = first_rel + (int32_t)P - 1;
        const int32_t m_lo = first_rel >> 4, m_hi = last_rel >> 4;
        const uint32_t nch = (HB + P + 15u) >> 4;  // image chunks
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            A[p][q] = make_uint4(0u, 0u, 0u, 0u);
            if (!on || (q == 1 && nch < 64u)) continue;  // uniform
            const int32_t m = (int32_t)(lane + 64u * q) - Q;
            const int32_t mc = m < m_lo ? m_lo : m > m_hi ? m_hi : m;  // dead lanes re-read a live chunk
            A[p][q] = ld16<kStream>(srcp + 16 * mc);
        }
    }
    // Three phases over the K packets, so the packets' dependency chains overlap (round 6: one packet at a
    // time, the wave waited on each packet's funnel -> sum -> reduction chain in turn): (1) each lane's
    // image chunks and payload halfword sums, (2) the K checksums (wave reductions), (3) the stores.
    // Header mask of lane k <= Q (the record's bytes: all of chunk k < Q, the first R of chunk Q).
    const uint4 mh = lane <= (uint32_t)Q ? rsk::keep_bytes16(make_uint4(~0u, ~0u, ~0u, ~0u), lane < (uint32_t)Q ? 16 : R)
                                         : make_uint4(0u, 0u, 0u, 0u);
    uint4 VI[K][2];
    uint32_t part[K];
#pragma unroll
    for (int p = 0; p < K; ++p) {
        VI[p][0] = VI[p][1] = make_uint4(0u, 0u, 0u, 0u);
        part[p] = 0u;
        const uint32_t P = Pp[p];
        if (!P) continue;  // uniform
        const uint32_t wlen = HB + P, nch = (wlen + 15u) >> 4;
        uint4 B[2];
        B[0] = make_uint4(wave_shl1(A[p][0].x), wave_shl1(A[p][0].y), wave_shl1(A[p][0].z), wave_shl1(A[p][0].w));
        B[1] = make_uint4(0u, 0u, 0u, 0u);
        if (nch >= 64u) {  // uniform
            const uint4 l0 = rdl4(A[p][1], 0);
            if (lane == 63u) B[0] = l0;
            B[1] = make_uint4(wave_shl1(A[p][1].x), wave_shl1(A[p][1].y), wave_shl1(A[p][1].z), wave_shl1(A[p][1].w));
        }
        // lane k's image chunk: the record's bytes under mh, the payload's elsewhere (zero past the
        // packet); summed: the payload bytes only (the record's are in its checksum share)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (q == 1 && nch <= 64u) continue;  // uniform
            const uint32_t k = lane + 64u * q;
            uint4 v = rsk::funnel16(A[p][q], B[q], shp[p]);
            const int lim = (int)wlen - 16 * (int)k;
            v = lim >= 16 ? v : lim > 0 ? rsk::keep_bytes16(v, lim) : make_uint4(0u, 0u, 0u, 0u);
            if (q == 0) {
                v = make_uint4(v.x & ~mh.x, v.y & ~mh.y, v.z & ~mh.z, v.w & ~mh.w);
                part[p] = hsum4(v, part[p]);
                const uint4 h = H[p];
                v = make_uint4(v.x | (h.x & mh.x), v.y | (h.y & mh.y), v.z | (h.z & mh.z), v.w | (h.w & mh.w));
            } else {
                part[p] = hsum4(v, part[p]);
            }
            VI[p][q] = v;
        }
    }
    uint32_t ck[K];
#pragma unroll
    for (int p = 0; p < K; ++p) ck[p] = ~fold16(wave_sum(part[p]) + rdl(H[p].w, (uint32_t)Q)) & 0xffffu;
#pragma unroll
    for (int p = 0; p < K; ++p) {
        const uint32_t P = Pp[p];
        if (!P) continue;  // uniform
        const uint32_t wlen = HB + P;
        uint8_t *dst = a.frame + rdl64(dfo, (uint32_t)p);
        if (lane == (uint32_t)(G::CK / 16)) {
            constexpr uint32_t kw = (G::CK & 15) >> 2, kb = 8 * (G::CK & 3);
            if (kw == 0) VI[p][0].x |= ck[p] << kb; else if (kw == 1) VI[p][0].y |= ck[p] << kb;
            else if (kw == 2) VI[p][0].z |= ck[p] << kb; else VI[p][0].w |= ck[p] << kb;
        }
        const uint32_t r = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);  // uniform
        uint8_t *d0 = dst - r;
        const uint32_t nst = (r + padded_len(dst, wlen, a.pad) + 15u) >> 4;
        const bool pad = a.pad != 0u;
        if (r == 0u) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const uint32_t k = lane + 64u * q;
                if (q == 1 && nst <= 64u) continue;  // uniform
                if (k < nst) store_last16<kStream>(d0 + 16u * k, VI[p][q], (int)wlen - 16 * (int)k, pad);
            }
        } else {
            const uint4 l63 = rdl4(VI[p][0], 63);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (q == 1 && nst <= 64u) continue;  // uniform
                uint4 prev = make_uint4(wave_shr1(VI[p][q].x), wave_shr1(VI[p][q].y), wave_shr1(VI[p][q].z),
                                        wave_shr1(VI[p][q].w));
                if (lane == 0u) prev = q == 0 ? make_uint4(0u, 0u, 0u, 0u) : l63;
                const uint4 d = rsk::funnel16(prev, VI[p][q], 16u - r);
                const uint32_t j = lane + 64u * q;
                if (j >= nst) continue;
                if (j == 0u) rsk::store_range16(d0, d, r, 16u);
                else store_last16<kStream>(d0 + 16u * j, d, (int)(r + wlen) - 16 * (int)j, pad);
            }
        }
    }
}

// The wire build's choice (round 6; tools/path_threshold.py --wire raw4 / eth, profiles/r06_wire_paths.json):
// under AUTO the per-set wire kernels below a mean payload of kWireTwoPassFrom, and for Ethernet packets
// from kWireEthPerSetFrom (4M x 1400 B: per-set 2.285, two-pass 2.296-2.373 ms); the two-pass form
// otherwise, with 4 packets per copy wave, RAW4 from kWireK2From 2 (4M x 1400 B: 2.200 vs 2.230 for 1,
// 2.288 per-set).
constexpr uint32_t kWireTwoPassFrom = 160;
constexpr uint32_t kWireEthPerSetFrom = 1300;
constexpr uint32_t kWireK2From = 1080;
constexpr uint64_t kWireChunk = 1ull << 20;
int wire_path(rsk_ctx *c, uint32_t n, const uint16_t *pay_len, hipStream_t st, bool eth) {
    if (c->enc_path) return c->enc_path == RSK_ENC_PATH_TWO_PASS ? RSK_ENC_PATH_TWO_PASS : RSK_ENC_PATH_PER_SET;
    const int ep = enc_path(c, n, pay_len, st);  // the first-call sample, and the statistic
    if (ep < 0) return ep;
    const uint32_t s = sampled_mean(c);
    if (n < kTwoPassMinPackets || !(s & kStatValid)) return RSK_ENC_PATH_PER_SET;
    const uint32_t mean = s & kStatMean;
    return mean < kWireTwoPassFrom || (eth && mean >= kWireEthPerSetFrom) ? RSK_ENC_PATH_PER_SET
                                                                          : RSK_ENC_PATH_TWO_PASS;
}
// packets per copy wave: forced (rsk__set_copy_k; -1, the framing encode's output-stationary copy, has
// no wire form and counts as 0 here), else by the sampled mean payload
int wire_k(rsk_ctx *c, bool eth) {
    if (c->copy_k > 0) return c->copy_k;
    const uint32_t s = sampled_mean(c);
    const uint32_t mean = (s & kStatValid) ? s & kStatMean : 1400u;
    return eth || mean < kWireK2From ? 4 : 2;
}

}  // namespace

extern "C" {

int rsk_encode_wire_batch(rsk_ctx *c, uint32_t n, const rsk_encode_in *in, const rsk_wire_in *wire,
                          const rsk_encode_out *out, void *stream) {
    if (!c || !in || !wire || !out) return RSK_EINVAL;
    if (n == 0) return RSK_OK;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;  // grids of one lane per packet
    EncArgs a;
    if (!enc_args(n, in, out, a)) return RSK_EINVAL;
    if (!wire->src || !wire->dst || !wire->sp || !wire->dp || !wire->seq || !wire->ack || !wire->flag || !wire->ip_id)
        return RSK_EINVAL;
    DeviceGuard g(c->device);
    if (!g.ok) return RSK_EDEVICE;
    WireArgs w;
    w.src = wire->src; w.dst = wire->dst; w.sp = wire->sp; w.dp = wire->dp; w.seq = wire->seq;
    w.ack = wire->ack; w.flag = wire->flag; w.ip_id = wire->ip_id;
    uint8_t eth[16] = {0};
    std::memcpy(eth, wire->eth, 14);
    std::memcpy(w.eth, eth, 16);
    const unsigned grid = enc_grid(n);
    const hipStream_t st = (hipStream_t)stream;
    const bool eth14 = wire->with_eth != 0;
    // the encode path the context is held to (rsk_set_encode_path: two-pass, or else the per-set wire
    // kernels), or AUTO's wire table (wire_path): the two-pass form -- k_wire_heads (header images,
    // 80 / 96-B records in the stream's scratch) + k_wire_copy with 1, 2 or 4 packets per copy wave
    // (round 6) -- from a mean payload of 160 B (Ethernet: up to 1300 B), the per-set kernels otherwise
    const int path = wire_path(c, n, in->pay_len, st, eth14);
    if (path < 0) return path;
    if (path == RSK_ENC_PATH_TWO_PASS) {
        void *hp = nullptr;
        const uint64_t recb = 16ull * (eth14 ? WireRec<14>::NC : WireRec<0>::NC);  // 96 / 80 B per packet
        // header pass then copy per chunk of kWireChunk packets: one chunk's records (80 / 96 MB at 1M)
        // stay in the Infinity Cache until its copy reads them (a whole C3 batch's, 320 MB, do not)
        const uint64_t chunk = n < kWireChunk ? (uint64_t)n : kWireChunk;
        if (rsk::stream_ws_if(c, st, rsk::WS_ENC, recb * chunk, &hp) == RSK_OK) {
            const int ck = wire_k(c, eth14);
            const dim3 bd(kBlock);
            uint4 *rec = static_cast<uint4 *>(hp);
            for (uint64_t c0 = 0; c0 < n; c0 += chunk) {
                EncArgs ac = a;
                ac.n = (uint32_t)std::min<uint64_t>(n, c0 + chunk);
                const uint64_t m = ac.n - c0;
                uint32_t *stat = c0 == 0 ? c->enc_stat_dev : nullptr;
                if (eth14) hipLaunchKernelGGL(k_wire_heads<14>, dim3(grid_for(m)), bd, 0, st, ac, w, c->ks, rec, stat, c0, chunk);
                else hipLaunchKernelGGL(k_wire_heads<0>, dim3(grid_for(m)), bd, 0, st, ac, w, c->ks, rec, stat, c0, chunk);
                const dim3 cg((unsigned)((m + 4ull * ck - 1ull) / (4ull * ck)));  // m <= kWireChunk: one launch
#define RSK_WCOPY(E, K) hipLaunchKernelGGL((k_wire_copy<E, K>), cg, bd, 0, st, ac, rec, c0, c0, chunk)
                if (eth14) {
                    if (ck == 2) RSK_WCOPY(14, 2); else if (ck == 4) RSK_WCOPY(14, 4); else RSK_WCOPY(14, 1);
                } else {
                    if (ck == 2) RSK_WCOPY(0, 2); else if (ck == 4) RSK_WCOPY(0, 4); else RSK_WCOPY(0, 1);
                }
#undef RSK_WCOPY
            }
            c->enc_last_path.store(RSK_ENC_PATH_TWO_PASS, std::memory_order_relaxed);
            c->enc_last_k.store(ck, std::memory_order_relaxed);
            return launch_check("k_wire_heads / k_wire_copy");
        }
        g_last_error[0] = 0;  // no records (a capture that would grow them, or no memory): one pass
    }
#define RSK_WIRE(E, M, PU, U) hipLaunchKernelGGL((k_encode_wire<E, M, PU, U>), dim3(grid), dim3(kBlock), 0, st, a, w, c->ks)
#define RSK_WIRE4(E, M, PU, U) hipLaunchKernelGGL((k_encode_wire_w4<E, M, PU, U>), dim3(grid), dim3(kBlock), 0, st, a, w, c->ks)
    // the per-set kernels: per-packet half (DPP copy, 8 packets per iteration, tag + payload prefix in
    // the copy loop for long-frame sets, 4 waves/SIMD) then the flat half
    if (eth14) { RSK_WIRE4(14, 5, 8, 2); RSK_WIRE(14, 4, 2, 2); }
    else { RSK_WIRE4(0, 5, 8, 2); RSK_WIRE(0, 4, 2, 2); }
#undef RSK_WIRE
#undef RSK_WIRE4
    c->enc_last_path.store(RSK_ENC_PATH_PER_SET, std::memory_order_relaxed);
    sample_next(c, n, in->pay_len, st, nullptr, 0u);  // as rsk_encode_batch
    return launch_check("k_encode_wire");
}

}  // extern "C"
