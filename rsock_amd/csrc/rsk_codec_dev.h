// rsk_codec_dev.h — what every codec kernel uses (rsk_kernels.hip, rsk_wire.hip): the block shape, readlane, the tag in its two modes and the EncHead words.
// Internal (not installed).  The helpers sit in an anonymous namespace, so every unit that includes this
// header gets its own copies (and its own LDS tag table), as the kernels do.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rsk_codec.h"
#include "rsk_device.h"
#include "rsk_md5.h"

using rsk::KeySched;

namespace {

constexpr int kBlock = 256;  // 4 waves of 64
constexpr int kWavesPerBlock = kBlock / 64;

__device__ __forceinline__ uint32_t rdl(uint32_t v, uint32_t j) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j);
}
__device__ __forceinline__ uint64_t rdl64(uint64_t v, uint32_t j) {
    return (uint64_t)rdl((uint32_t)v, j) | ((uint64_t)rdl((uint32_t)(v >> 32), j) << 32);
}

// ---- the tag (util/rhash.cpp:20-41): MD5(key || payload[0])[8..15].  Two modes, chosen per context
// at run time (rsk_set_tag_mode, uniform per launch through KeySched::tag_mode):
//   RSK_TAG_MD5 (default)  every lane runs the MD5 compression of rsk_md5.h for its packet, as the
//                          reference does per packet (rhash.cpp:20-41): the key's message words are
//                          kernel arguments (SGPRs), only the word holding payload[0] is per lane, the
//                          round constants are instruction immediates;
//   RSK_TAG_TABLE          the tag depends on one payload byte, so a key has 256 tags: k_tag_table
//                          computes them once per context and every kernel that frames or verifies
//                          stages the 2-KB table in LDS (one entry per thread of the 256-thread block,
//                          before any early exit) and looks the tag up with one ds_read_b64.
// Round 3 measured the MD5 round constants staged in LDS per block (the north star's "MD5 round
// constants ... staged in LDS") against instruction immediates and kept immediates
// (profiles/r03_ab_md5_lds.json; that build is in the git history).
__shared__ uint2 s_tags[256];

__device__ __forceinline__ void stage_tags(const KeySched &ks) {
    static_assert(kBlock == 256, "one tag-table entry per thread");
    if (ks.tag_mode == RSK_TAG_TABLE) {  // uniform: the whole block takes the barrier or none does
        s_tags[threadIdx.x] = ks.tab[threadIdx.x];
        __syncthreads();
    }
}

// LANE: the payload-word-specialised schedule (rsk_md5.h md5_tag_lane: 4 VALU per step instead of 5,
// 16 instantiations behind one scalar branch).  Who uses it: the decode kernels (registers to spare,
// ~1 %) and the two-pass header pass.  The framing kernels keep the generic schedule: in k_encode's
// per-packet sets the specialised one raised the register budget past 128 VGPRs (3 waves per SIMD
// instead of 4) and cost C2 / C4 13-16 % (profiles/r04_ab_md5_isa.json); for its flat sets (MODE 12)
// round 4 measured a gain on a build that specialised key word 2 only -- on the full build MODE 11
// (generic) is as fast or 1 % faster (C2 0.0498-0.0501 vs 0.0499-0.0503 ms; 128 / 200-B batches -1 %,
// profiles/r05_md5_mode11_vs_12.json), so the shipped per-set kernel is k_encode<11>.
template <bool LANE = false>
__device__ __forceinline__ void tag_of(const KeySched &ks, uint32_t b, uint32_t &t0, uint32_t &t1) {
    if (ks.tag_mode == RSK_TAG_TABLE) {
        const uint2 t = s_tags[b & 255u];
        t0 = t.x;
        t1 = t.y;
        return;
    }
    if constexpr (LANE) rsk::md5_tag_lane(ks, b & 255u, t0, t1);
    else rsk::md5_tag(ks, b & 255u, t0, t1);
}

// Frame bytes 8..31 as words H[2..7] (bean/EncHead.cpp:9-24 field order; byte 30 reserved = 0,
// byte 31 = payload[0], which belongs to the payload but shares the word).
__device__ __forceinline__ void head_words(uint32_t cmd, uint32_t id0, uint32_t id1, uint32_t conv,
                                           uint64_t key, uint32_t b0, uint32_t (&H)[8]) {
    H[2] = (uint32_t)RSK_ENC_HEAD_SIZE | (cmd << 8) | (id0 << 16);
    H[3] = (id0 >> 16) | (id1 << 16);
    H[4] = (id1 >> 16) | (conv << 16);
    H[5] = (conv >> 16) | ((uint32_t)key << 16);
    H[6] = (uint32_t)(key >> 16);
    H[7] = (uint32_t)(key >> 48) | (b0 << 24);
}

inline unsigned grid_for(uint64_t threads) { return (unsigned)((threads + kBlock - 1) / kBlock); }

}  // namespace
