// jxg_acrec.h -- the AC coding stage's interface: the 32-bit token record and
// a pass group's record space.
//
// The stage codes one 256x256-pixel pass group's AC coefficients.  Stream
// order: varblocks by first block raster, channels Y, X, B, slices; token
// order / contexts are those of oracle/encode.c group_tokens, [ext] libjxl
// dec_group DecodeACVarBlock.
//   ac_hist (jxg_ac_hist.hip) walks the coefficients once and writes every
//           token as a record at its stream position, beside the clustered
//           histograms, the exact token counts (ntok[g][3]) and a bit bound.
//   ac_emit (jxg_ac_emit.hip) writes prefix codes from the records alone.
//   ans_*   (jxg_ans.hip) is the rANS coder over the same records.
//   rate_kernel (jxg_rate.hip) prices the records with the code the frame wrote.
// The writer's task rules (who writes which record) are jxg_actask.h; the
// readers need only this header.  Plain constants and inline functions; the
// header includes nothing from HIP (JXG_HD, jxg_acmodel.h).
#pragma once
#include <stdint.h>

#include "jxg_acmodel.h"

namespace jxg {

// AC tokens are < 64: |q| <= 32767 -> packed value <= 65534 -> hybrid token
// <= 63; the non-zero count (<= 4032) token is <= 47.  Device tables use 64 columns.
constexpr int kAcTok = 64;

// The record: static cluster | token << 8 | raw-bit count << 14 | raw bits << 18
// (8 + 6 + 4 + 14 bits; a token carries at most 13 raw bits).
constexpr int kRecCluBits = 8, kRecTokBits = 6, kRecNbBits = 4, kRecRawBits = 14;
constexpr int kRecTokPos = kRecCluBits, kRecNbPos = kRecTokPos + kRecTokBits,
              kRecRawPos = kRecNbPos + kRecNbBits;
static_assert(kRecTokPos == 8 && kRecNbPos == 14 && kRecRawPos == 18 && kRecRawPos + kRecRawBits == 32,
              "the four fields tile the record's 32 bits");
static_assert(kAcTok == 1 << kRecTokBits, "a token fills its field");
static_assert(kMaxClusters <= 1 << kRecCluBits, "a cluster id fits its field");

JXG_HD inline __attribute__((always_inline)) uint32_t ac_record(uint32_t cluster, uint32_t tok,
                                                                uint32_t nbits, uint32_t bits) {
  return cluster | (tok << kRecTokPos) | (nbits << kRecNbPos) | (bits << kRecRawPos);
}
JXG_HD inline __attribute__((always_inline)) uint32_t rec_cluster(uint32_t r) {
  return r & ((1u << kRecCluBits) - 1);
}
JXG_HD inline __attribute__((always_inline)) uint32_t rec_token(uint32_t r) {
  return (r >> kRecTokPos) & ((1u << kRecTokBits) - 1);
}
JXG_HD inline __attribute__((always_inline)) uint32_t rec_nbits(uint32_t r) {
  return (r >> kRecNbPos) & ((1u << kRecNbBits) - 1);
}
JXG_HD inline __attribute__((always_inline)) uint32_t rec_bits(uint32_t r) { return r >> kRecRawPos; }

// records per pass group: 1024 blocks x 3 channels x <= 64 tokens per slice;
// per band (8 of the group's 32 block rows): a quarter of that.  Slot i of a
// launch (group glist[i] or g0 + i) has its record space at i * kGroupTokStride.
constexpr uint64_t kGroupTokStride = 1024ull * 3 * 64;
constexpr uint64_t kBandTokStride = 256ull * 3 * 64;
constexpr uint32_t kAnsMaxChunks = (uint32_t)(kGroupTokStride / 64);  // 64-record chunks (ans_sums)

// ac_hist runs one 256-thread workgroup per BAND of a pass group: 8 block
// rows (one row of 64x64 tiles) x 32 block columns.  Varblocks up to 64x64
// lie inside one 64x64 tile, so a band holds whole
// varblocks, and the group's token stream (varblocks by first block raster)
// is the concatenation of its four bands' streams: band j writes its records
// at [j * kBandTokStride, ...) of the group's record space and its token
// count to bandtok[g][j]; the coders read the group's stream through
// rec_index (a 4-entry prefix).  Four workgroups per group give small frames
// (1080p: 40 groups) 160 workgroups instead of 40.  At effort >= 8 varblocks
// of 128 / 256 px span bands: the kernel then runs with BR = 32 (one
// 1024-thread workgroup = one band = the whole group; bands 1-3 empty).
constexpr int kBands = 4;  // bandtok entries per group (the coders' view)
static_assert(kBands * kBandTokStride == kGroupTokStride, "band record spaces tile the group's");

// pass group of launch slot i: a shard's group list, or the range g0 + i
JXG_HD inline __attribute__((always_inline)) uint32_t slot_group(const uint32_t* glist, uint32_t g0,
                                                                 uint32_t i) {
  return glist ? glist[i] : g0 + i;
}
// tokens of group g (ntok: [ngroups][3], channels X, Y, B)
template <class G>
JXG_HD inline __attribute__((always_inline)) uint32_t group_tokens(const uint32_t* ntok, G g) {
  return ntok[g * 3] + ntok[g * 3 + 1] + ntok[g * 3 + 2];
}

// record space index of stream position k of a group whose band counts are bt[4]
// (band j holds stream positions [c_j, c_j+1), c_j = bt[0] + ... + bt[j-1];
// the bounds are cumulative, so k >= c_j holds for a prefix of the bands)
JXG_HD inline __attribute__((always_inline)) uint32_t rec_index(const uint32_t* bt, uint32_t k) {
  uint32_t j = 0, lo = 0, cum = 0;
#pragma unroll
  for (int i = 0; i < kBands - 1; i++) {
    cum += bt[i];
    const bool past = k >= cum;
    lo = past ? cum : lo;
    j += past ? 1u : 0u;
  }
  return j * (uint32_t)kBandTokStride + (k - lo);
}

}  // namespace jxg
