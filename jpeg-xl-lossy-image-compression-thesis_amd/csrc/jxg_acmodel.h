// jxg_acmodel.h -- the AC context model: its sizes and static clustering, the
// format's context functions (strategy shape and order, block context map,
// zero-density and non-zero buckets), and the layout of the ANS table blob the
// rANS kernels read.  Plain constants and inline functions shared by the
// encoder's kernels (jxg_device.h, jxg_kernels.h), the decoder
// (jxg_decode_core.h) and host-only units (jxg_codes.cpp, jxg_force.cpp): the
// header includes nothing from HIP (JXG_HD is empty for a host compiler).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JXG_HD __host__ __device__
#else
#define JXG_HD
#endif

namespace jxg {

constexpr int kBlockCtx = 15, kNzBuckets = 37, kZdCtx = 458;
constexpr int kAcCtx = kBlockCtx * (kNzBuckets + kZdCtx);  // 7425
constexpr int kMaxClusters = 132;
constexpr int kAlpha = 128;

JXG_HD inline __attribute__((always_inline)) int bclass(int bctx) {
  if (bctx < 7) return bctx == 0 ? 0 : (bctx == 1 ? 1 : 2);
  return bctx == 7 ? 3 : (bctx == 8 ? 4 : 5);
}
// static clustering of the 7425 AC contexts (the map is transmitted)
JXG_HD inline __attribute__((always_inline)) int ac_cluster(int ctx) {
  if (ctx < kBlockCtx * kNzBuckets) {
    int bucket = ctx / kBlockCtx, bctx = ctx % kBlockCtx;
    int nb = bucket == 0 ? 0 : (bucket <= 2 ? 1 : (bucket <= 8 ? 2 : 3));
    return bclass(bctx) * 4 + nb;
  }
  int z = ctx - kBlockCtx * kNzBuckets;
  int bctx = z / kZdCtx, zz = z % kZdCtx;
  int prev = zz & 1, base = zz >> 1;
  int bi = base >= 206 ? 7 : base >= 180 ? 6 : base >= 152 ? 5 : base >= 123 ? 4
         : base >= 93 ? 3 : base >= 62 ? 2 : base >= 31 ? 1 : 0;
  const int nzb_base = bi == 7 ? 206 : bi == 6 ? 180 : bi == 5 ? 152 : bi == 4 ? 123
                     : bi == 3 ? 93 : bi == 2 ? 62 : bi == 1 ? 31 : 0;
  int fc = base - nzb_base;
  int nzg = bi < 2 ? 0 : (bi < 4 ? 1 : 2);
  int fg = fc < 4 ? 0 : (fc < 12 ? 1 : 2);
  return 24 + ((bclass(bctx) * 3 + nzg) * 3 + fg) * 2 + prev;
}

// ---- the format's AC context model ([ext] libjxl ac_context.h), once for the
// encoder's kernels, the decoder (jxg_decode_core.h) and the host ----
// raw strategy id -> covered blocks (down | across << 8); 0: not a strategy
// this encoder writes
JXG_HD constexpr uint32_t strategy_shape(uint32_t t) {
  const uint16_t k[27] = {0x0101, 0x0101, 0x0101, 0x0101, 0x0202, 0x0404, 0x0102, 0x0201, 0,
                          0,      0x0204, 0x0402, 0x0101, 0x0101, 0,      0,      0,      0,
                          0x0808, 0x0408, 0x0804, 0x1010, 0x0810, 0x1008, 0x2020, 0x1020, 0x2010};
  return t < 27 ? k[t] : 0u;
}
// raw strategy id -> coefficient-order bucket
JXG_HD constexpr uint32_t strategy_order(uint32_t t) {
  const uint8_t k[27] = {0, 1, 1, 1, 2, 3, 4, 4, 5, 5, 6, 6, 1, 1,
                         1, 1, 1, 1, 7, 8, 8, 9, 10, 10, 11, 12, 12};
  return k[t];
}
// default block context map [channel (Y, X, B)][order]
JXG_HD constexpr uint32_t block_ctx(uint32_t i) {
  const uint8_t k[39] = {0, 1, 2, 2, 3,  3,  4,  5,  6,  6,  6,  6,  6,
                         7, 8, 9, 9, 10, 11, 12, 13, 14, 14, 14, 14, 14,
                         7, 8, 9, 9, 10, 11, 12, 13, 14, 14, 14, 14, 14};
  return k[i];
}
// the zero-density context tables of the format, as arithmetic (both sit on
// the token chain of the decoder's walk: a table load there is a memory
// latency per token)
JXG_HD constexpr uint32_t freq_ctx(uint32_t i) {  // i < 64: 0 0 1 .. 14, pairs 15 .. 22, fours 23 .. 30
  return i < 2 ? 0u : (i < 16 ? i - 1 : (i < 32 ? 15 + ((i - 16) >> 1) : 23 + ((i - 32) >> 2)));
}
JXG_HD constexpr uint32_t nnz_ctx(uint32_t i) {
  return i < 2 ? 0u
               : (i < 3 ? 31u
                        : (i < 5 ? 62u
                                 : (i < 9 ? 93u
                                          : (i < 13 ? 123u : (i < 21 ? 152u : (i < 33 ? 180u : 206u))))));
}
// context bucket of a predicted non-zero count
JXG_HD constexpr int nz_bucket(int n) {
  if (n >= 64) n = 64;
  return n < 8 ? n : 4 + n / 2;
}

// covered blocks of a raw strategy id as the encoder's kernels want them: log2
// and blocks across / down; an id without a shape counts as the 8x8 class
JXG_HD constexpr __attribute__((always_inline)) void varblock_dims(int type, int& lcb, int& cx,
                                                                  int& cy) {
  switch (type) {
    case 6: lcb = 1, cx = 1, cy = 2; break;   // 16x8
    case 7: lcb = 1, cx = 2, cy = 1; break;   // 8x16
    case 4: lcb = 2, cx = 2, cy = 2; break;   // 16x16
    case 10: lcb = 3, cx = 2, cy = 4; break;  // 32x16
    case 11: lcb = 3, cx = 4, cy = 2; break;  // 16x32
    case 5: lcb = 4, cx = 4, cy = 4; break;   // 32x32
    case 19: lcb = 5, cx = 4, cy = 8; break;  // 64x32
    case 20: lcb = 5, cx = 8, cy = 4; break;  // 32x64
    case 18: lcb = 6, cx = 8, cy = 8; break;  // 64x64
    case 22: lcb = 7, cx = 8, cy = 16; break;   // 128x64 (effort >= 8)
    case 23: lcb = 7, cx = 16, cy = 8; break;   // 64x128
    case 21: lcb = 8, cx = 16, cy = 16; break;  // 128x128
    case 25: lcb = 9, cx = 16, cy = 32; break;  // 256x128
    case 26: lcb = 9, cx = 32, cy = 16; break;  // 128x256
    case 24: lcb = 10, cx = 32, cy = 32; break; // 256x256
    default: lcb = 0, cx = 1, cy = 1; break;  // 8x8 class
  }
}
constexpr bool varblock_dims_match_shapes() {
  for (int t = 0; t < 27; t++) {
    int lcb = 0, cx = 0, cy = 0;
    varblock_dims(t, lcb, cx, cy);
    const uint32_t s = strategy_shape((uint32_t)t) ? strategy_shape((uint32_t)t) : 0x0101u;
    if ((uint32_t)cy != (s & 0xFF) || (uint32_t)cx != s >> 8 || 1 << lcb != cx * cy) return false;
  }
  return true;
}
static_assert(varblock_dims_match_shapes(), "varblock_dims restates strategy_shape");

// ANS table blob (AnsArgs::tab, jxg_ans.hip):
//   u32 [kAnsHists][128] symbol: f - 1 | cum << 12
//   u16 [kAnsHists][4096] alias inverse: slot of position cum + offset
//   u8 [kMaxClusters] static cluster -> histogram
#ifndef JXG_ANS_HISTS  // (jxg_bitstream.h kAnsMaxHists; experiment builds override it)
#define JXG_ANS_HISTS 8
#endif
constexpr uint32_t kAnsHists = JXG_ANS_HISTS;  // == kAnsMaxHists (jxg_bitstream.h)
constexpr uint32_t kAnsInvOff = kAnsHists * 128 * 4;
constexpr uint32_t kAnsMapOff = kAnsInvOff + kAnsHists * 4096 * 2;
constexpr uint32_t kAnsTabBytes = kAnsMapOff + 136;

}  // namespace jxg
