// jxg_acmodel.h -- the AC context model's sizes and static clustering, and the
// layout of the ANS table blob the rANS kernels read.  Plain constants and
// inline functions shared by the kernels (jxg_device.h, jxg_kernels.h) and the
// host-only code builder (jxg_codes.cpp): the header includes nothing from HIP
// (JXG_HD is empty for a host compiler, as in jxg_decode_core.h).
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

// ANS table blob (AnsArgs::tab, jxg_ac.hip):
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
