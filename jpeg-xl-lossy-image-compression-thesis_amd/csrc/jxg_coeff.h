// jxg_coeff.h -- the 8x8 class's strategy ids and coefficient layouts, shared
// by the kernels and the host-only table builders (jxg_front_tables.cpp): the
// natural (zigzag) order, the working-array slot -> raster position map of
// every 8x8-class transform, and the estimates' distortion weight.  Plain
// inline functions; the header includes nothing from HIP (JXG_HD is empty for
// a host compiler, as in jxg_decode_core.h).
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JXG_HD __host__ __device__
#else
#define JXG_HD
#endif

namespace jxg {

// raw AcStrategy ids returned by the thesis selector
// (proposals/combined.diff:227-233)
enum : int { kDCT8 = 0, kDCT4X4 = 3, kDCT4X8 = 12, kDCT8X4 = 13 };
// the two Haar-type 8x8 candidates of the strategy search [ext AcStrategy]
enum : int { kIDENTITY = 1, kDCT2X2 = 2 };

// natural coefficient order of an 8x8 varblock [ext coeff_order.cc]:
// zigzag index -> raster position, computable at compile time
struct Order64 {
  uint8_t v[64];
};
JXG_HD constexpr Order64 make_order64() {
  Order64 o{};
  int cur = 1;
  o.v[0] = 0;
  for (int i = 0; i < 8; i++)
    for (int j = 0; j <= i; j++) {
      int x = j, y = i - j;
      if (i & 1) {
        int t = x;
        x = y;
        y = t;
      }
      if (x == 0 && y == 0) continue;
      o.v[cur++] = (uint8_t)(y * 8 + x);
    }
  for (int ip = 7; ip > 0; ip--) {
    int i = ip - 1;
    for (int j = 0; j <= i; j++) {
      int x = 7 - (i - j), y = 7 - j;
      if (i & 1) {
        int t = x;
        x = y;
        y = t;
      }
      o.v[cur++] = (uint8_t)(y * 8 + x);
    }
  }
  return o;
}
JXG_HD constexpr int c_order_h(int j) { return make_order64().v[j]; }
JXG_HD constexpr int c_inv_order_h(int k) {
  const Order64 o = make_order64();
  for (int j = 0; j < 64; j++)
    if (o.v[j] == k) return j;
  return 0;
}
// transform working-array element (prow, pcol) -> raster position in the
// 8x8 coefficient layout of strategy T (oracle/front.c co_index); only
// (0, 0) maps to the DC slot
JXG_HD inline __attribute__((always_inline)) int co_index_rt(int T, int prow, int pcol) {
  if (T == kDCT8) return prow * 8 + pcol;
  // IDENTITY / DCT2X2: lane pcol's value prow (front kernel haar_lane)
  if (T == kIDENTITY) return ((pcol >> 2) + 2 * (pcol & 3)) * 8 + (prow >> 2) + 2 * (prow & 3);
  if (T == kDCT2X2) {
    const int q = pcol >> 1;
    const int row = (pcol & 1) ? 4 + q : (prow >= 4 ? q : ((q & 1) ? 2 + (q >> 1) : (q >> 1)));
    return row * 8 + prow;
  }
  if (T == kDCT4X4) return ((prow >> 2) + 2 * (prow & 3)) * 8 + (pcol >> 2) + 2 * (pcol & 3);
  if (T == kDCT8X4) return ((prow >> 2) + 2 * (prow & 3)) * 8 + pcol;
  return ((pcol >> 2) + 2 * (pcol & 3)) * 8 + prow;  // kDCT4X8
}

// distortion weight of a coefficient in the strategy search's estimates
// (== oracle/front.c jxo_dist_weight): sqrt(area / 64) * w0[c] / w, in
// double, rounded once; w0 = the DCT8 band-0 weights of X, Y, B (host tables
// only)
inline float dist_weight(int c, int area, float w) {
  static const float kW0[3] = {3150.0f, 560.0f, 512.0f};
  return (float)(std::sqrt((double)area / 64.0) * ((double)kW0[c] / (double)w));
}

}  // namespace jxg
