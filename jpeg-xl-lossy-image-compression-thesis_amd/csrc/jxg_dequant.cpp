// jxg_dequant.cpp -- binary16 dequantization parameters of the big kinds and
// HfGlobal's DequantMatrices (jxg_dequant.h); host only
#include "jxg_dequant.h"

#include <cmath>

#include "jxg_bitstream.h"

namespace jxg {

double f16_round(double v) {
  const double a = std::fabs(v);
  if (a == 0.0) return 0.0;
  int e;
  (void)std::frexp(a, &e);  // a = m * 2^e, m in [0.5, 1)
  int ue = e - 11;          // ulp exponent of an 11-bit significand
  if (ue < -24) ue = -24;   // subnormal spacing
  const double q = std::ldexp(std::nearbyint(std::ldexp(a, -ue)), ue);
  return v < 0 ? -q : q;
}
uint32_t f16_bits(double v) {
  const uint32_t sign = v < 0 ? 0x8000u : 0u;
  const double a = std::fabs(v);
  if (a == 0.0) return sign;
  if (a < std::ldexp(1.0, -14)) return sign | (uint32_t)std::ldexp(a, 24);
  int e;
  const double m = std::frexp(a, &e);
  return sign | (uint32_t)(e - 1 + 15) << 10 | (uint32_t)std::ldexp(2.0 * m - 1.0, 10);
}

// DCT128X64, DCT128X128, DCT256X128, DCT256X256: the bands of DCT64X32 /
// DCT64X64 with the first band scaled up with the size (== oracle/merge.c),
// rounded to the binary16 parameters the stream carries for them
// (write_dequant_matrices): the first band 64 * f16(band / 64), the others
// f16(v)
static const double kBigY32[3] = {23629.073922049845, 8611.3238710010046, 4492.2486445538634};
static const double kBigY64[3] = {26629.073922049845, 9311.3238710010046, 4992.2486445538634};
static const double kBigRest[3][7] = {
    {-1.025, -0.78, -0.65012, -0.19041574084286472, -0.20819395464, -0.421064,
     -0.32733845535848671},
    {-0.3041958212306401, -0.3633036457487539, -0.35660379990111464, -0.3443074455424403,
     -0.33699592683512467, -0.30180866526242109, -0.27321683125358037},
    {-1.2, -1.2, -0.8, -0.7, -0.7, -0.4, -0.5}};
static const double kBigScale[4] = {1.3, 1.7, 2.2, 3.0};
double big_param(int k, int c, int i) {
  if (i) return f16_round(kBigRest[c][i - 1]);
  return 64.0 * f16_round(kBigScale[k] * ((k & 1) ? kBigY64[c] : kBigY32[c]) / 64.0);
}

void write_dequant_matrices(BitWriter& w, uint32_t mask) {
  if (!mask) {
    w.put(1, 1);  // all_default
    return;
  }
  // quant table order DCT, IDENTITY, DCT2X2, DCT4X4, DCT16X16, DCT32X32,
  // DCT16X8, DCT32X8, DCT32X16, DCT64X64, DCT64X32, DCT4X8, AFV0, DCT128X128,
  // DCT128X64, DCT256X256, DCT256X128 -> big kind (0 128X64, 1 128X128,
  // 2 256X128, 3 256X256) or -1 (Library)
  static const int kTableBig[17] = {-1, -1, -1, -1, -1, -1, -1, -1, -1,
                                    -1, -1, -1, -1, 1,  0,  3,  2};
  w.put(1, 0);
  for (int t = 0; t < 17; t++) {
    const int k = kTableBig[t];
    if (k < 0 || !(mask >> k & 1)) {
      w.put(3, 0);  // Library
      continue;
    }
    w.put(3, 6);      // DCT
    w.put(4, 8 - 1);  // bands
    for (int c = 0; c < 3; c++)
      for (int i = 0; i < 8; i++) {
        const double v = big_param(k, c, i);
        w.put(16, f16_bits(i ? v : v / 64.0));
      }
  }
}

bool dequant_params_match(int k, const uint16_t* bits) {
  for (int c = 0; c < 3; c++)
    for (int i = 0; i < 8; i++) {
      const double v = big_param(k, c, i);
      if (bits[c * 8 + i] != f16_bits(i ? v : v / 64.0)) return false;
    }
  return true;
}

}  // namespace jxg
