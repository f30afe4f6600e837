// jxg_front_tables.cpp -- front_kernel's constant tables (jxg_front_tables.h)
#include "jxg_front_tables.h"

#include <cstring>

#include "jxg_coeff.h"

namespace jxg {

FrontTables build_front_tables(const float lut[256], const float wts[5][3][64]) {
  FrontTables t;
  std::memcpy(t.lut, lut, sizeof(t.lut));
  const int types[kNT] = {kDCT8, kDCT4X4, kDCT4X8, kDCT8X4, kDCT2X2, kIDENTITY};
  // quant kinds (quant_weights): DCT8 0, DCT4 1, DCT4X8 2, IDENTITY 3, DCT2X2 4
  const int qks[kNT] = {0, 1, 2, 2, 4, 3};
  for (int ti = 0; ti < kNT; ti++) {
    const int T = types[ti];
    const int qk = qks[ti];
    for (int r = 0; r < 8; r++)
      for (int k = 0; k < 8; k++) {
        const int co = co_index_rt(T, k, r);
        // area a coefficient's basis spans: the lowest-frequency combine slots
        // the whole block, other DCT4X4 coefficients a 4x4 sub-block, other
        // DCT4X8 / DCT8X4 ones a 4x8 half, DCT2X2 level-2 / level-1 ones a 4x4
        // quarter / 2x2 cell, IDENTITY residuals one pixel (oracle
        // jxo_frame_init)
        const int row = co >> 3, col = co & 7;
        int area = 64;
        if (ti == 1 && !(row < 2 && col < 2)) area = 16;
        if ((ti == 2 || ti == 3) && !(row < 2 && col == 0)) area = 32;
        if (ti == 4 && !(row < 2 && col < 2)) area = row < 4 && col < 4 ? 16 : 4;
        if (ti == 5 && !(row < 2 && col < 2)) area = 1;
        for (int c = 0; c < 3; c++) {
          t.wperm[((ti * 3 + c) * 8 + r) * 8 + k] = wts[qk][c][co];
          t.sdperm[((ti * 3 + c) * 8 + r) * 8 + k] = dist_weight(c, area, wts[qk][c][co]);
        }
        t.iwperm[(ti * 8 + r) * 8 + k] = 1.0f / wts[qk][1][co];
        t.zz[(ti * 8 + r) * 8 + k] = (uint8_t)c_inv_order_h(co);
      }
  }
  // AdjustQuantBias of a magnitude q: 0 -> 0, 1 -> kBias1, else q - 0.145 / q
  // (the single-precision division and subtraction the kernel does for a
  // magnitude >= 256; SSE rounds them as the GPU does, no contraction is
  // involved)
  t.btab[0] = 0.0f;
  t.btab[1] = 1.0f - 0.07005449891748593f;
  for (int q = 2; q < 256; q++) t.btab[q] = (float)q - 0.145f / (float)q;
  return t;
}

}  // namespace jxg
