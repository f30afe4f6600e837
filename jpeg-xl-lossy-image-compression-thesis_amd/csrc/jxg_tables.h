// jxg_tables.h -- host-side constant tables of the encoder (built once per
// process, uploaded to __constant__ / device memory by jxg_ctx.cpp init_constants and the stages):
// default quantization weights, the sRGB8 -> linear table, the masking AQ's
// erosion weights, and the merge stage's per-shape weight / distortion /
// natural-order tables and DCT constants.  [ext libjxl quant_weights.cc,
// coeff_order.cc; == oracle/front.c, oracle/merge.c, oracle/aq.c]
#pragma once
#include <cstdint>
#include <vector>

#include "jxg_dequant.h"

namespace jxg {

struct MergeTables {
  std::vector<float> wk, sdk, iwy;
  std::vector<uint16_t> nat;
  float lee_c[7][32], lee_s[7][64], llf_p[4][8], llf_ib[4][8][8];
};

// kinds: 0 DCT8, 1 DCT4X4, 2 DCT4X8 / DCT8X4, 3 IDENTITY, 4 DCT2X2
void quant_weights(float out[5][3][64]);
void aq_erosion_weights(float distance, float w[4]);
void srgb_lut(float lut[256]);
MergeTables build_merge_tables();
// the 128 / 256 px levels' tables (kBigTab* layout, jxg_kernels.h) and their
// natural orders (== oracle/merge.c kinds 6-9)
struct BigTables {
  std::vector<float> tab;
  std::vector<uint16_t> nat;
};
BigTables build_big_tables();

// decode-side reconstruction (jxg_recon.hip): the kRcTab* float blob and the
// kRcPos* position blob of jxg_kernels.h; the EPF sigma table is the only part
// that depends on the frame (its global scale)
struct ReconTables {
  std::vector<float> tab;
  std::vector<uint16_t> pos;
};
ReconTables build_recon_tables(uint32_t global_scale);
// the blob's kRcTabSigma part [256] alone (the rest does not depend on the scale)
void recon_sigma_table(uint32_t global_scale, float* out);

// (DequantMatrices, the big kinds' binary16 parameters: jxg_dequant.h)

}  // namespace jxg
