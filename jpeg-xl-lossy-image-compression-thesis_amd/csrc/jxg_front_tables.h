// jxg_front_tables.h -- front_kernel's constant tables, built on the host
// (jxg_front_tables.cpp; host only, no HIP include) and uploaded to the
// __constant__ tables of each of the kernel's translation units
// (jxg_front_kernel.h upload_front_tables).
#pragma once
#include <stdint.h>

namespace jxg {

// table index T: DCT8, DCT4X4, DCT4X8, DCT8X4, DCT2X2, IDENTITY
constexpr int kNT = 6;

// per-lane quantization tables: lane r of a block's 8-lane group holds the
// working-array column r, its value k the slot co_index_rt(T, k, r)
struct FrontTables {
  float lut[256];              // sRGB8 -> linear
  float wperm[kNT * 3 * 64];   // [T][c][lane r][row k] = w[qkind(T)][c][co_index(T,k,r)]
  float iwperm[kNT * 64];      // [T][r][k] = 1.0f / (Y weight) at the same slot
  float sdperm[kNT * 3 * 64];  // [T][c][r][k] distortion weight at the same slot
  float btab[256];             // [q] = AdjustQuantBias of a magnitude q < 256 (0, 1 - 0.0700..., q - 0.145 / q)
  uint8_t zz[kNT * 64];        // [T][r][k] = zigzag index of co_index(T,k,r)
};

// wts: quant_weights (jxg_tables.h), kinds 0 DCT8, 1 DCT4X4, 2 DCT4X8 / DCT8X4,
// 3 IDENTITY, 4 DCT2X2
FrontTables build_front_tables(const float lut[256], const float wts[5][3][64]);

}  // namespace jxg
