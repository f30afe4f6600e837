// jxg_dequant.h -- the dequantization parameters of the 128 / 256 px kinds as
// the stream carries them: binary16 rounding, the parameter tables and
// HfGlobal's DequantMatrices.  Host only (no HIP include): the code builder
// (jxg_codes.cpp), the payload assembler and the decoder share it, and
// build_big_tables (jxg_tables.cpp) quantizes with the same big_param.
#pragma once
#include <cstdint>

namespace jxg {

class BitWriter;
// DequantMatrices of HfGlobal [ext quant_weights.cc]: all_default when mask is
// 0, else Library for every table but those of the big kinds in mask (bit 0
// 128X64, 1 128X128, 2 256X128, 3 256X256: the kinds the frame uses, effort
// >= 8), which are written in mode DCT with the binary16 parameters
// build_big_tables quantizes with (== oracle/encode.c put_dequant_matrices),
// so no decoder default is involved for them
void write_dequant_matrices(BitWriter& w, uint32_t mask);
// whether bits[channel][band] (binary16 words of a DCT-mode table as the
// stream carries them) are the parameters write_dequant_matrices writes for
// big kind k -- the ones build_recon_tables reconstructs with (the decoder)
bool dequant_params_match(int k, const uint16_t* bits /* [3][8] */);
// band parameter i of channel c of big kind k, rounded to what the stream
// carries: the first band 64 * f16(band / 64), the others f16(v)
double big_param(int k, int c, int i);
// the binary16 value nearest v (ties to even) and its bits (== oracle/merge.c)
double f16_round(double v);
uint32_t f16_bits(double v);

}  // namespace jxg
