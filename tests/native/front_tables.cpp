// front_tables -- build_front_tables (csrc/jxg_front_tables.cpp, host only) run
// as itself, for tests/test_front_tables.py: built by g++ from this file and
// jxg_front_tables.cpp alone, under ASan + UBSan where the compiler has them.
//
// Inputs: the sRGB8 -> linear table by its formula, and synthetic weights
// w[kind][c][pos] = (64 (3 kind + c + 1) + pos) * 0.625 -- exact in binary32,
// all distinct, so a table entry names the (kind, channel, position) it was
// taken from, while 1 / w and the distortion weight round.
// Output: one line "NAME HEX" per table blob, in FrontTables' order.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../jpeg-xl-lossy-image-compression-thesis_amd/csrc/jxg_front_tables.h"

static void hex_line(const char* name, const void* p, size_t n) {
  std::printf("%s ", name);
  for (size_t i = 0; i < n; i++) std::printf("%02x", static_cast<const unsigned char*>(p)[i]);
  std::printf("\n");
}

int main() {
  static float lut[256], wts[5][3][64];
  for (int u = 0; u < 256; u++) {
    const double v = u / 255.0;
    lut[u] = (float)(v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4));
  }
  for (int k = 0; k < 5; k++)
    for (int c = 0; c < 3; c++)
      for (int i = 0; i < 64; i++) wts[k][c][i] = (float)(64 * (3 * k + c + 1) + i) * 0.625f;
  const jxg::FrontTables t = jxg::build_front_tables(lut, wts);
  if (std::memcmp(t.lut, lut, sizeof(lut)) != 0) return 3;
  hex_line("wperm", t.wperm, sizeof(t.wperm));
  hex_line("iwperm", t.iwperm, sizeof(t.iwperm));
  hex_line("sdperm", t.sdperm, sizeof(t.sdperm));
  hex_line("btab", t.btab, sizeof(t.btab));
  hex_line("zz", t.zz, sizeof(t.zz));
  return 0;
}
