// force_map -- jxg_check_strategy_map (csrc/jxg_force.cpp, host only) run as
// itself over a file of cases, for tests/test_force_map.py: built by g++ from
// this file and jxg_force.cpp alone, under ASan + UBSan where the compiler has
// them.  Every map is copied into a heap block of exactly its size, so a read
// past either end is the sanitizer's to report.
//
// case file: u32 n, then per case u32 xsize, ysize, bytes and the map's bytes
// (bytes == 0xFFFFFFFF: a null map).  Output: "status bad_block" per case.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/jxg.h"

static bool rd32(FILE* f, uint32_t* v) { return std::fread(v, 4, 1, f) == 1; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n = 0;
  if (!rd32(f, &n)) return 2;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t w, h, bytes;
    if (!rd32(f, &w) || !rd32(f, &h) || !rd32(f, &bytes)) return 2;
    uint32_t bad = 0xDEADBEEFu;
    jxg_status st;
    if (bytes == 0xFFFFFFFFu) {
      st = jxg_check_strategy_map(nullptr, w, h, &bad);
    } else {
      uint8_t* map = new uint8_t[bytes ? bytes : 1];
      if (bytes && std::fread(map, 1, bytes, f) != bytes) return 2;
      st = jxg_check_strategy_map(map, w, h, &bad);
      // (a null bad_block is allowed: same verdict)
      if (jxg_check_strategy_map(map, w, h, nullptr) != st) return 3;
      delete[] map;
    }
    std::printf("%d %u\n", (int)st, bad);
  }
  std::fclose(f);
  return 0;
}
