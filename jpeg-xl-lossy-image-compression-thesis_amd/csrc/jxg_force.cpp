// jxg_force.cpp -- the validator of a caller's AC-strategy map
// (jxg_check_strategy_map).  Host only, no HIP include: the
// CPU tests and a stand-alone sanitizer program compile this file alone.
// The forced encode runs it before anything is uploaded or launched, so no
// kernel ever indexes by a map that did not pass.
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/jxg.h"
#include "jxg_acmodel.h"

namespace {

// blocks down / across of an accepted raw id; 0: not accepted
struct Extent {
  uint8_t cy, cx;
};
// (the shapes of up to 64 px: what fits one 64x64 tile)
Extent extent_of(uint8_t id) {
  const uint32_t s = jxg::strategy_shape(id);
  const uint8_t cy = (uint8_t)(s & 0xFF), cx = (uint8_t)(s >> 8);
  return cy <= 8 && cx <= 8 ? Extent{cy, cx} : Extent{0, 0};
}

constexpr uint8_t kConflict = 0xFF;  // claimed by two varblocks (0x80 | 0x7F is no accepted id)

}  // namespace

// One raster pass.  `claim` holds, per block a merged varblock covers beyond
// its first, the byte the map must show there (0: unclaimed).  A varblock's
// first block precedes every block it covers in raster order, so a block's
// byte is judged when the pass reaches it, against what the first blocks
// before it claimed: the block reported is the first offending one in raster
// order.  Two varblocks claiming one block make that block the offender.
extern "C" jxg_status jxg_check_strategy_map(const uint8_t* acs, uint32_t xsize, uint32_t ysize,
                                             uint32_t* bad_block) {
  if (bad_block) *bad_block = 0;
  if (!acs || xsize == 0 || ysize == 0 || xsize > (1u << 18) || ysize > (1u << 18))
    return JXG_ERR_INVALID_ARG;
  const uint32_t bxs = (xsize + 7) / 8, bys = (ysize + 7) / 8;
  const size_t nb = (size_t)bxs * bys;
  if (nb > 0xFFFFFFFFull) return JXG_ERR_INVALID_ARG;
  std::vector<uint8_t> claim;
  try {
    claim.assign(nb, 0);
  } catch (const std::bad_alloc&) {
    return JXG_ERR_OOM;
  }
  auto refuse = [&](size_t b, jxg_status st) {
    if (bad_block) *bad_block = (uint32_t)b;
    return st;
  };
  for (uint32_t by = 0; by < bys; by++)
    for (uint32_t bx = 0; bx < bxs; bx++) {
      const size_t b = (size_t)by * bxs + bx;
      const uint8_t v = acs[b];
      if (v & 0x80) {  // covered: claimed by exactly one varblock of this id
        if (claim[b] != v || v == kConflict) return refuse(b, JXG_ERR_INVALID_ARG);
        continue;
      }
      if (claim[b]) return refuse(b, JXG_ERR_INVALID_ARG);  // a first block inside a varblock
      const Extent e = extent_of(v);
      if (!e.cy) return refuse(b, JXG_ERR_UNSUPPORTED);
      if (e.cy == 1 && e.cx == 1) continue;
      if (by + e.cy > bys || bx + e.cx > bxs || (by & 7u) + e.cy > 8 || (bx & 7u) + e.cx > 8)
        return refuse(b, JXG_ERR_INVALID_ARG);
      for (uint32_t iy = 0; iy < e.cy; iy++)
        for (uint32_t ix = iy ? 0u : 1u; ix < e.cx; ix++) {
          uint8_t& c = claim[b + (size_t)iy * bxs + ix];
          c = c ? kConflict : (uint8_t)(0x80 | v);
        }
    }
  return JXG_OK;
}
