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

namespace jxg {
jxg_status check_strategy_map(const uint8_t* acs, uint32_t xsize, uint32_t ysize,
                              uint32_t* bad_block, uint32_t* big_kinds);
}

namespace {

// blocks down / across of an accepted raw id; 0: not accepted
struct Extent {
  uint8_t cy, cx;
};
// the shapes of up to 64 px (what fits one 64x64 tile) and the six kinds of
// 128 / 256 px (ids 21 - 26: 16 or 32 blocks a side); AFV (8, 9), 32X8 / 8X32
// (14 - 17) and ids >= 27 have no shape here
Extent extent_of(uint8_t id) {
  const uint32_t s = jxg::strategy_shape(id);
  return Extent{(uint8_t)(s & 0xFF), (uint8_t)(s >> 8)};
}
// kind of a big id in big_list_kernel's numbering: 0 128X64 (22, 23),
// 1 128X128 (21), 2 256X128 (25, 26), 3 256X256 (24)
uint32_t big_kind_of(uint8_t id) { return id == 21 ? 1u : (id == 24 ? 3u : (id <= 23 ? 0u : 2u)); }

constexpr uint8_t kConflict = 0xFF;  // claimed by two varblocks (0x80 | 0x7F is no accepted id)

}  // namespace

// One raster pass.  `claim` holds, per block a merged varblock covers beyond
// its first, the byte the map must show there (0: unclaimed).  A varblock's
// first block precedes every block it covers in raster order, so a block's
// byte is judged when the pass reaches it, against what the first blocks
// before it claimed: the block reported is the first offending one in raster
// order.  Two varblocks claiming one block make that block the offender.
//
// Placement.  A shape of up to 64 px lies anywhere inside one 64x64 tile.  A
// kind of 128 / 256 px is accepted on its own grid alone -- block row a
// multiple of its blocks down, block column a multiple of its blocks across:
// the placements the search produces, none of which crosses a 256x256 pass
// group.  The decoder reads some other placements of these kinds (any that
// stays inside a pass group on the 64 px grid), but this encoder has no
// transform path for them: off its grid a big id is JXG_ERR_UNSUPPORTED, like
// an id without a shape.  The checks on a first block, in order: claimed ->
// id / placement supported -> fits the frame (and, up to 64 px, the tile).
//
// big_kinds (may be null): bit k set when the accepted map holds a varblock of
// big kind k (big_kind_of), so the encode knows on the host whether the 128 /
// 256 px write pass has anything to do.
jxg_status jxg::check_strategy_map(const uint8_t* acs, uint32_t xsize, uint32_t ysize,
                                   uint32_t* bad_block, uint32_t* big_kinds) {
  if (bad_block) *bad_block = 0;
  if (big_kinds) *big_kinds = 0;
  uint32_t kinds = 0;
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
      const bool big = e.cy > 8 || e.cx > 8;
      if (big && (by % e.cy || bx % e.cx)) return refuse(b, JXG_ERR_UNSUPPORTED);
      if (by + e.cy > bys || bx + e.cx > bxs ||
          (!big && ((by & 7u) + e.cy > 8 || (bx & 7u) + e.cx > 8)))
        return refuse(b, JXG_ERR_INVALID_ARG);
      if (big) kinds |= 1u << big_kind_of(v);
      for (uint32_t iy = 0; iy < e.cy; iy++)
        for (uint32_t ix = iy ? 0u : 1u; ix < e.cx; ix++) {
          uint8_t& c = claim[b + (size_t)iy * bxs + ix];
          c = c ? kConflict : (uint8_t)(0x80 | v);
        }
    }
  if (big_kinds) *big_kinds = kinds;
  return JXG_OK;
}

extern "C" jxg_status jxg_check_strategy_map(const uint8_t* acs, uint32_t xsize, uint32_t ysize,
                                             uint32_t* bad_block) {
  return jxg::check_strategy_map(acs, xsize, ysize, bad_block, nullptr);
}
