// jxg_shapes.h -- the nine merged shapes of the 64x64 tile stage (16x8 ..
// 64x64 px; == oracle jxo_shapes) and everything sized by them: the one table
// the merge kernels, the search trace and the host's quant-table builder read.
// No HIP include: host-only units use it as it is.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "jxg_acmodel.h"  // strategy_shape

namespace jxg {

// raw id, blocks down / across (log2), cost multiplier.  16 bytes: the kernels
// index the table with a shift.  The weight kind is no column of its own: the
// kinds are the six varblock areas in rising order (shape_kind).
struct ShapeDesc {
  int type, lcy, lcx;
  float tmul;
};
constexpr int kNumShapes = 9;
constexpr ShapeDesc kShapes[kNumShapes] = {
    {6, 1, 0, 1.0f},   {7, 0, 1, 1.0f},   {4, 1, 1, 1.0f},
    {10, 2, 1, 1.02f}, {11, 1, 2, 1.02f}, {5, 2, 2, 1.03f},
    {19, 3, 2, 1.05f}, {20, 2, 3, 1.05f}, {18, 3, 3, 1.05f}};

// weight kinds (stored orientation, rows <= cols): 8x16, 16x16, 16x32, 32x32,
// 32x64, 64x64; a tall shape reads its kind's table transposed
constexpr int kNumKinds = 6;
constexpr int kKindOff[kNumKinds + 1] = {0, 128, 384, 896, 1920, 3968, 8064};
constexpr int shape_kind(int si) { return kShapes[si].lcy + kShapes[si].lcx - 1; }

// the shapes' pixel-orientation tables (MergeArgs::wk ...): 64 floats per
// covered block, shape si at kShapeOff[si]
constexpr int kShapeOff[kNumShapes + 1] = {0, 128, 256, 512, 1024, 1536, 2560, 4608, 6656, 10752};
// merge_write's varblock lists (MergeArgs::work): a tile holds at most
// 64 / (blocks of the shape) varblocks of a shape, so list si has room for
// ntiles * kShapeSlots[si] entries (every block pair merged: 105 per tile)
constexpr int kMergeWorkHead = 16;  // the nine counts, padded
constexpr int kShapeSlots[kNumShapes] = {32, 32, 16, 8, 8, 4, 2, 2, 1};
constexpr int kShapeSlotOff[kNumShapes + 1] = {0, 32, 64, 80, 88, 96, 100, 102, 104, 105};
constexpr size_t merge_list_off(int si, uint32_t ntiles) {
  return kMergeWorkHead + (size_t)ntiles * kShapeSlotOff[si];
}
constexpr size_t merge_work_words(uint32_t ntiles) { return merge_list_off(kNumShapes, ntiles); }

// the literals above against the table
constexpr bool shape_tables_ok() {
  int off = 0, slot = 0;
  for (int si = 0; si < kNumShapes; si++) {
    const int blocks = 1 << (kShapes[si].lcy + kShapes[si].lcx), k = shape_kind(si);
    if (kShapeOff[si] != off || kShapeSlotOff[si] != slot || kShapeSlots[si] != 64 / blocks) return false;
    if (k < 0 || k >= kNumKinds || kKindOff[k + 1] - kKindOff[k] != 64 * blocks) return false;
    // blocks down | across << 8 of the raw id, as the AC context model has them
    if (strategy_shape((uint32_t)kShapes[si].type) != (1u << kShapes[si].lcy | 256u << kShapes[si].lcx)) return false;
    off += 64 * blocks;
    slot += 64 / blocks;
  }
  return kShapeOff[kNumShapes] == off && kShapeSlotOff[kNumShapes] == slot;
}
static_assert(shape_tables_ok(),
              "kShapeOff / kShapeSlots / kShapeSlotOff / kKindOff restate kShapes, kShapes strategy_shape");

}  // namespace jxg
