// jxg_decode_plan.h -- the batch decoder's plan (jxg_decode_batch_rgb8), as
// plain host data: which frames share a device arena (chunks), where each
// frame's buffers lie in it, and the pass-group kernel's work lists.  Host only
// (no HIP include): jxg_decode_batch.cpp launches from these,
// tests/native/decode_batch_plan.cpp prints them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#pragma GCC visibility push(hidden)
namespace jxg {

// ---------------------------------------------------------------------------
// The pass-group kernels' dynamic LDS (jxg_decode.hip): [non-zero map 3 KB |
// pending coefficients | context-map slice of one preset | histogram
// descriptors | the symbol tables when they fit], parts 8-byte aligned.
// decode_groups_lds (one frame) and the planner (per frame of a batch) apply
// the same rule; jxg_decode.hip asserts that the constants are its own.
// ---------------------------------------------------------------------------
constexpr uint32_t kDecPlanNzs = 3 * 1024 + 512 * 4;   // non-zero map + dec::kPendCoefs words
constexpr uint32_t kDecPlanMap = (7425 + 7) & ~7u;     // dec::kAcCtxPerPreset bytes
constexpr uint32_t kDecPlanHistBytes = 12;             // sizeof(dec::HistDesc)
constexpr uint32_t kDecPlanLdsMax = 60 * 1024;
// LDS bytes of a workgroup of a frame with `nhist` histograms and `tab_bytes`
// of symbol tables; *staged: the tables go to LDS too
uint32_t decode_lds_bytes(uint32_t nhist, uint32_t tab_bytes, bool* staged);

constexpr size_t kDecBatchDefaultBytes = (size_t)2 << 30;  // jxg_set_decode_batch_bytes(0)
constexpr size_t kDecArenaAlign = 256;  // every slice; the kernels need 8 (64-bit stream words)

// what the planner needs of one parsed frame
struct DecPlanFrame {
  uint32_t bxs = 0, bys = 0;  // blocks across / down
  uint32_t ntiles = 0;        // 64x64 tiles
  size_t stream_words = 0;    // the padded codestream, 64-bit words
  size_t table_bytes = 0;     // the decode-table blob [hist | atab or ptab | ctxmap]
  uint32_t nhist = 0, tab_bytes = 0;  // as DecodeArgs
  uint32_t ngroups = 0;
  const uint64_t* sec = nullptr;  // [ngroups][2] first / end bit of every pass group
};

// byte offsets of a frame's slices in its chunk's arena
struct DecSlices {
  size_t acs = 0, qf = 0, dc = 0, ac = 0, cmap = 0, stream = 0, sec = 0, tab = 0;
  size_t end = 0;  // the next frame's first byte
};
// the bytes of each slice (unaligned), in the order of DecSlices
struct DecSliceBytes {
  size_t acs, qf, dc, ac, cmap, stream, sec, tab;
};
DecSliceBytes decode_slice_bytes(const DecPlanFrame& f);
// the frame's device footprint: its slices, each rounded up to kDecArenaAlign
size_t decode_footprint(const DecPlanFrame& f);

struct DecWork {
  uint32_t frame;  // index into the call's frames
  uint32_t group;
};

struct DecChunk {
  uint32_t first = 0, end = 0;      // frames [first, end) of the planned list
  size_t bytes = 0;                 // the arena
  std::vector<DecSlices> at;        // [end - first]
  std::vector<uint32_t> status_base;  // [end - first] first status word of each frame
  uint32_t nstatus = 0;             // sum of the frames' pass groups
  // launch classes: work items of frames whose symbol tables are staged in LDS,
  // and of those whose tables stay in memory; each sorted by section length in
  // bits, longest first, ties by (frame, group); LDS of a launch: the largest
  // of its frames'
  std::vector<DecWork> staged, unstaged;
  uint32_t lds_staged = 0, lds_unstaged = 0;
};

// Consecutive runs of frames whose footprints fit `budget` bytes (0: the
// default); a frame larger than the budget is a chunk of its own.
std::vector<DecChunk> plan_decode_batch(const std::vector<DecPlanFrame>& frames, size_t budget);

}  // namespace jxg
#pragma GCC visibility pop
