// jxg_trace.hip -- the search trace of a traced encode (jxg_encode_traced_rgb8
// / jxg_search_trace): the merge stage's and the 128 / 256 px
// levels' candidate estimates as planes over the block grid, and an
// exact-integer summary of the 8x8 scan's decisions.
//
// trace_planes_kernel   one thread per block: for each of the nine merged
//   shapes (kShapes, jxg_shapes.h) and the six big ones (level x {tall, wide,
//   full}, the order of jxg_bigvb.hip kBig) the estimate of the candidate varblock whose first
//   block this is, read from merge_eval's mcost[tile][9][32] / big_eval's
//   cost[group][30]; NaN wherever no candidate was evaluated.  merge_eval and
//   big_eval leave the entries of unsearched levels and of regions that do not
//   fit the frame's blocks unwritten, so an entry is copied only when the
//   tests of setup_varblocks (merge_eval's shape loop) / big_region say it was
//   written by this encode.  Also the final per-block estimate (`ent`).
// trace_summary_kernel  one thread per block: counters as integer atomics on
//   LDS, then on global memory (order-free: the same words from run to run).
// Both run on the encode's stream right behind its merge stage, before
// anything can reuse mcost.
#include <float.h>

#include "jxg_device.h"
#include "jxg_kernels.h"

namespace jxg {

namespace {

constexpr int kTraceThreads = 256;

// scan index of an 8x8-class raw id (front_kernel's si): DCT8 0, DCT4X4 1,
// DCT2X2 2, DCT4X8 3, DCT8X4 4, IDENTITY 5; -1: not of the class
__device__ __forceinline__ int scan_index(int id) {
  return id == kDCT8 ? 0
                     : (id == kDCT4X4 ? 1
                                      : (id == kDCT2X2 ? 2
                                                       : (id == kDCT4X8 ? 3
                                                                        : (id == kDCT8X4 ? 4
                                                                                         : (id == kIDENTITY ? 5 : -1)))));
}

// front_kernel's order on (estimate, scan index)
__device__ __forceinline__ bool trace_beats(float ea, int ia, float eb, int ib) {
  const bool va = ea < FLT_MAX, vb = eb < FLT_MAX;
  if (va && vb) return ea < eb || (ea == eb && ia < ib);
  if (va != vb) return va;
  return ia < ib;
}

}  // namespace

__global__ __launch_bounds__(kTraceThreads) void trace_planes_kernel(TraceArgs a) {
  const size_t nb = (size_t)a.bxs * a.bys;
  const float nan = __builtin_nanf("");
  for (size_t gb = (size_t)blockIdx.x * kTraceThreads + threadIdx.x; gb < nb;
       gb += (size_t)gridDim.x * kTraceThreads) {
    const int bx = (int)(gb % a.bxs), by = (int)(gb / a.bxs);
    // ---- levels up to 64 px: the tile's candidates ----
    const int tx = bx >> 3, ty = by >> 3, lbx = bx & 7, lby = by & 7;
    const int nbx = min(8, (int)a.bxs - tx * 8), nby = min(8, (int)a.bys - ty * 8);
    const size_t tile = (size_t)ty * a.tiles_x + tx;
    const int maxl = a.max_s >= 8 ? 3 : (a.max_s >= 4 ? 2 : 1);
#pragma unroll
    for (int si = 0; si < kNumShapes; si++) {
      const int lcy = kShapes[si].lcy, lcx = kShapes[si].lcx, ls = max(lcy, lcx);
      // searched at this effort; this is a first block on the shape's grid;
      // its level region lies inside the frame's blocks (setup_varblocks)
      const bool first = (lbx & ((1 << lcx) - 1)) == 0 && (lby & ((1 << lcy) - 1)) == 0;
      const bool fits = (((lbx >> ls) + 1) << ls) <= nbx && (((lby >> ls) + 1) << ls) <= nby;
      float e = nan;
      if (a.mcost && ls <= maxl && first && fits) {
        const int v = ((lby >> lcy) << (3 - lcx)) | (lbx >> lcx);  // < 64 >> (lcy + lcx) <= 32
        e = a.mcost[(tile * kNumShapes + si) * 32 + v];
      }
      a.merged[(size_t)si * nb + gb] = e;
    }
    // ---- levels 128 / 256 px: the pass group's candidates ----
    const uint32_t g = (uint32_t)(by >> 5) * a.gxs + (uint32_t)(bx >> 5);
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const int L = k / 3, form = k % 3;  // 0 tall, 1 wide, 2 full (kBig)
      const int s = 16 << L, h = s >> 1;
      // big_region: region r of level L of the group
      const int gx0 = (bx >> 5) * 32, gy0 = (by >> 5) * 32;
      const int rx = L == 0 ? ((bx - gx0) >> 4) : 0, ry = L == 0 ? ((by - gy0) >> 4) : 0;
      const int bx0 = gx0 + rx * 16, by0 = gy0 + ry * 16, r = ry * 2 + rx;
      const bool fits = bx0 + s <= (int)a.bxs && by0 + s <= (int)a.bys;
      // big_cand: 0 full, 1 / 2 tall halves (left / right), 3 / 4 wide halves (top / bottom)
      int j = -1;
      if (form == 2 && bx == bx0 && by == by0) j = 0;
      if (form == 0 && by == by0) j = bx == bx0 ? 1 : (bx == bx0 + h ? 2 : -1);
      if (form == 1 && bx == bx0) j = by == by0 ? 3 : (by == by0 + h ? 4 : -1);
      float e = nan;
      if (a.big_cost && g < a.ngroups && fits && j >= 0)
        e = a.big_cost[(size_t)g * 30 + (L == 0 ? r * 5 + j : 20 + j)];
      a.big[(size_t)k * nb + gb] = e;
    }
    a.chosen[gb] = a.ent ? a.ent[gb] : nan;
  }
}

// summary words (jxg_trace_summary): blocks, max_px, flip[6][6], hook_p[6],
// merged_over[6], margin[6][8], margin_skipped[6]
constexpr int kSumFlip = 2, kSumHookP = kSumFlip + 36, kSumOver = kSumHookP + 6,
              kSumMargin = kSumOver + 6, kSumSkipped = kSumMargin + 48;
static_assert(kSumSkipped + 6 == (int)kTraceSummaryWords, "summary layout");

__global__ __launch_bounds__(kTraceThreads) void trace_summary_kernel(TraceArgs a) {
  __shared__ uint32_t sCnt[kTraceSummaryWords];
  const size_t nb = (size_t)a.bxs * a.bys;
  for (int i = threadIdx.x; i < (int)kTraceSummaryWords; i += kTraceThreads) sCnt[i] = 0;
  __syncthreads();
  for (size_t gb = (size_t)blockIdx.x * kTraceThreads + threadIdx.x; gb < nb;
       gb += (size_t)gridDim.x * kTraceThreads) {
    float e[6], er[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
      e[i] = a.cand8[(size_t)i * nb + gb];
      er[i] = a.cand8_raw[(size_t)i * nb + gb];
    }
    // the scan replayed on the raw estimates; best and second of the compared ones
    int wr = 0, b1 = 0;
#pragma unroll
    for (int i = 1; i < 6; i++) {
      if (trace_beats(er[i], i, er[wr], wr)) wr = i;
      if (trace_beats(e[i], i, e[b1], b1)) b1 = i;
    }
    int b2 = b1 == 0 ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
      if (i != b1 && i != b2 && trace_beats(e[i], i, e[b2], b2)) b2 = i;
    const int sw = scan_index((int)a.scan8[gb]), fw = scan_index((int)a.front8[gb]);
    if (sw < 0 || fw < 0) continue;  // (never: the front kernel writes 8x8-class ids)
    atomicAdd(&sCnt[kSumFlip + wr * 6 + sw], 1u);
    if (a.front8[gb] != a.scan8[gb]) atomicAdd(&sCnt[kSumHookP + fw], 1u);
    if (scan_index((int)(a.acs[gb] & 0x7F)) < 0) atomicAdd(&sCnt[kSumOver + sw], 1u);
    const float best = e[b1], second = e[b2];
    if (!(best < FLT_MAX) || best <= 0.0f) {
      atomicAdd(&sCnt[kSumSkipped + sw], 1u);
    } else {
      // one multiply and one compare per k; 1 + 2^-k is exact in f32
      int bucket = 0;
      float step = 1.0f;
#pragma unroll
      for (int k = 0; k < 7; k++) {
        bucket += second >= best * (1.0f + step) ? 1 : 0;
        step *= 0.5f;
      }
      atomicAdd(&sCnt[kSumMargin + sw * 8 + bucket], 1u);
    }
  }
  __syncthreads();
  for (int i = kSumFlip + threadIdx.x; i < (int)kTraceSummaryWords; i += kTraceThreads)
    if (sCnt[i]) atomicAdd(a.summary + i, sCnt[i]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.summary[0] = (uint32_t)nb;
    a.summary[1] = a.max_px;
  }
}

hipError_t launch_trace(const TraceArgs& a, hipStream_t s) {
  const size_t nb = (size_t)a.bxs * a.bys;
  if (!nb) return hipSuccess;
  const uint32_t nwg = (uint32_t)std::min<size_t>((nb + kTraceThreads - 1) / kTraceThreads, 2048);
  hipError_t e = hipMemsetAsync(a.summary, 0, kTraceSummaryWords * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(trace_planes_kernel, dim3(nwg), dim3(kTraceThreads), 0, s, a);
  hipLaunchKernelGGL(trace_summary_kernel, dim3(nwg), dim3(kTraceThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace jxg
