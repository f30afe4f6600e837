// jxg_merge.hip -- merge stage of the AC-strategy search on gfx950:
// 8x8-class decisions -> 16x8 ... 64x64 varblocks, and the transform,
// quantization and LLF-derived DC of every merged varblock.
//
// Three launches over the 64x64 tiles (the unit of libjxl's ProcessRectACS,
// combined.diff:346 context): merge_eval (this unit: every candidate's
// estimate), then merge_resolve (the decisions, and the chosen varblocks as
// one list per shape) and merge_write (the chosen varblocks' coefficients),
// both jxg_merge_write.hip.  launch_merge / launch_force_merge below are the
// stage's entries; what eval and write share is jxg_merge_kernel.h.
//
//   merge_eval    one 256-thread workgroup per (tile, width family): the
//                 candidate shapes whose rows are equally wide (16x8 | 8x16,
//                 16x16, 32x16 | 16x32, 32x32, 64x32 | 32x64, 64x64).  A
//                 shape's varblocks tile the 64x64 area, so every shape is
//                 the same amount of work -- no idle lanes at barriers -- and
//                 the row DCTs of the tile are the same for every shape of a
//                 width, so the workgroup runs them once:
//                   rows    lane = (channel, image row, C-wide segment),
//                           C-point DCT in registers (64-point: two lanes,
//                           Lee's even / odd halves, wave-uniform), read from
//                           the tile's XYB planes (written once by the front
//                           kernel); Y and X stay in 32 registers per thread,
//                           B goes to plane 2 of the LDS image (three planes,
//                           53.7 KB, 3 workgroups per CU);
//                 then per shape of the family that is searched and fits:
//                   write   the held Y / X rows -> planes 0 / 1 (the shape's
//                           valid varblocks);
//                   columns lane = (channel, band, column pair), in place
//                           (B: from plane 2 into plane 1 once X is done;
//                           the family's last shape: see below);
//                   quant   lane = (channel, 16-row chunk, varblock, column):
//                           Y first (its dequantized values replace its
//                           coefficients for the B residual), then X and B;
//                   reduce  lane = (varblock, column): chunk partials,
//                           (Y + X) + B, C-lane XOR tree -> estimate (+hook F).
//                 The last shape a workgroup evaluates (family_last: 16x8,
//                 32x16, 64x32, 64x64 on a full tile at efforts 6 - 7) has no
//                 next shape to keep plane 2 for: one column pass over Y, X
//                 and B, each in place in its own plane, one barrier, then
//                 Y, X and B quantized back to back (B from plane 2) -- two
//                 barriers, one table wait and the half-filled B column pass
//                 fewer than the earlier shapes' path, same float ops.
//                 The grid keeps a slot per (tile, shape); the four family
//                 workgroups of a tile are the slots of each family's first
//                 shape, with ids congruent mod 8, so they land on one XCD
//                 and share its L2.
// Float op order == oracle/merge.c (jxo_varblock, jxo_merge_tile).
#include <float.h>

#include <cstdio>
#include <type_traits>

#include "jxg_device.h"
#include "jxg_kernels.h"

#ifndef JXG_MERGE_WPE
// eval: 3 waves / SIMD (168 VGPRs): a family workgroup holds the row-transformed
// Y and X of its tile in 32 registers per thread, and its three-plane LDS
// image (EvalLds) admits three workgroups per CU
#define JXG_MERGE_WPE 3
#endif
// JXG_MERGE_PROFILE (experiment builds only): per (shape, phase) cycle sums
// of thread 0 of every eval workgroup, printed by dump_merge_profile(); a
// family's row phase is booked under its first shape; B's section is split
// into columns / tables + barrier / quantization + end barrier (a family's
// last shape has only the third).  quant_pass's zero votes: counted once per
// wave and vote ([channel][0 votes, 1 all-zero]), printed with the cycle sums;
// MZERO_COUNT is defined ahead of the kernel header, whose quant_pass uses it.
#ifdef JXG_MERGE_PROFILE
namespace jxg {
__device__ unsigned long long g_mprof[16][10];
__device__ unsigned long long g_mzero[3][2];
}  // namespace jxg
#define MPROF_MARK(si, k)                                           \
  do {                                                                \
    if (threadIdx.x == 0) {                                           \
      const unsigned long long now_ = __builtin_readcyclecounter();   \
      if ((k) > 0) atomicAdd(&g_mprof[(si)][(k)], now_ - mprof_t0);   \
      mprof_t0 = now_;                                                \
    }                                                                 \
  } while (0)
#define MZERO_COUNT(ch, hit)                                                        \
  do {                                                                                \
    if ((int)(threadIdx.x & 63) == __ffsll((unsigned long long)__ballot(1)) - 1) {    \
      atomicAdd(&g_mzero[(ch)][0], 1ull);                                             \
      if (hit) atomicAdd(&g_mzero[(ch)][1], 1ull);                                    \
    }                                                                                 \
  } while (0)
#else
#define MPROF_MARK(si, k) \
  do {                    \
  } while (0)
#endif

#include "jxg_merge_kernel.h"

namespace jxg {

// The LDS image: planes 0 and 1 as merge_write has them (plane 0 holds Y, its
// dequantized values after the Y quantization; plane 1 X, then B) and a third
// plane, the tile's row-transformed B, written once per workgroup, read by
// every shape of the family and consumed in place by the last one.  No LLF.
// gfx950 allocates LDS in 1280-byte granules: 53 696 B are 42 of them, three
// workgroups per CU.
struct EvalLds {
  static constexpr bool kWrite = false;
  float co[3 * kMPlane];  // coefficient image of the tile's varblocks
  float qsum[3][4][32];   // [Y, X, B][chunk][varblock]: column-tree chunk sums
  float btab[256];        // AdjustQuantBias of a magnitude q < 256 (setup_tile)
  float vr3[32][3];       // hook F: similarity indices of each top-left block
  int vbits[32];          // per varblock: rate bits
  int vnz[32][3];         //               non-zeros per channel
  int vraw[32];           //               max quant field
  int valid[32];
  uint8_t braw[64];       // front-kernel quant field (raw) of the tile's blocks
};
static_assert(sizeof(EvalLds) <= 42 * 1280, "three eval workgroups per CU: 42 LDS granules each");
// workgroup id -> (tile, shape): the nine shapes of a tile share b % 8 (XCD);
// per XCD the tiles go in chunks of JXG_MERGE_CHUNK, shape-major inside a
// chunk, so the workgroups resident on a CU at a time mostly run one shape's
// code (the kernel is 53 KB of code; interleaved shapes, chunk 1, took 1.595
// ms at 8K, chunk 64 1.545 ms: profiles/r02s4_merge_chunk) while a chunk's
// tiles are still in the XCD's L2: chunk 32 (1.5 MB of XYB per XCD) fetches
// 448 MB per 8K launch, chunk 64 650 MB (the nine shape passes no longer
// find the tiles in L2), at the same merge-stage time (1.81 ms;
// chunk 16: 435 MB, 1.84 ms -- profiles/r04p/merge_chunk).
// (a shard's tiles come through a list: tile = list[index])
// Since the family workgroups (merge_eval_kernel) a tile's slots 0, 1, 4 and 7
// -- the first shape of each row width -- do the work of their family and the
// other five leave at once: shape-major slots are family-major workgroups, and
// a chunk's tiles are read by four workgroups each instead of nine.
#ifndef JXG_MERGE_CHUNK
#define JXG_MERGE_CHUNK 32
#endif
__device__ __forceinline__ bool decode_wg(const MergeArgs& a, int& tile, int& si) {
  constexpr int T = JXG_MERGE_CHUNK;
  const int b = blockIdx.x, x = b & 7, q = b >> 3;
  const int r = q % (kNumShapes * T);
  si = r / T;
  tile = ((q / (kNumShapes * T)) * T + r % T) * 8 + x;
  if (tile >= (int)a.ntiles) return false;
  if (a.tile_list) tile = (int)a.tile_list[tile];
  return true;
}
// distortion of varblock v: chunk sums in order per channel, (Y + X) + B
__device__ __forceinline__ float varblock_dist(const Pass& P, const EvalLds& S, int v) {
  const int nch = P.lcy == 0 ? 1 : P.R() >> 4;
  float pc[3];
#pragma unroll
  for (int ci = 0; ci < 3; ci++) {
    float t = S.qsum[ci][0][v];
    for (int ch = 1; ch < nch; ch++) t = t + S.qsum[ci][ch][v];
    pc[ci] = t;
  }
  return (pc[0] + pc[1]) + pc[2];
}
// eval, once per workgroup: the blocks' quant field and the bias table go to
// LDS (read after the first shape's setup barrier)
__device__ __forceinline__ void setup_tile(const MergeArgs& a, EvalLds& S, int tx, int ty, int nbx,
                                           int nby) {
  const int t = threadIdx.x;
  if (t < 64) {
    const int lbx = t & 7, lby = t >> 3;
    const bool in = lbx < nbx && lby < nby;
    const size_t gb = (size_t)(ty * 8 + lby) * a.bxs + tx * 8 + lbx;
    S.braw[t] = in ? a.qf[gb] : 0;
  }
  fill_btab(S);
}
// eval, per shape, before the barrier that precedes the write-out: validity
// (the level region lies inside the frame's blocks), hook-F indices, sums
// reset (the varblock maxima are taken after the barrier: vraw_pass).  Thread
// v alone touched these words in the previous shape's estimate.
__device__ __forceinline__ void setup_varblocks(const MergeArgs& a, const Pass& P, EvalLds& S,
                                                int nbx, int nby) {
  const int t = threadIdx.x;
  if (t < 32) {
    const int v = t;
    bool ok = false;
    if (v < P.NV()) {
      const int bx0 = P.bx0(v), by0 = P.by0(v);
      const size_t gb0 = (size_t)(P.ty * 8 + by0) * a.bxs + P.tx * 8 + bx0;
      ok = (((bx0 >> P.ls) + 1) << P.ls) <= nbx && (((by0 >> P.ls) + 1) << P.ls) <= nby;
      if (ok && (a.proposals & 2u)) {
        S.vr3[v][0] = a.homog[gb0 * 3 + 0];
        S.vr3[v][1] = a.homog[gb0 * 3 + 1];
        S.vr3[v][2] = a.homog[gb0 * 3 + 2];
      }
    }
    S.valid[v] = ok;
    S.vraw[v] = 0;  // (vraw_pass: atomic max over the covered blocks)
    S.vbits[v] = 0;
    S.vnz[v][0] = S.vnz[v][1] = S.vnz[v][2] = 0;
  }
}
// varblock quant field = max raw over its covered blocks (after a barrier):
// one thread per block, an LDS atomic max into its varblock (round 6: one
// thread per varblock walked up to 64 blocks in a row of dependent LDS reads
// while its wave's row pass waited; max is order-free, so the result is the
// same); visible to the quantization after the row pass's barrier
__device__ __forceinline__ void vraw_pass(const MergeArgs& a, const Pass& P, EvalLds& S) {
  (void)a;
  const int b = threadIdx.x;
  if (b < 64) {
    const int lbx = b & 7, lby = b >> 3;
    const int v = ((lby >> P.lcy) << P.lGX()) | (lbx >> P.lcx);
    if (v < P.NV() && S.valid[v]) atomicMax(&S.vraw[v], (int)S.braw[b] + 1);
  }
}
// ---------------------------------------------------------------------------
// merge_eval: one workgroup per (tile, width family).  Family f holds the
// shapes whose rows are C = 8 << f wide: 16x8 | 8x16, 16x16, 32x16 | 16x32,
// 32x32, 64x32 | 32x64, 64x64.  A C-point row DCT depends on the row segment
// alone -- its channel, image row Y and segment gx -- not on the height of the
// varblock it lies in, so the workgroup transforms the tile's rows once:
//   Y, X  32 scaled outputs per thread, held in registers (hv) for the whole
//         workgroup and written to planes 0 / 1 at the start of every shape
//         (only into the varblocks valid for that shape);
//   B     to plane 2, where it stays; every shape's B column pass reads it
//         and writes plane 1 (col_pass<R, 1, true>) -- but for the last shape
//         the workgroup evaluates, which transforms it in place with Y and X
//         (col_pass<R, 3>) and quantizes B from plane 2.
// The float ops of a row are those of merge_write's row_pass<C>: the same
// lee<C> on row pairs (f2) for C < 64, and for C = 64 the two-lane form with
// one row per lane pair instead of two (dct64_first / dct64_rest on float;
// 256 items of 32 outputs, so that a thread holds 32 values for every C).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int family_first(int f) { return f ? 3 * f - 2 : 0; }  // 0, 1, 4, 7
__device__ __forceinline__ int family_count(int f) { return f == 0 ? 1 : (f == 3 ? 2 : 3); }

// The last shape of the family that the shape loop evaluates (its own test:
// the level is searched at this effort and a region of it fits the tile);
// wave-uniform.  Full tile at efforts 6 and 7: 16x8, 32x16, 64x32, 64x64; at
// effort 5 or with 4 - 7 blocks: 16x8, 32x16, 32x32; with 2 - 3 blocks: 16x8,
// 16x16.  Never 8x16 (16x16 is the same level), so its columns have 16 points
// or more.  JXG_MERGE_LAST=0 (experiment builds): no shape takes the last form.
#ifndef JXG_MERGE_LAST
#define JXG_MERGE_LAST 1
#endif
__device__ __forceinline__ int family_last(int f, int si0, int maxl, int nbx, int nby) {
  int last = -1;
  for (int si = si0; si < si0 + family_count(f); si++) {
    const int ls = max(kShapes[si].lcy, kShapes[si].lcx);
    if (ls <= maxl && (1 << ls) <= nbx && (1 << ls) <= nby) last = si;
  }
  return JXG_MERGE_LAST && last >= 0 && kShapes[last].lcy >= 1 ? last : -1;
}

// (family_rows calls the 64-point halves through these: with dctN_*<64> called
// directly the eval kernel compiles to other code, 41 mnemonic lines of 14583)
template <class T>
__device__ __forceinline__ T dct64_first(T xi, T xm, int i, int h) {
  return dctN_first<64>(xi, xm, i, h);
}
template <class T, class Out>
__device__ __forceinline__ void dct64_rest(T* t, int h, Out out) {
  dctN_rest<64>(t, h, out);
}

template <int LCX>
__device__ __forceinline__ void family_rows(const MergeArgs& a, int tile, EvalLds& S, int nbx,
                                            int nby, float (&hv)[32]) {
  constexpr int C = 8 << LCX;
  // A segment is needed if some shape of the family has a valid varblock over
  // it: validity at a level implies validity at the levels below, so the
  // family's lowest level (16 px for C <= 16, else C) decides.
  constexpr int LM = LCX ? LCX : 1;
  auto need = [&](int Y, int gx) {
    const int bx0 = gx << LCX, by = Y >> 3;
    return (((bx0 >> LM) + 1) << LM) <= nbx && (((by >> LM) + 1) << LM) <= nby;
  };
  const float* tsrc = a.xyb + (size_t)tile * (3 * 4096);
  float* bdst = S.co + 2 * kMPlane;
  if constexpr (C == 64) {
    // item = (row, half h), h wave-uniform; waves 0 and 1 also take B's rows
    const int i = threadIdx.x, h = (i >> 6) & 1, row = ((i >> 7) << 6) | (i & 63);
    const int c = row >> 6, Y = row & 63;
    auto half_row = [&](const float* src, float* t) {
      const float4* s0 = reinterpret_cast<const float4*>(src);
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const float4 a0 = s0[q], b0 = s0[15 - q];
        const float fa0[4] = {a0.x, a0.y, a0.z, a0.w}, fb0[4] = {b0.x, b0.y, b0.z, b0.w};
#pragma unroll
        for (int j = 0; j < 4; j++) t[4 * q + j] = dct64_first(fa0[j], fb0[3 - j], 4 * q + j, h);
      }
    };
    if (!need(Y, 0)) return;
    {
      float t[32];
      half_row(tsrc + pass_src(0, c) * 4096 + Y * 64, t);
      dct64_rest(t, h, [&](int k, float o) { hv[k] = o; });
    }
    if (i < 128) {  // (row == Y, c == 0)
      float t[32];
      half_row(tsrc + 2 * 4096 + Y * 64, t);
      dct64_rest(t, h, [&](int k, float o) { bdst[Y * kMS + 2 * k + h] = o; });
    }
  } else {
    constexpr int l = ilog2c<C>(), lgx = 3 - LCX, lch = 9 - LCX;  // 1 << lch segments per channel
    constexpr int PER = (2 << lch) / kMThreads;                   // Y and X: 4, 2, 1 per thread
    constexpr int NB = 1 << lch, PB = (NB + kMThreads - 1) / kMThreads;  // B: 2, 1, 1 (C = 32: half the threads)
    // segment r of a pass: gx is the fastest index, so a wave reads whole
    // 256-byte tile rows
    auto seg_of = [&](int r, int& c, int& Y, int& gx) {
      c = r >> lch;
      const int i = r & (NB - 1);
      gx = i & ((1 << lgx) - 1);
      Y = i >> lgx;
    };
    float buf[PER][C], bb[PB][C];
#pragma unroll
    for (int k = 0; k < PER; k++) {
      int c, Y, gx;
      seg_of(threadIdx.x + k * kMThreads, c, Y, gx);
      load_row<C>(tsrc + pass_src(0, c) * 4096 + Y * 64 + gx * C, buf[k]);
    }
#pragma unroll
    for (int k = 0; k < PB; k++) {
      const int r = threadIdx.x + k * kMThreads;
      if (r < NB) {
        int c, Y, gx;
        seg_of(r, c, Y, gx);
        load_row<C>(tsrc + 2 * 4096 + Y * 64 + gx * C, bb[k]);
      } else {
#pragma unroll
        for (int q = 0; q < C; q++) bb[k][q] = 0.0f;
      }
    }
#pragma unroll
    for (int k = 0; k < PER; k += 2) {
      int c0, Y0, gx0, c1 = 0, Y1 = 0, gx1 = 0;
      seg_of(threadIdx.x + k * kMThreads, c0, Y0, gx0);
      if (k + 1 < PER) seg_of(threadIdx.x + (k + 1) * kMThreads, c1, Y1, gx1);
      const bool n0 = need(Y0, gx0), n1 = k + 1 < PER && need(Y1, gx1);
      if (!n0 && !n1) continue;
      if constexpr (PER >= 2) {
        f2 x[C];
#pragma unroll
        for (int q = 0; q < C; q++) x[q] = f2{buf[k][q], buf[k + 1][q]};
        lee<C>(x);
#pragma unroll
        for (int q = 0; q < C; q++) {
          const f2 o = x[q] * kLeeS[l][q];
          hv[k * C + q] = o.x;
          hv[(k + 1) * C + q] = o.y;
        }
      } else {
        float* x = buf[k];
        lee<C>(x);
#pragma unroll
        for (int q = 0; q < C; q++) hv[q] = x[q] * kLeeS[l][q];
      }
    }
#pragma unroll
    for (int k = 0; k < PB; k += 2) {
      const int r0 = threadIdx.x + k * kMThreads, r1 = r0 + kMThreads;
      if (r0 >= NB) continue;
      int c0, Y0, gx0, c1 = 0, Y1 = 0, gx1 = 0;
      seg_of(r0, c0, Y0, gx0);
      if (k + 1 < PB) seg_of(r1, c1, Y1, gx1);
      const bool n0 = need(Y0, gx0), n1 = k + 1 < PB && r1 < NB && need(Y1, gx1);
      if (!n0 && !n1) continue;
      if constexpr (PB >= 2) {
        f2 x[C];
#pragma unroll
        for (int q = 0; q < C; q++) x[q] = f2{bb[k][q], bb[k + 1][q]};
        lee<C>(x);
        float* d0 = bdst + Y0 * kMS + gx0 * C;
        float* d1 = bdst + Y1 * kMS + gx1 * C;
#pragma unroll
        for (int q = 0; q < C; q++) {
          const f2 o = x[q] * kLeeS[l][q];
          if (n0) d0[q] = o.x;
          if (n1) d1[q] = o.y;
        }
      } else {
        float* x = bb[k];
        lee<C>(x);
        float* d0 = bdst + Y0 * kMS + gx0 * C;
#pragma unroll
        for (int q = 0; q < C; q++) d0[q] = x[q] * kLeeS[l][q];
      }
    }
  }
}

// the held Y / X rows -> planes 0 / 1, for the varblocks valid in this shape
// (the thread <-> segment map of family_rows)
template <int LCX>
__device__ __forceinline__ void family_writeout(const Pass& P, EvalLds& S, const float (&hv)[32]) {
  constexpr int C = 8 << LCX;
  if constexpr (C == 64) {
    const int i = threadIdx.x, h = (i >> 6) & 1, row = ((i >> 7) << 6) | (i & 63);
    const int c = row >> 6, Y = row & 63;
    if (!S.valid[Y >> P.lR()]) return;
    float* d = S.co + pass_plane(0, c) * kMPlane + Y * kMS + h;
#pragma unroll
    for (int k = 0; k < 32; k++) d[2 * k] = hv[k];
  } else {
    constexpr int lgx = 3 - LCX, lch = 9 - LCX, PER = (2 << lch) / kMThreads;
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int r = threadIdx.x + k * kMThreads;
      const int c = r >> lch, i = r & ((1 << lch) - 1), gx = i & ((1 << lgx) - 1), Y = i >> lgx;
      if (!S.valid[((Y >> P.lR()) << lgx) | gx]) continue;
      float* d = S.co + pass_plane(0, c) * kMPlane + Y * kMS + gx * C;
#pragma unroll
      for (int q = 0; q < C; q++) d[q] = hv[k * C + q];
    }
  }
}

// The grid keeps one slot per (tile, shape) (decode_wg); a family's workgroup
// is the slot of its first shape, the other five slots of a tile leave at
// once.  Shape-major slots are family-major workgroups.
__global__ __launch_bounds__(kMThreads) __attribute__((amdgpu_waves_per_eu(JXG_MERGE_WPE)))
void merge_eval_kernel(Batch<MergeArgs> bt_) {
  const MergeArgs& a = bt_.a[blockIdx.z];  // the batch's frame
  __shared__ __attribute__((aligned(16))) EvalLds S;
  if (blockIdx.x == 0 && threadIdx.x < kNumShapes) a.work[threadIdx.x] = 0;  // merge_resolve's list counts
  int tile, si0;
  if (!decode_wg(a, tile, si0)) return;
  const int fam = kShapes[si0].lcx;
  if (si0 != family_first(fam)) return;
  // the family's lowest level: if it is not searched at this effort or no
  // region of it fits the tile, none of the family's shapes has work
  const int lm = max(fam, 1), maxl = max_level(a);
  const int tx = tile % (int)a.tiles_x, ty = tile / (int)a.tiles_x;
  const int nbx = min(8, (int)a.bxs - tx * 8), nby = min(8, (int)a.bys - ty * 8);
  if (lm > maxl || (1 << lm) > nbx || (1 << lm) > nby) return;
#ifdef JXG_MERGE_PROFILE
  unsigned long long mprof_t0 = 0;
#endif
  MPROF_MARK(si0, 0);
  setup_tile(a, S, tx, ty, nbx, nby);
  float hv[32];
#pragma unroll
  for (int q = 0; q < 32; q++) hv[q] = 0.0f;
  switch (fam) {
    case 0: family_rows<0>(a, tile, S, nbx, nby, hv); break;
    case 1: family_rows<1>(a, tile, S, nbx, nby, hv); break;
    case 2: family_rows<2>(a, tile, S, nbx, nby, hv); break;
    default: family_rows<3>(a, tile, S, nbx, nby, hv); break;
  }
  MPROF_MARK(si0, 6);
  const int si_last = family_last(fam, si0, maxl, nbx, nby);
  for (int si = si0; si < si0 + family_count(fam); si++) {
    const Pass P = make_pass(a, tile, si);
    // level not searched at this effort, or no region of it fits
    if (P.ls > maxl || (1 << P.ls) > nbx || (1 << P.ls) > nby) continue;
    MPROF_MARK(si, 0);
    setup_varblocks(a, P, S, nbx, nby);
    __syncthreads();  // validity; the previous shape's reads of planes 0 / 1 are over
    vraw_pass(a, P, S);
    switch (fam) {
      case 0: family_writeout<0>(P, S, hv); break;
      case 1: family_writeout<1>(P, S, hv); break;
      case 2: family_writeout<2>(P, S, hv); break;
      default: family_writeout<3>(P, S, hv); break;
    }
    __syncthreads();
    MPROF_MARK(si, 5);
    // The family's last shape has no next shape to keep plane 2 for: B's
    // columns run with Y's and X's, in place, and B is quantized from plane 2
    // right behind X -- no barrier until the estimate.
    const bool last = JXG_MERGE_LAST && si == si_last;
    if (last) {
      switch (P.lcy) {  // (never 8 rows: family_last)
        case 1: col_pass<16, 3>(P, S, 0); break;
        case 2: col_pass<32, 3>(P, S, 0); break;
        default: col_pass<64, 3>(P, S, 0); break;
      }
    } else {
      switch (P.lcy) {
        case 0: col_pass<8, 2>(P, S, 0); break;
        case 1: col_pass<16, 2>(P, S, 0); break;
        case 2: col_pass<32, 2>(P, S, 0); break;
        default: col_pass<64, 2>(P, S, 0); break;
      }
    }
    MPROF_MARK(si, 1);
    // Y first: its dequantized values replace its coefficients (X / B
    // residuals); then X; then, for a shape that is not the last, B's columns
    // go from plane 2 into X's plane behind a barrier, and B's tables wait out
    // a second one.  Every pass's tables are in flight across the barrier
    // before it; the last shape's B tables are issued where X's die.  A lane's
    // X / B items read the Y values its own Y item wrote.
    auto quant_yx = [&](auto rpc_tag) {
      constexpr int RPC = decltype(rpc_tag)::value;
      {
        QTab<RPC> ty_;
        load_qtab<RPC, false, 1>(a, P, ty_);
        __syncthreads();
        MPROF_MARK(si, 2);
        quant_pass<RPC, 1>(a, P, S, ty_);
      }
      QTab<RPC> tx_;
      load_qtab<RPC, false, 0>(a, P, tx_);
      quant_pass<RPC, 0>(a, P, S, tx_);
    };
    auto quant_b = [&](auto rpc_tag) {
      constexpr int RPC = decltype(rpc_tag)::value;
      QTab<RPC> tb;
      load_qtab<RPC, false, 2>(a, P, tb);
      if (!last) {
        __syncthreads();
        MPROF_MARK(si, 8);
      }
      quant_pass<RPC, 2>(a, P, S, tb, last ? 2 : 1);
    };
    if (P.lcy == 0) quant_yx(std::integral_constant<int, 8>());
    else quant_yx(std::integral_constant<int, 16>());
    if (!last) {
      __syncthreads();  // plane 1 (X) fully read
      MPROF_MARK(si, 3);
      switch (P.lcy) {
        case 0: col_pass<8, 1, true>(P, S, 1); break;
        case 1: col_pass<16, 1, true>(P, S, 1); break;
        case 2: col_pass<32, 1, true>(P, S, 1); break;
        default: col_pass<64, 1, true>(P, S, 1); break;
      }
      MPROF_MARK(si, 7);
    } else {
      MPROF_MARK(si, 3);
    }
    if (P.lcy == 0) quant_b(std::integral_constant<int, 8>());
    else quant_b(std::integral_constant<int, 16>());
    __syncthreads();
    MPROF_MARK(si, 4);
    const int v = threadIdx.x;
    if (v < P.NV() && S.valid[v]) {
      const float dist = varblock_dist(P, S, v);
      const int tb = bitlen_u((uint32_t)S.vnz[v][0]) + bitlen_u((uint32_t)S.vnz[v][1]) +
                     bitlen_u((uint32_t)S.vnz[v][2]);
      float e = ((float)(S.vbits[v] + tb) + 8.0f * dist) * P.tmul;
      if (a.proposals & 2u) e = hook_f(e, S.vr3[v][0], S.vr3[v][1], S.vr3[v][2]);
      a.cost[((size_t)tile * kNumShapes + si) * 32 + v] = e;
    }
  }
}
#ifdef JXG_MERGE_PROFILE
void dump_merge_profile() {
  unsigned long long h[16][10];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_mprof), sizeof(h)) != hipSuccess) return;
  std::fprintf(stderr, "merge_eval cycles (thread 0 sums, Mcycles): shape rows(family) "
                       "setup+writeout cols(Y,X) qtab quantY+X colsB qtabB quantB\n");
  for (int si = 0; si < kNumShapes; si++)
    std::fprintf(stderr, "  %dx%d %8.1f %8.1f %8.1f %8.1f %8.1f %8.1f %8.1f %8.1f\n", 8 << kShapes[si].lcy,
                 8 << kShapes[si].lcx, h[si][6] / 1e6, h[si][5] / 1e6, h[si][1] / 1e6, h[si][2] / 1e6,
                 h[si][3] / 1e6, h[si][7] / 1e6, h[si][8] / 1e6, h[si][4] / 1e6);
  unsigned long long z[3][2];
  if (hipMemcpyFromSymbol(z, HIP_SYMBOL(g_mzero), sizeof(z)) != hipSuccess) return;
  for (int c = 0; c < 3; c++)
    std::fprintf(stderr, "quant_pass zero votes, channel %c: %llu of %llu row pairs\n", "XYB"[c],
                 z[c][1], z[c][0]);
}
#else
void dump_merge_profile() {}
#endif
// k frames of one size (same tile count): one launch of each kernel
hipError_t launch_merge(const MergeArgs* a, uint32_t k, hipStream_t s) {
  if (!k || !a[0].ntiles) return hipSuccess;
  const Batch<MergeArgs> b = make_batch(a, k);
  const uint32_t ntiles = a[0].ntiles;
  constexpr uint32_t T = JXG_MERGE_CHUNK;
  const uint32_t nwg = (((ntiles + 7) / 8 + T - 1) / T) * T * 8 * kNumShapes;
  hipLaunchKernelGGL(merge_eval_kernel, dim3(nwg, 1, k), dim3(kMThreads), 0, s, b);
  launch_merge_resolve(b, k, s);
  launch_merge_write(b, k, s);
  return hipGetLastError();
}
// forced encode: the lists from the caller's map, then merge_write as above
hipError_t launch_force_merge(const MergeArgs& a, hipStream_t s) {
  if (!a.ntiles || !a.force) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(a.work, 0, kMergeWorkHead * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  launch_force_list(a, s);
  launch_merge_write(make_batch(&a, 1), 1, s);
  return hipGetLastError();
}

}  // namespace jxg
