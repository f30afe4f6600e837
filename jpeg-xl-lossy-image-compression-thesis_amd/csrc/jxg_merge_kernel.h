// jxg_merge_kernel.h -- what merge_eval (jxg_merge.hip) and merge_write
// (jxg_merge_write.hip) share (device only): the 64x64 LDS coefficient image
// of a 256-thread workgroup, the (tile, shape) index math, the column DCTs and
// the quantization.  The two kernels differ in their row passes, in what a
// slot of the image holds (a tile's varblock / any tile's) and in what the
// quantization leaves behind (an estimate / coefficients and the LLF); the
// last is a property of the kernel's LDS type L:
//   L::kWrite  false: EvalLds, distortion sums for the estimate
//              true:  WriteLds, coefficients to their natural-order slices,
//                     LLF to L::llf, chroma-from-luma factors per slot
// Float op order == oracle/merge.c (jxo_varblock).
#pragma once
#include "jxg_device.h"
#include "jxg_kernels.h"
#include "jxg_lee.h"

// quant_pass's zero votes: counted by profile builds of the eval unit, which
// defines this before it includes the header
#ifndef MZERO_COUNT
#define MZERO_COUNT(ch, hit) \
  do {                       \
  } while (0)
#endif

namespace jxg {

constexpr int kMThreads = 256;
constexpr int kMS = 65;  // LDS row stride (floats)
constexpr int kMPlane = 64 * kMS;
__device__ __forceinline__ int bitlen_u(uint32_t v) { return 32 - __clz(v); }
// the two transform passes of a tile: pass 0 = Y (plane 0) and X (plane 1),
// pass 1 = B (plane 1); local channel lc of a pass -> frame channel (X 0, Y 1,
// B 2) and LDS plane
__device__ __forceinline__ int pass_src(int pass, int lc) { return pass ? 2 : 1 - lc; }
__device__ __forceinline__ int pass_plane(int pass, int lc) { return pass ? 1 : lc; }
__device__ __forceinline__ constexpr int chan_plane(int ch) { return ch == 1 ? 0 : 1; }

// one (tile, shape) workgroup: all index math is shifts and masks
struct Pass {
  int si, type, lcy, lcx, soff, ls, tx, ty, tile;
  float tmul;
  __device__ __forceinline__ int cy() const { return 1 << lcy; }
  __device__ __forceinline__ int cx() const { return 1 << lcx; }
  __device__ __forceinline__ int R() const { return 8 << lcy; }
  __device__ __forceinline__ int C() const { return 8 << lcx; }
  __device__ __forceinline__ int lR() const { return 3 + lcy; }
  __device__ __forceinline__ int lC() const { return 3 + lcx; }
  __device__ __forceinline__ int lGX() const { return 3 - lcx; }
  __device__ __forceinline__ int lNV() const { return 6 - lcx - lcy; }
  __device__ __forceinline__ int NV() const { return 1 << lNV(); }
  __device__ __forceinline__ int bx0(int v) const { return (v & ((1 << lGX()) - 1)) << lcx; }
  __device__ __forceinline__ int by0(int v) const { return (v >> lGX()) << lcy; }
  __device__ __forceinline__ int off(int v, int plane) const {
    return plane * kMPlane + by0(v) * 8 * kMS + bx0(v) * 8;
  }
};
__device__ __forceinline__ Pass make_pass(const MergeArgs& a, int tile, int si) {
  Pass P;
  P.si = si;
  const ShapeDesc& D = kShapes[si];
  P.type = D.type;
  P.lcy = D.lcy;
  P.lcx = D.lcx;
  P.tmul = D.tmul;
  P.soff = kShapeOff[si];
  P.ls = max(D.lcy, D.lcx);  // level: the s x s region (log2 blocks) of the shape
  P.tile = tile;
  P.tx = tile % (int)a.tiles_x;
  P.ty = tile / (int)a.tiles_x;
  return P;
}

// a C-float row segment of the tile-major XYB copy, in 16-byte loads (the two
// kernels' row passes)
template <int C>
__device__ __forceinline__ void load_row(const float* src, float* d) {
#pragma unroll
  for (int q = 0; q < C / 4; q++) {
    const float4 u = reinterpret_cast<const float4*>(src)[q];
    d[4 * q] = u.x;
    d[4 * q + 1] = u.y;
    d[4 * q + 2] = u.z;
    d[4 * q + 3] = u.w;
  }
}
// columns: R-point DCT of every column, in place.  A lane transforms the
// columns X and X + 32 (X < 32) of one band of R rows and one channel (f2
// lanes; any two columns of a band have the same length, whatever varblocks
// they belong to): the two LDS reads of a pair are one ds_read2 and the 32
// lanes of a band read 64 consecutive columns.  64-point: item = (pair, h).
// B2 (eval, NCH = 1): out of place, from the row-transformed B in plane 2 to
// plane 1 -- plane 2 stays as it is for the family's next shape, and the
// two-lane form needs no barrier between its reads and its writes.
template <int R, int NCH, bool B2 = false, class L>
__device__ __forceinline__ void col_pass(const Pass& P, L& S, int pass) {
  static_assert(!B2 || NCH == 1, "the out-of-place form is B's");
  constexpr int lR = ilog2c<R>(), nb = 64 / R, lnb = 6 - lR;
  constexpr int npairs = NCH * nb * 32;  // (channel, band, X)
  constexpr int dst = B2 ? -kMPlane : 0;  // store offset from the load's
  const int lGX = P.lGX(), lC = P.lC();
  auto col_of = [&](int pidx, int& off, bool& okA, bool& okB) {
    const int X = pidx & 31, band = (pidx >> 5) & (nb - 1), c = pidx >> (5 + lnb);
    off = (B2 ? 2 : pass_plane(pass, c)) * kMPlane + band * R * kMS + X;
    okA = S.valid[(band << lGX) | (X >> lC)];
    okB = S.valid[(band << lGX) | ((X + 32) >> lC)];
  };
  // Two lanes per column pair (Lee halves, h wave-uniform: waves alternate h
  // over 64 pairs) for 64-point columns, and (round 6) for 16 / 32-point
  // columns whenever one lane per pair would leave threads idle (<= 128
  // pairs: R = 32, and the B pass at R = 16) -- each lane then runs half the
  // transform, every thread busy; a barrier separates the column reads from
  // the in-place writes.
  // NCH = 3 (eval, a family's last shape): Y, X and B in place in planes 0, 1
  // and 2 (pass_plane(0, c) == c).  R = 64: 96 pairs, 192 threads, one
  // iteration.  R = 32: 192 pairs in two iterations of the two-lane form (Y
  // and X, then B on half the threads, as the B pass had it), each with its
  // own read -> write barrier; one lane per pair would hold 32 f2 values
  // beside the family's 32 held rows.  R = 16: 384 pairs, one lane each.
  if constexpr (R == 64 || (R >= 16 && npairs <= kMThreads / 2) || (NCH == 3 && R == 32)) {
    constexpr int H = R / 2;
    constexpr int n = ((npairs + 63) >> 6) << 7;
    for (int i0 = 0; i0 < n; i0 += kMThreads) {
      const int i = i0 + threadIdx.x;
      const int h = (i >> 6) & 1, p = ((i >> 7) << 6) | (i & 63);
      int off = 0;
      bool okA = false, okB = false;
      if (p < npairs) col_of(p, off, okA, okB);
      const bool act = okA || okB;
      f2 o[H];
      if (act) {
        const float* q0 = S.co + off;
        f2 t[H];
#pragma unroll
        for (int j = 0; j < H; j++)
          t[j] = dctN_first<R>(f2{q0[j * kMS], q0[j * kMS + 32]},
                               f2{q0[(R - 1 - j) * kMS], q0[(R - 1 - j) * kMS + 32]}, j, h);
        dctN_rest<R>(t, h, [&](int k, f2 u) { o[k] = u; });
      }
      if constexpr (!B2) __syncthreads();
      if (act) {
#pragma unroll
        for (int k = 0; k < H; k++) {
          if (okA) S.co[off + dst + (2 * k + h) * kMS] = o[k].x;
          if (okB) S.co[off + dst + 32 + (2 * k + h) * kMS] = o[k].y;
        }
      }
    }
  } else {
    for (int p = threadIdx.x; p < npairs; p += kMThreads) {
      int off;
      bool okA, okB;
      col_of(p, off, okA, okB);
      if (!okA && !okB) continue;
      float* col = S.co + off;
      f2 o[R];
#pragma unroll
      for (int k = 0; k < R; k++) o[k] = f2{col[k * kMS], col[k * kMS + 32]};
      lee<R>(o);
#pragma unroll
      for (int k = 0; k < R; k++) {
        const f2 u = o[k] * kLeeS[lR][k];
        if (okA) col[dst + k * kMS] = u.x;
        if (okB) col[dst + k * kMS + 32] = u.y;
      }
    }
  }
}

// quantization, phase 0 = Y, phase 1 = X and B; lane = (channel, chunk of
// RPC rows, varblock, column).  Chunk partial: fmaf(e, e) over its rows
// ascending.  The lane's weights, inverse Y weights and natural positions
// come in 16-byte loads of four rows each (row-quad tables, load_qtab).
// Rate bits and non-zeros are summed over the varblock's C lanes in-wave and
// added to LDS by one lane.  L::kWrite: coefficients to their natural-order
// slices, LLF to LDS, no distortion sums.
template <int N>
__device__ __forceinline__ void load_f(const float* p, float* d) {
#pragma unroll
  for (int i = 0; i < N / 4; i++) {
    const float4 v = reinterpret_cast<const float4*>(p)[i];
    d[4 * i] = v.x;
    d[4 * i + 1] = v.y;
    d[4 * i + 2] = v.z;
    d[4 * i + 3] = v.w;
  }
}
// A thread's quantization tables for one channel: its NIT items' weights,
// distortion weights and (Y) inverse weights.  They are loaded before the
// barrier that precedes the channel's pass (load_qtab), so their L2 latency
// overlaps the barrier wait (-1 % measured; a build without any table loads
// ran 13 % faster, so the loads' issue, not their latency, is what costs).
template <int RPC>
struct QTab {
  static constexpr int NIT = RPC == 8 ? 2 : 1;  // items per thread: 512 or 256 / 256
  float w[NIT][RPC], sd[NIT][RPC], iw[NIT][RPC];
};
// Tables in row quads ([ky / 4][kx][ky % 4], host quant tables): one 16-byte
// load per lane and four rows, the wave's 64 lanes 1 KB contiguous.
__device__ __forceinline__ int qtab_index(const Pass& P, int ky, int x) {
  return P.soff + ((ky >> 2) * P.C() + x) * 4;
}
template <int RPC, bool WRITE, int CH>
__device__ __forceinline__ void load_qtab(const MergeArgs& a, const Pass& P, QTab<RPC>& T) {
  constexpr int STOT = kShapeOff[kNumShapes];
#pragma unroll
  for (int it = 0; it < QTab<RPC>::NIT; it++) {
    const int j = threadIdx.x + it * kMThreads;
    const int ch = j >> (P.lNV() + P.lC()), x = j & (P.C() - 1);
#pragma unroll
    for (int kk = 0; kk < RPC; kk += 4) {
      const int ti = qtab_index(P, ch * RPC + kk, x);
      load_f<4>(a.wk + (size_t)CH * STOT + ti, &T.w[it][kk]);
      if (!WRITE) load_f<4>(a.sdk + (size_t)CH * STOT + ti, &T.sd[it][kk]);
      if (CH == 1) load_f<4>(a.iwy + ti, &T.iw[it][kk]);
    }
  }
}
// All-reduce over an aligned group of C lanes (C = 8 .. 64, the group fully
// active) as the XOR butterfly v += v(lane ^ m), m = 1, 2, 4, ...: every
// step's partner value comes from DPP / ds_swizzle / readlane instead of a
// ds_bpermute chain (round 6).  Exactness: each step adds the partner's
// value, which is what lane ^ m holds -- xor 1 / 2 / 4 are exact lane
// permutations (quad_perm, quad_perm + row_half_mirror), xor 8 is
// row_half_mirror + row_mirror ((i ^ 7) ^ 15 = i ^ 8), xor 16 a ds_swizzle
// xor mask; for xor 32 the two 32-lane halves are uniform by then, so the
// partner is the other half's lane 0 / 32, and a + b = b + a.
template <int M>
__device__ __forceinline__ uint32_t grp_xor(uint32_t v) {
  if constexpr (M == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);
  if constexpr (M == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);
  if constexpr (M == 4) {
    const int t = __builtin_amdgcn_mov_dpp((int)v, 0x1B, 0xF, 0xF, false);
    return (uint32_t)__builtin_amdgcn_mov_dpp(t, 0x141, 0xF, 0xF, false);
  }
  if constexpr (M == 8) {
    const int t = __builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, false);
    return (uint32_t)__builtin_amdgcn_mov_dpp(t, 0x140, 0xF, 0xF, false);
  }
  if constexpr (M == 16) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);
  if constexpr (M == 32) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
    return (threadIdx.x & 32) ? lo : hi;
  }
}
template <int M>
__device__ __forceinline__ void grp_step(float& cp, int& packed) {
  cp += __uint_as_float(grp_xor<M>(__float_as_uint(cp)));
  packed += (int)grp_xor<M>((uint32_t)packed);
}
__device__ __forceinline__ void group_all_reduce(float& cp, int& packed, int C) {
  grp_step<1>(cp, packed);
  grp_step<2>(cp, packed);
  grp_step<4>(cp, packed);
  if (C > 8) grp_step<8>(cp, packed);
  if (C > 16) grp_step<16>(cp, packed);
  if (C > 32) grp_step<32>(cp, packed);
}

template <int RPC, int CH, class L>
__device__ __forceinline__ void quant_pass(const MergeArgs& a, const Pass& P, L& S, const QTab<RPC>& T,
                                           int plane = chan_plane(CH)) {
  constexpr bool WRITE = L::kWrite;
  constexpr int cidx = CH == 1 ? 0 : (CH == 0 ? 1 : 2);  // 0 Y, 1 X, 2 B
  // the wave-uniform zero path: the estimate's X and B passes (about 65 % and
  // 63 % of their row pairs on the 8K bench frames).  Not Y (17 %: the vote
  // costs more than it saves) and not the write pass.
  constexpr bool ZERO = !WRITE && CH != 1;
  const int C = P.C(), NV = P.NV();
  // chroma from luma of the tile (front kernel): X - kx Yd, B - kb Yd
  // (write: of the slot's tile, from setup_slots)
  float kc = 0.0f;
  if (!WRITE && CH != 1) {
    const float f = (float)a.cmap[(CH == 0 ? 0u : a.ntiles_all) + (uint32_t)P.tile];
    kc = CH == 0 ? f * (1.0f / 84.0f) : 1.0f + f * (1.0f / 84.0f);
  }
#pragma unroll
  for (int it = 0; it < QTab<RPC>::NIT; it++) {
    const int j = threadIdx.x + it * kMThreads;
    const int ch = j >> (P.lNV() + P.lC()), v = (j >> P.lC()) & (NV - 1), x = j & (C - 1);
    if (!S.valid[v]) continue;  // the varblock's C lanes leave together
    const int bx0 = P.bx0(v), by0 = P.by0(v);  // image position (the LLF's index)
    if constexpr (WRITE && CH != 1) kc = S.skc[CH == 0 ? 0 : 1][v];
    const float scale = (float)a.G * (float)S.vraw[v] / 65536.0f;
    float* cplane = S.co + P.off(v, plane) + x;
    const float* yd = S.co + P.off(v, 0) + x;
    const float* w = T.w[it];
    const float* sd = T.sd[it];
    float iw[RPC];
    if (CH == 1) {
      const float inv_scale = 1.0f / scale;
#pragma unroll
      for (int kk = 0; kk < RPC; kk++) iw[kk] = T.iw[it][kk] * inv_scale;
    }
    uint16_t nat[RPC];
    if (WRITE) {
#pragma unroll
      for (int kk = 0; kk < RPC; kk += 4) {
        const uint2 u = *reinterpret_cast<const uint2*>(a.nat + qtab_index(P, ch * RPC + kk, x));
        nat[kk] = (uint16_t)u.x;
        nat[kk + 1] = (uint16_t)(u.x >> 16);
        nat[kk + 2] = (uint16_t)u.y;
        nat[kk + 3] = (uint16_t)(u.y >> 16);
      }
    }
    // the LLF (first cy rows x cx columns) only occurs in chunk 0
    const bool llf_col = ch == 0 && x < P.cx();
    float cp = 0.0f;
    // exponent sums of the rows below 8 and from 8 on: non-zeros from each
    // (nz = sum / 127, exact for eight values: jxg_front.hip nz_of_esum)
    uint32_t eb8[2] = {0u, 0u};
    // rows in pairs: the float multiplies / adds of the two rows are one
    // packed op each (f2, no contraction: each half is the scalar op order);
    // the distortion chain stays in row order
    auto scaled = [&](int kk) {
      const int ky = ch * RPC + kk;
      const f2 coef = f2{cplane[ky * kMS], cplane[(ky + 1) * kMS]};
      if constexpr (WRITE) {
        if (llf_col) {
          if (kk < P.cy()) S.llf[CH][(by0 + ky) * 8 + bx0 + x] = coef.x;
          if (kk + 1 < P.cy()) S.llf[CH][(by0 + ky + 1) * 8 + bx0 + x] = coef.y;
        }
      }
      f2 rv = coef;
      if (CH != 1) rv = rv - f2{kc, kc} * f2{yd[ky * kMS], yd[(ky + 1) * kMS]};
      // LLF positions carry weight 0 (host tables): vq = +-0 quantizes to 0
      // and contributes nothing
      return rv * (f2{w[kk], w[kk + 1]} * f2{scale, scale});
    };
    // ZERO: the scaled values of all the lane's rows first (the LDS reads stay
    // one pipelined batch), then one wave vote per row pair (a vote per chunk,
    // alone or ahead of these, and values formed inside the loop all measured
    // slower: profiles/r09zero/variants.md)
    f2 vqs[ZERO ? RPC / 2 : 1];
    if constexpr (ZERO) {
#pragma unroll
      for (int kk = 0; kk < RPC; kk += 2) vqs[kk >> 1] = scaled(kk);
    }
#pragma unroll
    for (int kk = 0; kk < RPC; kk += 2) {
      const int ky = ch * RPC + kk;
      f2 vq;
      if constexpr (ZERO) vq = vqs[kk >> 1];
      else vq = scaled(kk);
      if constexpr (ZERO) {
        // (the negated compare: a NaN takes the full path, as its select does)
        const bool allz = !__any(!(fabsf(vq.x) < 0.58f) || !(fabsf(vq.y) < 0.58f));
        MZERO_COUNT(CH, allz);
        if (allz) {
          // every active lane of the wave (an invalid varblock's lanes have
          // left) quantizes both rows to 0: no rate, no non-zeros, sq = +-0
          // and vq - sq == vq (a -0 becomes +0: e * e is +0 for either)
          const f2 e = vq * f2{sd[kk], sd[kk + 1]};
          cp = fmaf(e.x, e.x, cp);
          cp = fmaf(e.y, e.y, cp);
          continue;
        }
      }
      float sqs[2], qfs[2];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const float vqh = h ? vq.y : vq.x;
        const float av = fabsf(vqh);
        // qa = (int)(min(av, 32767) + 0.5) as an integer-valued float (the
        // truncation of a positive value is its floor): no conversions
        // needed for the error and the rate
        qfs[h] = av < 0.58f ? 0.0f : floorf(fminf(av, 32767.0f) + 0.5f);
        sqs[h] = __builtin_copysignf(qfs[h], vqh);
      }
      if (CH == 1) {
        // AdjustQuantBias from the table below 256; one wave vote per row pair
        // for the (rare) larger magnitudes
        float adj[2];
#pragma unroll
        for (int h = 0; h < 2; h++) adj[h] = S.btab[min((int)qfs[h], 255)];
        if (__builtin_expect(__any(fmaxf(qfs[0], qfs[1]) >= 256.0f), 0)) {
#pragma unroll
          for (int h = 0; h < 2; h++)
            if (qfs[h] >= 256.0f) adj[h] = qfs[h] - 0.145f / qfs[h];
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
          // (vq = -0: a -0 that no result sees; jxg_front.hip)
          const float a1 = __builtin_copysignf(adj[h], h ? vq.y : vq.x);
          cplane[(ky + h) * kMS] = a1 * iw[kk + h];  // LLF: 0 (its value lives in WriteLds::llf)
        }
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const float qf = qfs[h];
        // 2 + 2 bitlen(qa) per non-zero = 2 E - 250, E = biased exponent of
        // qf (qf = 0 has E = 0 and is not counted in nzc)
        eb8[kk >= 8] += __float_as_uint(qf) >> 23;
        if constexpr (WRITE) {
          const int qq = (int)sqs[h];  // (vq < 0 ? -qa : qa)
          const int p = nat[kk + h];
          const int sl = p >> 6;
          // covered block sl of the slot's varblock, from its first block
          const size_t gb = (size_t)S.sgb[v] + (size_t)(sl >> P.lcx) * a.bxs + (sl & (P.cx() - 1));
          a.ac[(gb * 3 + CH) * 64 + (p & 63)] = (int16_t)qq;
        }
      }
      // error in steps times the distortion weight (oracle jxo_dist_weight);
      // the write pass needs no estimate
      // (the signed error: (vq - sq) sd = +-(|vq| - qf) sd exactly, the same
      // square; jxg_front.hip signed_err)
      if (!WRITE) {
        const f2 e = (vq - f2{sqs[0], sqs[1]}) * f2{sd[kk], sd[kk + 1]};
        cp = fmaf(e.x, e.x, cp);
        cp = fmaf(e.y, e.y, cp);
      }
    }
    const int nzc = (int)(eb8[0] / 127u) + (int)(eb8[1] / 127u);
    const int bits = 2 * (int)(eb8[0] + eb8[1]) - 250 * nzc;
    // the chunk's column partials, tree-summed over the varblock's C lanes
    // (an aligned group inside one wave); bits | non-zeros << 20 likewise
    int packed = bits | nzc << 20;
    group_all_reduce(cp, packed, C);
    if (x == 0) {
      S.qsum[cidx][ch][v] = cp;
      if (packed & 0xFFFFF) atomicAdd(&S.vbits[v], packed & 0xFFFFF);
      if (packed >> 20) atomicAdd(&S.vnz[v][CH], packed >> 20);
    }
  }
}
// AdjustQuantBias of q: 0 -> 0, 1 -> 1 - 0.0700..., else q - 0.145 / q (the
// per-coefficient expression, tabulated)
template <class L>
__device__ __forceinline__ void fill_btab(L& S) {
  for (int i = threadIdx.x; i < 256; i += kMThreads)
    S.btab[i] = i == 0 ? 0.0f : (i == 1 ? 1.0f - 0.07005449891748593f : (float)i - 0.145f / (float)i);
}
__device__ __forceinline__ int max_level(const MergeArgs& a) {
  return a.max_s >= 8 ? 3 : (a.max_s >= 4 ? 2 : 1);
}

}  // namespace jxg
