// jxg_lee.h -- Lee's recursive DCT-II in registers (device only): the 1-D
// transform of the merge stage (jxg_merge_kernel.h, up to 64 points) and of
// the 128 / 256 px levels' 32-point leaves (jxg_bigvb.hip).  Constants:
// jxg_lee_tables.h (generated).  Float op order == oracle/merge.c lee.
#pragma once
#include <hip/hip_runtime.h>

#include "jxg_lee_tables.h"

namespace jxg {

template <int N>
constexpr int ilog2c() {
  return N <= 1 ? 0 : 1 + ilog2c<N / 2>();
}

// Two independent transforms per lane: f2 holds the same element of two rows
// (or columns), so every butterfly is one packed op (v_pk_add_f32 /
// v_pk_mul_f32) with no operand shuffles; each half sees exactly the float ops
// of the scalar transform (no contraction), so results are bit-identical.
typedef float f2 __attribute__((ext_vector_type(2)));

// unnormalized DCT-II in registers, Lee's recursive even/odd split
// (== oracle/merge.c lee); T = float or f2
template <int N, class T>
__device__ __forceinline__ void lee(T* x) {
  if constexpr (N > 1) {
    constexpr int h = N / 2, l = ilog2c<N>();
    T a[h], b[h];
#pragma unroll
    for (int i = 0; i < h; i++) {
      a[i] = x[i] + x[N - 1 - i];
      b[i] = (x[i] - x[N - 1 - i]) * kLeeC[l][i];
    }
    lee<h>(a);
    lee<h>(b);
#pragma unroll
    for (int k = 0; k < h; k++) x[2 * k] = a[k];
#pragma unroll
    for (int k = 0; k < h - 1; k++) x[2 * k + 1] = b[k] + b[k + 1];
    x[N - 1] = b[h - 1];
  }
}
// half h of the normalized N-point DCT (Lee's first split: h = 0 the even
// outputs 2k from the sums, h = 1 the odd outputs 2k+1 from the scaled
// differences) -- the same float ops as lee<N>, spread over two lanes.
// dctN_first: t[i] from x[i] and its mirror x[N - 1 - i]; dctN_rest: the
// N/2-point transform of t and the output scaling, out(k, value) for output
// 2k + h.  T = f2: two independent rows / columns with the same h.
template <int N, class T>
__device__ __forceinline__ T dctN_first(T xi, T xm, int i, int h) {
  return h == 0 ? xi + xm : (xi - xm) * kLeeC[ilog2c<N>()][i];
}
template <int N, class T, class Out>
__device__ __forceinline__ void dctN_rest(T* t, int h, Out out) {
  constexpr int l = ilog2c<N>(), H = N / 2;
  lee<H>(t);
  if (h == 0) {
#pragma unroll
    for (int k = 0; k < H; k++) out(k, t[k] * kLeeS[l][2 * k]);
  } else {
#pragma unroll
    for (int k = 0; k < H - 1; k++) out(k, (t[k] + t[k + 1]) * kLeeS[l][2 * k + 1]);
    out(H - 1, t[H - 1] * kLeeS[l][N - 1]);
  }
}

}  // namespace jxg
