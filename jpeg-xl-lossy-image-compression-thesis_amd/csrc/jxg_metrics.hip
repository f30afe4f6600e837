// jxg_metrics.hip -- decode-side image quality on gfx950: the harness's
// MSE / PSNR (benchmark-jpegxl/src/image_reader.rs:555-606, metrics.rs:28-53)
// and SSIM (metrics.rs:55-84 shells out to ImageMagick `compare -metric SSIM`;
// restated here as the Gaussian-window SSIM of Wang et al., parity unpinned).
//
//   sse_kernel    sum over samples of (orig - comp)^2 as exact 64-bit
//                 integers.  The reference accumulates the same squares in
//                 f64 one sample at a time; every partial sum stays below
//                 2^53 (<= 65025 per sample), so the f64 sum is exact and
//                 equals this integer sum bit for bit, in any order.
//                 HBM-bound: 6 B read per pixel.
//   ssim_kernel   one 256-thread workgroup per (32 x 32 output tile, channel):
//                 the 42 x 42 input window of both images -> LDS, horizontal
//                 11-tap Gaussian sums of a, b, a^2, b^2, ab (f64, taps in
//                 ascending order) -> LDS, vertical sums (same order), the SSIM
//                 of every valid window centre, per-workgroup partial (fixed
//                 tree) -> partials[]; ssim_reduce_kernel sums the partials in
//                 a fixed order, so the result is deterministic.
//   ms_pyramid_kernel / ssim_cs_kernel / ms_reduce_kernel   MS-SSIM (Wang,
//                 Simoncelli, Bovik 2003): exact f32 box pyramids of both
//                 images, ssim_kernel's tiling per scale with the
//                 contrast-structure term beside the SSIM, one fixed-order
//                 reduction of the ten sums.
// Op order == oracle/metrics.py (no FMA contraction: -ffp-contract=off).
#include "jxg_kernels.h"

namespace jxg {

__constant__ double c_gauss[11];  // normalized exp(-(k-5)^2 / (2 * 1.5^2))

constexpr int kSsimT = 32;             // output tile edge
constexpr int kSsimIn = kSsimT + 10;   // input window edge (5 px halo)

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid-stride over rows; thread = 4-byte word of a row (byte tail: lane loop)
__global__ __launch_bounds__(256) void sse_kernel(MetricArgs a) {
  __shared__ uint64_t sW[4];
  const size_t rowb = (size_t)a.w * 3;
  uint64_t acc = 0;
  for (uint32_t y = blockIdx.x; y < a.h; y += gridDim.x) {
    const uint8_t* p = a.orig + (size_t)y * a.so;
    const uint8_t* q = a.comp + (size_t)y * a.sc;
    uint32_t racc = 0;  // <= ceil(rowb / 256) * 4 * 65025 < 2^32 for rows < 4 M samples
    const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & 3) == 0;
    const size_t nw = al ? rowb / 4 : 0;
    for (size_t i = threadIdx.x; i < nw; i += blockDim.x) {
      const uint32_t u = reinterpret_cast<const uint32_t*>(p)[i];
      const uint32_t v = reinterpret_cast<const uint32_t*>(q)[i];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int d = (int)((u >> (8 * k)) & 0xFF) - (int)((v >> (8 * k)) & 0xFF);
        racc += (uint32_t)(d * d);
      }
    }
    for (size_t i = nw * 4 + threadIdx.x; i < rowb; i += blockDim.x) {
      const int d = (int)p[i] - (int)q[i];
      racc += (uint32_t)(d * d);
    }
    acc += racc;
  }
  acc = wave_sum_u64(acc);
  if ((threadIdx.x & 63) == 0) sW[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.sse),
                                  (unsigned long long)(sW[0] + sW[1] + sW[2] + sW[3]));
}

__global__ __launch_bounds__(256) void ssim_kernel(MetricArgs a) {
  __shared__ float sA[kSsimIn][kSsimIn + 1], sB[kSsimIn][kSsimIn + 1];
  __shared__ double sH[5][kSsimIn][kSsimT];
  __shared__ double sRed[4];
  const int c = blockIdx.z;
  const int x0 = blockIdx.x * kSsimT, y0 = blockIdx.y * kSsimT;  // first window centre - 5
  const int t = threadIdx.x;
  for (int i = t; i < kSsimIn * kSsimIn; i += 256) {
    const int ly = i / kSsimIn, lx = i - ly * kSsimIn;
    const int gx = x0 + lx, gy = y0 + ly;
    float va = 0.0f, vb = 0.0f;
    if (gx < (int)a.w && gy < (int)a.h) {
      va = (float)a.orig[(size_t)gy * a.so + 3 * (size_t)gx + c];
      vb = (float)a.comp[(size_t)gy * a.sc + 3 * (size_t)gx + c];
    }
    sA[ly][lx] = va;
    sB[ly][lx] = vb;
  }
  __syncthreads();
  // horizontal: window centre column x0 + 5 + j, all 42 input rows
  for (int i = t; i < kSsimIn * kSsimT; i += 256) {
    const int ly = i / kSsimT, j = i - ly * kSsimT;
    double ha = 0.0, hb = 0.0, haa = 0.0, hbb = 0.0, hab = 0.0;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const double g = c_gauss[k];
      const double va = (double)sA[ly][j + k], vb = (double)sB[ly][j + k];
      ha = ha + g * va;
      hb = hb + g * vb;
      haa = haa + g * (va * va);
      hbb = hbb + g * (vb * vb);
      hab = hab + g * (va * vb);
    }
    sH[0][ly][j] = ha;
    sH[1][ly][j] = hb;
    sH[2][ly][j] = haa;
    sH[3][ly][j] = hbb;
    sH[4][ly][j] = hab;
  }
  __syncthreads();
  // vertical + SSIM: thread = (column j, 4 rows)
  const int j = t & 31, r0 = (t >> 5) * 4;
  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  double part = 0.0;
  for (int r = r0; r < r0 + 4; r++) {
    const int cx = x0 + 5 + j, cy = y0 + 5 + r;  // window centre
    if (cx + 5 >= (int)a.w || cy + 5 >= (int)a.h) continue;
    double m[5];
#pragma unroll
    for (int q = 0; q < 5; q++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 11; k++) s = s + c_gauss[k] * sH[q][r + k][j];
      m[q] = s;
    }
    const double mab = m[0] * m[1], maa = m[0] * m[0], mbb = m[1] * m[1];
    const double vaa = m[2] - maa, vbb = m[3] - mbb, cab = m[4] - mab;
    const double num = (2.0 * mab + C1) * (2.0 * cab + C2);
    const double den = (maa + mbb + C1) * (vaa + vbb + C2);
    part = part + num / den;
  }
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if ((t & 63) == 0) sRed[t >> 6] = part;
  __syncthreads();
  if (t == 0) {
    const uint32_t wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.partials[wg] = (sRed[0] + sRed[1]) + (sRed[2] + sRed[3]);
  }
}

// one workgroup: thread-strided partial sums in index order, then a fixed tree
__global__ __launch_bounds__(256) void ssim_reduce_kernel(const double* partials, uint32_t n,
                                                          double* out) {
  __shared__ double s[256];
  double v = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += 256) v = v + partials[i];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = s[0];
}

// ---- MS-SSIM ----
// Pyramid: one workgroup per 128 x 16 pixel tile (eight 16 x 16 blocks) reads
// the tile's RGB8 once -- 4-byte words where the row is aligned, bytes
// otherwise and in the tail -- and writes the tile's samples of all four
// levels.  A level-j sample is the sum of its 4^j pixels (an integer below
// 2^16) times 4^-j: exact in f32, and equal to the 2 x 2 means taken level by
// level in any order.  Sample (x, y) of level j exists when x < (w >> j) and
// y < (h >> j); its pixels are then all inside the image.
constexpr int kPyrW = 128, kPyrH = 16;
constexpr int kPyrWords = kPyrW * 3 / 4;  // per tile row
struct PyrArgs {
  const uint8_t* img;
  size_t stride;
  uint32_t w, h;
  float* lvl[4];  // planes [3][h >> j][w >> j] of level j = index + 1
};

__global__ __launch_bounds__(256) void ms_pyramid_kernel(PyrArgs a) {
  __shared__ uint32_t sPx[kPyrH][kPyrWords];
  __shared__ uint32_t sL1[3][8][64], sL2[3][4][32], sL3[3][2][16];
  const int t = threadIdx.x;
  const uint32_t x0 = blockIdx.x * kPyrW, y0 = blockIdx.y * kPyrH;
  const size_t left = ((size_t)a.w - x0) * 3;  // bytes of a row from x0 on (x0 < w)
  const uint32_t nb = left < (size_t)kPyrW * 3 ? (uint32_t)left : (uint32_t)kPyrW * 3;
  for (int i = t; i < kPyrH * kPyrWords; i += 256) {
    const int ly = i / kPyrWords, wi = i - ly * kPyrWords;
    uint32_t v = 0;
    if (y0 + ly < a.h) {
      const uint8_t* p = a.img + (size_t)(y0 + ly) * a.stride + (size_t)x0 * 3;
      if ((reinterpret_cast<uintptr_t>(p) & 3) == 0 && 4u * wi + 4u <= nb) {
        v = reinterpret_cast<const uint32_t*>(p)[wi];
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
          if (4u * wi + k < nb) v |= (uint32_t)p[4u * wi + k] << (8 * k);
      }
    }
    sPx[ly][wi] = v;
  }
  __syncthreads();
  const uint8_t* px = reinterpret_cast<const uint8_t*>(&sPx[0][0]);
  {
    const uint32_t wl = a.w >> 1, hl = a.h >> 1;
    for (int i = t; i < 3 * 8 * 64; i += 256) {
      const int c = i >> 9, r = (i >> 6) & 7, x = i & 63;
      const uint8_t* q = px + (2 * r) * (kPyrW * 3) + (2 * x) * 3 + c;
      const uint32_t sum = ((uint32_t)q[0] + q[3]) + ((uint32_t)q[kPyrW * 3] + q[kPyrW * 3 + 3]);
      sL1[c][r][x] = sum;
      const uint32_t gx = (x0 >> 1) + x, gy = (y0 >> 1) + r;
      if (gx < wl && gy < hl) a.lvl[0][((size_t)c * hl + gy) * wl + gx] = (float)sum * 0.25f;
    }
  }
  __syncthreads();
  {
    const uint32_t wl = a.w >> 2, hl = a.h >> 2;
    for (int i = t; i < 3 * 4 * 32; i += 256) {
      const int c = i >> 7, r = (i >> 5) & 3, x = i & 31;
      const uint32_t sum = (sL1[c][2 * r][2 * x] + sL1[c][2 * r][2 * x + 1]) +
                           (sL1[c][2 * r + 1][2 * x] + sL1[c][2 * r + 1][2 * x + 1]);
      sL2[c][r][x] = sum;
      const uint32_t gx = (x0 >> 2) + x, gy = (y0 >> 2) + r;
      if (gx < wl && gy < hl) a.lvl[1][((size_t)c * hl + gy) * wl + gx] = (float)sum * 0.0625f;
    }
  }
  __syncthreads();
  if (t < 3 * 2 * 16) {
    const uint32_t wl = a.w >> 3, hl = a.h >> 3;
    const int c = t >> 5, r = (t >> 4) & 1, x = t & 15;
    const uint32_t sum = (sL2[c][2 * r][2 * x] + sL2[c][2 * r][2 * x + 1]) +
                         (sL2[c][2 * r + 1][2 * x] + sL2[c][2 * r + 1][2 * x + 1]);
    sL3[c][r][x] = sum;
    const uint32_t gx = (x0 >> 3) + x, gy = (y0 >> 3) + r;
    if (gx < wl && gy < hl) a.lvl[2][((size_t)c * hl + gy) * wl + gx] = (float)sum * 0.015625f;
  }
  __syncthreads();
  if (t < 3 * 8) {
    const uint32_t wl = a.w >> 4, hl = a.h >> 4;
    const int c = t >> 3, x = t & 7;
    const uint32_t sum = (sL3[c][0][2 * x] + sL3[c][0][2 * x + 1]) +
                         (sL3[c][1][2 * x] + sL3[c][1][2 * x + 1]);
    const uint32_t gx = (x0 >> 4) + x, gy = y0 >> 4;
    if (gx < wl && gy < hl) a.lvl[3][((size_t)c * hl + gy) * wl + gx] = (float)sum * 0.00390625f;
  }
}

// One scale: ssim_kernel's tiling, window, taps and expressions on either
// input (kF32: planes [3][h][w] of floats, rows of sa / sb floats; otherwise
// RGB8 interleaved rows of sa / sb bytes), plus the contrast-structure term;
// two per-workgroup partials.  The ssim partial of the RGB8 instantiation is
// ssim_kernel's, bit for bit.
struct MsScaleArgs {
  const void* a;
  const void* b;
  size_t sa, sb;
  uint32_t w, h;
  double* part_ssim;
  double* part_cs;
};

template <bool kF32>
__global__ __launch_bounds__(256) void ssim_cs_kernel(MsScaleArgs a) {
  __shared__ float sA[kSsimIn][kSsimIn + 1], sB[kSsimIn][kSsimIn + 1];
  __shared__ double sH[5][kSsimIn][kSsimT];
  __shared__ double sRed[2][4];
  const int c = blockIdx.z;
  const int x0 = blockIdx.x * kSsimT, y0 = blockIdx.y * kSsimT;  // first window centre - 5
  const int t = threadIdx.x;
  for (int i = t; i < kSsimIn * kSsimIn; i += 256) {
    const int ly = i / kSsimIn, lx = i - ly * kSsimIn;
    const int gx = x0 + lx, gy = y0 + ly;
    float va = 0.0f, vb = 0.0f;
    if (gx < (int)a.w && gy < (int)a.h) {
      if constexpr (kF32) {
        va = static_cast<const float*>(a.a)[((size_t)c * a.h + gy) * a.sa + gx];
        vb = static_cast<const float*>(a.b)[((size_t)c * a.h + gy) * a.sb + gx];
      } else {
        va = (float)static_cast<const uint8_t*>(a.a)[(size_t)gy * a.sa + 3 * (size_t)gx + c];
        vb = (float)static_cast<const uint8_t*>(a.b)[(size_t)gy * a.sb + 3 * (size_t)gx + c];
      }
    }
    sA[ly][lx] = va;
    sB[ly][lx] = vb;
  }
  __syncthreads();
  for (int i = t; i < kSsimIn * kSsimT; i += 256) {
    const int ly = i / kSsimT, j = i - ly * kSsimT;
    double ha = 0.0, hb = 0.0, haa = 0.0, hbb = 0.0, hab = 0.0;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const double g = c_gauss[k];
      const double va = (double)sA[ly][j + k], vb = (double)sB[ly][j + k];
      ha = ha + g * va;
      hb = hb + g * vb;
      haa = haa + g * (va * va);
      hbb = hbb + g * (vb * vb);
      hab = hab + g * (va * vb);
    }
    sH[0][ly][j] = ha;
    sH[1][ly][j] = hb;
    sH[2][ly][j] = haa;
    sH[3][ly][j] = hbb;
    sH[4][ly][j] = hab;
  }
  __syncthreads();
  const int j = t & 31, r0 = (t >> 5) * 4;
  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  double part = 0.0, pcs = 0.0;
  for (int r = r0; r < r0 + 4; r++) {
    const int cx = x0 + 5 + j, cy = y0 + 5 + r;  // window centre
    if (cx + 5 >= (int)a.w || cy + 5 >= (int)a.h) continue;
    double m[5];
#pragma unroll
    for (int q = 0; q < 5; q++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 11; k++) s = s + c_gauss[k] * sH[q][r + k][j];
      m[q] = s;
    }
    const double mab = m[0] * m[1], maa = m[0] * m[0], mbb = m[1] * m[1];
    const double vaa = m[2] - maa, vbb = m[3] - mbb, cab = m[4] - mab;
    const double num = (2.0 * mab + C1) * (2.0 * cab + C2);
    const double den = (maa + mbb + C1) * (vaa + vbb + C2);
    part = part + num / den;
    pcs = pcs + (2.0 * cab + C2) / (vaa + vbb + C2);
  }
  for (int o = 32; o > 0; o >>= 1) {
    part += __shfl_xor(part, o, 64);
    pcs += __shfl_xor(pcs, o, 64);
  }
  if ((t & 63) == 0) {
    sRed[0][t >> 6] = part;
    sRed[1][t >> 6] = pcs;
  }
  __syncthreads();
  if (t == 0) {
    const uint32_t wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.part_ssim[wg] = (sRed[0][0] + sRed[0][1]) + (sRed[0][2] + sRed[0][3]);
    a.part_cs[wg] = (sRed[1][0] + sRed[1][1]) + (sRed[1][2] + sRed[1][3]);
  }
}

// ssim_reduce_kernel for the ten sums of one MS-SSIM: workgroup b reduces
// part[off[b] .. off[b] + n[b]) in that kernel's order into out[b]
struct MsReduceArgs {
  const double* part;
  uint32_t off[2 * kMsScales], n[2 * kMsScales];
  double* out;
};

__global__ __launch_bounds__(256) void ms_reduce_kernel(MsReduceArgs a) {
  __shared__ double s[256];
  const double* partials = a.part + a.off[blockIdx.x];
  const uint32_t n = a.n[blockIdx.x];
  double v = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += 256) v = v + partials[i];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.out[blockIdx.x] = s[0];
}

uint32_t ssim_partials(uint32_t w, uint32_t h) {
  if (w < 11 || h < 11) return 0;
  const uint32_t tx = (w - 10 + kSsimT - 1) / kSsimT, ty = (h - 10 + kSsimT - 1) / kSsimT;
  return tx * ty * 3;
}

hipError_t set_gauss_table(const double* g, hipStream_t s) {
  return hipMemcpyToSymbolAsync(HIP_SYMBOL(c_gauss), g, 11 * sizeof(double), 0,
                                hipMemcpyHostToDevice, s);
}

void launch_ssim(const MetricArgs& a, hipStream_t s) {
  if (a.ssim && a.w >= 11 && a.h >= 11) {
    const uint32_t tx = (a.w - 10 + kSsimT - 1) / kSsimT, ty = (a.h - 10 + kSsimT - 1) / kSsimT;
    hipLaunchKernelGGL(ssim_kernel, dim3(tx, ty, 3), dim3(256), 0, s, a);
    hipLaunchKernelGGL(ssim_reduce_kernel, dim3(1), dim3(256), 0, s, a.partials, tx * ty * 3,
                       a.ssim);
  }
}

void launch_metrics(const MetricArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(sse_kernel, dim3(a.h < 2048 ? a.h : 2048), dim3(256), 0, s, a);
  launch_ssim(a, s);
}

size_t ms_level_offset(uint32_t w, uint32_t h, int j) {
  size_t o = 0;
  for (int k = 1; k < j; k++) o += (size_t)3 * (w >> k) * (h >> k);
  return o;
}

size_t ms_pyramid_floats(uint32_t w, uint32_t h) { return ms_level_offset(w, h, kMsScales); }

// [scale][ssim | cs][workgroup]; sums 0 .. 4: ssim, 5 .. 9: cs
static uint32_t ms_layout(uint32_t w, uint32_t h, uint32_t* off, uint32_t* n) {
  uint32_t o = 0;
  for (int j = 0; j < kMsScales; j++) {
    const uint32_t np = ssim_partials(w >> j, h >> j);
    if (off) {
      off[j] = o;
      off[kMsScales + j] = o + np;
      n[j] = n[kMsScales + j] = np;
    }
    o += 2 * np;
  }
  return o;
}

uint32_t ms_partials(uint32_t w, uint32_t h) { return ms_layout(w, h, nullptr, nullptr); }

void launch_ms_pyramid(const uint8_t* img, size_t stride, uint32_t w, uint32_t h, float* pyr,
                       hipStream_t s) {
  PyrArgs a{img, stride, w, h, {}};
  for (int j = 1; j < kMsScales; j++) a.lvl[j - 1] = pyr + ms_level_offset(w, h, j);
  hipLaunchKernelGGL(ms_pyramid_kernel, dim3((w + kPyrW - 1) / kPyrW, (h + kPyrH - 1) / kPyrH),
                     dim3(256), 0, s, a);
}

void launch_msssim(const MsArgs& a, hipStream_t s) {
  MsReduceArgs r{};
  ms_layout(a.w, a.h, r.off, r.n);
  r.part = a.partials;
  r.out = a.out;
  for (int j = 0; j < kMsScales; j++) {
    const uint32_t w = a.w >> j, h = a.h >> j;
    const dim3 grid((w - 10 + kSsimT - 1) / kSsimT, (h - 10 + kSsimT - 1) / kSsimT, 3);
    double* ps = a.partials + r.off[j];
    double* pc = a.partials + r.off[kMsScales + j];
    if (j == 0) {
      const MsScaleArgs k{a.orig, a.comp, a.so, a.sc, w, h, ps, pc};
      hipLaunchKernelGGL(ssim_cs_kernel<false>, grid, dim3(256), 0, s, k);
    } else {
      const size_t o = ms_level_offset(a.w, a.h, j);
      const MsScaleArgs k{a.pyr_o + o, a.pyr_c + o, w, w, w, h, ps, pc};
      hipLaunchKernelGGL(ssim_cs_kernel<true>, grid, dim3(256), 0, s, k);
    }
  }
  hipLaunchKernelGGL(ms_reduce_kernel, dim3(2 * kMsScales), dim3(256), 0, s, r);
}

}  // namespace jxg
