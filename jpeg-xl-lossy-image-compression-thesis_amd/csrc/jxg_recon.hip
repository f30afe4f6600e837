// jxg_recon.hip -- decode-side reconstruction on gfx950: the image a decoder
// rebuilds from the frame this context encoded, computed from the quantized
// coefficients still in device memory (no bitstream parse).  f32 restatement
// of oracle/jxl_decode.py reconstruct() [ext: libjxl's decoder, parity with
// djxl unpinned]; DESIGN.md §3.11.
//
//   recon_tile_kernel    one 1024-thread workgroup per 64x64 tile; the tile's
//                        X, Y, B coefficient planes and a second set for the
//                        separable passes in LDS (6 x 64 x 65 f32 = 97.5 KB).
//                        Dequantization (AdjustQuantBias, inverse weights,
//                        chroma from luma) scatters the natural-order slices
//                        to coefficient positions; the LLF corner of merged
//                        varblocks is rebuilt from the covered blocks' DCs;
//                        inverse transforms are plain products against cosine
//                        tables (column pass, row pass), the 4x4 / 4x8 / 2x2 /
//                        identity blocks one thread per (block, channel).
//                        Lanes always run along x, so every pass reads LDS
//                        rows at consecutive or equal addresses.  Writes the
//                        planes, or RGB8 directly when no filter follows.
//                        Varblocks of 128 / 256 px are listed for
//   recon_big_kernel     one workgroup per listed varblock, planes in global
//                        memory (its own area of the two plane sets), tables
//                        in global memory.  Not tuned (rare, effort >= 8).
//   recon_gab_kernel     decoder Gaborish (3x3, edge-repeating).
//   recon_epf_kernel     one EPF pass over a 64x16 tile with a 3 px halo in LDS.
//   recon_colour_kernel  XYB -> sRGB8 alone (128 / 256 px varblocks, no filter).
//   recon_colour_sse_kernel  the same conversion fused with the squared error
//                        against the original (jxg_sweep_rgb8); stores RGB8
//                        only for SSIM.
//   recon_colour_sse_map_kernel  the same, and one squared-error word per 8x8
//                        block (the strategy report).
// The last kernel of the chain writes RGB8 cropped to the image size.
#include <algorithm>

#include "jxg_kernels.h"

namespace jxg {

constexpr int kRT = 1024;       // recon_tile_kernel threads
constexpr int kRS = 65;         // LDS row stride of a 64-wide tile row
constexpr int kRP = 64 * kRS;   // floats of one LDS plane
constexpr int kRB = 512;        // recon_big_kernel threads

// raw strategy id -> blocks down, blocks across, weight kind (0xFF: 8x8 class)
// (the host twin initialises the device table, so that its first two columns
// can be checked against strategy_shape where they are typed)
struct RcShapes {
  uint8_t v[27][3];
};
constexpr RcShapes kRcShapes = {{
    {1, 1, 0xFF}, {1, 1, 0xFF}, {1, 1, 0xFF}, {1, 1, 0xFF}, {2, 2, 1},     {4, 4, 3},    {2, 1, 0},
    {1, 2, 0},    {0, 0, 0xFF}, {0, 0, 0xFF}, {4, 2, 2},    {2, 4, 2},     {1, 1, 0xFF}, {1, 1, 0xFF},
    {0, 0, 0xFF}, {0, 0, 0xFF}, {0, 0, 0xFF}, {0, 0, 0xFF}, {8, 8, 5},     {8, 4, 4},    {4, 8, 4},
    {16, 16, 7},  {16, 8, 6},   {8, 16, 6},   {32, 32, 9},  {32, 16, 8},   {16, 32, 8}}};
constexpr bool rc_shapes_are_the_models() {
  for (uint32_t t = 0; t < 27; t++)
    if ((kRcShapes.v[t][0] | kRcShapes.v[t][1] << 8) != (int)strategy_shape(t)) return false;
  return true;
}
static_assert(rc_shapes_are_the_models(), "c_rc_shape's blocks down / across restate strategy_shape");
__constant__ RcShapes c_rc_shape = kRcShapes;
__constant__ int c_rc_koff[10] = {0, 128, 384, 896, 1920, 3968, 8064, 16256, 32640, 65408};
// raw id of the 8x8 class -> weight table of kRcTabW8 (DCT8, DCT4X4, DCT4X8 /
// DCT8X4, IDENTITY, DCT2X2)
__device__ __forceinline__ int rc_w8_kind(int t) {
  return t == 0 ? 0 : t == 3 ? 1 : t == 1 ? 3 : t == 2 ? 4 : 2;
}
__device__ __forceinline__ int rc_log2(int n) { return 31 - __clz(n); }

__device__ __forceinline__ float rc_adjust(int q, float b1, float b3) {
  if (q == 0) return 0.0f;
  if (q == 1) return b1;
  if (q == -1) return -b1;
  return (float)q - b3 / (float)q;
}

// XYB -> sRGB8 of one pixel (oracle/jxl_decode.py xyb_to_srgb8): the one
// conversion of every kernel that ends a chain
__device__ __forceinline__ void rc_xyb_to_rgb8(const ReconArgs& a, float X, float Y, float B,
                                               uint8_t out[3]) {
  const float L = (Y + X) + a.cbias, M = (Y - X) + a.cbias, S = B + a.cbias;
  const float m0 = L * L * L - a.obias, m1 = M * M * M - a.obias, m2 = S * S * S - a.obias;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float v = (m0 * a.cm[c * 3] + m1 * a.cm[c * 3 + 1]) + m2 * a.cm[c * 3 + 2];
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    v = v <= 0.0031308f ? v * 12.92f : 1.055f * powf(v, 1.0f / 2.4f) - 0.055f;
    v = floorf(v * 255.0f + 0.5f);
    out[c] = (uint8_t)fminf(fmaxf(v, 0.0f), 255.0f);
  }
}
__device__ __forceinline__ void rc_store_rgb(const ReconArgs& a, uint32_t gx, uint32_t gy, float X,
                                             float Y, float B) {
  uint8_t v[3];
  rc_xyb_to_rgb8(a, X, Y, B, v);
  uint8_t* o = a.rgb + (size_t)gy * a.stride + (size_t)gx * 3;
  o[0] = v[0];
  o[1] = v[1];
  o[2] = v[2];
}

template <bool kToRgb>
__global__ __launch_bounds__(kRT) void recon_tile_kernel(ReconArgs a) {
  __shared__ float sC[3 * kRP];   // coefficients, then pixels
  __shared__ float sT[3 * kRP];   // after the column pass
  __shared__ uint8_t sHead[64];   // block -> its varblock's first block in the tile (0xFF: none here)
  __shared__ uint8_t sType[64];   // raw id at first blocks
  const int tid = threadIdx.x;
  const uint32_t tx = blockIdx.x, ty = blockIdx.y;
  const uint32_t bx0 = tx * 8, by0 = ty * 8;
  const size_t nb = (size_t)a.bxs * a.bys;
  const float* tab = a.tab;

  if (tid < 64) {
    sHead[tid] = 0xFF;
    sType[tid] = 0xFF;
  }
  __syncthreads();
  if (tid < 64) {
    const uint32_t bx = bx0 + (tid & 7), by = by0 + (tid >> 3);
    if (bx < a.bxs && by < a.bys) {
      const int raw = a.acs[(size_t)by * a.bxs + bx];
      if (!(raw & 0x80) && raw < 27) {
        const int cy = c_rc_shape.v[raw][0], cx = c_rc_shape.v[raw][1];
        if (raw >= 21) {  // 128 / 256 px: recon_big_kernel
          const uint32_t i = atomicAdd(a.biglist, 1u);
          if (i < a.bigcap) a.biglist[1 + i] = by * a.bxs + bx;
        } else if (cy && (tid & 7) + cx <= 8 && (tid >> 3) + cy <= 8) {
          sType[tid] = (uint8_t)raw;
          for (int iy = 0; iy < cy; iy++)
            for (int ix = 0; ix < cx; ix++) sHead[tid + iy * 8 + ix] = (uint8_t)tid;
        }
      }
    }
  }
  __syncthreads();

  // chroma from luma of the tile
  const float cfx = (float)a.cmap[(size_t)ty * a.tiles_x + tx] * (1.0f / 84.0f);
  const float cfb =
      1.0f + (float)a.cmap[(size_t)a.ntiles_all + (size_t)ty * a.tiles_x + tx] * (1.0f / 84.0f);

  // dequantization: slice sample (block b, k) -> its coefficient position
  for (int e = tid; e < 4096; e += kRT) {
    const int b = e >> 6, k = e & 63;
    const int hb = sHead[b];
    if (hb == 0xFF) continue;
    const int t = sType[hb];
    const int hx = hb & 7, hy = hb >> 3;
    const int cy = c_rc_shape.v[t][0], cx = c_rc_shape.v[t][1], kind = c_rc_shape.v[t][2];
    int ky, kx;
    float wx, wy, wb;
    if (kind == 0xFF) {
      if (k == 0) continue;  // the DC slot
      const int r = a.pos[k];
      ky = r >> 3;
      kx = r & 7;
      const float* w8 = tab + kRcTabW8 + rc_w8_kind(t) * 192;
      wx = w8[k];
      wy = w8[64 + k];
      wb = w8[128 + k];
    } else {
      const int p = (((b >> 3) - hy) * cx + ((b & 7) - hx)) * 64 + k;
      if (p < cy * cx) continue;  // LLF slots: rebuilt from the DCs below
      const int st = a.pos[kRcPosKinds + c_rc_koff[kind] + p];
      const int lc = 3 + rc_log2(cx > cy ? cx : cy);  // log2 of the stored columns
      const int sy = st >> lc, sx = st & ((1 << lc) - 1);
      ky = cx >= cy ? sy : sx;
      kx = cx >= cy ? sx : sy;
      const float* iw = tab + kRcTabIw + c_rc_koff[kind] + p;
      wx = iw[0];
      wy = iw[kRcKindOff[10]];
      wb = iw[2 * kRcKindOff[10]];
    }
    const size_t gb = (size_t)(by0 + (b >> 3)) * a.bxs + bx0 + (b & 7);
    const size_t gh = (size_t)(by0 + hy) * a.bxs + bx0 + hx;
    const float sc = a.inv_g / (float)((int)a.qf[gh] + 1);
    const int16_t* q = a.ac + gb * 192 + k;
    const float vy = (rc_adjust(q[64], a.bias[1], a.bias[3]) * wy) * sc;
    const float vx = ((rc_adjust(q[0], a.bias[0], a.bias[3]) * wx) * sc) * a.xmul + cfx * vy;
    const float vb = ((rc_adjust(q[128], a.bias[2], a.bias[3]) * wb) * sc) * a.bmul + cfb * vy;
    const int o = (hy * 8 + ky) * kRS + hx * 8 + kx;
    sC[o] = vx;
    sC[kRP + o] = vy;
    sC[2 * kRP + o] = vb;
  }
  // DC of the 8x8 class; LLF corner of merged varblocks (the covered block
  // (iy, ix) computes LLF coefficient (iy, ix))
  for (int e = tid; e < 192; e += kRT) {
    const int b = e & 63, c = e >> 6;
    const int hb = sHead[b];
    if (hb == 0xFF) continue;
    const int t = sType[hb];
    const int hx = hb & 7, hy = hb >> 3;
    const int cy = c_rc_shape.v[t][0], cx = c_rc_shape.v[t][1];
    const int ky = (b >> 3) - hy, kx = (b & 7) - hx;
    const float* fy = tab + kRcTabFwd + rc_fwd_off(rc_log2(cy)) + ky * cy;
    const float* fx = tab + kRcTabFwd + rc_fwd_off(rc_log2(cx)) + kx * cx;
    const size_t gh = (size_t)(by0 + hy) * a.bxs + bx0 + hx;
    float acc = 0.0f;
    for (int jy = 0; jy < cy; jy++) {
      float u = 0.0f;
      for (int jx = 0; jx < cx; jx++) {
        const size_t g = gh + (size_t)jy * a.bxs + jx;
        float d = (float)a.dc[(size_t)c * nb + g] * a.dc_step[c];
        if (c == 2) d += (float)a.dc[nb + g] * a.dc_step[1];
        u += d * fx[jx];
      }
      acc += u * fy[jy];
    }
    sC[c * kRP + (hy * 8 + ky) * kRS + hx * 8 + kx] = acc;
  }
  __syncthreads();

  // column pass of DCT8 and the merged shapes: sT(y, x) = sum_k I_R[y][k] sC(k, x)
  for (int e = tid; e < 3 * 4096; e += kRT) {
    const int c = e >> 12, y = (e >> 6) & 63, x = e & 63;
    const int hb = sHead[(y >> 3) * 8 + (x >> 3)];
    if (hb == 0xFF) continue;
    const int t = sType[hb];
    if (t == 1 || t == 2 || t == 3 || t == 12 || t == 13) continue;
    const int R = 8 * c_rc_shape.v[t][0];
    const int y0 = (hb >> 3) * 8;
    const float* m = tab + kRcTabIdct + rc_idct_off(rc_log2(R)) + (y - y0);
    const float* src = sC + c * kRP + y0 * kRS + x;
    float acc = 0.0f;
    for (int k = 0; k < R; k++) acc += m[k * R] * src[k * kRS];
    sT[c * kRP + y * kRS + x] = acc;
  }
  // the other 8x8 strategies, one thread per (block, channel), in place
  // (oracle/jxl_decode.py inverse_transform); sT's block area is scratch
  if (tid < 192) {
    const int b = tid & 63, c = tid >> 6;
    const int t = sHead[b] == b ? sType[b] : 0xFF;
    float* S = sC + c * kRP + (b >> 3) * 8 * kRS + (b & 7) * 8;
    float* T = sT + c * kRP + (b >> 3) * 8 * kRS + (b & 7) * 8;
    const float* i4 = tab + kRcTabIdct + rc_idct_off(2);
    const float* i8 = tab + kRcTabIdct + rc_idct_off(3);
    if (t == 3 || t == 1) {
      const float A = S[0], B = S[1], C = S[kRS], D = S[kRS + 1];
      const float d0 = A + B + C + D, d1 = A + B - C - D, d2 = A - B + C - D, d3 = A - B - C + D;
      if (t == 3) {  // DCT4X4: four interleaved 4x4 blocks, their DCs from the 2x2 corner
        S[0] = d0;
        S[1] = d1;
        S[kRS] = d2;
        S[kRS + 1] = d3;
        _Pragma("nounroll") for (int sy = 0; sy < 2; sy++)
          _Pragma("nounroll") for (int sx = 0; sx < 2; sx++)
            _Pragma("nounroll") for (int iy = 0; iy < 4; iy++)
              _Pragma("nounroll") for (int x = 0; x < 4; x++) {
                float acc = 0.0f;
                _Pragma("nounroll") for (int ix = 0; ix < 4; ix++) acc += S[(sy + 2 * iy) * kRS + sx + 2 * ix] * i4[ix * 4 + x];
                T[(4 * sy + iy) * kRS + 4 * sx + x] = acc;
              }
        _Pragma("nounroll") for (int sy = 0; sy < 2; sy++)
          _Pragma("nounroll") for (int y = 0; y < 4; y++)
            _Pragma("nounroll") for (int x = 0; x < 8; x++) {
              float acc = 0.0f;
              _Pragma("nounroll") for (int iy = 0; iy < 4; iy++) acc += i4[iy * 4 + y] * T[(4 * sy + iy) * kRS + x];
              S[(4 * sy + y) * kRS + x] = acc;
            }
      } else {  // IDENTITY
        const float dcs[4] = {d0, d1, d2, d3};
        _Pragma("nounroll") for (int sy = 0; sy < 2; sy++)
          _Pragma("nounroll") for (int sx = 0; sx < 2; sx++) {
            float sum = 0.0f;
            _Pragma("nounroll") for (int iy = 0; iy < 4; iy++)
              _Pragma("nounroll") for (int ix = 0; ix < 4; ix++) sum += S[(sy + 2 * iy) * kRS + sx + 2 * ix];
            const float r00 = S[sy * kRS + sx], r11 = S[(sy + 2) * kRS + sx + 2];
            const float p11 = dcs[sy * 2 + sx] - (sum - r00) / 16.0f;
            _Pragma("nounroll") for (int iy = 0; iy < 4; iy++)
              _Pragma("nounroll") for (int ix = 0; ix < 4; ix++)
                T[(4 * sy + iy) * kRS + 4 * sx + ix] = S[(sy + 2 * iy) * kRS + sx + 2 * ix] + p11;
            T[(4 * sy + 1) * kRS + 4 * sx + 1] = p11;
            T[(4 * sy) * kRS + 4 * sx] = r11 + p11;
          }
        _Pragma("nounroll") for (int y = 0; y < 8; y++)
          _Pragma("nounroll") for (int x = 0; x < 8; x++) S[y * kRS + x] = T[y * kRS + x];
      }
    } else if (t == 2) {  // DCT2X2: inverse 2x2 Haar steps over 2, 4, 8
      _Pragma("nounroll") for (int n = 1; n <= 4; n *= 2) {
        _Pragma("nounroll") for (int y = 0; y < n; y++)
          _Pragma("nounroll") for (int x = 0; x < n; x++) {
            const float c00 = S[y * kRS + x], c01 = S[y * kRS + n + x];
            const float c10 = S[(n + y) * kRS + x], c11 = S[(n + y) * kRS + n + x];
            T[(2 * y) * kRS + 2 * x] = c00 + c01 + c10 + c11;
            T[(2 * y) * kRS + 2 * x + 1] = c00 + c01 - c10 - c11;
            T[(2 * y + 1) * kRS + 2 * x] = c00 - c01 + c10 - c11;
            T[(2 * y + 1) * kRS + 2 * x + 1] = c00 - c01 - c10 + c11;
          }
        _Pragma("nounroll") for (int y = 0; y < 2 * n; y++)
          _Pragma("nounroll") for (int x = 0; x < 2 * n; x++) S[y * kRS + x] = T[y * kRS + x];
      }
    } else if (t == 12 || t == 13) {
      const float d0 = S[0], d1 = S[kRS];
      S[0] = d0 + d1;
      S[kRS] = d0 - d1;
      if (t == 13) {  // DCT8X4: two 4 (rows) x 8 halves stacked, rows interleaved
        _Pragma("nounroll") for (int sy = 0; sy < 2; sy++)
          _Pragma("nounroll") for (int iy = 0; iy < 4; iy++)
            _Pragma("nounroll") for (int x = 0; x < 8; x++) {
              float acc = 0.0f;
              _Pragma("nounroll") for (int k = 0; k < 8; k++) acc += S[(sy + 2 * iy) * kRS + k] * i8[k * 8 + x];
              T[(4 * sy + iy) * kRS + x] = acc;
            }
        _Pragma("nounroll") for (int sy = 0; sy < 2; sy++)
          _Pragma("nounroll") for (int y = 0; y < 4; y++)
            _Pragma("nounroll") for (int x = 0; x < 8; x++) {
              float acc = 0.0f;
              _Pragma("nounroll") for (int iy = 0; iy < 4; iy++) acc += i4[iy * 4 + y] * T[(4 * sy + iy) * kRS + x];
              S[(4 * sy + y) * kRS + x] = acc;
            }
      } else {  // DCT4X8: two 8 x 4 halves side by side, coefficients transposed
        _Pragma("nounroll") for (int sx = 0; sx < 2; sx++)
          _Pragma("nounroll") for (int cx = 0; cx < 4; cx++)
            _Pragma("nounroll") for (int y = 0; y < 8; y++) {
              float acc = 0.0f;
              _Pragma("nounroll") for (int k = 0; k < 8; k++) acc += i8[k * 8 + y] * S[(sx + 2 * cx) * kRS + k];
              T[y * kRS + 4 * sx + cx] = acc;
            }
        _Pragma("nounroll") for (int sx = 0; sx < 2; sx++)
          _Pragma("nounroll") for (int y = 0; y < 8; y++)
            _Pragma("nounroll") for (int x = 0; x < 4; x++) {
              float acc = 0.0f;
              _Pragma("nounroll") for (int cx = 0; cx < 4; cx++) acc += T[y * kRS + 4 * sx + cx] * i4[cx * 4 + x];
              S[y * kRS + 4 * sx + x] = acc;
            }
      }
    }
  }
  __syncthreads();
  // row pass: sC(y, x) = sum_k sT(y, k) I_C[x][k]
  for (int e = tid; e < 3 * 4096; e += kRT) {
    const int c = e >> 12, y = (e >> 6) & 63, x = e & 63;
    const int hb = sHead[(y >> 3) * 8 + (x >> 3)];
    if (hb == 0xFF) continue;
    const int t = sType[hb];
    if (t == 1 || t == 2 || t == 3 || t == 12 || t == 13) continue;
    const int C = 8 * c_rc_shape.v[t][1];
    const int x0 = (hb & 7) * 8;
    const float* m = tab + kRcTabIdct + rc_idct_off(rc_log2(C)) + (x - x0);
    const float* src = sT + c * kRP + y * kRS + x0;
    float acc = 0.0f;
    for (int k = 0; k < C; k++) acc += src[k] * m[k * C];
    sC[c * kRP + y * kRS + x] = acc;
  }
  __syncthreads();
  // pixels out
  const size_t plane = (size_t)a.xp * a.yp;
  for (int e = tid; e < 4096; e += kRT) {
    const int y = e >> 6, x = e & 63;
    if (sHead[(y >> 3) * 8 + (x >> 3)] == 0xFF) continue;
    const uint32_t gx = bx0 * 8 + x, gy = by0 * 8 + y;
    const int o = y * kRS + x;
    if (kToRgb) {
      if (gx < a.w && gy < a.h) rc_store_rgb(a, gx, gy, sC[o], sC[kRP + o], sC[2 * kRP + o]);
    } else {
      const size_t g = (size_t)gy * a.xp + gx;
      a.pa[g] = sC[o];
      a.pa[plane + g] = sC[kRP + o];
      a.pa[2 * plane + g] = sC[2 * kRP + o];
    }
  }
}

// one varblock of 128 / 256 px per workgroup: coefficients -> its area of
// plane set pa, column pass -> pb, row pass -> pa
__global__ __launch_bounds__(kRB) void recon_big_kernel(ReconArgs a) {
  __shared__ float sD[32 * 33], sU[32 * 33];
  const int tid = threadIdx.x;
  const uint32_t count = min(a.biglist[0], a.bigcap);
  if (blockIdx.x >= count) return;
  const uint32_t gh = a.biglist[1 + blockIdx.x];
  const uint32_t bx = gh % a.bxs, by = gh / a.bxs;
  const int t = a.acs[gh];
  if (t < 21 || t > 26) return;
  const int cy = c_rc_shape.v[t][0], cx = c_rc_shape.v[t][1], kind = c_rc_shape.v[t][2];
  if (bx + cx > a.bxs || by + cy > a.bys) return;
  const int R = 8 * cy, C = 8 * cx;
  const int lcx = rc_log2(cx), lC = lcx + 3, lR = rc_log2(R);
  const size_t nb = (size_t)a.bxs * a.bys, plane = (size_t)a.xp * a.yp;
  const size_t org = (size_t)by * 8 * a.xp + (size_t)bx * 8;
  const float* tab = a.tab;
  const uint32_t tx = bx >> 3, ty = by >> 3;
  const float cfx = (float)a.cmap[(size_t)ty * a.tiles_x + tx] * (1.0f / 84.0f);
  const float cfb =
      1.0f + (float)a.cmap[(size_t)a.ntiles_all + (size_t)ty * a.tiles_x + tx] * (1.0f / 84.0f);
  const float sc = a.inv_g / (float)((int)a.qf[gh] + 1);
  const int lc = 3 + rc_log2(cx > cy ? cx : cy);

  for (int p = tid; p < R * C; p += kRB) {
    if (p < cy * cx) continue;
    const int i = p >> 6, k = p & 63;
    const size_t gb = (size_t)(by + (i >> lcx)) * a.bxs + bx + (i & (cx - 1));
    const int st = a.pos[kRcPosKinds + c_rc_koff[kind] + p];
    const int sy = st >> lc, sx = st & ((1 << lc) - 1);
    const int ky = cx >= cy ? sy : sx, kx = cx >= cy ? sx : sy;
    const float* iw = tab + kRcTabIw + c_rc_koff[kind] + p;
    const int16_t* q = a.ac + gb * 192 + k;
    const float vy = (rc_adjust(q[64], a.bias[1], a.bias[3]) * iw[kRcKindOff[10]]) * sc;
    const float vx = ((rc_adjust(q[0], a.bias[0], a.bias[3]) * iw[0]) * sc) * a.xmul + cfx * vy;
    const float vb = ((rc_adjust(q[128], a.bias[2], a.bias[3]) * iw[2 * kRcKindOff[10]]) * sc) * a.bmul +
                     cfb * vy;
    const size_t o = org + (size_t)ky * a.xp + kx;
    a.pa[o] = vx;
    a.pa[plane + o] = vy;
    a.pa[2 * plane + o] = vb;
  }
  // LLF corner: (F_cy dcs) F_cx^T through LDS
  const float* fy = tab + kRcTabFwd + rc_fwd_off(rc_log2(cy));
  const float* fx = tab + kRcTabFwd + rc_fwd_off(lcx);
  for (int c = 0; c < 3; c++) {
    for (int e = tid; e < cy * cx; e += kRB) {
      const int jy = e >> lcx, jx = e & (cx - 1);
      const size_t g = (size_t)(by + jy) * a.bxs + bx + jx;
      float d = (float)a.dc[(size_t)c * nb + g] * a.dc_step[c];
      if (c == 2) d += (float)a.dc[nb + g] * a.dc_step[1];
      sD[jy * 33 + jx] = d;
    }
    __syncthreads();
    for (int e = tid; e < cy * cx; e += kRB) {
      const int ky = e >> lcx, jx = e & (cx - 1);
      float u = 0.0f;
      for (int jy = 0; jy < cy; jy++) u += fy[ky * cy + jy] * sD[jy * 33 + jx];
      sU[ky * 33 + jx] = u;
    }
    __syncthreads();
    for (int e = tid; e < cy * cx; e += kRB) {
      const int ky = e >> lcx, kx = e & (cx - 1);
      float v = 0.0f;
      for (int jx = 0; jx < cx; jx++) v += sU[ky * 33 + jx] * fx[kx * cx + jx];
      a.pa[(size_t)c * plane + org + (size_t)ky * a.xp + kx] = v;
    }
    __syncthreads();
  }
  const float* mr = tab + kRcTabIdct + rc_idct_off(lR);
  const float* mc = tab + kRcTabIdct + rc_idct_off(lC);
  for (int e = tid; e < 3 * R * C; e += kRB) {
    const int c = e >> (lR + lC), y = (e >> lC) & (R - 1), x = e & (C - 1);
    const float* src = a.pa + (size_t)c * plane + org + x;
    float acc = 0.0f;
    for (int k = 0; k < R; k++) acc += mr[k * R + y] * src[(size_t)k * a.xp];
    a.pb[(size_t)c * plane + org + (size_t)y * a.xp + x] = acc;
  }
  __syncthreads();
  for (int e = tid; e < 3 * R * C; e += kRB) {
    const int c = e >> (lR + lC), y = (e >> lC) & (R - 1), x = e & (C - 1);
    const float* src = a.pb + (size_t)c * plane + org + (size_t)y * a.xp;
    float acc = 0.0f;
    for (int k = 0; k < C; k++) acc += src[k] * mc[k * C + x];
    a.pa[(size_t)c * plane + org + (size_t)y * a.xp + x] = acc;
  }
}

// decoder Gaborish over the block-padded planes, edges repeated
constexpr float kGabW1 = 0.115169525f, kGabW2 = 0.061248592f;
template <bool kLast>
__global__ __launch_bounds__(256) void recon_gab_kernel(ReconArgs a, const float* src, float* dst) {
  const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63);
  const uint32_t y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.xp || y >= a.yp) return;
  if (kLast && (x >= a.w || y >= a.h)) return;
  const size_t plane = (size_t)a.xp * a.yp;
  const size_t xm = x ? x - 1 : 0, xq = x + 1 < a.xp ? x + 1 : x;
  const size_t r0 = (size_t)(y ? y - 1 : 0) * a.xp, r1 = (size_t)y * a.xp,
               r2 = (size_t)(y + 1 < a.yp ? y + 1 : y) * a.xp;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float* p = src + c * plane;
    const float s1 = (p[r0 + x] + p[r2 + x]) + (p[r1 + xm] + p[r1 + xq]);
    const float s2 = (p[r0 + xm] + p[r0 + xq]) + (p[r2 + xm] + p[r2 + xq]);
    v[c] = (p[r1 + x] + kGabW1 * s1 + kGabW2 * s2) / (1.0f + 4.0f * kGabW1 + 4.0f * kGabW2);
  }
  if (kLast) {
    rc_store_rgb(a, x, y, v[0], v[1], v[2]);
  } else {
    dst[r1 + x] = v[0];
    dst[plane + r1 + x] = v[1];
    dst[2 * plane + r1 + x] = v[2];
  }
}

// one EPF pass (oracle/jxl_decode.py epf / _epf_step): 64 x 16 output tile,
// 3 px mirrored halo, the three planes in LDS
constexpr int kEW = 64, kEH = 16, kEPad = 3, kES = kEW + 2 * kEPad, kER = kEH + 2 * kEPad;
template <int kPass, bool kLast>
__global__ __launch_bounds__(256) void recon_epf_kernel(ReconArgs a, const float* src, float* dst) {
  __shared__ float sQ[3 * kER * kES];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kEW, y0 = blockIdx.y * kEH;
  const int W = (int)a.xp, H = (int)a.yp;
  const size_t plane = (size_t)a.xp * a.yp;
  for (int e = tid; e < kER * kES; e += 256) {
    int gy = y0 + e / kES - kEPad, gx = x0 + e % kES - kEPad;
    // symmetric mirroring; positions past the plane's far halo are never used
    gy = gy < 0 ? -gy - 1 : gy >= H ? 2 * H - 1 - gy : gy;
    gx = gx < 0 ? -gx - 1 : gx >= W ? 2 * W - 1 - gx : gx;
    const bool in = gy >= 0 && gx >= 0;
    const size_t g = in ? (size_t)gy * a.xp + gx : 0;
#pragma unroll
    for (int c = 0; c < 3; c++) sQ[c * kER * kES + e] = in ? src[c * plane + g] : 0.0f;
  }
  __syncthreads();
  constexpr int kNN = kPass == 0 ? 12 : 4;
  constexpr int kDy[12] = {-1, 0, 0, 1, -1, -1, 1, 1, -2, 0, 0, 2};
  constexpr int kDx[12] = {0, -1, 1, 0, -1, 1, -1, 1, 0, -2, 2, 0};
  constexpr int kOy[5] = {0, -1, 1, 0, 0};
  constexpr int kOx[5] = {0, 0, 0, -1, 1};
  constexpr int kNP = kPass == 2 ? 1 : 5;
  constexpr float kPassScale = kPass == 0 ? 0.9f : kPass == 1 ? 1.0f : 6.5f;
  constexpr float kChan[3] = {40.0f, 5.0f, 3.5f};
  const int lx = tid & 63;
  const int gx = x0 + lx;
  for (int r = 0; r < kEH / 4; r++) {
    const int ly = (tid >> 6) + 4 * r;
    const int gy = y0 + ly;
    if (gx >= W || gy >= H) continue;
    if (kLast && (gx >= (int)a.w || gy >= (int)a.h)) continue;
    const float* q = sQ + (ly + kEPad) * kES + lx + kEPad;
    const float inv = a.tab[kRcTabSigma + a.qf[(size_t)(gy >> 3) * a.bxs + (gx >> 3)]];
    float v[3] = {q[0], q[kER * kES], q[2 * kER * kES]};
    if (!(inv > 0.0f)) {
      const bool border = (gy & 7) == 0 || (gy & 7) == 7 || (gx & 7) == 0 || (gx & 7) == 7;
      const float ipx = (inv * (border ? (float)(2.0 / 3.0) : 1.0f)) * kPassScale;
      float wsum = 1.0f;
#pragma unroll
      for (int n = 0; n < kNN; n++) {
        float sad = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float* qc = q + c * kER * kES;
          float s = 0.0f;
#pragma unroll
          for (int k = 0; k < kNP; k++)
            s += fabsf(qc[(kDy[n] + kOy[k]) * kES + kDx[n] + kOx[k]] - qc[kOy[k] * kES + kOx[k]]);
          sad += kChan[c] * s;
        }
        const float wgt = fmaxf(0.0f, 1.0f + sad * ipx);
        wsum += wgt;
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] += wgt * q[c * kER * kES + kDy[n] * kES + kDx[n]];
      }
#pragma unroll
      for (int c = 0; c < 3; c++) v[c] = v[c] / wsum;
    }
    if (kLast) {
      rc_store_rgb(a, gx, gy, v[0], v[1], v[2]);
    } else {
      const size_t g = (size_t)gy * a.xp + gx;
      dst[g] = v[0];
      dst[plane + g] = v[1];
      dst[2 * plane + g] = v[2];
    }
  }
}

__global__ __launch_bounds__(256) void recon_colour_kernel(ReconArgs a, const float* src) {
  const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63);
  const uint32_t y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.w || y >= a.h) return;
  const size_t plane = (size_t)a.xp * a.yp, g = (size_t)y * a.xp + x;
  rc_store_rgb(a, x, y, src[g], src[plane + g], src[2 * plane + g]);
}

// the fused last stage of a sweep's chain: XYB -> sRGB8 as
// recon_colour_kernel, compared on the spot with the original's pixel -- the
// exact integer sum of squared sample differences sse_kernel computes from the
// stored image.  The RGB8 is stored (rows of a.stride bytes) only when SSIM
// will read it (kStore).  Workgroup = 64 columns x 4 rows, striding down the
// image; threads past the image add nothing and stay for the reduction; one
// 64-bit atomic per workgroup.
constexpr uint32_t kRcSseRows = 32;  // workgroups down the image, at most
template <bool kStore>
__global__ __launch_bounds__(256) void recon_colour_sse_kernel(ReconArgs a, const float* src,
                                                               const uint8_t* orig, size_t so,
                                                               unsigned long long* sse) {
  __shared__ uint64_t sW[4];
  const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63);
  const size_t plane = (size_t)a.xp * a.yp;
  uint64_t acc = 0;
  if (x < a.w)
    for (uint32_t y = blockIdx.y * 4 + (threadIdx.x >> 6); y < a.h; y += gridDim.y * 4) {
      const size_t g = (size_t)y * a.xp + x;
      uint8_t v[3];
      rc_xyb_to_rgb8(a, src[g], src[plane + g], src[2 * plane + g], v);
      const uint8_t* p = orig + (size_t)y * so + (size_t)x * 3;
      uint32_t d2 = 0;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int d = (int)p[c] - (int)v[c];
        d2 += (uint32_t)(d * d);
      }
      acc += d2;
      if (kStore) {
        uint8_t* o = a.rgb + (size_t)y * a.stride + (size_t)x * 3;
        o[0] = v[0];
        o[1] = v[1];
        o[2] = v[2];
      }
    }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) sW[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(sse, (unsigned long long)(sW[0] + sW[1] + sW[2] + sW[3]));
}

// the form that keeps the block structure (strategy report):
// the same conversion and comparison, and beside the frame's sum one u32 per
// 8x8 block (image pixels only).  Workgroup = 64 columns (8 blocks) x 4 waves;
// a wave takes a block row at a time, striding down the image, and adds its 8
// pixel rows in a register; the 8 lanes of a block then reduce by shuffles and
// the first of them stores the block's word (its column is inside the image
// exactly when the block exists).  Lanes past the image add nothing and stay
// for the shuffles.  Integer sums: the frame total is the other forms' u64.
template <bool kStore>
__global__ __launch_bounds__(256) void recon_colour_sse_map_kernel(ReconArgs a, const float* src,
                                                                   const uint8_t* orig, size_t so,
                                                                   unsigned long long* sse,
                                                                   uint32_t* bmap) {
  __shared__ uint64_t sW[4];
  const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63);
  const size_t plane = (size_t)a.xp * a.yp;
  uint64_t acc = 0;
  for (uint32_t by = blockIdx.y * 4 + (threadIdx.x >> 6); by < a.bys; by += gridDim.y * 4) {
    uint32_t blk = 0;
    if (x < a.w) {
      const uint32_t y1 = min(by * 8 + 8, a.h);
      for (uint32_t y = by * 8; y < y1; y++) {
        const size_t g = (size_t)y * a.xp + x;
        uint8_t v[3];
        rc_xyb_to_rgb8(a, src[g], src[plane + g], src[2 * plane + g], v);
        const uint8_t* p = orig + (size_t)y * so + (size_t)x * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const int d = (int)p[c] - (int)v[c];
          blk += (uint32_t)(d * d);
        }
        if (kStore) {
          uint8_t* o = a.rgb + (size_t)y * a.stride + (size_t)x * 3;
          o[0] = v[0];
          o[1] = v[1];
          o[2] = v[2];
        }
      }
    }
    acc += blk;
    for (int o = 1; o < 8; o <<= 1) blk += __shfl_xor(blk, o, 64);
    if ((threadIdx.x & 7) == 0 && x < a.w) bmap[(size_t)by * a.bxs + (x >> 3)] = blk;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) sW[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(sse, (unsigned long long)(sW[0] + sW[1] + sW[2] + sW[3]));
}

hipError_t launch_recon_colour_sse(const ReconArgs& a, const float* src, const uint8_t* orig,
                                   size_t orig_stride, uint64_t* sse, bool store, hipStream_t s,
                                   uint32_t* block_sse) {
  unsigned long long* out = reinterpret_cast<unsigned long long*>(sse);
  if (block_sse) {
    const dim3 bgrid((a.w + 63) / 64, std::min((a.bys + 3) / 4, kRcSseRows));
    if (store)
      recon_colour_sse_map_kernel<true>
          <<<bgrid, 256, 0, s>>>(a, src, orig, orig_stride, out, block_sse);
    else
      recon_colour_sse_map_kernel<false>
          <<<bgrid, 256, 0, s>>>(a, src, orig, orig_stride, out, block_sse);
    return hipGetLastError();
  }
  const dim3 grid((a.w + 63) / 64, std::min((a.h + 3) / 4, kRcSseRows));
  if (store)
    recon_colour_sse_kernel<true><<<grid, 256, 0, s>>>(a, src, orig, orig_stride, out);
  else
    recon_colour_sse_kernel<false><<<grid, 256, 0, s>>>(a, src, orig, orig_stride, out);
  return hipGetLastError();
}

hipError_t launch_recon_tiles(const ReconArgs& a, bool to_rgb, hipStream_t s) {
  const dim3 grid(a.tiles_x, (a.bys + 7) / 8);
  if (to_rgb)
    recon_tile_kernel<true><<<grid, kRT, 0, s>>>(a);
  else
    recon_tile_kernel<false><<<grid, kRT, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_recon_big(const ReconArgs& a, uint32_t nbig, hipStream_t s) {
  if (!nbig) return hipSuccess;
  recon_big_kernel<<<nbig, kRB, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_recon_gab(const ReconArgs& a, const float* src, float* dst, bool last,
                            hipStream_t s) {
  const dim3 grid((a.xp + 63) / 64, (a.yp + 3) / 4);
  if (last)
    recon_gab_kernel<true><<<grid, 256, 0, s>>>(a, src, dst);
  else
    recon_gab_kernel<false><<<grid, 256, 0, s>>>(a, src, dst);
  return hipGetLastError();
}

hipError_t launch_recon_epf(const ReconArgs& a, int pass, const float* src, float* dst, bool last,
                            hipStream_t s) {
  const dim3 grid((a.xp + kEW - 1) / kEW, (a.yp + kEH - 1) / kEH);
  if (pass == 0) {
    if (last)
      recon_epf_kernel<0, true><<<grid, 256, 0, s>>>(a, src, dst);
    else
      recon_epf_kernel<0, false><<<grid, 256, 0, s>>>(a, src, dst);
  } else if (pass == 1) {
    if (last)
      recon_epf_kernel<1, true><<<grid, 256, 0, s>>>(a, src, dst);
    else
      recon_epf_kernel<1, false><<<grid, 256, 0, s>>>(a, src, dst);
  } else {
    if (last)
      recon_epf_kernel<2, true><<<grid, 256, 0, s>>>(a, src, dst);
    else
      recon_epf_kernel<2, false><<<grid, 256, 0, s>>>(a, src, dst);
  }
  return hipGetLastError();
}

hipError_t launch_recon_colour(const ReconArgs& a, const float* src, hipStream_t s) {
  const dim3 grid((a.w + 63) / 64, (a.h + 3) / 4);
  recon_colour_kernel<<<grid, 256, 0, s>>>(a, src);
  return hipGetLastError();
}

}  // namespace jxg
