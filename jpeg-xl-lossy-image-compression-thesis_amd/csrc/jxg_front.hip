// jxg_front.hip -- the search instantiations of front_kernel
// (jxg_front_kernel.h) and the standalone thesis selector, homog_kernel.
#include <cstdio>

#define JXG_FRONT_NS search_tu
#include "jxg_front_kernel.h"

namespace jxg {
namespace search_tu {

// standalone thesis selector over a given XYB frame (parity entry point)
__global__ __launch_bounds__(kThreads) void homog_kernel(HomogArgs a) {
  __shared__ float sPix[3 * kPlane];
  __shared__ float sH[8][64];
  __shared__ uint64_t sLapBits[64];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x, ty = blockIdx.y;
  const int ox = tx * kTile - 1, oy = ty * kTile - 1;
  for (int i = tid; i < kRows * 66; i += kThreads) {
    const int ly = i / 66, lx = i - ly * 66;
    const int gx = ox + lx, gy = oy + ly;
    const bool in = gx >= 0 && gy >= 0 && gx < (int)a.xsize && gy < (int)a.ysize;
    const size_t o = (size_t)gy * a.stride + gx;
    const int l = lds_at(lx, ly);
    sPix[l] = in ? a.xyb[o] : 0.0f;
    sPix[kPlane + l] = in ? a.xyb[a.plane + o] : 0.0f;
    sPix[2 * kPlane + l] = in ? a.xyb[2 * a.plane + o] : 0.0f;
  }
  __syncthreads();
  const int bxs = (int)a.xsize / 8, bys = (int)a.ysize / 8;
  const int wave = tid >> 6, lane = tid & 63;
  const int lbx = lane & 7, lby = lane >> 3;
  const bool valid = tx * 8 + lbx < bxs && ty * 8 + lby < bys;
  const Tile tile{sPix, sPix + kPlane, sPix + 2 * kPlane, ox, oy};
  lap_bits(tile, edge_threshold(a.distance), sLapBits);
  __syncthreads();
  if (valid)
    sH[wave][lane] = homog_region(tile, sLapBits, wave, tx * kTile + lbx * 8, ty * kTile + lby * 8,
                                  a.distance, (int)a.ysize, a.h1_int);
  __syncthreads();
  if (tid < 64 && valid) {
    float h[8];
#pragma unroll
    for (int r = 0; r < 8; r++) h[r] = sH[r][lane];
    float rh, rv, rd;
    similarity(h, rh, rv, rd);
    const size_t b = (size_t)(ty * 8 + lby) * bxs + tx * 8 + lbx;
    a.r3[b * 3 + 0] = rh;
    a.r3[b * 3 + 1] = rv;
    a.r3[b * 3 + 2] = rd;
    a.type[b] = partition_of(rh, rv, rd, a.distance);
  }
}

}  // namespace search_tu

using namespace search_tu;

hipError_t upload_front_tables_search(const FrontTables& t, hipStream_t s) {
  return upload_front_tables(t, s);
}
// (the frames of a batch share their size and parameters)
void launch_front(const FrontArgs* a, uint32_t k, uint32_t tiles_x, uint32_t tiles_y, hipStream_t s) {
  if (!k) return;
  const Batch<FrontArgs> b = make_batch(a, k);
  const uint32_t nwg = 8 * ((tiles_x * tiles_y + 7) / 8);  // XCD-aware order (front_kernel)
  if (a[0].proposals & 1u)
    hipLaunchKernelGGL((front_kernel<true, false, false>), dim3(nwg, 1, k), dim3(kThreads), 0, s, b);
  else
    hipLaunchKernelGGL((front_kernel<false, false, false>), dim3(nwg, 1, k), dim3(kThreads), 0, s, b);
}
void launch_front_list(const FrontArgs* a, uint32_t k, uint32_t ntiles, hipStream_t s) {
  if (!ntiles || !k) return;
  const Batch<FrontArgs> b = make_batch(a, k);
  if (a[0].proposals & 1u)
    hipLaunchKernelGGL((front_kernel<true, false, false>), dim3(ntiles, 1, k), dim3(kThreads), 0, s, b);
  else
    hipLaunchKernelGGL((front_kernel<false, false, false>), dim3(ntiles, 1, k), dim3(kThreads), 0, s, b);
}
void launch_homog(const HomogArgs& a, uint32_t tiles_x, uint32_t tiles_y, hipStream_t s) {
  hipLaunchKernelGGL(homog_kernel, dim3(tiles_x, tiles_y), dim3(kThreads), 0, s, a);
}

#ifdef JXG_FRONT_PROFILE
void dump_front_profile() {
  unsigned long long h[12];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_fprof), sizeof(h)) != hipSuccess) return;
  static const char* kNames[10] = {"workgroups", "tables", "tile+ring load", "gab sweep",
                                   "xyb copy", "phase A", "phase B", "dc+aq", "phase C",
                                   "phase D"};
  std::fprintf(stderr, "front_kernel thread-0 shader cycles (Mcycles summed over workgroups):\n");
  for (int k = 0; k < 10; k++)
    std::fprintf(stderr, "  %-16s %12.3f\n", kNames[k], k ? h[k] / 1e6 : (double)h[0]);
  unsigned long long z[2];
  if (hipMemcpyFromSymbol(z, HIP_SYMBOL(g_fzero), sizeof(z)) != hipSuccess) return;
  std::fprintf(stderr, "quant_xb zero votes: %llu of %llu (wave, k)\n", z[1], z[0]);
}
#else
void dump_front_profile() {}
#endif

}  // namespace jxg
