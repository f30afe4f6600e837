// jxg_vb_list.hip -- varblock lists of the LF groups (AC metadata channel of
// size count x 2): block indices of the varblocks' first blocks in LF-group
// raster order, taken from the final strategy map behind every merge level.
#include "jxg_device.h"
#include "jxg_kernels.h"

namespace jxg {

// Varblock list of one LF group: the frame-raster block index of every
// varblock's first block, in raster order inside the LF group.  Thread t
// holds the first-block flags of blocks t, t + 1024, ... (all 64 loads in
// flight at once); per-(chunk, wave) counts -> one workgroup scan -> stores.
__global__ __launch_bounds__(1024) void vb_list_kernel(Batch<VbArgs> bt_) {
  const VbArgs& a = bt_.a[blockIdx.z];
  __shared__ uint32_t sCnt[64 * 16];
  __shared__ uint32_t sWave[16];
  const uint32_t lg = blockIdx.x;
  if (a.lf_mine && !a.lf_mine[lg]) return;  // LF group of another shard
  const uint32_t bx0 = (lg % a.lfxs) * 256, by0 = (lg / a.lfxs) * 256;
  const uint32_t bw = min(256u, a.bxs - bx0), bh = min(256u, a.bys - by0);
  const uint32_t n = bw * bh;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  // (row, column) of element i = k * 1024 + threadIdx.x in the group, stepped
  // by (1024 / bw, 1024 % bw) with a carry: no integer division per element
  const uint32_t dq = 1024u / bw, dr = 1024u % bw;
  const uint32_t y0 = threadIdx.x / bw, x0 = threadIdx.x % bw;
  auto step = [&](uint32_t& y, uint32_t& x) {
    x += dr;
    y += dq;
    if (x >= bw) {
      x -= bw;
      y++;
    }
  };
  uint64_t fl = 0;  // bit k: block k * 1024 + threadIdx.x starts a varblock
  {
    uint32_t y = y0, x = x0;
#pragma unroll 16
    for (int k = 0; k < 64; k++) {
      const uint32_t i = (uint32_t)k * 1024 + threadIdx.x;
      if (i < n && !(a.acs[(size_t)(by0 + y) * a.bxs + bx0 + x] & 0x80)) fl |= 1ull << k;
      step(y, x);
    }
  }
  for (int k = 0; k < 64; k++) {
    const uint64_t bal = __ballot((fl >> k) & 1);
    if (lane == 0) sCnt[k * 16 + wv] = (uint32_t)__popcll(bal);
  }
  __syncthreads();
  // exclusive scan of the 1024 (chunk, wave) counts in (chunk, wave) order
  const uint32_t v = sCnt[threadIdx.x];
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  if (lane == 63) sWave[wv] = incl;
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (int w = 0; w < 16; w++) {
    before += w < wv ? sWave[w] : 0u;
    total += sWave[w];
  }
  sCnt[threadIdx.x] = before + incl - v;
  __syncthreads();
  uint32_t y = y0, x = x0;
  for (int k = 0; k < 64; k++) {
    const bool f = (fl >> k) & 1;
    const uint64_t bal = __ballot(f);
    if (f)
      a.vb[(size_t)lg * 65536 + sCnt[k * 16 + wv] + (uint32_t)__popcll(bal & lt)] =
          (uint32_t)((size_t)(by0 + y) * a.bxs + bx0 + x);
    step(y, x);
  }
  if (threadIdx.x == 0) a.count[lg] = total;
}
void launch_vb_list(const VbArgs* a, uint32_t k, uint32_t nlf, hipStream_t s) {
  if (k) hipLaunchKernelGGL(vb_list_kernel, dim3(nlf, 1, k), dim3(1024), 0, s, make_batch(a, k));
}

}  // namespace jxg
