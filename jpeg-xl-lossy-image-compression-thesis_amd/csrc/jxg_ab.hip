// jxg_ab.hip -- A/B report of two encodes of one image on gfx950
// (jxg_ab_report_rgb8, a sweep's lane): which strategy every
// 8x8 block had in A and in B, with the bits and the error of both sides.
//
//   ab_share_kernel  one lane per block of one side: the block's share of its
//                    varblock's coded cost C (the first-block map of
//                    rate_kernel), C / n + (k < C % n) for covered block k of
//                    n in raster order inside the varblock.  Gather form: the
//                    first block is first_block's (jxg_actask.h): the block's
//                    position rounded down to the varblock's size, which the
//                    search guarantees for every shape -- up to 64 px by the
//                    merge stage's construction inside 64x64 tiles (a forced
//                    map's off-grid varblock is found from the map instead),
//                    for the 128 / 256 px shapes by
//                    big_region / big_cand (jxg_bigvb.hip): a region starts at
//                    a multiple of 16 (32) blocks of a pass group that starts
//                    at a multiple of 32, and a half candidate at the region's
//                    origin or half its size further.  n is a power of two.
//   ab_report_kernel a workgroup of 4 waves takes chunks of 256 blocks,
//                    striding over the frame; one lane per block reads the two
//                    strategy bytes, error words and shares and derives its
//                    image pixels from its position.  Neighbouring blocks
//                    mostly share a (from, to) pair, so the wave first sums
//                    the lanes of each pair present and one lane adds the six
//                    sums to the workgroup's 27 x 27 x 6 table in LDS.  A
//                    wave's error sums fit u32 (64 x 64 x 3 x 255^2 < 2^32);
//                    its share sums do not (64 x 1.5e9), so the low and high
//                    16 bits of the shares are summed apart (64 x 65535 each)
//                    and put together in 64 bits.  The same pass writes the
//                    two delta planes when asked for (every word).  At the end
//                    one 64-bit global add per non-empty cell.
// Every sum is an integer: the table does not depend on the order of the adds.
#include <algorithm>

#include "jxg_actask.h"

namespace jxg {

constexpr uint32_t kAbChunk = 256;  // blocks per workgroup step
constexpr uint32_t kAbGrid = 1024;  // workgroups, at most

__global__ __launch_bounds__(256) void ab_share_kernel(AbShareArgs a) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nb) return;
  int lcb, cx, cy;
  varblock_dims(a.acs[b] & 0x7F, lcb, cx, cy);
  const uint32_t bx = b % a.bxs, by = b / a.bxs;
  // (ox <= bx, oy <= by: the first block is inside the frame)
  int fx, fy;
  first_block(a.acs, a.bxs, a.acs[b] & 0x7F, lcb, cx, cy, (int)bx, (int)by, fx, fy);
  const uint32_t ox = (uint32_t)fx, oy = (uint32_t)fy;
  const uint32_t C = a.block_cost[(size_t)oy * a.bxs + ox];
  const uint32_t k = (by - oy) * (uint32_t)cx + (bx - ox);
  a.share[b] = (C >> lcb) + (k < (C & ((1u << lcb) - 1u)) ? 1u : 0u);
}

__global__ __launch_bounds__(256) void ab_report_kernel(AbArgs a) {
  __shared__ unsigned long long sT[kAbWords];
  lds_table_zero<256>(sT, kAbWords);
  __syncthreads();
  const uint32_t nchunks = (a.nb + kAbChunk - 1) / kAbChunk;
  for (uint32_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const uint32_t b = ch * kAbChunk + threadIdx.x;
    const bool in = b < a.nb;
    uint32_t pair = 0xFFFFu, px = 0, ea = 0, eb = 0, ca = 0, cb = 0;
    bool todo = false;
    if (in) {
      const uint32_t from = a.acs_a[b] & 0x7Fu, to = a.acs_b[b] & 0x7Fu;
      const uint32_t bx = b % a.bxs, by = b / a.bxs;
      px = min(8u, a.w - bx * 8) * min(8u, a.h - by * 8);
      ea = a.sse_a[b];
      eb = a.sse_b[b];
      ca = a.share_a[b];
      cb = a.share_b[b];
      if (a.delta) {
        a.delta[b] = (int32_t)eb - (int32_t)ea;
        a.delta[(size_t)a.nb + b] = (int32_t)cb - (int32_t)ca;
      }
      // (other ids: not a stream this encoder writes)
      todo = from < kAbStrategies && to < kAbStrategies;
      pair = from * kAbStrategies + to;
    }
    // (the shares' low and high halves apart: a wave's sum of either fits u32)
    const uint32_t v[8] = {1u, px, ea, eb, ca & 0xFFFFu, ca >> 16, cb & 0xFFFFu, cb >> 16};
    wave_sum_by_key(todo, pair, v, [&](uint32_t p0, const uint32_t* s) {
      unsigned long long* r = sT + p0 * kAbCols;
      atomicAdd(r + 0, (unsigned long long)s[0]);
      atomicAdd(r + 1, (unsigned long long)s[1]);
      atomicAdd(r + 2, (unsigned long long)s[2]);
      atomicAdd(r + 3, (unsigned long long)s[3]);
      atomicAdd(r + 4, ((unsigned long long)s[5] << 16) + s[4]);
      atomicAdd(r + 5, ((unsigned long long)s[7] << 16) + s[6]);
    });
  }
  __syncthreads();
  lds_table_flush<256>(sT, a.table, kAbWords);
}

hipError_t launch_ab_share(const AbShareArgs& a, hipStream_t s) {
  ab_share_kernel<<<(a.nb + 255) / 256, 256, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_ab_report(const AbArgs& a, hipStream_t s) {
  const uint32_t nchunks = (a.nb + kAbChunk - 1) / kAbChunk;
  ab_report_kernel<<<std::min(nchunks, kAbGrid), 256, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace jxg
