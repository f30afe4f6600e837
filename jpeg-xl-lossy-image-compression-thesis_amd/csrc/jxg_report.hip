// jxg_report.hip -- per-strategy statistics of an encoded frame on gfx950
// (jxg_strategy_report_rgb8, a sweep's lane): one reduction
// over the blocks that keeps the strategy structure.
//
//   strategy_report_kernel  a workgroup of 4 waves takes chunks of 256 blocks,
//                        striding over the frame.
//                        Block pass: one lane per block reads its strategy
//                        byte, quant field and squared error (the block map of
//                        recon_colour_sse_map_kernel) and derives its image
//                        pixels from its position.  Neighbouring blocks mostly
//                        share a strategy, so the wave first sums the lanes of
//                        each strategy present (a wave's sums fit u32: 64
//                        blocks x 64 x 3 x 255^2 < 2^32) and one lane adds the
//                        five sums to the workgroup's table in LDS.
//                        Coefficient pass: the chunk's `ac` slices are one
//                        contiguous range; a wave reads 8 slices per step, 16
//                        bytes per lane, counts the non-zero coefficients and
//                        reduces within the 8 lanes of a slice, whose first
//                        lane adds the count to its block's strategy row.
//                        At the end one 64-bit global add per non-empty cell.
// Every sum is an integer: the table does not depend on the order of the adds.
#include <algorithm>

#include "jxg_device.h"
#include "jxg_kernels.h"

namespace jxg {

constexpr uint32_t kRepChunk = 256;  // blocks per workgroup step
constexpr uint32_t kRepGrid = 1024;  // workgroups, at most

__global__ __launch_bounds__(256) void strategy_report_kernel(ReportArgs a) {
  __shared__ unsigned long long sT[kReportCells];
  lds_table_zero<256>(sT, kReportCells);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t nchunks = (a.nb + kRepChunk - 1) / kRepChunk;
  for (uint32_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const uint32_t b0 = ch * kRepChunk;
    // ---- block pass ----
    {
      const uint32_t b = b0 + threadIdx.x;
      const bool in = b < a.nb;
      uint32_t id = 0xFFu, first = 0, px = 0, q = 0, e = 0;
      if (in) {
        const uint32_t s = a.acs[b];
        id = s & 0x7Fu;
        first = (s >> 7) ^ 1u;
        const uint32_t bx = b % a.bxs, by = b / a.bxs;
        px = min(8u, a.w - bx * 8) * min(8u, a.h - by * 8);
        q = (uint32_t)a.qf[b] + 1u;
        e = a.block_sse[b];
      }
      // (other ids: not a stream this encoder writes)
      const uint32_t v[5] = {first, 1u, px, q, e};
      wave_sum_by_key(in && id < kReportStrategies, id, v, [&](uint32_t id0, const uint32_t* s) {
        unsigned long long* r = sT + id0 * kReportCols;
        atomicAdd(r + 0, (unsigned long long)s[0]);
        atomicAdd(r + 1, (unsigned long long)s[1]);
        atomicAdd(r + 2, (unsigned long long)s[2]);
        atomicAdd(r + 6, (unsigned long long)s[3]);
        atomicAdd(r + 7, (unsigned long long)s[4]);
      });
    }
    // ---- coefficient pass: slices [b0 * 3, min(b0 + 256, nb) * 3) of 64 int16 ----
    {
      const uint32_t s0 = b0 * 3, s1 = min(b0 + kRepChunk, a.nb) * 3;
      for (uint32_t sb = s0 + wave * 8; sb < s1; sb += 32) {
        const uint32_t sl = sb + (lane >> 3);
        uint32_t cnt = 0;
        if (sl < s1) {
          const uint4 v = reinterpret_cast<const uint4*>(a.ac)[(size_t)sl * 8 + (lane & 7)];
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int k = 0; k < 4; k++)
            cnt += ((w[k] & 0xFFFFu) != 0) + ((w[k] >> 16) != 0);
        }
        for (int o = 1; o < 8; o <<= 1) cnt += __shfl_xor(cnt, o, 64);
        if ((lane & 7) == 0 && sl < s1 && cnt) {
          const uint32_t b = sl / 3, c = sl - b * 3;
          const uint32_t id = a.acs[b] & 0x7Fu;
          if (id < kReportStrategies)
            atomicAdd(sT + id * kReportCols + 3 + c, (unsigned long long)cnt);
        }
      }
    }
  }
  __syncthreads();
  lds_table_flush<256>(sT, a.table, kReportCells);
}

hipError_t launch_strategy_report(const ReportArgs& a, hipStream_t s) {
  const uint32_t nchunks = (a.nb + kRepChunk - 1) / kRepChunk;
  strategy_report_kernel<<<std::min(nchunks, kRepGrid), 256, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace jxg
