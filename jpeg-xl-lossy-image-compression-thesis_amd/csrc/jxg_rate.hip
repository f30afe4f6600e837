// jxg_rate.hip -- coded bits per varblock and per strategy on gfx950
// (jxg_rate_report, a sweep's lane): one pass over the token
// records ac_hist_kernel left, each priced with the code the frame wrote.
//
//   rate_kernel<BR>  one workgroup per (pass group, band), the geometry of
//                    ac_hist_kernel (BR = 8; BR = 32 = the whole group where
//                    128 / 256 px varblocks are possible).  The workgroup
//                    rebuilds every (slice, channel) task's record range with
//                    the rules ac_hist wrote them by (jxg_actask.h): the task
//                    token counts, the scan over the band's varblocks, the
//                    task's offset inside its varblock.
//                    Cost table in LDS, u16 per (static cluster, token) in
//                    1 / 256 bit: 256 x the prefix code's length, or the ANS
//                    histogram's frequency mapped through the host's 4097-entry
//                    table (jxg_rate_symbol_cost), composed through the
//                    cluster -> histogram map.
//                    Walk: a wave takes its 64 threads' tasks eight at a time,
//                    lane = record (a task holds at most 64, contiguous: one
//                    coalesced read; the eight reads are issued together),
//                    looks the symbol cost up, adds the raw bits, reduces over
//                    the wave; one lane adds the sum to the varblock's channel
//                    cell at its first block (LDS atomic).
//                    Then one plain store per block of the map (covered blocks
//                    0), per-wave sums by strategy id into the workgroup's
//                    27 x 6 table (LDS atomics) and one 64-bit global add per
//                    non-empty cell.
// Every sum is an integer: the result does not depend on the order of the adds.
#include <algorithm>

#include "jxg_actask.h"

namespace jxg {

#ifndef JXG_RATE_BATCH  // (experiment builds override it)
#define JXG_RATE_BATCH 8
#endif
constexpr int kRateBatch = JXG_RATE_BATCH;  // tasks whose record loads are in flight together

template <int BR>
__global__ __launch_bounds__(BR * 32) void rate_kernel(RateArgs ra) {
  constexpr int kBandBlocks = BR * 32, kWgBands = 32 / BR;
  // records of the workgroup's band space (the whole group's with BR = 32)
  constexpr uint32_t kSpace = (uint32_t)(BR == 32 ? kGroupTokStride : kBandTokStride);
  const AcArgs& a = ra.ac;
  __shared__ uint16_t sCost[kMaxClusters * kAcTok];
  __shared__ AcLds<BR> L;
  __shared__ uint32_t sTask[3][kBandBlocks];  // tokens per (channel slot Y, X, B; slice task)
  __shared__ uint32_t sBase[kBandBlocks];     // first record of each varblock (first block)
  __shared__ uint32_t sCell[3][kBandBlocks];  // cost per (channel X, Y, B; first block)
  __shared__ uint32_t sWave[kBandBlocks / 64];
  __shared__ unsigned long long sT[kRateCells];
  const uint32_t slot = blockIdx.x / kWgBands, band = blockIdx.x % kWgBands;
  const int g = (int)slot_group(a.glist, a.g0, slot);
  const GroupGeom G = group_geom(a, g);
  const int y0 = (int)band * BR;
  if (y0 >= G.gh) return;  // below a partial bottom group: no block, no record
  const int me = threadIdx.x;
  for (int i = me; i < kMaxClusters * kAcTok; i += kBandBlocks) {
    const uint32_t clu = (uint32_t)i / kAcTok, tok = (uint32_t)i % kAcTok;
    uint32_t cost;
    if (ra.ans_tab) {
      const uint32_t h = min((uint32_t)ra.ans_tab[kAnsMapOff + clu], kAnsHists - 1);
      const uint32_t e = reinterpret_cast<const uint32_t*>(ra.ans_tab)[h * 128 + tok];
      cost = h < ra.nhist ? ra.ftab[(e & 0xFFFu) + 1u] : 0u;
    } else {
      cost = (a.codes[clu * kAlpha + tok] >> 16) * kRateUnit;
    }
    sCost[i] = (uint16_t)cost;
  }
  for (int i = me; i < 3 * kBandBlocks; i += kBandBlocks) (&sCell[0][0])[i] = 0;
  lds_table_zero<kBandBlocks>(sT, kRateCells);
  const SliceTask t = slice_task(a, G, y0);
  fill_slices(a, G, t, L, y0);
  __syncthreads();
  if (t.valid) {
#pragma unroll 1
    for (int ci = 0; ci < 3; ci++) sTask[ci][me] = task_token_count(a, t, L, channel_of(ci), y0);
  }
  __syncthreads();
  uint32_t total;
  const uint32_t off = varblock_base<BR>(t, sTask, sWave, y0, &total);
  if (t.valid && t.sl == 0) sBase[me] = off;
  __syncthreads();
  const uint32_t* rec = a.tokens + (uint64_t)slot * kGroupTokStride + (uint64_t)band * kBandTokStride;
  const int first = (t.oby - y0) * 32 + t.obx;  // the varblock's first block, band-local
  uint32_t pos = t.valid ? sBase[first] : 0u;
  const int lane = me & 63;
  uint32_t vtok[3] = {0, 0, 0};  // the varblock's tokens X, Y, B (first blocks)
#pragma unroll 1
  for (int ci = 0; ci < 3; ci++) {
    const int c = channel_of(ci);
    uint32_t idx = 0, cnt = 0;
    if (t.valid) {
      const uint32_t p0 = pos;
      task_records<BR>(t, sTask, ci, y0, pos, idx, cnt);
      if (t.sl == 0) vtok[c] = pos - p0;
    }
    // tasks with records, kRateBatch at a time: their loads are issued
    // together (one memory latency per batch, as ac_hist's walk does).  A task
    // holds at most 64 records (task_token_count: 1 + 63 for an 8x8-class
    // block, 64 for a later slice), one per lane.
    uint64_t M = __ballot(cnt > 0);
    while (M) {
      int js[kRateBatch];
#pragma unroll
      for (int u = 0; u < kRateBatch; u++) {
        js[u] = M ? (int)__builtin_ctzll(M) : -1;
        M = M ? M & (M - 1) : 0ull;
      }
      uint32_t r8[kRateBatch];
      bool on8[kRateBatch];
#pragma unroll
      for (int u = 0; u < kRateBatch; u++) {
        r8[u] = 0;
        on8[u] = false;
        if (js[u] >= 0) {
          const uint32_t idxj = (uint32_t)__builtin_amdgcn_readlane((int)idx, js[u]);
          const uint32_t cntj = (uint32_t)__builtin_amdgcn_readlane((int)cnt, js[u]);
          // (idxj + lane < kSpace always: a band's tokens fit its record space)
          on8[u] = (uint32_t)lane < cntj && idxj + (uint32_t)lane < kSpace;
          if (on8[u]) r8[u] = rec[idxj + lane];
        }
      }
#pragma unroll
      for (int u = 0; u < kRateBatch; u++) {
        if (js[u] < 0) break;
        const uint32_t r = r8[u];
        const uint32_t clu = min(rec_cluster(r), (uint32_t)kMaxClusters - 1);
        const uint32_t cost = (uint32_t)sCost[clu * kAcTok + rec_token(r)] + rec_nbits(r) * kRateUnit;
        const uint32_t sum = wave_sum(on8[u] ? cost : 0u);
        const int cell = __builtin_amdgcn_readlane(first, js[u]);
        if (lane == 0 && sum) atomicAdd(&sCell[c][cell], sum);
      }
    }
  }
  __syncthreads();
  // the map, and the workgroup's table: first blocks by strategy id.  A wave's
  // sums fit u32: a band holds < 2^18 tokens of at most 7680 units each.
  const bool head = t.valid && t.sl == 0;
  uint32_t vc[3] = {0, 0, 0};
  if (head) {
#pragma unroll
    for (int c = 0; c < 3; c++) vc[c] = sCell[c][me];
  }
  if (t.valid && ra.block_cost) ra.block_cost[t.gb] = vc[0] + vc[1] + vc[2];
  const uint32_t v[6] = {vtok[0], vtok[1], vtok[2], vc[0], vc[1], vc[2]};
  wave_sum_by_key(head && t.type < (int)kRateStrategies, (uint32_t)t.type, v,
                  [&](uint32_t id0, const uint32_t* s) {
#pragma unroll
                    for (int k = 0; k < 6; k++)
                      if (s[k]) atomicAdd(sT + id0 * kRateCols + k, (unsigned long long)s[k]);
                  });
  __syncthreads();
  lds_table_flush<kBandBlocks>(sT, ra.table, kRateCells);
}

hipError_t launch_rate(const RateArgs& a, uint32_t ngroups, bool whole_group, hipStream_t s) {
  if (whole_group)
    hipLaunchKernelGGL(rate_kernel<32>, dim3(ngroups), dim3(1024), 0, s, a);
  else
    hipLaunchKernelGGL(rate_kernel<8>, dim3(ngroups * kBands), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace jxg
