// jxg_ac_hist.hip -- the pass groups' AC token walk on gfx950: statistics and
// the token records the coders read (jxg_acrec.h).
//
// One workgroup per band of a 256x256-pixel pass group (jxg_acrec.h kBands):
// thread = 8x8 block
// = one 64-coefficient slice of a varblock (an 8x8-class block is a varblock
// of one slice; a merged varblock covering cb blocks keeps slice i of its
// natural-order coefficients in covered block i, raster order).  A slice's
// walk state at its first coefficient -- non-zeros left and the
// previous-coefficient flag -- follows from the per-slice non-zero counts of
// the earlier slices (LDS), so every slice of a 64x64 varblock is independent.
// The token walk is wave-parallel: a wave takes the tasks (slice, channel) of
// its 64 threads one at a time, lane = coefficient; ballot + popcount give
// each coefficient its non-zeros-left context, so a task costs one pass
// whatever its token count and its records are stored contiguously.
//   ac_hist : non-zero counts -> predicted-nz + zero-density contexts ->
//             clustered histograms (LDS, one global atomic per non-empty bin),
//             exact per-group token counts, per-group bit upper bound; then a
//             workgroup scan over varblocks (stream order: varblocks by first
//             block raster, channels Y, X, B, slices) and the wave-parallel
//             walk that writes every token as a 32-bit record (ac_record) at
//             its stream position.
#include "jxg_device.h"
#include "jxg_kernels.h"
#include "jxg_actask.h"

namespace jxg {

// context -> static cluster id (padded to whole 16-byte words: ac_hist copies
// it to LDS with 16-byte loads; the pad stays 0)
constexpr int kAcCtxPad = (kAcCtx + 15) & ~15;
__constant__ __attribute__((aligned(16))) uint8_t c_cluster[kAcCtxPad];

// coefficient loads of this many tasks are in flight together
#ifndef JXG_AC_BATCH  // (experiment builds override it)
#define JXG_AC_BATCH 8
#endif
constexpr int kAcBatch = JXG_AC_BATCH;

// The fill of the walk's LDS tables sFreqCtx / sNnzCtx keeps the expression
// forms ac_hist_kernel was built with (the decoder's forms of jxg_acmodel.h
// cost its prologue instructions, DESIGN.md §3.13 "The AC coding stage's
// units"); the values are the model's, checked here.
constexpr int fill_freq_ctx(int k) {
  return k < 16 ? (k > 1 ? k - 1 : 0) : (k < 32 ? 15 + ((k - 16) >> 1) : 23 + ((k - 32) >> 2));
}
constexpr int fill_nnz_ctx(int n) {
  return n < 2 ? 0 : n < 3 ? 31 : n < 5 ? 62 : n < 9 ? 93 : n < 13 ? 123 : n < 21 ? 152
       : n < 33 ? 180 : 206;
}
constexpr bool fill_ctx_is_the_models() {
  for (int i = 0; i < 64; i++)
    if ((uint32_t)fill_freq_ctx(i) != freq_ctx(i) || (uint32_t)fill_nnz_ctx(i) != nnz_ctx(i)) return false;
  return true;
}
static_assert(fill_ctx_is_the_models(), "sFreqCtx / sNnzCtx hold jxg_acmodel.h's freq_ctx / nnz_ctx");

__device__ __forceinline__ int block_ctx_of(int c, int acs) {
  return (int)block_ctx((c < 2 ? c ^ 1 : 2) * 13 + strategy_order(acs));
}

// predicted non-zeros of group-local block (bx, by) from the band's nz image
// (row 0 = the row above the band); neighbours inside the group only
__device__ __forceinline__ int predict_nz(const uint8_t* nzc, int bx, int by, int y0) {
  const int r = by - y0 + 1;
  if (bx == 0) return by == 0 ? 32 : nzc[(r - 1) * 32 + bx];
  if (by == 0) return nzc[r * 32 + bx - 1];
  return (nzc[(r - 1) * 32 + bx] + nzc[r * 32 + bx - 1] + 1) / 2;
}

// walk state of task (t, c) at its first coefficient; nz = varblock count
template <int BR>
__device__ __forceinline__ void slice_state(const SliceTask& t, const AcLds<BR>& L, int c, int y0,
                                            int nz, int& left, int& prev) {
  const int cb = 1 << t.lcb;
  left = nz;
  prev = nz > cb * 4 ? 0 : 1;  // nz > size / 16
  if (t.sl > 0) {
    for (int j = 0; j < t.sl; j++) left -= L.snz[c][block_of_slice(t, j, y0)];
    if (t.sl * 64 - 1 >= cb) prev = L.last[c][block_of_slice(t, t.sl - 1, y0)];
  }
}

// JXG_FRONT_PROFILE (experiment builds only): ac_hist phase clock sums of
// thread 0 of every band workgroup, printed by dump_hist_profile()
#ifdef JXG_FRONT_PROFILE
__device__ unsigned long long g_hprof[8];
#define HPROF(k)                                                     \
  do {                                                               \
    if (threadIdx.x == 0) {                                          \
      const unsigned long long now_ = __builtin_readcyclecounter();  \
      if ((k) > 0) atomicAdd(&g_hprof[(k)], now_ - hprof_t0);       \
      else atomicAdd(&g_hprof[0], 1ull);                             \
      hprof_t0 = now_;                                               \
    }                                                                \
  } while (0)
void dump_hist_profile() {
  unsigned long long h[8];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_hprof), sizeof(h)) != hipSuccess) return;
  static const char* kNames[6] = {"workgroups", "fill slices", "token counts", "scan", "walk", "flush"};
  std::fprintf(stderr, "ac_hist thread-0 shader cycles (Mcycles summed over workgroups):\n");
  for (int k = 0; k < 6; k++) std::fprintf(stderr, "  %-16s %12.3f\n", kNames[k], k ? h[k] / 1e6 : (double)h[0]);
}
#else
#define HPROF(k) \
  do {           \
  } while (0)
void dump_hist_profile() {}
#endif
// The band's clustered histogram in LDS.  An 8-row band (BR = 8) has at most
// 256 x 3 x 64 + 768 = 49920 tokens, so its counts are u16, two bins per word,
// and a half never carries.  The whole-group form (BR = 32, effort >= 8) walks
// up to 1024 x 3 x 64 + 3072 tokens, and one bin can pass 65535 (a DCT256X256
// whose X and B hold only their last coefficient puts ~129 K zero tokens into
// one cluster; tests/test_gpu_bigvb.py::test_whole_group_histogram_bin_above_u16):
// u32 bins there (67.6 KB of LDS for the histogram).
template <int BR>
__global__ __launch_bounds__(BR * 32) void ac_hist_kernel(Batch<AcArgs> bt_) {
  constexpr int kBandBlocks = BR * 32, kHistThreads = kBandBlocks, kWgBands = 32 / BR;
  const AcArgs& a = bt_.a[blockIdx.z];  // the batch's frame
  constexpr bool kWide = BR == 32;  // u32 bins
  constexpr int kHistWords = kWide ? kMaxClusters * kAcTok : kMaxClusters * kAcTok / 2;
  __shared__ uint32_t sHist[kHistWords];
  __shared__ AcLds<BR> L;
  __shared__ __attribute__((aligned(16))) uint8_t sClu[kAcCtxPad];
  __shared__ uint32_t sTask[3][kBandBlocks];  // tokens per (channel, slice task)
  __shared__ uint32_t sBase[kBandBlocks];     // first token of each varblock (first block)
  __shared__ uint32_t sWave[kHistThreads / 64];
  __shared__ uint32_t sBound, sNtok[3];
  __shared__ uint16_t sNnzCtx[64];
  __shared__ uint8_t sFreqCtx[64];
  const uint32_t slot = blockIdx.x / kWgBands, band = blockIdx.x % kWgBands;
  const int g = (int)slot_group(a.glist, a.g0, slot);
  const GroupGeom G = group_geom(a, g);
  const int y0 = (int)band * BR;
  if (BR == 32 && threadIdx.x > 0 && threadIdx.x < kBands)
    a.bandtok[g * kBands + threadIdx.x] = 0;  // one band holds the whole group's stream
  if (y0 >= G.gh) {  // below a partial bottom group: an empty band
    if (threadIdx.x == 0) a.bandtok[g * kBands + band] = 0;
    return;
  }
#ifdef JXG_FRONT_PROFILE
  unsigned long long hprof_t0 = 0;
#endif
  HPROF(0);
  for (int i = threadIdx.x; i < kHistWords; i += blockDim.x) sHist[i] = 0;
  if (threadIdx.x < 64) {
    sNnzCtx[threadIdx.x] = (uint16_t)fill_nnz_ctx(threadIdx.x);
    sFreqCtx[threadIdx.x] = (uint8_t)fill_freq_ctx(threadIdx.x);
  }
  {  // the cluster map: 16-byte loads, all issued before the stores
    constexpr int kQ = kAcCtxPad / 16, kQIt = (kQ + kHistThreads - 1) / kHistThreads;
    uint4 q[kQIt];
#pragma unroll
    for (int it = 0; it < kQIt; it++) {
      const int i = threadIdx.x + it * kHistThreads;
      q[it] = i < kQ ? reinterpret_cast<const uint4*>(c_cluster)[i] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int it = 0; it < kQIt; it++) {
      const int i = threadIdx.x + it * kHistThreads;
      if (i < kQ) reinterpret_cast<uint4*>(sClu)[i] = q[it];
    }
  }
  if (threadIdx.x < 3) sNtok[threadIdx.x] = 0;
  if (threadIdx.x == 0) sBound = 0;
  const SliceTask t = slice_task(a, G, y0);
  uint32_t nzo[3];  // the varblock's non-zero counts (the walk's start state)
#pragma unroll
  for (int c = 0; c < 3; c++) nzo[c] = t.valid ? a.nz[c * (size_t)a.bxs * a.bys + t.ogb] : 0u;
  fill_slices(a, G, t, L, y0);
  __syncthreads();
  HPROF(1);
  const int me = threadIdx.x;
  // token counts per task without a walk -> stream positions (varblocks by
  // first block raster, channels Y, X, B, slices): one scan over varblocks
  if (t.valid) {
#pragma unroll 1
    for (int ci = 0; ci < 3; ci++) sTask[ci][me] = task_token_count(a, t, L, channel_of(ci), y0);
  }
  __syncthreads();
  HPROF(2);
  uint32_t total;
  const uint32_t off = varblock_base<BR>(t, sTask, sWave, y0, &total);
  if (t.valid && t.sl == 0) sBase[me] = off;
  __syncthreads();
  HPROF(3);
  // one walk: clustered histogram, bit bound, and every token's 32-bit record
  // at its stream position.  Wave-parallel: each thread derives the walk state
  // of its own task (slice, channel); the wave then takes its 64 tasks one at
  // a time with lane = coefficient, so a task costs one pass whatever its token
  // count (no walk divergence) and its records are stored contiguously.
  // Per coefficient k >= lo: left_k = left - (non-zeros in [lo, k)) (ballot +
  // popcount), prev_k = the walk's start flag at lo, else (coef k-1 != 0);
  // token iff left_k > 0 -- the serial walk of block_tokens /
  // varblock_slice_tokens, restated.
  uint32_t bound = 0, nt[3] = {0, 0, 0};
  uint32_t* rec = a.tokens + (uint64_t)slot * kGroupTokStride + (uint64_t)band * kBandTokStride;
  uint32_t pos = t.valid ? sBase[(t.oby - y0) * 32 + t.obx] : 0u;
  const int lane = threadIdx.x & 63;
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  auto hist_add = [&](uint32_t clu, uint32_t tok) {
    const uint32_t bin = clu * kAcTok + tok;
    if (kWide)
      atomicAdd(&sHist[bin], 1u);
    else
      atomicAdd(&sHist[bin >> 1], 1u << ((bin & 1u) * 16u));
  };
#pragma unroll 1
  for (int ci = 0; ci < 3; ci++) {
    const int c = channel_of(ci);
    uint32_t idx = 0, cnt = 0, info = 0, info2 = 0, tok0 = 0;
    if (t.valid) {
      task_records<BR>(t, sTask, ci, y0, pos, idx, cnt);
      const int nz = (int)nzo[c];
      int left, prev;
      slice_state(t, L, c, y0, nz, left, prev);
      const int bctx = block_ctx_of(c, t.type);
      // info: left (16 bits) | prev << 16 | lcb << 17 (4 bits) | bctx << 21;
      // info2: the slice index (varblocks of up to 1024 blocks)
      info = (uint32_t)left | ((uint32_t)prev << 16) | ((uint32_t)t.lcb << 17) |
             ((uint32_t)bctx << 21);
      info2 = (uint32_t)t.sl;
      if (t.sl == 0) {  // the non-zero count token, written by the task's own thread
        const int pred = predict_nz(L.nz[c], t.bx, t.by, y0);
        uint32_t tok, nb, bits;
        hybrid420((uint32_t)nz, tok, nb, bits);
        const uint32_t clu = sClu[nz_bucket(pred) * kBlockCtx + bctx];
        hist_add(clu, tok);
        bound += 15u + nb;
        tok0 = ac_record(clu, tok, nb, bits);
        rec[idx] = tok0;
      }
      nt[0] += c == 0 ? cnt : 0u;
      nt[1] += c == 1 ? cnt : 0u;
      nt[2] += c == 2 ? cnt : 0u;
    }
    // tasks with coefficient tokens, taken kAcBatch at a time: their coefficient
    // loads are issued together (one memory latency per batch)
    const bool need = t.valid && cnt > (t.sl == 0 ? 1u : 0u);
    const uint32_t qoff = (uint32_t)((t.gb * 3 + c) * 64);
    uint64_t M = __ballot(need);
    while (M) {
      int js[kAcBatch];
#pragma unroll
      for (int u = 0; u < kAcBatch; u++) {
        js[u] = M ? (int)__builtin_ctzll(M) : -1;
        M = M ? M & (M - 1) : 0ull;
      }
      int32_t v8[kAcBatch];
#pragma unroll
      for (int u = 0; u < kAcBatch; u++)
        v8[u] = js[u] >= 0 ? a.ac[(uint32_t)__builtin_amdgcn_readlane((int)qoff, js[u]) + lane] : 0;
#pragma unroll
      for (int u = 0; u < kAcBatch; u++) {
        if (js[u] < 0) break;
        const int j = js[u];
        const uint32_t ij = (uint32_t)__builtin_amdgcn_readlane((int)info, j);
        const uint32_t idxj = (uint32_t)__builtin_amdgcn_readlane((int)idx, j);
        const int slj = __builtin_amdgcn_readlane((int)info2, j), lcbj = (ij >> 17) & 15;
        const int leftj = ij & 0xFFFF, prevj = (ij >> 16) & 1, bctxj = ij >> 21;
        const int cbj = 1 << lcbj;
        const int k = slj * 64 + lane;
        const int lo = max(slj * 64, cbj);
        const int32_t v = v8[u];
        const bool on = k >= cbj;
        const uint64_t m = __ballot(on && v != 0);
        const int left_k = leftj - __popcll(m & below);
        if (on && left_k > 0) {
          const int prev_k = k == lo ? prevj : (int)((m >> (lane - 1)) & 1);
          const int ctx = kBlockCtx * kNzBuckets + kZdCtx * bctxj +
                          (sNnzCtx[(left_k + cbj - 1) >> lcbj] + sFreqCtx[k >> lcbj]) * 2 + prev_k;
          uint32_t tok, nb, bits;
          hybrid420(pack_signed(v), tok, nb, bits);
          const uint32_t clu = sClu[ctx];
          hist_add(clu, tok);
          bound += 15u + nb;
          rec[idxj + (slj == 0 ? 1u : 0u) + (uint32_t)(k - lo)] = ac_record(clu, tok, nb, bits);
        }
      }
    }
  }
  atomicAdd(&sBound, bound);
  atomicAdd(&sNtok[0], nt[0]);
  atomicAdd(&sNtok[1], nt[1]);
  atomicAdd(&sNtok[2], nt[2]);
  __syncthreads();
  HPROF(4);
  for (int i = threadIdx.x; i < kHistWords; i += blockDim.x) {
    const uint32_t w = sHist[i];
    if (!w) continue;
    if (kWide) {
      atomicAdd(&a.hist[(i / kAcTok) * kAlpha + (i % kAcTok)], w);
      continue;
    }
    const int bin = 2 * i;
    if (w & 0xFFFFu) atomicAdd(&a.hist[(bin / kAcTok) * kAlpha + (bin % kAcTok)], w & 0xFFFFu);
    if (w >> 16) atomicAdd(&a.hist[((bin + 1) / kAcTok) * kAlpha + ((bin + 1) % kAcTok)], w >> 16);
  }
  // (bound and ntok: zeroed with the statistics arena; bandtok written here)
  if (threadIdx.x == 0) {
    atomicAdd(&a.bound[g], sBound);
    atomicAdd(&a.ntok[g * 3 + 0], sNtok[0]);
    atomicAdd(&a.ntok[g * 3 + 1], sNtok[1]);
    atomicAdd(&a.ntok[g * 3 + 2], sNtok[2]);
    a.bandtok[g * kBands + band] = total;
  }
  HPROF(5);
}
void launch_ac_hist(const AcArgs* a, uint32_t k, uint32_t ngroups, hipStream_t s, bool whole_group) {
  if (!ngroups || !k) return;
  if (whole_group)  // varblocks of 128 / 256 px (effort >= 8) span bands
    hipLaunchKernelGGL(ac_hist_kernel<32>, dim3(ngroups, 1, k), dim3(1024), 0, s, make_batch(a, k));
  else
    hipLaunchKernelGGL(ac_hist_kernel<8>, dim3(ngroups * kBands, 1, k), dim3(256), 0, s, make_batch(a, k));
}
hipError_t set_cluster_table(const uint8_t* tab, hipStream_t s) {
  return hipMemcpyToSymbolAsync(HIP_SYMBOL(c_cluster), tab, kAcCtx, 0, hipMemcpyHostToDevice, s);
}

}  // namespace jxg
