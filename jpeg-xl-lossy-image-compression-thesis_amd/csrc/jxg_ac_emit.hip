// jxg_ac_emit.hip -- prefix-code emission of the pass groups' AC tokens on
// gfx950, from the token records ac_hist_kernel wrote (jxg_acrec.h) alone: no
// coefficient walk.  One 1024-thread workgroup per pass group: a contiguous
// record range per wave, coalesced reads, wave scans of the code lengths ->
// LDS bit buffer (ds_or), copied out with plain 4-byte stores (global atomics
// only for groups larger than the buffer).
#include "jxg_device.h"
#include "jxg_kernels.h"
#include "jxg_acrec.h"

namespace jxg {

constexpr int kAcThreads = 1024;
// LDS bit buffer of ac_emit (groups whose exact size exceeds it
// fall back to global atomics): 96 KiB = 786432 bits = 12 bpp over a full
// 256x256 group, so only near-incompressible groups take the slow path
// (ac_emit: 96 KiB + 33 KiB of code tables, one 1024-thread workgroup per CU)
constexpr int kEmitLdsWords = 24576;

// wave w owns a contiguous record range; lanes read consecutive records
// (coalesced), the wave's bit total -> workgroup offsets; then per 64
// records a wave inclusive scan of the lengths gives every record its bit
// position, and each lane ORs its <= 28 bits into the LDS bit buffer (global
// atomics for groups larger than the buffer)
__global__ __launch_bounds__(kAcThreads) void ac_emit_kernel(AcArgs a) {
  __shared__ uint32_t sCode[kMaxClusters * kAcTok];
  __shared__ __attribute__((aligned(16))) uint32_t sBits[kEmitLdsWords];
  __shared__ uint32_t sWave[kAcThreads / 64];
  const int g = (int)slot_group(a.glist, a.g0, blockIdx.x);
  for (int i = threadIdx.x; i < kMaxClusters * kAcTok; i += blockDim.x)
    sCode[i] = a.codes[(i / kAcTok) * kAlpha + (i % kAcTok)];
  for (int i = threadIdx.x; i < kEmitLdsWords / 4; i += blockDim.x)
    reinterpret_cast<uint4*>(sBits)[i] = make_uint4(0, 0, 0, 0);
  const uint32_t n = group_tokens(a.ntok, g);
  const uint32_t* rec = a.tokens + (uint64_t)blockIdx.x * kGroupTokStride;
  uint32_t bt[kBands];
#pragma unroll
  for (int i = 0; i < kBands; i++) bt[i] = a.bandtok[g * kBands + i];
  constexpr int kWaves = kAcThreads / 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t chunk = ((n + kWaves * 64 - 1) / (kWaves * 64)) * 64;
  const uint32_t lo = min(n, wv * chunk), hi = min(n, lo + chunk);
  __syncthreads();
  auto code_of = [&](uint32_t r) { return sCode[rec_cluster(r) * kAcTok + rec_token(r)]; };
  uint32_t tot = 0;
  for (uint32_t k = lo + lane; k < hi; k += 64) {
    const uint32_t r = rec[rec_index(bt, k)];
    tot += (code_of(r) >> 16) + rec_nbits(r);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) tot += __shfl_xor(tot, d, 64);
  if (lane == 0) sWave[wv] = tot;
  __syncthreads();
  uint32_t run = 0, total = 0;
#pragma unroll
  for (int i = 0; i < kWaves; i++) {
    const uint32_t x = sWave[i];
    run += i < wv ? x : 0u;
    total += x;
  }
  const uint64_t base = a.base[g];  // word aligned
  const bool lds = total <= (uint32_t)kEmitLdsWords * 32u;
  if (!lds) {  // the section's scratch words zeroed before the global ORs (no arena memset)
    for (uint32_t i = threadIdx.x; i < (total + 31) / 32; i += blockDim.x) a.scratch[(base >> 5) + i] = 0;
    __threadfence();
    __syncthreads();
  }
  uint32_t* buf = lds ? sBits : a.scratch;
  const uint64_t bias = lds ? 0 : base;
  for (uint32_t k0 = lo; k0 < hi; k0 += 64) {
    const uint32_t k = k0 + lane;
    uint32_t len = 0, val = 0;
    if (k < hi) {
      const uint32_t r = rec[rec_index(bt, k)], cl = code_of(r);
      len = (cl >> 16) + rec_nbits(r);
      // code (<= 15 bits) and raw bits (<= 13): one <= 28-bit value
      val = (cl & 0xFFFFu) | (rec_bits(r) << (cl >> 16));
    }
    const uint32_t incl = wave_incl_scan(len);
    if (len) {
      const uint64_t pos = bias + run + incl - len;
      const uint64_t w = pos >> 5;
      const uint32_t sh = (uint32_t)(pos & 31);
      atomicOr(&buf[w], val << sh);
      if (sh + len > 32) atomicOr(&buf[w + 1], val >> (32 - sh));
    }
    run += __shfl(incl, 63, 64);
  }
  if (lds) {
    __syncthreads();
    const uint32_t nw = (total + 31) / 32;
    uint32_t* dst = a.scratch + (base >> 5);
    for (uint32_t i = threadIdx.x; i < nw; i += blockDim.x) dst[i] = sBits[i];
  }
  if (threadIdx.x == 0) a.bits[g] = total;
}

void launch_ac_emit(const AcArgs& a, uint32_t ngroups, hipStream_t s) {
  if (ngroups) hipLaunchKernelGGL(ac_emit_kernel, dim3(ngroups), dim3(kAcThreads), 0, s, a);
}

}  // namespace jxg
