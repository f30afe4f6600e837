// jxg_decode.hip -- the decoder's pass groups on the GPU:
// one wave per pass group runs the token walk of jxg_decode_core.h, the same
// code the host path runs.  A pass group is one serial entropy stream (every
// token's context depends on the previous one and, with rANS, on the coder
// state), so the walk's state -- reader position, ANS state, left, k, the
// previous-token flag -- is wave-uniform: it derives from kernel arguments and
// blockIdx only, stays in scalar registers and the control flow never
// diverges.  The lanes do what is parallel around the chain: zeroing the
// group's coefficient area (a stream leaves most coefficients unwritten),
// filling the non-zero map of a varblock of several blocks (LDS, 3 KB),
// writing out the non-zero coefficients the chain collected in LDS (up to 512
// at a time) into the int16 natural-order slices recon_tile_kernel reads, and
// staging the decode tables in LDS: every token reads a context-map byte, a
// histogram descriptor and a table entry, each address depending on the load
// before, so their latency is the chain's step.  The stream's words are loaded
// with uniform addresses of consecutive words, which the caches serve; that
// is what stages the section's bytes.
#include <hip/hip_runtime.h>

#include <type_traits>

#define JXG_WAVE_SYNC() __syncthreads()
#define JXG_UNIFORM32(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#include "jxg_decode_plan.h"
#include "jxg_kernels.h"

namespace jxg {

constexpr int kDecLanes = 64;
// dynamic LDS: [non-zero map 3 KB | pending coefficients 2 KB | context-map slice of one preset | histogram
// descriptors | symbol tables when they fit], parts 8-byte aligned
constexpr uint32_t kDecNzs = 3 * 1024 + dec::kPendCoefs * 4;  // and the pending coefficients
constexpr uint32_t kDecMap = (dec::kAcCtxPerPreset + 7) & ~7u;
constexpr uint32_t kDecLdsMax = 60 * 1024;  // of the 64 KB a workgroup gets by default
// the batch planner (jxg_decode_plan.cpp, host only) restates the layout
static_assert(kDecPlanNzs == kDecNzs && kDecPlanMap == kDecMap && kDecPlanLdsMax == kDecLdsMax &&
                  kDecPlanHistBytes == sizeof(dec::HistDesc),
              "jxg_decode_plan.h: the LDS layout of the pass-group kernels");

uint32_t decode_groups_lds(DecodeArgs* a) {
  const uint32_t base = kDecNzs + kDecMap + ((a->nhist * (uint32_t)sizeof(dec::HistDesc) + 7) & ~7u);
  a->stage_tab = a->tab_bytes && a->tab_bytes <= kDecLdsMax - base ? 1u : 0u;
  return base + (a->stage_tab ? (a->tab_bytes + 7) & ~7u : 0u);
}

#define JXG_LDS __attribute__((address_space(3)))
// the walk's tables with LDS-qualified pointers (kTabLds: the symbol tables too)
template <bool kTabLds>
struct SymReaderLds {
  const JXG_LDS uint8_t* ctxmap;
  const JXG_LDS dec::HistDesc* hist;
  typename std::conditional<kTabLds, const JXG_LDS uint16_t*, const uint16_t*>::type ptab;
  typename std::conditional<kTabLds, const JXG_LDS dec::AnsEntry*, const dec::AnsEntry*>::type atab;
  uint32_t nctx, prefix, log_alpha, ctx_bias;
};

// one pass group `g` of the frame `a`, by the one-wave workgroup: the body of
// both kernels below
template <bool kTabLds>
__device__ __forceinline__ void decode_group(const DecodeArgs& a, const uint32_t g) {
  extern __shared__ __align__(8) uint8_t lds[];
  JXG_LDS uint8_t* nzs = (JXG_LDS uint8_t*)lds;
  JXG_LDS uint32_t* pend = (JXG_LDS uint32_t*)(lds + 3 * 1024);
  const uint32_t lane = threadIdx.x;
  const uint32_t gx = g % a.gxs, gy = g / a.gxs;
  dec::GroupGeom geom;
  geom.bx0 = gx * 32;
  geom.by0 = gy * 32;
  geom.gw = min(32u, a.bxs - geom.bx0);
  geom.gh = min(32u, a.bys - geom.by0);
  geom.bxs = a.bxs;
  dec::BitReader br{a.stream, a.sec[2 * g], a.sec[2 * g + 1], 0u, 0u, 0ull};
  // the preset the walk is about to read (it checks the range again): its
  // slice of the context map is what this group needs
  dec::BitReader ahead = br;
  const uint32_t preset = dec::br_read(ahead, a.preset_bits);
  if (ahead.err || preset >= a.npresets ||
      ((uint64_t)preset + 1) * dec::kAcCtxPerPreset > a.sym.nctx) {
    if (lane == 0) a.status[g] = (uint32_t)dec::kInvalid;  // as the walk would say
    return;
  }
  SymReaderLds<kTabLds> S;
  S.nctx = a.sym.nctx;
  S.prefix = a.sym.prefix;
  S.log_alpha = a.sym.log_alpha;
  S.ctx_bias = preset * dec::kAcCtxPerPreset;
  {
    uint8_t* map = lds + kDecNzs;
    const uint8_t* src = a.sym.ctxmap + (size_t)preset * dec::kAcCtxPerPreset;
    for (uint32_t i = lane; i < dec::kAcCtxPerPreset; i += kDecLanes) map[i] = src[i];
    S.ctxmap = (const JXG_LDS uint8_t*)map;
    // descriptors and tables: 4-byte words (both arrays are 4-byte aligned and sized)
    uint32_t* hist = reinterpret_cast<uint32_t*>(lds + kDecNzs + kDecMap);
    const uint32_t hw = a.nhist * (uint32_t)(sizeof(dec::HistDesc) / 4);
    const uint32_t* hsrc = reinterpret_cast<const uint32_t*>(a.sym.hist);
    for (uint32_t i = lane; i < hw; i += kDecLanes) hist[i] = hsrc[i];
    S.hist = (const JXG_LDS dec::HistDesc*)hist;
    if constexpr (kTabLds) {
      uint32_t* tab = hist + ((hw + 1) & ~1u);
      const uint32_t* tsrc = a.sym.prefix ? reinterpret_cast<const uint32_t*>(a.sym.ptab)
                                          : reinterpret_cast<const uint32_t*>(a.sym.atab);
      for (uint32_t i = lane; i < (a.tab_bytes + 3) / 4; i += kDecLanes) tab[i] = tsrc[i];
      S.ptab = (const JXG_LDS uint16_t*)tab;
      S.atab = (const JXG_LDS dec::AnsEntry*)tab;
    } else {
      S.ptab = a.sym.ptab;
      S.atab = a.sym.atab;
    }
  }
  // a row of the group's blocks is contiguous: gw * 192 int16 = gw * 96 words
  for (uint32_t by = 0; by < geom.gh; by++) {
    uint32_t* row = reinterpret_cast<uint32_t*>(
        a.ac + ((size_t)(geom.by0 + by) * a.bxs + geom.bx0) * 192);
    for (uint32_t i = lane; i < geom.gw * 96; i += kDecLanes) row[i] = 0u;
  }
  for (uint32_t i = lane; i < 3 * 1024; i += kDecLanes) nzs[i] = 0;
  __syncthreads();  // the tables are staged; the zeroes land before the coefficient stores
  const int st = dec::decode_pass_group(br, S, a.npresets, a.preset_bits, a.acs, geom, nzs, pend,
                                        a.ac, lane, kDecLanes);
  if (lane == 0) a.status[g] = (uint32_t)st;
}

template <bool kTabLds>
__global__ __launch_bounds__(kDecLanes) void decode_groups_kernel(DecodeArgs a) {
  decode_group<kTabLds>(a, blockIdx.x);
}

// Batch (jxg_decode_batch_rgb8): one wave per work item (frame, group) of a
// list that spans the frames of a chunk; the frame's arguments come from a
// descriptor in memory.  Work item and descriptor are read at addresses that
// depend on kernel arguments and blockIdx only, and every field is named
// uniform, so the walk's state stays in scalar registers as in the kernel
// above.  a.status of a descriptor is the frame's first status word.

// A pointer read from the descriptor: uniform, and named a global-memory
// pointer -- one loaded from memory is generic to the compiler, which would
// make every access through it a flat operation (they wait on both memory
// counters) where the kernel above, whose pointers are kernel arguments, has
// global loads and scalar loads.
template <class T>
__device__ __forceinline__ T* uni_global(T* p) {
  typedef T __attribute__((address_space(1))) * Global;
  return (T*)(Global)dec::uni64(reinterpret_cast<uint64_t>(p));
}

template <bool kTabLds>
__global__ __launch_bounds__(kDecLanes) void decode_batch_kernel(
    const DecodeArgs* __restrict__ frames, const DecWork* __restrict__ work) {
  const uint32_t frame = dec::uni(work[blockIdx.x].frame);
  const uint32_t g = dec::uni(work[blockIdx.x].group);
  const DecodeArgs* d = frames + frame;
  DecodeArgs a;
  a.stream = uni_global(d->stream);
  a.sec = uni_global(d->sec);
  a.sym.ctxmap = uni_global(d->sym.ctxmap);
  a.sym.hist = uni_global(d->sym.hist);
  a.sym.ptab = uni_global(d->sym.ptab);
  a.sym.atab = uni_global(d->sym.atab);
  a.sym.nctx = dec::uni(d->sym.nctx);
  a.sym.prefix = dec::uni(d->sym.prefix);
  a.sym.log_alpha = dec::uni(d->sym.log_alpha);
  a.sym.ctx_bias = 0u;
  a.npresets = dec::uni(d->npresets);
  a.preset_bits = dec::uni(d->preset_bits);
  a.acs = uni_global(d->acs);
  a.ac = uni_global(d->ac);
  a.status = uni_global(d->status);
  a.bxs = dec::uni(d->bxs);
  a.bys = dec::uni(d->bys);
  a.gxs = dec::uni(d->gxs);
  a.nhist = dec::uni(d->nhist);
  a.tab_bytes = dec::uni(d->tab_bytes);
  a.stage_tab = kTabLds ? 1u : 0u;
  decode_group<kTabLds>(a, g);
}

hipError_t launch_decode_batch(const DecodeArgs* d_frames, const DecWork* d_work, uint32_t nwork,
                               bool staged, uint32_t lds, hipStream_t s) {
  if (nwork == 0) return hipSuccess;
  if (staged)
    hipLaunchKernelGGL(decode_batch_kernel<true>, dim3(nwork), dim3(kDecLanes), lds, s, d_frames,
                       d_work);
  else
    hipLaunchKernelGGL(decode_batch_kernel<false>, dim3(nwork), dim3(kDecLanes), lds, s, d_frames,
                       d_work);
  return hipGetLastError();
}

hipError_t launch_decode_groups(const DecodeArgs& a, uint32_t ngroups, hipStream_t s) {
  DecodeArgs b = a;
  const uint32_t lds = decode_groups_lds(&b);
  if (b.stage_tab)
    hipLaunchKernelGGL(decode_groups_kernel<true>, dim3(ngroups), dim3(kDecLanes), lds, s, b);
  else
    hipLaunchKernelGGL(decode_groups_kernel<false>, dim3(ngroups), dim3(kDecLanes), lds, s, b);
  return hipGetLastError();
}

}  // namespace jxg
