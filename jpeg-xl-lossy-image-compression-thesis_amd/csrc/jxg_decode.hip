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
#include "jxg_kernels.h"

namespace jxg {

constexpr int kDecLanes = 64;
// dynamic LDS: [non-zero map 3 KB | pending coefficients 2 KB | context-map slice of one preset | histogram
// descriptors | symbol tables when they fit], parts 8-byte aligned
constexpr uint32_t kDecNzs = 3 * 1024 + dec::kPendCoefs * 4;  // and the pending coefficients
constexpr uint32_t kDecMap = (dec::kAcCtxPerPreset + 7) & ~7u;
constexpr uint32_t kDecLdsMax = 60 * 1024;  // of the 64 KB a workgroup gets by default

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

template <bool kTabLds>
__global__ __launch_bounds__(kDecLanes) void decode_groups_kernel(DecodeArgs a) {
  extern __shared__ __align__(8) uint8_t lds[];
  JXG_LDS uint8_t* nzs = (JXG_LDS uint8_t*)lds;
  JXG_LDS uint32_t* pend = (JXG_LDS uint32_t*)(lds + 3 * 1024);
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
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
