// jxg_merge_write.hip -- the merge stage behind merge_eval (jxg_merge.hip):
// the chosen varblocks, from the decisions to the coefficients.  The three
// kernels share one contract, the per-shape lists in MergeArgs::work
// (jxg_shapes.h: merge_list_off, kShapeSlots).
//   merge_resolve one wave per tile: per level (16, 32, 64 px) and region,
//                 keep / full / two tall / two wide halves with the
//                 TryMergeAcs comparison (`candidate >= current` keeps: NaN
//                 estimates are accepted, combined.diff:294 context).  Every
//                 chosen varblock (tile, first block) is appended to the list
//                 of its shape.
//   force_list    a forced encode's producer of the same lists, from the
//                 caller's strategy map.
//   merge_write   persistent workgroups over dense passes: a pass is one shape
//                 and up to NV(shape) entries of its list, entry k in slot k
//                 of the 64x64 LDS image whatever tile it comes from, so a
//                 pass costs what the chosen area costs (one workgroup per
//                 (tile, shape) ran 0.28 full at 8K).  The transform +
//                 quantization of jxg_merge_kernel.h with the source tile, the
//                 block origin and the chroma-from-luma factors per slot
//                 (WriteLds), coefficients scattered to natural-order slices
//                 of the covered blocks, non-zero counts, quant field, and the
//                 DC of each covered block from the LLF.  A varblock's results
//                 depend on its own pixels and blocks only, not on its slot or
//                 pass.
// Float op order == oracle/merge.c (jxo_varblock, jxo_llf_dc, jxo_merge_tile).
// (merge_write shares its unit with the two list kernels for its code's sake
// too: compiled as the only kernel of a unit it comes out as other code, 145
// mnemonic lines of 16156 -- DESIGN.md 3.13.)
#include <type_traits>

#include "jxg_merge_kernel.h"

namespace jxg {

// one wave per tile (16 tiles per workgroup): levels in order, one lane per
// region; then every chosen varblock (tile << 6 | first block) goes to its
// shape's merge_write list (one global atomic per workgroup and shape; list
// order varies from run to run, what merge_write stores does not)
constexpr int kResolveWaves = 16;
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__global__ __launch_bounds__(64 * kResolveWaves) void merge_resolve_kernel(Batch<MergeArgs> bt_) {
  const MergeArgs& a = bt_.a[blockIdx.z];
  __shared__ float sEntW[kResolveWaves][64];
  __shared__ uint8_t sAcsW[kResolveWaves][64];
  __shared__ uint32_t sCnt[kResolveWaves][kNumShapes];
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  float* sEnt = sEntW[wv];
  uint8_t* sAcs = sAcsW[wv];
  const int idx = blockIdx.x * kResolveWaves + wv;
  int my = -1;  // shape of the chosen varblock whose first block is this lane's
  int tile = 0;
  if (idx < (int)a.ntiles) {
    tile = a.tile_list ? (int)a.tile_list[idx] : idx;
    const int tx = tile % (int)a.tiles_x, ty = tile / (int)a.tiles_x;
    const int nbx = min(8, (int)a.bxs - tx * 8), nby = min(8, (int)a.bys - ty * 8);
    const int lbx = t & 7, lby = t >> 3;
    const bool in = lbx < nbx && lby < nby;
    const size_t gb = (size_t)(ty * 8 + lby) * a.bxs + tx * 8 + lbx;
    sEnt[t] = in ? a.ent[gb] : 0.0f;
    sAcs[t] = in ? a.acs[gb] : 0;
    wave_sync_lds();
    const float* cost = a.cost + (size_t)tile * kNumShapes * 32;
    for (int s = 2; s <= a.max_s && s <= nbx && s <= nby; s *= 2) {
      const int nr = 8 / s;
      const int full = s == 2 ? 2 : (s == 4 ? 5 : 8);
      const int tall = s == 2 ? 0 : (s == 4 ? 3 : 6);
      if (t < nr * nr) {
        const int rx = t % nr, ry = t / nr;
        if ((rx + 1) * s <= nbx && (ry + 1) * s <= nby) {
          float cur = 0.0f;
          for (int iy = 0; iy < s; iy++)
            for (int ix = 0; ix < s; ix++) cur += sEnt[(ry * s + iy) * 8 + rx * s + ix];
          // varblock grid indices: full (8/s per row), tall (16/s), wide (8/s)
          const int vf = ry * nr + rx, vl = ry * (16 / s) + 2 * rx, vt = (2 * ry) * nr + rx;
          const float e0 = cost[full * 32 + vf];
          const float el = cost[tall * 32 + vl], er = cost[tall * 32 + vl + 1];
          const float etop = cost[(tall + 1) * 32 + vt], ebot = cost[(tall + 1) * 32 + vt + nr];
          const float et = el + er, ew = etop + ebot;
          float best = cur;
          int choice = 0;
          if (!(e0 >= best)) {
            best = e0;
            choice = 1;
          }
          if (!(et >= best)) {
            best = et;
            choice = 2;
          }
          if (!(ew >= best)) {
            best = ew;
            choice = 3;
          }
          for (int j = 0; choice && j < (choice == 1 ? 1 : 2); j++) {
            int sh, bx, by;
            float e;
            if (choice == 1) {
              sh = full, bx = rx * s, by = ry * s, e = e0;
            } else if (choice == 2) {
              sh = tall, bx = rx * s + j * (s / 2), by = ry * s, e = j ? er : el;
            } else {
              sh = tall + 1, bx = rx * s, by = ry * s + j * (s / 2), e = j ? ebot : etop;
            }
            const int cy = 1 << kShapes[sh].lcy, cx = 1 << kShapes[sh].lcx;
            for (int iy = 0; iy < cy; iy++)
              for (int ix = 0; ix < cx; ix++) {
                const int b = (by + iy) * 8 + bx + ix;
                sAcs[b] = (uint8_t)(kShapes[sh].type | ((iy | ix) ? 0x80 : 0));
                sEnt[b] = (iy | ix) ? 0.0f : e;
              }
          }
        }
      }
      wave_sync_lds();
    }
    if (in) {
      a.acs[gb] = sAcs[t];
      a.ent[gb] = sEnt[t];  // the decisions' estimates: the 128 / 256 px levels' "current"
    }
    // the chosen varblock this block starts, if any
    if (in && !(sAcs[t] & 0x80)) {
#pragma unroll
      for (int si = 0; si < kNumShapes; si++) my = sAcs[t] == kShapes[si].type ? si : my;
    }
  }
  // per shape: the wave's varblocks counted, then one slot range per
  // workgroup (one atomic per shape that has any), lanes in block order
  uint32_t rank = 0;
#pragma unroll
  for (int si = 0; si < kNumShapes; si++) {
    const uint64_t bal = __ballot(my == si);
    if (t == 0) sCnt[wv][si] = (uint32_t)__popcll(bal);
    if (my == si) rank = (uint32_t)__popcll(bal & ((1ull << t) - 1ull));
  }
  __syncthreads();
  if (threadIdx.x < kNumShapes) {
    const int si = threadIdx.x;
    uint32_t tot = 0;
    for (int w = 0; w < kResolveWaves; w++) tot += sCnt[w][si];
    uint32_t base = tot ? atomicAdd(a.work + si, tot) : 0u;
    for (int w = 0; w < kResolveWaves; w++) {  // count -> the wave's first slot
      const uint32_t n = sCnt[w][si];
      sCnt[w][si] = base;
      base += n;
    }
  }
  __syncthreads();
  if (my >= 0)
    a.work[merge_list_off(my, a.ntiles) + sCnt[wv][my] + rank] = (uint32_t)tile << 6 | (uint32_t)t;
}

// Forced encode (jxg_encode_forced_rgb8): the second producer
// of merge_write's lists, in the place of merge_eval + merge_resolve.  One wave
// per tile, one lane per block: the bytes of the caller's map (a.force,
// validated on the host: every merged varblock lies inside its tile and the
// frame, none overlap) that belong to merged varblocks go into a.acs -- the
// front kernel wrote the 8x8-class ones -- and every merged first block is
// appended to its shape's list by resolve's scheme (a ballot per shape, one
// global atomic per workgroup and shape).  A tile holds at most 64 / blocks
// varblocks of a shape at any placement, which is the lists' capacity.  The
// nine counts are zeroed by the launch (launch_force_merge), not here: a
// workgroup cannot clear what another may already have added to.
__global__ __launch_bounds__(64 * kResolveWaves) void force_list_kernel(MergeArgs a) {
  __shared__ uint32_t sCnt[kResolveWaves][kNumShapes];
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  const int idx = blockIdx.x * kResolveWaves + wv;
  int my = -1;  // shape of the forced varblock whose first block is this lane's
  int tile = 0;
  if (idx < (int)a.ntiles) {
    tile = a.tile_list ? (int)a.tile_list[idx] : idx;
    const int tx = tile % (int)a.tiles_x, ty = tile / (int)a.tiles_x;
    const int nbx = min(8, (int)a.bxs - tx * 8), nby = min(8, (int)a.bys - ty * 8);
    const int lbx = t & 7, lby = t >> 3;
    if (lbx < nbx && lby < nby) {
      const size_t gb = (size_t)(ty * 8 + lby) * a.bxs + tx * 8 + lbx;
      const uint8_t v = a.force[gb];
      int sh = -1;
#pragma unroll
      for (int si = 0; si < kNumShapes; si++) sh = (v & 0x7F) == kShapes[si].type ? si : sh;
      if (sh >= 0) a.acs[gb] = v;
      if (!(v & 0x80)) my = sh;
      a.ent[gb] = 0.0f;
    }
  }
  uint32_t rank = 0;
#pragma unroll
  for (int si = 0; si < kNumShapes; si++) {
    const uint64_t bal = __ballot(my == si);
    if (t == 0) sCnt[wv][si] = (uint32_t)__popcll(bal);
    if (my == si) rank = (uint32_t)__popcll(bal & ((1ull << t) - 1ull));
  }
  __syncthreads();
  if (threadIdx.x < kNumShapes) {
    const int si = threadIdx.x;
    uint32_t tot = 0;
    for (int w = 0; w < kResolveWaves; w++) tot += sCnt[w][si];
    uint32_t base = tot ? atomicAdd(a.work + si, tot) : 0u;
    for (int w = 0; w < kResolveWaves; w++) {  // count -> the wave's first slot
      const uint32_t n = sCnt[w][si];
      sCnt[w][si] = base;
      base += n;
    }
  }
  __syncthreads();
  if (my >= 0)
    a.work[merge_list_off(my, a.ntiles) + sCnt[wv][my] + rank] = (uint32_t)tile << 6 | (uint32_t)t;
}

void launch_merge_resolve(const Batch<MergeArgs>& b, uint32_t k, hipStream_t s) {
  hipLaunchKernelGGL(merge_resolve_kernel,
                     dim3((b.a[0].ntiles + kResolveWaves - 1) / kResolveWaves, 1, k),
                     dim3(64 * kResolveWaves), 0, s, b);
}
void launch_force_list(const MergeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(force_list_kernel, dim3((a.ntiles + kResolveWaves - 1) / kResolveWaves),
                     dim3(64 * kResolveWaves), 0, s, a);
}

// ---------------------------------------------------------------------------
// merge_write
// ---------------------------------------------------------------------------
__constant__ float c_llf_p[4 * 8];   // [log2 M][k]
__constant__ float c_llf_ib[4 * 64]; // [log2 M][n][k]
#ifndef JXG_MERGE_WRITE_WPE
// write: 3 waves / SIMD (168 VGPRs, 8 B of scratch since round 6's column
// halves; 2: 195 VGPRs, no scratch, merge stage 1.94 vs 1.85 ms in round 5,
// profiles/r05zp).  4 (128 VGPRs, 120 B = 39 spilled VGPRs, past
// tests/test_isa_lint.py's 32) ran 0.301 vs 0.308 ms (profiles/r06mw): not
// worth the spill traffic it hides
#define JXG_MERGE_WRITE_WPE 3
#endif
// Two working coefficient planes: plane 0 holds Y (its dequantized values
// after the Y quantization, for the X / B residuals), plane 1 X, then B -- B
// is transformed into plane 1 once X is quantized.  gfx950 allocates LDS in
// 1280-byte granules: the two planes (38.3 KB) leave room for three
// workgroups per CU.
// Slot v of the image holds a varblock of any tile (a dense pass), so what the
// eval kernel derives from (P.tile, P.by0(v), P.bx0(v)) is per slot here; the
// image position of a slot stays P.off(v, plane).
struct WriteLds {
  static constexpr bool kWrite = true;
  float co[2 * kMPlane];  // coefficient image of the pass's varblocks
  float llf[3][64];       // the LLF of covered block b of the image, per channel
  float qsum[3][4][32];   // [Y, X, B][chunk][varblock]: column-tree chunk sums
  float btab[256];        // AdjustQuantBias of a magnitude q < 256 (setup_slots)
  float vr3[32][3];       // (unused; the image keeps its size)
  int vbits[32];          // per varblock: rate bits
  int vnz[32][3];         //               non-zeros per channel
  int vraw[32];           //               max quant field
  int valid[32];
  uint8_t braw[64];       // (unused, as is `any`)
  int any;
  uint32_t ssrc[32];  // a.xyb offset (floats) of the varblock's first pixel, channel 0
  uint32_t sgb[32];   // frame block index of its first block
  float skc[2][32];   // its tile's chroma-from-luma factors: X, B
};
// rows: C-point DCT of every row of every valid varblock, read straight
// from the tile-major XYB copy (16-byte loads; a thread issues all its rows'
// loads before the first transform; the source row comes from the slot's own
// tile and origin) into the LDS coefficient image.  For C = 64 two lanes
// share a row (Lee halves), each reading the whole row.
template <int C, int NCH>
__device__ __forceinline__ void row_pass(const MergeArgs& a, const Pass& P, WriteLds& S, int pass) {
  const int R = P.R(), lvr = P.lNV() + P.lR();
  if constexpr (C == 64) {
    // item = (row pair, half h): rows r and r + 1 of one varblock and channel
    // (R >= 32: pairs never straddle a varblock); h is wave-uniform: waves
    // alternate h over 64-pair chunks
    const int npairs = NCH * P.NV() * R / 2;  // 64 / 32
    const int n = ((npairs + 63) >> 6) << 7;
    for (int i = threadIdx.x; i < n; i += kMThreads) {
      const int h = (i >> 6) & 1, pp = ((i >> 7) << 6) | (i & 63), r = pp * 2;
      if (pp >= npairs) continue;
      const int c = r >> lvr, v = (r >> P.lR()) & (P.NV() - 1), y = r & (R - 1);
      if (!S.valid[v]) continue;
      const float* src0 = a.xyb + S.ssrc[v] + pass_src(pass, c) * 4096 + y * 64;
      const float4* s0 = reinterpret_cast<const float4*>(src0);
      const float4* s1 = s0 + 16;  // row y + 1
      f2 t[32];
      // 16-byte loads of x[4q..4q+3] and of its mirror x[60-4q..63-4q]
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const float4 a0 = s0[q], b0 = s0[15 - q], a1 = s1[q], b1 = s1[15 - q];
        const float fa0[4] = {a0.x, a0.y, a0.z, a0.w}, fb0[4] = {b0.x, b0.y, b0.z, b0.w};
        const float fa1[4] = {a1.x, a1.y, a1.z, a1.w}, fb1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int j = 0; j < 4; j++)
          t[4 * q + j] = dctN_first<64>(f2{fa0[j], fa1[j]}, f2{fb0[3 - j], fb1[3 - j]}, 4 * q + j, h);
      }
      const int off = P.off(v, pass_plane(pass, c)) + y * kMS;
      dctN_rest<64>(t, h, [&](int k, f2 o) {
        S.co[off + 2 * k + h] = o.x;
        S.co[off + kMS + 2 * k + h] = o.y;
      });
    }
  } else {
    // thread: row pairs (r, r + 256) -- two rows per transform (f2 lanes).
    // Row r of a channel: the varblock column is the fastest index, so the
    // lanes of a wave read whole 256-byte tile rows (coalesced) instead of
    // one C-float chunk per cache line
    constexpr int PER = (NCH * 4096 / C + kMThreads - 1) / kMThreads;  // 2 ch: 4, 2, 1
    const int nrows = NCH * P.NV() * R;
    const int lgx = P.lGX();
    auto row_of = [&](int rr, int& c, int& v, int& y) {
      c = rr >> lvr;
      const int i = rr & ((1 << lvr) - 1);
      y = (i >> lgx) & (R - 1);
      v = ((i >> (lgx + P.lR())) << lgx) | (i & ((1 << lgx) - 1));
    };
    float buf[PER][C];
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int r = threadIdx.x + k * kMThreads;
      if (r < nrows) {
        int c, v, y;
        row_of(r, c, v, y);
        // (an empty slot reads tile 0: in bounds, never stored)
        load_row<C>(a.xyb + S.ssrc[v] + pass_src(pass, c) * 4096 + y * 64, buf[k]);
      } else {
#pragma unroll
        for (int q = 0; q < C; q++) buf[k][q] = 0.0f;
      }
    }
    constexpr int l = ilog2c<C>();
#pragma unroll
    for (int k = 0; k < PER; k += 2) {
      const int r0 = threadIdx.x + k * kMThreads, r1 = r0 + kMThreads;
      if (r0 >= nrows) continue;
      int c0, v0, y0, c1, v1, y1;
      row_of(r0, c0, v0, y0);
      row_of(r1, c1, v1, y1);
      const bool ok0 = S.valid[v0], ok1 = k + 1 < PER && r1 < nrows && S.valid[v1];
      if (!ok0 && !ok1) continue;
      if (k + 1 < PER) {
        f2 x[C];
#pragma unroll
        for (int q = 0; q < C; q++) x[q] = f2{buf[k][q], buf[k + 1][q]};
        lee<C>(x);
        const int off0 = P.off(v0, pass_plane(pass, c0)) + y0 * kMS,
                  off1 = P.off(v1, pass_plane(pass, c1)) + y1 * kMS;
#pragma unroll
        for (int q = 0; q < C; q++) {
          const f2 o = x[q] * kLeeS[l][q];
          if (ok0) S.co[off0 + q] = o.x;
          if (ok1) S.co[off1 + q] = o.y;
        }
      } else {
        float* x = buf[k];
        lee<C>(x);
        const int off0 = P.off(v0, pass_plane(pass, c0)) + y0 * kMS;
#pragma unroll
        for (int q = 0; q < C; q++) S.co[off0 + q] = x[q] * kLeeS[l][q];
      }
    }
  }
}
// transform + quantize every valid varblock of the pass; leaves per-varblock
// bits / non-zeros in LDS.  (merge_eval runs the same lee / col_pass /
// quant_pass bodies with the row pass shared by the shapes of a width:
// family_rows, jxg_merge.hip.)
__device__ __forceinline__ void transform_quant(const MergeArgs& a, const Pass& P, WriteLds& S) {
  auto transform = [&](auto nch_tag, int pass) {
    constexpr int NCH = decltype(nch_tag)::value;
    switch (P.lcx) {
      case 0: row_pass<8, NCH>(a, P, S, pass); break;
      case 1: row_pass<16, NCH>(a, P, S, pass); break;
      case 2: row_pass<32, NCH>(a, P, S, pass); break;
      default: row_pass<64, NCH>(a, P, S, pass); break;
    }
    __syncthreads();
    switch (P.lcy) {
      case 0: col_pass<8, NCH>(P, S, pass); break;
      case 1: col_pass<16, NCH>(P, S, pass); break;
      case 2: col_pass<32, NCH>(P, S, pass); break;
      default: col_pass<64, NCH>(P, S, pass); break;
    }
  };
  transform(std::integral_constant<int, 2>(), 0);  // Y -> plane 0, X -> plane 1
  // Y first: its dequantized values replace its coefficients (X / B
  // residuals); then X; then B is transformed into X's plane.  Every pass's
  // tables are in flight across the barrier before it.  A lane's X / B items
  // read the Y values its own Y item wrote (same item map).
  auto quant_yx = [&](auto rpc_tag) {
    constexpr int RPC = decltype(rpc_tag)::value;
    {
      QTab<RPC> ty;
      load_qtab<RPC, true, 1>(a, P, ty);
      __syncthreads();
      quant_pass<RPC, 1>(a, P, S, ty);
    }
    QTab<RPC> tx;
    load_qtab<RPC, true, 0>(a, P, tx);
    quant_pass<RPC, 0>(a, P, S, tx);
  };
  auto quant_b = [&](auto rpc_tag) {
    constexpr int RPC = decltype(rpc_tag)::value;
    QTab<RPC> tb;
    load_qtab<RPC, true, 2>(a, P, tb);
    __syncthreads();
    quant_pass<RPC, 2>(a, P, S, tb);
  };
  if (P.lcy == 0) quant_yx(std::integral_constant<int, 8>());
  else quant_yx(std::integral_constant<int, 16>());
  __syncthreads();  // plane 1 (X) fully read
  transform(std::integral_constant<int, 1>(), 1);  // B -> plane 1
  if (P.lcy == 0) quant_b(std::integral_constant<int, 8>());
  else quant_b(std::integral_constant<int, 16>());
  __syncthreads();
}
// write: slot v takes entry first + v of the shape's list (n entries in this
// pass; the empty slots of a shape's last pass are invalid): its tile's XYB
// and chroma-from-luma factors, its first block in the frame; sums reset
__device__ __forceinline__ void setup_slots(const MergeArgs& a, const Pass& P, WriteLds& S,
                                            const uint32_t* list, uint32_t first, uint32_t n) {
  (void)P;
  const int v = threadIdx.x;
  if (v < 32) {
    const bool ok = (uint32_t)v < n;
    uint32_t src = 0, gb0 = 0;
    float kx = 0.0f, kb = 0.0f;
    if (ok) {
      const uint32_t e = list[first + v], tile = e >> 6, by = (e >> 3) & 7u, bx = e & 7u;
      const uint32_t tx = tile % a.tiles_x, ty = tile / a.tiles_x;
      src = tile * (3u * 4096u) + by * (8u * 64u) + bx * 8u;
      gb0 = (ty * 8u + by) * a.bxs + tx * 8u + bx;
      // chroma from luma of the tile (front kernel): X - kx Yd, B - kb Yd
      kx = (float)a.cmap[tile] * (1.0f / 84.0f);
      kb = 1.0f + (float)a.cmap[a.ntiles_all + tile] * (1.0f / 84.0f);
    }
    S.ssrc[v] = src;
    S.sgb[v] = gb0;
    S.skc[0][v] = kx;
    S.skc[1][v] = kb;
    S.valid[v] = ok;
    S.vraw[v] = 0;  // (vraw_slots: atomic max over the covered blocks)
    S.vbits[v] = 0;
    S.vnz[v][0] = S.vnz[v][1] = S.vnz[v][2] = 0;
  }
  fill_btab(S);
}
// write: the varblock quant field as in vraw_pass, one thread per image
// block, the block's front-kernel value read from the slot's own varblock:
// no other pass stores to those blocks (varblocks are disjoint), and this
// slot stores them only after the maxima are taken
__device__ __forceinline__ void vraw_slots(const MergeArgs& a, const Pass& P, WriteLds& S) {
  const int b = threadIdx.x;
  if (b < 64) {
    const int lbx = b & 7, lby = b >> 3;
    const int v = ((lby >> P.lcy) << P.lGX()) | (lbx >> P.lcx);
    if (v < P.NV() && S.valid[v]) {
      const size_t gb = (size_t)S.sgb[v] + (size_t)(lby & (P.cy() - 1)) * a.bxs + (lbx & (P.cx() - 1));
      atomicMax(&S.vraw[v], (int)a.qf[gb] + 1);
    }
  }
}
// one dense pass: entries first .. first + n - 1 of shape si's list, entry k
// in slot k of the image; returns after its last LDS use
__device__ __forceinline__ void write_pass(const MergeArgs& a, int si, uint32_t first, uint32_t n,
                                           WriteLds& S) {
  const Pass P = make_pass(a, 0, si);  // (tile, tx, ty: per slot, S.ssrc / S.sgb)
  setup_slots(a, P, S, a.work + merge_list_off(si, a.ntiles), first, n);
  __syncthreads();
  vraw_slots(a, P, S);
  transform_quant(a, P, S);
  // per covered block: non-zero counts, quant field, LLF-derived DC
  const int cb = P.cy() * P.cx(), lcb = P.lcy + P.lcx;
  const size_t nb = (size_t)a.bxs * a.bys;
  const int ly = P.lcy, lx = P.lcx;
  for (int i = threadIdx.x; i < P.NV() * cb; i += kMThreads) {
    const int v = i >> lcb, k = i & (cb - 1);
    if (!S.valid[v]) continue;
    const int iy = k >> P.lcx, ix = k & (P.cx() - 1);
    const int bx0 = P.bx0(v), by0 = P.by0(v);  // image position (the LLF's index)
    const size_t gb = (size_t)S.sgb[v] + (size_t)iy * a.bxs + ix;
    for (int c = 0; c < 3; c++) {
      const int n = S.vnz[v][c];
      a.nz[c * nb + gb] = (uint16_t)(k == 0 ? n : (n + cb - 1) >> lcb);
    }
    // the LLF -> DC tables of this block in registers (static indices, loop
    // bounds cx, cy <= 8 as predicates): no dependent constant loads
    float px[8], py[8], ibx[8], iby[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      px[k] = c_llf_p[lx * 8 + k];
      py[k] = c_llf_p[ly * 8 + k];
      ibx[k] = c_llf_ib[lx * 64 + ix * 8 + k];
      iby[k] = c_llf_ib[ly * 64 + iy * 8 + k];
    }
    const int cx = P.cx(), cy = P.cy();
    float dc[3];
#pragma unroll 1
    for (int c = 0; c < 3; c++) {
      float acc = 0.0f;
#pragma unroll
      for (int ky = 0; ky < 8; ky++) {
        if (ky < cy) {
          float u = 0.0f;
#pragma unroll
          for (int kx = 0; kx < 8; kx++) {
            if (kx < cx) {
              const float tt = (S.llf[c][(by0 + ky) * 8 + bx0 + kx] * py[ky]) * px[kx];
              u = fmaf(tt, ibx[kx], u);
            }
          }
          acc = fmaf(u, iby[ky], acc);
        }
      }
      dc[c] = acc;
    }
    int32_t q[3];
    quant_dc3(dc, a.dc_mul, a.dc_step, q);
    a.dc[gb] = q[0];
    a.dc[nb + gb] = q[1];
    a.dc[2 * nb + gb] = q[2];
    a.qf[gb] = (uint8_t)(S.vraw[v] - 1);
  }
}

// persistent workgroups over the dense passes of the nine lists the resolve
// kernel filled: a pass is one shape and up to NV(shape) chosen varblocks, so
// only the chosen area costs anything (the last pass of a shape is partly
// filled).  Pass order: 64x64 first -- the longest passes, one varblock each
// -- then the shapes by falling size.
__global__ __launch_bounds__(kMThreads) __attribute__((amdgpu_waves_per_eu(JXG_MERGE_WRITE_WPE)))
void merge_write_kernel(Batch<MergeArgs> bt_) {
  const MergeArgs& a = bt_.a[blockIdx.z];
  __shared__ __attribute__((aligned(16))) WriteLds S;
  uint32_t cnt[kNumShapes], total = 0;
#pragma unroll
  for (int si = 0; si < kNumShapes; si++) {
    cnt[si] = __builtin_amdgcn_readfirstlane(((volatile uint32_t*)a.work)[si]);
    total += (cnt[si] + kShapeSlots[si] - 1) / kShapeSlots[si];
  }
  for (uint32_t w = blockIdx.x; w < total; w += gridDim.x) {
    int si = 0;
    uint32_t first = 0, n = 0, start = 0;
#pragma unroll
    for (int j = kNumShapes - 1; j >= 0; j--) {
      const uint32_t np = (cnt[j] + kShapeSlots[j] - 1) / kShapeSlots[j];
      if (w >= start && w - start < np) {
        si = j;
        first = (w - start) * kShapeSlots[j];
        n = min((uint32_t)kShapeSlots[j], cnt[j] - first);
      }
      start += np;
    }
    write_pass(a, si, first, n, S);
    __syncthreads();  // LDS reuse by the next pass
  }
}

// the persistent write workgroups: nwrite over the whole launch of k frames
void launch_merge_write(const Batch<MergeArgs>& b, uint32_t k, hipStream_t s) {
  const uint32_t nw = max(1u, min(b.a[0].nwrite / k, b.a[0].ntiles * (uint32_t)kNumShapes));
  hipLaunchKernelGGL(merge_write_kernel, dim3(nw, 1, k), dim3(kMThreads), 0, s, b);
}
hipError_t set_merge_constants(const float* llf_p, const float* llf_ib, hipStream_t s) {
  hipError_t e = hipMemcpyToSymbolAsync(HIP_SYMBOL(c_llf_p), llf_p, sizeof(float) * 4 * 8, 0,
                                        hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = hipMemcpyToSymbolAsync(HIP_SYMBOL(c_llf_ib), llf_ib, sizeof(float) * 4 * 64, 0,
                               hipMemcpyHostToDevice, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  return e != hipSuccess ? e : e2;
}

}  // namespace jxg
