// jxg_actask.h -- the task rules of a pass group's AC token stream: which
// (slice, channel) task a thread of a band workgroup owns, how many tokens the
// task holds without walking it, and where its records lie.  Shared by the
// kernel that writes the records (ac_hist_kernel, jxg_ac_hist.hip) and the one
// that prices them (rate_kernel, jxg_rate.hip), so the two
// cannot disagree about a record's owner; first_block also serves the A/B
// report (jxg_ab.hip).  What a reader of a group's stream needs -- the record,
// slot_group, kBands, rec_index -- is jxg_acrec.h; varblock_dims is
// jxg_acmodel.h's.  Device code only.
#pragma once
#include "jxg_device.h"
#include "jxg_kernels.h"
#include "jxg_acrec.h"

namespace jxg {

struct GroupGeom {
  int bx0, by0, gw, gh;
};
__device__ __forceinline__ GroupGeom group_geom(const AcArgs& a, int g) {
  GroupGeom r;
  const int gx = g % (int)a.gxs, gy = g / (int)a.gxs;
  r.bx0 = gx * 32;
  r.by0 = gy * 32;
  r.gw = min(32, (int)a.bxs - r.bx0);
  r.gh = min(32, (int)a.bys - r.by0);
  return r;
}

__device__ __forceinline__ void load_coefs(const int16_t* q, uint32_t* w) {
  const uint4* p = reinterpret_cast<const uint4*>(q);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint4 t = p[i];
    w[4 * i + 0] = t.x;
    w[4 * i + 1] = t.y;
    w[4 * i + 2] = t.z;
    w[4 * i + 3] = t.w;
  }
}
// coefficient k (zigzag) of a register-resident block; k must be static
__device__ __forceinline__ int32_t coef(const uint32_t* w, int k) {
  return (int32_t)(int16_t)(w[k >> 1] >> ((k & 1) * 16));
}

__device__ __forceinline__ int channel_of(int ci) { return ci == 0 ? 1 : (ci == 1 ? 0 : 2); }

// The first block (ox, oy) of the varblock of strategy `type` that covers
// frame block (bx, by).  The search places a varblock on its shape's own grid,
// where masking the position finds it; a forced map (jxg_encode_forced_rgb8)
// may place a shape of up to 64 px anywhere inside its 64x64 tile.  The masked
// position lies inside every such varblock's reach, and a first block of this
// id within reach covers the block (varblocks do not overlap), so: the masked
// guess when its byte is the id -- one byte and one compare on the grid -- else
// the one position within reach, inside the tile, whose byte is.
__device__ __forceinline__ void first_block(const uint8_t* acs, uint32_t bxs, int type, int lcb,
                                            int cx, int cy, int bx, int by, int& ox, int& oy) {
  ox = bx & ~(cx - 1);
  oy = by & ~(cy - 1);
  if (lcb == 0 || lcb > 6 || acs[(size_t)oy * bxs + ox] == (uint8_t)type) return;
  const int ylo = max(by - cy + 1, by & ~7), xlo = max(bx - cx + 1, bx & ~7);
  for (int y = ylo; y <= by; y++)
    for (int x = xlo; x <= bx; x++)
      if (acs[(size_t)y * bxs + x] == (uint8_t)type) {
        ox = x;
        oy = y;
      }
}

// One thread per block of the band: slice `sl` of the varblock whose first
// block is (obx, oby) (group-local; first_block).
struct SliceTask {
  bool valid;
  int bx, by, obx, oby, sl, lcb, cx, type;
  size_t gb, ogb;
};
// (BR: the band's block rows, 8 or 32; thread = block of the band)
__device__ __forceinline__ SliceTask slice_task(const AcArgs& a, const GroupGeom& G, int y0) {
  SliceTask t;
  const int b = threadIdx.x;
  t.bx = b & 31;
  t.by = y0 + (b >> 5);
  t.valid = t.bx < G.gw && t.by < G.gh;
  if (!t.valid) t.bx = t.by = 0;
  t.gb = (size_t)(G.by0 + t.by) * a.bxs + G.bx0 + t.bx;
  t.type = t.valid ? (a.acs[t.gb] & 0x7F) : 0;
  int cy;
  varblock_dims(t.type, t.lcb, t.cx, cy);
  // (a group's origin is a multiple of 32 blocks: masks and tiles agree with the frame's)
  first_block(a.acs, a.bxs, t.type, t.lcb, t.cx, cy, G.bx0 + t.bx, G.by0 + t.by, t.obx, t.oby);
  t.obx -= G.bx0;
  t.oby -= G.by0;
  t.sl = (t.by - t.oby) * t.cx + (t.bx - t.obx);
  t.ogb = (size_t)(G.by0 + t.oby) * a.bxs + G.bx0 + t.obx;
  return t;
}
// band-local index of slice j of t's varblock
__device__ __forceinline__ int block_of_slice(const SliceTask& t, int j, int y0) {
  return (t.oby - y0 + j / t.cx) * 32 + t.obx + j % t.cx;
}

template <int BR>
struct AcLds {
  uint8_t nz[3][(BR + 1) * 32];  // predicted-nz image, band rows and the row above
  uint8_t snz[3][BR * 32];   // non-zeros of each slice (positions >= cb)
  uint8_t last[3][BR * 32];  // last coefficient of the slice != 0
  int8_t lastk[3][BR * 32];  // highest slice-local index >= cb - 64 sl holding a non-zero, or -1
};

// tokens of task (t, c) without walking it: the walk runs from the slice's
// first position >= cb up to the varblock's last non-zero K (1 + K for an
// 8x8-class block), plus the non-zero count token on slice 0
template <int BR>
__device__ __forceinline__ uint32_t task_token_count(const AcArgs& a, const SliceTask& t,
                                                     const AcLds<BR>& L, int c, int y0) {
  if (t.lcb == 0) {
    uint32_t w[32];
    load_coefs(a.ac + (t.gb * 3 + c) * 64, w);
    int last = 0;
#pragma unroll
    for (int kk = 1; kk < 64; kk++) last = coef(w, kk) != 0 ? kk : last;
    return 1u + (uint32_t)last;
  }
  const int cb = 1 << t.lcb;
  int K = -1;
  for (int j = 0; j < cb; j++) {
    const int lk = L.lastk[c][block_of_slice(t, j, y0)];
    K = lk >= 0 ? j * 64 + lk : K;
  }
  const int lo = max(t.sl * 64, cb), hi = min(t.sl * 64 + 63, K);
  return (t.sl == 0 ? 1u : 0u) + (hi >= lo ? (uint32_t)(hi - lo + 1) : 0u);
}

// predicted-nz image (the band and the row above) and per-slice non-zero counts.
// Round 6: every position's loads (its strategy byte, three counts) are
// issued before the first LDS store -- the strided loop waited a memory
// latency per position and channel (the phase clock put ~90 K cycles per band
// workgroup here, a third of its time).
template <int BR>
__device__ __forceinline__ void fill_slices(const AcArgs& a, const GroupGeom& G,
                                            const SliceTask& t, AcLds<BR>& L, int y0) {
  const size_t nb = (size_t)a.bxs * a.bys;
  constexpr int kPos = (BR + 1) * 32, kNT = BR * 32, kIt = (kPos + kNT - 1) / kNT;
  uint32_t acsv[kIt], nzv[kIt][3];
  bool in[kIt];
#pragma unroll
  for (int it = 0; it < kIt; it++) {
    const int i = threadIdx.x + it * kNT, r = i >> 5, bx = i & 31, by = y0 - 1 + r;
    in[it] = i < kPos && bx < G.gw && by >= 0 && by < G.gh;
    const size_t gb = in[it] ? (size_t)(G.by0 + by) * a.bxs + G.bx0 + bx : 0;
    acsv[it] = in[it] ? a.acs[gb] : 0u;
#pragma unroll
    for (int c = 0; c < 3; c++) nzv[it][c] = in[it] ? a.nz[c * nb + gb] : 0u;
  }
#pragma unroll
  for (int it = 0; it < kIt; it++) {
    if (!in[it]) continue;
    const int i = threadIdx.x + it * kNT;
    int l, cx, cy;
    varblock_dims((int)acsv[it], l, cx, cy);  // covered blocks (flag set) hold scaled counts
#pragma unroll
    for (int c = 0; c < 3; c++) L.nz[c][i] = (uint8_t)((nzv[it][c] + (1u << l) - 1) >> l);
  }
  if (t.valid && t.lcb > 0) {
    const int cb = 1 << t.lcb, me = threadIdx.x;
#pragma unroll 1
    for (int c = 0; c < 3; c++) {
      uint32_t w[32];
      load_coefs(a.ac + (t.gb * 3 + c) * 64, w);
      int n = 0, lk = -1;
#pragma unroll
      for (int kk = 0; kk < 64; kk++) {
        const bool on = (t.sl * 64 + kk >= cb) && coef(w, kk) != 0;
        n += on;
        lk = on ? kk : lk;
      }
      L.snz[c][me] = (uint8_t)n;
      L.last[c][me] = coef(w, 63) != 0;
      L.lastk[c][me] = (int8_t)lk;
    }
  }
}

// workgroup (NT threads) exclusive scan; *total = sum of all values.  Holds a
// barrier.  (jxg_entropy.hip block_excl_scan256 is the same scan in the form
// lf_code_kernel was built with; DESIGN.md §3.13 "The AC coding stage's units".)
template <int NT>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sWave,
                                                    uint32_t* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t incl = wave_incl_scan(v);
  if (lane == 63) sWave[wv] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; i++) {
    const uint32_t x = sWave[i];
    before += i < wv ? x : 0u;
    all += x;
  }
  *total = all;
  return before + incl - v;
}

// a varblock's stream position within its band (its first block's thread):
// the sum of its tasks' token counts, scanned over the band's varblocks in
// first-block raster order.  sTask: [3 Y, X, B][band blocks] task token counts
// (complete); returns the varblock's first record for first blocks (other
// threads: unspecified), *total = the band's tokens.  Holds a barrier.
template <int BR>
__device__ __forceinline__ uint32_t varblock_base(const SliceTask& t, const uint32_t (*sTask)[BR * 32],
                                                  uint32_t* sWave, int y0, uint32_t* total) {
  uint32_t vtot = 0;
  const int cb = 1 << t.lcb;
  if (t.valid && t.sl == 0) {
    for (int ci = 0; ci < 3; ci++)
      for (int j = 0; j < cb; j++) vtot += sTask[ci][block_of_slice(t, j, y0)];
  }
  return block_excl_scan<BR * 32>(vtot, sWave, total);
}
// the first record and the record count of task (t, channel slot ci) given its
// varblock's position `pos` at channel ci; advances pos to the next channel
template <int BR>
__device__ __forceinline__ void task_records(const SliceTask& t, const uint32_t (*sTask)[BR * 32],
                                             int ci, int y0, uint32_t& pos, uint32_t& idx,
                                             uint32_t& cnt) {
  const int cb = 1 << t.lcb;
  uint32_t before = 0, chan_total = 0;
  for (int j = 0; j < cb; j++) {
    const uint32_t b = sTask[ci][block_of_slice(t, j, y0)];
    before += j < t.sl ? b : 0u;
    chan_total += b;
  }
  idx = pos + before;
  cnt = sTask[ci][threadIdx.x];
  pos += chan_total;
}

}  // namespace jxg
