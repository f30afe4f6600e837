// jxg_actask.h -- the task rules of a pass group's AC token stream: which
// (slice, channel) task a thread of a band workgroup owns, how many tokens the
// task holds without walking it, and where its records lie.  Shared by the
// kernel that writes the records (ac_hist_kernel, jxg_ac.hip) and the one that
// prices them (rate_kernel, jxg_rate.hip), so the two cannot
// disagree about a record's owner.  Device code only.
#pragma once
#include "jxg_device.h"
#include "jxg_kernels.h"

namespace jxg {

struct GroupGeom {
  int bx0, by0, gw, gh;
};
// pass group of launch slot i: a shard's group list, or the range g0 + i
__device__ __forceinline__ uint32_t slot_group(const uint32_t* glist, uint32_t g0, uint32_t i) {
  return glist ? glist[i] : g0 + i;
}
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

// covered blocks of a raw strategy id: log2 and blocks across / down
__device__ __forceinline__ void varblock_dims(int type, int& lcb, int& cx, int& cy) {
  switch (type) {
    case 6: lcb = 1, cx = 1, cy = 2; break;   // 16x8
    case 7: lcb = 1, cx = 2, cy = 1; break;   // 8x16
    case 4: lcb = 2, cx = 2, cy = 2; break;   // 16x16
    case 10: lcb = 3, cx = 2, cy = 4; break;  // 32x16
    case 11: lcb = 3, cx = 4, cy = 2; break;  // 16x32
    case 5: lcb = 4, cx = 4, cy = 4; break;   // 32x32
    case 19: lcb = 5, cx = 4, cy = 8; break;  // 64x32
    case 20: lcb = 5, cx = 8, cy = 4; break;  // 32x64
    case 18: lcb = 6, cx = 8, cy = 8; break;  // 64x64
    case 22: lcb = 7, cx = 8, cy = 16; break;   // 128x64 (effort >= 8)
    case 23: lcb = 7, cx = 16, cy = 8; break;   // 64x128
    case 21: lcb = 8, cx = 16, cy = 16; break;  // 128x128
    case 25: lcb = 9, cx = 16, cy = 32; break;  // 256x128
    case 26: lcb = 9, cx = 32, cy = 16; break;  // 128x256
    case 24: lcb = 10, cx = 32, cy = 32; break; // 256x256
    default: lcb = 0, cx = 1, cy = 1; break;  // 8x8 class
  }
}

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

// ac_hist runs one 256-thread workgroup per BAND of a pass group: 8 block
// rows (one row of 64x64 tiles) x 32 block columns.  Varblocks up to 64x64
// lie inside one 64x64 tile, so a band holds whole
// varblocks, and the group's token stream (varblocks by first block raster)
// is the concatenation of its four bands' streams: band j writes its records
// at [j * kBandTokStride, ...) of the group's record space and its token
// count to bandtok[g][j]; the coders read the group's stream through
// rec_index (a 4-entry prefix).  Four workgroups per group give small frames
// (1080p: 40 groups) 160 workgroups instead of 40.  At effort >= 8 varblocks
// of 128 / 256 px span bands: the kernel then runs with BR = 32 (one
// 1024-thread workgroup = one band = the whole group; bands 1-3 empty).
constexpr int kBands = 4;  // bandtok entries per group (the coders' view)
static_assert(kBands * kBandTokStride == kGroupTokStride, "band record spaces tile the group's");

// record space index of stream position k of a group whose band counts are bt[4]
// (band j holds stream positions [c_j, c_j+1), c_j = bt[0] + ... + bt[j-1];
// the bounds are cumulative, so k >= c_j holds for a prefix of the bands)
__device__ __forceinline__ uint32_t rec_index(const uint32_t* bt, uint32_t k) {
  uint32_t j = 0, lo = 0, cum = 0;
#pragma unroll
  for (int i = 0; i < kBands - 1; i++) {
    cum += bt[i];
    const bool past = k >= cum;
    lo = past ? cum : lo;
    j += past ? 1u : 0u;
  }
  return j * (uint32_t)kBandTokStride + (k - lo);
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

// workgroup (NT threads) exclusive scan; *total = sum of all values
template <int NT>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sWave,
                                                    uint32_t* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
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
