// jxg_kernels.h -- kernel argument blocks and device-symbol setup shared by
// the HIP translation units and the host orchestrator (jxg_host.cpp).
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "jxg_acmodel.h"
#include "jxg_acrec.h"
#include "jxg_coeff.h"
#include "jxg_decode_core.h"
#include "jxg_shapes.h"

namespace jxg {

// Batched launches (the streaming pipeline's super-frames): up
// to kMaxBatch frames of one size go through each per-frame kernel as ONE
// launch -- the argument blocks of all of them in the kernel arguments,
// blockIdx.z = the frame.  One-at-a-time encodes launch batches of one.
constexpr uint32_t kMaxBatch = 4;
template <class A>
struct Batch {
  A a[kMaxBatch];
};
template <class A>
inline Batch<A> make_batch(const A* a, uint32_t k) {
  Batch<A> b{};
  for (uint32_t i = 0; i < k && i < kMaxBatch; i++) b.a[i] = a[i];
  return b;
}

struct FrontArgs {
  const uint8_t* rgb;
  uint32_t w, h;
  size_t stride;
  uint32_t bxs, bys, xp, yp, tiles_x;
  float distance;
  int effort;
  uint32_t proposals;
  int h1_int;
  int gab;        // inverse Gaborish on the XYB tile before every other stage
  float qf_base, inv_g;
  uint32_t G;
  float dc_mul[3], dc_step[3];
  uint8_t* acs;   // [nb] raw strategy
  uint8_t* qf;    // [nb] raw-1
  int32_t* dc;    // [3][nb] X,Y,B
  int16_t* ac;    // [nb][3 X,Y,B][64 zigzag]
  uint16_t* nz;   // [3][nb] non-zero AC count per block and channel
  float* homog;   // [nb][3] or null
  float* ent;     // [nb] best 8x8 estimate (merge stage input) or null
  float* xyb_out; // [tiles][3][64][64] XYB tiles (merge stage input) or null
  const uint32_t* tile_list;  // shard: tile ids (ty * tiles_x + tx), 1-D grid; or null
  int8_t* cmap;   // [2][tiles] chroma from luma ytox, ytob per 64x64 tile (out)
  uint32_t ntiles_all;  // tiles_x * tiles_y (cmap plane stride)
  uint4* zero;          // the frame's statistics arena, zeroed by the workgroups (or null)
  uint32_t zero_quads;  //   its size in 16-byte units
  const uint8_t* qf_in; // [nb] raw - 1 of the masking quant field (jxg_aq.hip) or of a forced
                        //   encode's caller, or null: the activity heuristic
  const uint8_t* force; // [nb] forced encode: the caller's validated strategy map (the
                        //   FORCED instantiation alone reads it), or null
  // traced encode (jxg_encode_traced_rgb8; the trace instantiations alone write them), or null:
  // (two pointers, not four: a 256-byte block would turn the batch index's
  // multiply into a shift in the search kernels)
  float* tr_est;        // [2][6 scan index][nb] every candidate's estimate before hook F,
                        //   then the same as compared (after hook F)
  uint8_t* tr_ids;      // [2][nb] raw id of the scan's winner, then after hook P's override
};
// libjxl-shaped masking quant field (jxg_aq.hip, oracle/aq.c)
struct AqArgs {
  const uint8_t* rgb;
  uint32_t w, h;
  size_t stride;
  uint32_t xp, yp, bxs, bys, tiles_x;
  const float* lut;      // [256] sRGB8 -> linear (device)
  float ew[4];           // fuzzy-erosion weights (aq_erosion_weights)
  float mul, add, inv_g; // quant field = pow2(...) mul + add; raw = round(qf inv_g)
  uint8_t* qf;           // [nb] raw - 1 (out)
  const uint32_t* tile_list;  // shard: tile ids, or null: every tile (1-D grid)
};
void launch_aq(const AqArgs* a, uint32_t k, uint32_t ntiles, hipStream_t s);

// merge stage (jxg_merge.hip: eval and the entries; jxg_merge_write.hip: the rest);
// the nine merged shapes and their table / list offsets: jxg_shapes.h
struct MergeArgs {
  const float* xyb;    // [tiles][3][64][64] XYB tiles (front kernel)
  uint32_t bxs, bys, tiles_x, ntiles;  // ntiles: entries of tile_list (or all tiles)
  const uint32_t* tile_list;           // shard: tile ids, or null
  uint32_t proposals;
  int max_s;      // largest merged square in blocks (2, 4 or 8)
  uint32_t G;
  float dc_mul[3], dc_step[3];
  float* ent;           // [nb] per-block estimate (front kernel; resolve rewrites)
  const float* homog;   // [nb][3] (hook F) or null
  uint8_t* acs;         // in/out: raw id, bit 7 on covered non-first blocks
  uint8_t* qf;          // in/out: raw - 1
  int32_t* dc;          // out (merged varblocks)
  int16_t* ac;          // out (merged varblocks), natural order slices
  uint16_t* nz;         // out (merged varblocks): full count at the first block,
                        //   (nz + cb - 1) >> log2 cb at covered blocks
  float* cost;          // [tiles][9 shapes][32 varblocks] candidate estimates
  const float* wk;      // [3][kShapeOff[9]] weights per shape, pixel orientation, row quads ([ky/4][kx][ky%4])
  const float* iwy;     // [kShapeOff[9]] 1 / Y weight
  const float* sdk;     // [3][kShapeOff[9]] distortion weights (dist_weight), same layout
  const uint16_t* nat;  // [kShapeOff[9]] natural-order position
  uint32_t* work;       // [merge_work_words(tiles)]: the nine shapes' counts, then per shape
                        //   the (tile << 6 | first block) of every chosen varblock, list of
                        //   shape si at merge_list_off(si, ntiles) (resolve -> write)
  uint32_t nwrite;      // merge_write workgroups (persistent loop over the dense passes)
  const int8_t* cmap;   // [2][tiles_all] chroma from luma (front kernel)
  uint32_t ntiles_all;
  const uint8_t* force; // [nb] forced encode: the caller's validated strategy map
                        //   (force_list_kernel in the place of eval + resolve), or null
};
// merge levels 128 / 256 px (effort >= 8; jxg_bigvb.hip): kinds 64x128,
// 128x128, 128x256, 256x256 (stored orientation rows <= cols), and the
// layout of their table blob (floats): weights [3][n], distortion weights
// [3][n], 1 / Y weight [n], Lee constants [9][128] / scales [9][256], LLF
// scales [6][32] and inverse basis [6][32][32]; natural orders separately
constexpr int kBigKindOff[5] = {0, 8192, 24576, 57344, 122880};
constexpr uint32_t kBigSlots = 512;          // persistent workgroups of the 128 / 256 px levels (two per CU)
constexpr size_t kBigPlanes = 3 * 65536;     // floats of a slot's scratch: X, Y, B planes of up to 256 x 256
constexpr size_t kBigTabW = 0, kBigTabSd = 3 * 122880, kBigTabIw = 6 * 122880,
                 kBigTabLeeC = 7 * 122880, kBigTabLeeS = kBigTabLeeC + 9 * 128,
                 kBigTabLlfP = kBigTabLeeS + 9 * 256, kBigTabLlfIb = kBigTabLlfP + 6 * 32,
                 kBigTabFloats = kBigTabLlfIb + 6 * 32 * 32;
struct BigArgs {
  MergeArgs m;             // the frame's merge arguments (xyb tiles, maps, outputs)
  const float* tab;        // kBigTab* blob
  const uint16_t* nat;     // [kBigKindOff[4]] natural-order position per stored index
  float* scratch;          // [slots][3][65536] column-major planes X, Y (dequantized after its quantization), B
  uint32_t slots;          // persistent workgroups (one scratch slot each)
  float* cost;             // [ng][30] candidate estimates (level 128: 4 x 5, level 256: 5), the regions' current sums (4 + 1)
  uint32_t* work;          // [1 + ng * 16]: count, then first blocks of the chosen varblocks
  uint32_t* kinds;         // [4] varblocks chosen per big kind (statistics arena; the host writes the used kinds' quant tables)
  const uint32_t* glist;   // the plan's pass groups: glist[i], or g0 + i
  uint32_t g0, ng, gxs;
  int trace;               // traced encode: big_eval evaluates every candidate in full (no +inf)
};
hipError_t launch_big(const BigArgs* a, uint32_t k, hipStream_t s);
// forced encode (one frame): force_big_list_kernel's list of the big first
// blocks of a.m.force, then big_write (no eval, no resolve)
hipError_t launch_force_big(const BigArgs& a, hipStream_t s);
// search trace (jxg_trace.hip), behind a traced encode's merge
// stage.  The planes are over the block grid, nb = bxs * bys.
constexpr uint32_t kTraceSummaryWords = 2 + 36 + 6 + 6 + 48 + 6;  // jxg_trace_summary as u32 words
struct TraceArgs {
  const float* mcost;      // [tiles][9][32] (merge_eval), or null: no merge stage ran
  const float* big_cost;   // [ng][30] (big_eval), or null: effort < 8
  const float* ent;        // [nb] the final estimates
  const uint8_t* acs;      // [nb] the final strategy bytes
  uint32_t bxs, bys, tiles_x, gxs, ngroups;
  int max_s;               // largest merged square searched by merge_eval, in blocks (4 or 8)
  uint32_t max_px;         // largest level searched (summary)
  const float* cand8;      // [6][nb] (front kernel, trace mode), as compared
  const float* cand8_raw;  // [6][nb] before hook F
  const uint8_t* scan8;    // [nb]
  const uint8_t* front8;   // [nb]
  float* merged;           // [9][nb] out
  float* big;              // [6][nb] out
  float* chosen;           // [nb] out
  uint32_t* summary;       // [kTraceSummaryWords] out (pre-zeroed)
};
hipError_t launch_trace(const TraceArgs& a, hipStream_t s);

// per-LF-group varblock lists (AC metadata channel)
struct VbArgs {
  const uint8_t* acs;
  uint32_t bxs, bys, lfxs;
  const uint8_t* lf_mine;  // [nlf] 1 = this shard owns the LF group (null: all)
  uint32_t* vb;     // [nlf][65536] block index (frame raster) of each varblock
  uint32_t* count;  // [nlf]
};

struct HomogArgs {
  const float* xyb;  // [3][ysize][stride]
  uint32_t xsize, ysize;
  size_t stride, plane;
  float distance;
  int h1_int;
  float* r3;
  uint8_t* type;
};

// AC (pass group) token kernels
struct AcArgs {
  const uint8_t* acs;
  const int16_t* ac;  // [nb][3][64 zigzag]
  const uint16_t* nz;  // [3][nb] non-zero counts (front / merge kernels)
  uint32_t bxs, bys, gxs;
  uint32_t g0;           // first pass group of the launch (contiguous shard / whole frame)
  const uint32_t* glist; // [slots] pass group of each slot (a shard's non-contiguous
                         //   group set), or null: slot i = group g0 + i
  uint32_t* hist;        // [kMaxClusters][kAlpha]      (hist pass)
  uint32_t* bound;       // [ngroups] bit upper bound   (hist pass)
  uint32_t* ntok;        // [ngroups][3] token counts   (hist pass)
  const uint32_t* codes; // [kMaxClusters][kAlpha] (code | len << 16)  (emit pass)
  const uint64_t* base;  // [ngroups] scratch bit offset (emit pass)
  uint32_t* scratch;     // bit buffer (emit pass, zeroed)
  uint32_t* bits;        // [ngroups] exact bits (emit pass)
  uint32_t* tokens;      // token records (jxg_acrec.h ac_record),
                         //   slot i (group glist[i] or g0 + i) at i * kGroupTokStride,
                         //   band j of it at + j * kBandTokStride (hist pass writes them)
  uint32_t* bandtok;     // [ngroups][4] tokens of each 8-block-row band (hist pass)
};
// (kGroupTokStride, kBandTokStride, kAnsMaxChunks: jxg_acrec.h)

// ANS coding of the pass groups' token records (jxg_ans.hip)
// (the table blob's layout, kAnsHists / kAnsInvOff / kAnsMapOff / kAnsTabBytes:
// jxg_acmodel.h)
struct AnsArgs {
  const uint32_t* tokens;  // token records of ac_hist_kernel (kGroupTokStride per group)
  uint32_t* val;           // [records] emitted bits: 16-bit chunk (if any) then raw bits
  uint8_t* len;            // [records] number of emitted bits
  const uint32_t* ntok;    // [ngroups][3]
  const uint32_t* bandtok; // [ngroups][4] tokens per band (the group's stream = its bands')
  const uint8_t* tab;      // table blob (kAnsInvOff / kAnsMapOff):
                           //  u32 [8][128] symbol: f - 1 | cum << 12
                           //  u16 [8][4096] alias inverse: slot of position cum + offset
                           //  u8 [132] static cluster -> histogram
  uint32_t nhist;          // histograms in use (<= kAnsMaxHists)
  uint32_t* state;         // [ngroups] final encoder state (= stream's first 32 bits)
  const uint64_t* base;    // [ngroups] scratch bit offset
  uint32_t* scratch;
  uint32_t* bits;          // [ngroups] exact bits
  uint32_t g0, n;          // slots [0, n): group glist[i], or g0 + i when glist is null
  const uint32_t* glist;
  const uint32_t* order;   // chain order of the n slots (longest group first)
  uint32_t* csum;          // [slots][kAnsMaxChunks] emitted bits of every 64-record chunk
  uint32_t max_tokens;     // most tokens of any group (ans_emit's segments per group)
};
// rANS chains + bit placement of k frames (same plan); streamed: the frames
// belong to the streaming pipeline (other frames' kernels share the GPU)
void launch_ans(const AnsArgs* a, uint32_t k, hipStream_t s, bool streamed);

// LF-group modular streams: rows of (lf group, stream, channel, y)
// One segment of <= kLfSeg samples of a channel row (long rows -- the
// 2 x count AC-strategy/quant-field channel -- are split so every workgroup
// does one pass).
constexpr uint32_t kLfSeg = 256;
struct LfRow {
  uint32_t lg;      // LF group
  uint16_t stream;  // 0 = DC, 1 = AC metadata
  uint16_t chan;
  uint32_t y, x0, width;  // samples [x0, x0 + width) of row y
  uint32_t sid;           // stream index = lg*2 + stream
};
// A chunk: consecutive segments of ONE stream, <= kLfChunkSamples samples
// and <= kLfChunkRows segments; one workgroup (256 threads, <= 16 samples
// each, contiguous in stream order) per chunk.
constexpr uint32_t kLfChunkSamples = 4096, kLfChunkRows = 64, kLfPer = 16;
struct LfChunk {
  uint32_t row0, nrows, sid, nsamp;
};
struct LfArgs {
  const LfRow* rows;
  const LfChunk* chunks;
  const int32_t* dc;  // [3][nb]
  const uint8_t* acs;
  const uint8_t* qf;
  const uint32_t* vb;     // [nlf][65536] varblock -> block index
  const uint32_t* vcount; // [nlf] varblocks per LF group
  uint32_t bxs, bys, lfxs;
  const int8_t* cmap;     // [2][tiles_y][tiles_x] ytox, ytob (AC metadata channels 0, 1)
  uint32_t tiles_x, ntiles_all;
  uint32_t* hist;         // [nstreams][4 leaves][kAlpha]  (hist)
  uint32_t* sbound;       // [nstreams] (hist)
  const uint32_t* codes;  // [nstreams][4][kAlpha] (lf_code)
  uint64_t* status;       // [nchunks] look-back word (lf_hist clears, lf_code)
  const uint32_t* stream_chunks;  // [nstreams+1] first chunk of each stream
  const uint64_t* stream_base;  // [nstreams] scratch bit offset of each stream
  uint32_t* stream_bits;        // [nstreams] exact bits (lf_code)
  uint32_t* scratch;
};

struct ConcatPiece {
  uint64_t src_bit;  // bit offset into the source arena
  uint64_t dst_bit;  // bit offset into the output
  uint64_t nbits;
  uint32_t arena;    // 0 = device scratch, 1 = host-chunk upload, 2 = second scratch
  uint32_t pad;
};

// (dist_weight, the estimates' distortion weight: jxg_coeff.h)
// front_kernel's three translation units (jxg_front.hip: the search;
// jxg_front_forced.hip; jxg_front_trace.hip), each with constant tables of its
// own: the host's tables (jxg_front_tables.h) to one unit's, asynchronously --
// `t` outlives the copies
struct FrontTables;
hipError_t upload_front_tables_search(const FrontTables& t, hipStream_t s);
hipError_t upload_front_tables_forced(const FrontTables& t, hipStream_t s);
hipError_t upload_front_tables_trace(const FrontTables& t, hipStream_t s);
// the search: k frames of a batch, every tile / a shard's tile list
void launch_front(const FrontArgs* a, uint32_t k, uint32_t tiles_x, uint32_t tiles_y, hipStream_t s);
void launch_front_list(const FrontArgs* a, uint32_t k, uint32_t ntiles, hipStream_t s);
// one frame of a forced (a.force) / traced (a.tr_est) job, every tile
void launch_front_forced(const FrontArgs& a, uint32_t tiles_x, uint32_t tiles_y, hipStream_t s);
void launch_front_trace(const FrontArgs& a, uint32_t tiles_x, uint32_t tiles_y, hipStream_t s);
// shard exchange: per-group block records (acs, qf, dc) <-> frame arrays
struct PackArgs {
  uint8_t* acs;
  uint8_t* qf;
  int32_t* dc;
  uint32_t bxs, bys, gxs;
  int8_t* cmap;           // [2][ntiles_all] chroma from luma of the group's 4 x 4 tiles
  uint32_t tiles_x, tiles_y;
  uint8_t* xbuf;          // n group records back to back
  const uint32_t* list;   // [n] group of each record
  uint32_t n;
};
void launch_pack(const PackArgs& a, hipStream_t s);    // frame arrays -> records
// a rank's sections (runs of consecutive section bytes of its payload body)
// -> their codestream offsets in mapped host memory; piece i takes workgroups
// [wg0, next wg0) of 1024 destination dwords each
struct ScatterPiece {
  uint64_t src, dst;
  uint32_t len, wg0;
};
constexpr int kMaxScatterPieces = 64;
struct ScatterArgs {
  const uint8_t* src;
  uint8_t* dst;
  uint32_t n;
  ScatterPiece p[kMaxScatterPieces];
};
void launch_scatter(const ScatterArgs& a, uint32_t nwg, hipStream_t s);
void launch_unpack(const PackArgs& a, hipStream_t s);  // records -> frame arrays
void launch_homog(const HomogArgs& a, uint32_t tiles_x, uint32_t tiles_y, hipStream_t s);
// whole_group: one 1024-thread workgroup per group (varblocks of 128 / 256 px
// span the 8-row bands; effort >= 8)
void launch_ac_hist(const AcArgs* a, uint32_t k, uint32_t ngroups, hipStream_t s,
                    bool whole_group = false);
void launch_ac_emit(const AcArgs& a, uint32_t ngroups, hipStream_t s);
void launch_lf_hist(const LfArgs* a, uint32_t k, uint32_t nchunks, hipStream_t s);
void launch_lf_code(const LfArgs* a, uint32_t k, uint32_t nchunks, hipStream_t s);
hipError_t set_cluster_table(const uint8_t* tab, hipStream_t s);
hipError_t set_merge_constants(const float* llf_p /*[4][8]*/, const float* llf_ib /*[4][8][8]*/,
                         hipStream_t s);
// merge stage of k frames of one size: eval, resolve, write (jxg_merge.hip)
hipError_t launch_merge(const MergeArgs* a, uint32_t k, hipStream_t s);
// forced encode (one frame): the lists from a.force, then merge_write
hipError_t launch_force_merge(const MergeArgs& a, hipStream_t s);
// the stage's other unit, launched by the two above: the list producers and
// the dense write passes (jxg_merge_write.hip)
void launch_merge_resolve(const Batch<MergeArgs>& b, uint32_t k, hipStream_t s);
void launch_force_list(const MergeArgs& a, hipStream_t s);
void launch_merge_write(const Batch<MergeArgs>& b, uint32_t k, hipStream_t s);
void dump_merge_profile();  // JXG_MERGE_PROFILE experiment builds; no-op otherwise
void dump_front_profile();  // JXG_FRONT_PROFILE experiment builds; no-op otherwise
void dump_hist_profile();   // (the same builds: ac_hist's phase clock)
void launch_vb_list(const VbArgs* a, uint32_t k, uint32_t nlf, hipStream_t s);  // jxg_vb_list.hip
// decode-side quality (jxg_metrics.hip): orig / comp RGB8 interleaved rows
struct MetricArgs {
  const uint8_t* orig;
  const uint8_t* comp;
  size_t so, sc;  // row strides (bytes)
  uint32_t w, h;
  uint64_t* sse;      // out: sum of squared sample differences (pre-zeroed)
  double* partials;   // [ssim_partials(w, h)] per-workgroup SSIM sums
  double* ssim;       // out: sum of window SSIMs over all channels, or null (skip SSIM)
};
uint32_t ssim_partials(uint32_t w, uint32_t h);
hipError_t set_gauss_table(const double* g, hipStream_t s);
void launch_metrics(const MetricArgs& a, hipStream_t s);
void launch_ssim(const MetricArgs& a, hipStream_t s);  // the SSIM kernels of launch_metrics alone
// MS-SSIM (jxg_metrics.hip): five scales, scale j of
// (w >> j) x (h >> j).  Scale 0 is the RGB8 images; scales 1 .. 4 are exact
// f32 planes [3][h_j][w_j] (2 x 2 box means), the four levels of one image back
// to back in one buffer of ms_pyramid_floats(w, h).
constexpr int kMsScales = 5;
constexpr uint32_t kMsMinEdge = 176;  // scale 4 is at least 11 x 11
size_t ms_pyramid_floats(uint32_t w, uint32_t h);
size_t ms_level_offset(uint32_t w, uint32_t h, int j);  // j = 1 .. 4, in floats
uint32_t ms_partials(uint32_t w, uint32_t h);  // doubles: [scale][ssim | cs][workgroup]
void launch_ms_pyramid(const uint8_t* img, size_t stride, uint32_t w, uint32_t h, float* pyr,
                       hipStream_t s);
struct MsArgs {
  const uint8_t* orig;
  const uint8_t* comp;
  size_t so, sc;  // row strides (bytes)
  uint32_t w, h;  // min(w, h) >= kMsMinEdge
  const float* pyr_o;  // the two images' pyramids (launch_ms_pyramid)
  const float* pyr_c;
  double* partials;    // [ms_partials(w, h)]
  double* out;         // [10]: window sums of ssim[0 .. 4], then of cs[0 .. 4]
};
void launch_msssim(const MsArgs& a, hipStream_t s);
// decode-side reconstruction (jxg_recon.hip): the decoded
// image from the context's quantized coefficients.  Table blob (floats, built
// in double by build_recon_tables): inverse-DCT matrices [k][x] for n = 4 ..
// 256, the LLF forward matrices (normalised DCT / LLF scale) for n = 1 .. 32,
// the 8x8-class inverse weights in slice order [5 kinds][3][64], the merged
// kinds' inverse weights in natural order [3][kRcKindOff[10]], the EPF's
// qf -> inverse sigma table [256] (> 0: the block is not filtered).  Position
// blob (u16): the zig-zag order of the 8x8 class [64], then every merged
// kind's natural order [position] -> stored raster index.
constexpr int kRcKindOff[11] = {0,    128,   384,   896,   1920,  3968,
                                8064, 16256, 32640, 65408, 130944};
constexpr int rc_idct_off(int l) { return ((1 << (2 * l)) - 16) / 3; }  // n = 1 << l, l = 2 .. 8
constexpr int rc_fwd_off(int l) { return ((1 << (2 * l)) - 1) / 3; }    // n = 1 << l, l = 0 .. 5
constexpr size_t kRcTabIdct = 0, kRcTabFwd = kRcTabIdct + rc_idct_off(9),
                 kRcTabW8 = kRcTabFwd + rc_fwd_off(6), kRcTabIw = kRcTabW8 + 5 * 3 * 64,
                 kRcTabSigma = kRcTabIw + 3 * (size_t)kRcKindOff[10],
                 kRcTabFloats = kRcTabSigma + 256;
constexpr size_t kRcPosKinds = 64, kRcPosWords = kRcPosKinds + kRcKindOff[10];
struct ReconArgs {
  const uint8_t* acs;   // [nb] raw strategy, bit 7 on covered non-first blocks
  const uint8_t* qf;    // [nb] raw - 1
  const int32_t* dc;    // [3][nb]
  const int16_t* ac;    // [nb][3][64] natural-order slices
  const int8_t* cmap;   // [2][ntiles_all]
  uint32_t w, h, bxs, bys, xp, yp, tiles_x, ntiles_all;
  float inv_g;          // 65536 / global_scale
  float dc_step[3];
  float bias[4];        // AdjustQuantBias
  const float* tab;     // kRcTab* blob
  const uint16_t* pos;  // kRcPos* blob
  float* pa;            // [3][yp][xp] planes (transform output, filter ping)
  float* pb;            // [3][yp][xp] planes (filter pong; the big kernel's column pass)
  uint32_t* biglist;    // [0]: count, then the first blocks of the 128 / 256 px varblocks
  uint32_t bigcap;      //   capacity of the list
  uint8_t* rgb;         // RGB8 out
  size_t stride;
  float cbias, obias;   // cbrt(opsin bias), opsin bias
  float xmul, bmul;     // frame header x_qm / b_qm: 1.25^(2 - scale), 1 for this encoder
  float cm[9];          // inverse opsin matrix, row-major
};
// the 64x64 tiles' varblocks (<= 64 px); to_rgb: no filter follows, RGB8 is written
hipError_t launch_recon_tiles(const ReconArgs& a, bool to_rgb, hipStream_t s);
hipError_t launch_recon_big(const ReconArgs& a, uint32_t nbig, hipStream_t s);
// filters over the planes src -> dst, or -> RGB8 when `last`; epf pass: 0 (12
// neighbours), 1 (4 neighbours), 2 (4 neighbours, one-pixel SADs)
hipError_t launch_recon_gab(const ReconArgs& a, const float* src, float* dst, bool last,
                            hipStream_t s);
hipError_t launch_recon_epf(const ReconArgs& a, int pass, const float* src, float* dst, bool last,
                            hipStream_t s);
hipError_t launch_recon_colour(const ReconArgs& a, const float* src, hipStream_t s);
// the same conversion fused with the squared error against the original
// (orig: RGB8 rows of orig_stride bytes; *sse pre-zeroed, the exact integer sum
// launch_metrics gives for the stored image); store: RGB8 also written to a.rgb
// block_sse: also one u32 per 8x8 block, [bys][bxs], the squared error of the
// block's image pixels (every word written; the strategy report's form)
hipError_t launch_recon_colour_sse(const ReconArgs& a, const float* src, const uint8_t* orig,
                                   size_t orig_stride, uint64_t* sse, bool store, hipStream_t s,
                                   uint32_t* block_sse = nullptr);
// per-strategy statistics (jxg_report.hip): the table is
// jxg_strategy_report as u64 cells [27 raw ids][8: varblocks, blocks, pixels,
// non-zeros X / Y / B, quant-field sum, squared error], added into (pre-zeroed)
constexpr uint32_t kReportStrategies = 27, kReportCols = 8,
                   kReportCells = kReportStrategies * kReportCols;
struct ReportArgs {
  const uint8_t* acs;         // [nb] raw strategy, bit 7 on covered non-first blocks
  const uint8_t* qf;          // [nb] raw - 1
  const int16_t* ac;          // [nb][3][64], 16-byte aligned
  const uint32_t* block_sse;  // [nb] (launch_recon_colour_sse)
  uint32_t w, h, bxs, nb;
  unsigned long long* table;  // [kReportCells]
};
hipError_t launch_strategy_report(const ReportArgs& a, hipStream_t s);
// coded bits per varblock and strategy (jxg_rate.hip): the
// table is jxg_rate_report's rows as u64 cells [27 raw ids][6: tokens X / Y / B,
// cost X / Y / B in 1 / kRateUnit bit], added into (pre-zeroed)
constexpr uint32_t kRateStrategies = 27, kRateCols = 6, kRateCells = kRateStrategies * kRateCols,
                   kRateUnit = 256, kRateFreqs = 4097;
struct RateArgs {
  AcArgs ac;                  // of the encode: acs, ac, nz, geometry, group slots, tokens, and
                              //   with prefix codes `codes`; the rest unused
  const uint8_t* ans_tab;     // the encode's ANS table blob (AnsArgs::tab), or null: prefix codes
  uint32_t nhist;             //   its histograms in use
  const uint16_t* ftab;       // [kRateFreqs] jxg_rate_symbol_cost(f) (ANS)
  uint32_t* block_cost;       // [bys][bxs] out: a varblock's cost at its first block, 0 at
                              //   covered blocks (every word written), or null
  unsigned long long* table;  // [kRateCells]
};
// one workgroup per (group, band) as launch_ac_hist; whole_group as there
hipError_t launch_rate(const RateArgs& a, uint32_t ngroups, bool whole_group, hipStream_t s);
// A/B report of two encodes (jxg_ab.hip).  The share pass
// turns one side's first-block cost map into a cost per block; the table is
// jxg_ab_report's cells as u64 words [27 from][27 to][6: blocks, pixels, sse_a,
// sse_b, cost_a, cost_b], added into (pre-zeroed)
constexpr uint32_t kAbStrategies = 27, kAbCols = 6,
                   kAbWords = kAbStrategies * kAbStrategies * kAbCols;
struct AbShareArgs {
  const uint8_t* acs;          // [nb] strategy bytes
  const uint32_t* block_cost;  // [nb] RateArgs::block_cost
  uint32_t* share;             // [nb] out, every word written
  uint32_t bxs, nb;
};
hipError_t launch_ab_share(const AbShareArgs& a, hipStream_t s);
struct AbArgs {
  const uint8_t *acs_a, *acs_b;  // [nb] strategy bytes of the two sides
  const uint32_t *sse_a, *sse_b;      // [nb] block error maps
  const uint32_t *share_a, *share_b;  // [nb] cost shares (ab_share_kernel)
  uint32_t w, h, bxs, nb;
  int32_t* delta;              // [2][nb] out: sse_b - sse_a, share_b - share_a; or null
  unsigned long long* table;   // [kAbWords]
};
hipError_t launch_ab_report(const AbArgs& a, hipStream_t s);
// the decoder's pass groups (jxg_decode.hip): one wave per
// group walks its section of the codestream with the decode core and writes
// the non-zero coefficients into `ac` (it zeroes the group's area first)
struct DecodeArgs {
  const uint64_t* stream;  // the codestream as 64-bit words, zero padded
  const uint64_t* sec;     // [ngroups][2] first / end bit of every pass group
  dec::SymReader sym;      // the AC stream's decode tables (device pointers)
  uint32_t npresets, preset_bits;
  const uint8_t* acs;      // [nb] decoded strategy map
  int16_t* ac;             // [nb][3][64] out
  uint32_t* status;        // [ngroups] out: 0 or a dec::k* code
  uint32_t bxs, bys, gxs;
  // LDS staging of the decode tables (every token reads a context-map byte, a
  // histogram descriptor and a table entry, each depending on the one before):
  // the group's preset's slice of the context map and the descriptors always,
  // the symbol tables (tab_bytes of alias entries or prefix table words) when
  // they fit (stage_tab)
  uint32_t nhist, tab_bytes, stage_tab;
};
// the kernel's dynamic LDS for these arguments; sets stage_tab
uint32_t decode_groups_lds(DecodeArgs* a);
hipError_t launch_decode_groups(const DecodeArgs& a, uint32_t ngroups, hipStream_t s);
// the batch form (jxg_decode_batch.cpp): one wave per work item of d_work
// (jxg_decode_plan.h), whose frame indexes d_frames -- descriptors in device
// memory with `status` the frame's first status word; every frame of a launch
// is of one class (symbol tables staged in LDS or not) and `lds` the largest
// decode_lds_bytes of them
struct DecWork;
hipError_t launch_decode_batch(const DecodeArgs* d_frames, const DecWork* d_work, uint32_t nwork,
                               bool staged, uint32_t lds, hipStream_t s);
// synthetic benchmark input (jxg_synth.hip): RGB8 rows of `stride` bytes
hipError_t launch_synth(uint8_t* out, uint32_t w, uint32_t h, size_t stride, uint64_t seed,
                        hipStream_t s);
// every word of out[0, out_words) written once (bits no piece covers: 0)
void launch_concat(const ConcatPiece* pieces, uint32_t npieces, uint64_t out_words,
                   const uint32_t* scratch, const uint32_t* chunks, const uint32_t* scratch2,
                   uint32_t* out, hipStream_t s);

}  // namespace jxg
