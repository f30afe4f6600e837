/*
 * jxg.h -- C ABI of the MI355X-native JPEG XL VarDCT encode path and of the
 * decoder of the codestreams it writes (jxg_decode_*, at the end).
 *
 * Drop-in boundary: this library replaces what the benchmark harness reaches
 * through `docker exec ... /libjxl/build/tools/cjxl IN OUT --distance=D
 * --effort=E` (pscoro/JPEG-XL-Lossy-Image-Compression-Thesis,
 * benchmark-jpegxl/src/docker_manager.rs:100-137 DockerManager::execute_cjxl,
 * called from benchmark-jpegxl/src/benchmark.rs:654-677).  The encoder
 * internals it re-implements are libjxl's VarDCT heuristics with the thesis
 * hooks of proposals/combined.diff (HomogeneityPartition :213-235 hooked into
 * FindBest8x8Transform :270-274; EstimateEntropy factor :247-253).
 *
 * Conventions: status 0 = OK, negative on error (never aborts); one context
 * per host thread; device memory is owned by the context; output buffers are
 * allocated by the library and released with jxg_buffer_free.
 *
 * Device inputs (jxg_encode_rgb8_device, jxg_submit_rgb8_device,
 * jxg_shard_submit_device, jxg_shard_begin, jxg_compare_rgb8_device,
 * jxg_msssim_rgb8_device) are read on the library's own HIP streams.  Either
 * the caller's writes to them are complete before the call (e.g.
 * hipStreamSynchronize of the producing
 * stream), or the caller names its producing stream with
 * jxg_set_input_stream: every later device-input call then orders its reads
 * after all work submitted to that stream so far (an event recorded on it,
 * waited on by the library's stream -- no host synchronisation).
 *
 * A context with streamed frames pending (jxg_pending > 0) serves them as a
 * pipeline lane: the one-at-a-time, batch, sharded-begin/end, homogeneity,
 * compare, MS-SSIM (jxg_msssim_rgb8, jxg_set_sweep_msssim), reconstruct and
 * decode entry points return JXG_ERR_INVALID_ARG until they are received.
 */
#ifndef JXG_H_
#define JXG_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  JXG_OK = 0,
  JXG_ERR_INVALID_ARG = -1,
  JXG_ERR_NO_DEVICE = -2,
  JXG_ERR_HIP = -3,
  JXG_ERR_OOM = -4,
  JXG_ERR_UNSUPPORTED = -5,
  JXG_ERR_INTERNAL = -6
} jxg_status;

/* proposals bitmask: the thesis patches (proposals/ directory) */
#define JXG_PROPOSAL_P 1u /* homogeneity-partitioning.diff:272-276 */
#define JXG_PROPOSAL_F 2u /* homogeneity-factored-entropy.diff:247-253 */

/* flags */
#define JXG_FLAG_H1_INT_ABS 1u /* thesis SML with int abs(int) */
#define JXG_FLAG_KEEP_MAPS 2u  /* keep per-block maps for jxg_get_stats */
#define JXG_FLAG_ANS 4u        /* ANS (12-bit rANS) for the AC stream instead of prefix codes */
#define JXG_FLAG_FORCE_ONE_STREAM 8u /* testing: the split assembly takes its one-stream
                                      * fallback (as when its prefix bound is exceeded);
                                      * same bytes */
/* restoration filters (cjxl --gaborish / --epf), off by
 * default: GABORISH applies the encoder's inverse Gaborish to the XYB image
 * before every other stage and enables the decoder's 3x3 Gaborish; EPF enables
 * the decoder's edge-preserving filter (iterations from the distance: 1 below
 * d 1.5, 2 below d 4, else 3; constant sharpness 4 per block).  Both are
 * signalled in the frame header (LoopFilter) [ext, parity with libjxl
 * unpinned; DESIGN.md §3.8] */
#define JXG_FLAG_GABORISH 16u
#define JXG_FLAG_EPF 32u
/* libjxl-shaped adaptive quantization: the masking-based initial quant field
 * (InitialQuantField / AdaptiveQuantizationMap [ext]: gamma-weighted local
 * differences, fuzzy erosion, mask, HF and gamma modulation; restated as
 * recalled, parity with libjxl unpinned; oracle/aq.c) instead of the
 * activity heuristic; one extra kernel per frame (csrc/jxg_aq.hip) */
#define JXG_FLAG_AQ_MASKING 64u
/* What `cjxl IN OUT --distance=D --effort=E` with no other flag encodes (the
 * harness's argv, benchmark-jpegxl/src/docker_manager.rs:126-136): cjxl's
 * VarDCT defaults [ext] -- ANS, Gaborish, EPF iterations by distance, the
 * masking quant field.  jxg_cjxl starts from this set, INTEGRATION.md's
 * execute_cjxl over the C ABI passes it, and bench.py's headline value is
 * measured with it; the same (image, distance, effort, proposals) give the
 * same bytes through either route (tests/test_gpu_cli.py). */
#define JXG_FLAGS_CJXL_DEFAULTS (JXG_FLAG_ANS | JXG_FLAG_GABORISH | JXG_FLAG_EPF | JXG_FLAG_AQ_MASKING)

/* opaque encoder context (one HIP device, its streams and buffers) */
typedef struct jxg_ctx jxg_ctx;

/* The bottom of the distance range.  0 < distance <= 25 is accepted (<= 0, NaN
 * and > 25 are JXG_ERR_INVALID_ARG); a context or a sweep point computes with
 * the effective distance max(distance, JXG_MIN_DISTANCE).  Below about 1e-4
 * everything derived from the distance is already at its clamp (global scale
 * 73727, raw quant field 256, quant_dc), so any two distances <= 1e-6 give the
 * same bytes, and no codestream of a distance >= 1e-6 depends on the floor.
 * It keeps the quant field's float -> int conversion (qf_base * inv_g < 2^21)
 * inside int range; without it a distance below ~3.3e-10 overflowed it. */
#define JXG_MIN_DISTANCE 1e-6f

typedef struct {
  float distance;      /* cjxl --distance (butteraugli target), (0, 25]; see JXG_MIN_DISTANCE */
  int effort;          /* cjxl --effort 1..9 (>=5: 8x8-class ACS search) */
  uint32_t proposals;  /* JXG_PROPOSAL_* */
  int num_devices;     /* informative; multi-GPU runs one context per rank */
  uint32_t flags;      /* JXG_FLAG_* */
  int device;          /* HIP device ordinal */
} jxg_params;

typedef struct {
  uint8_t* data;
  size_t size;
} jxg_buffer;

typedef struct {
  uint32_t xsize, ysize, xsize_blocks, ysize_blocks;
  uint32_t num_groups, num_lf_groups;
  uint32_t global_scale, quant_dc;
  size_t bytes;
  /* valid until the next encode on this context (JXG_FLAG_KEEP_MAPS) */
  const uint8_t* ac_strategy;  /* [ysize_blocks][xsize_blocks] raw strategy */
  const uint8_t* quant_field;  /* raw quant field - 1 */
  const int32_t* dc;           /* [3][blocks] quantized DC (X, Y, B) */
  const int32_t* ac;           /* [blocks][3][64] quantized AC, natural order */
  const uint32_t* ac_tokens;   /* [num_groups][3] AC token counts (X, Y, B) */
  const float* homogeneity;    /* [blocks][3] r_h r_v r_d (if P|F) */
  /* device time per stage, milliseconds (last encode) */
  float ms_front, ms_histogram, ms_emit, ms_assemble, ms_total;
  /* host wall clock of the whole call and of the host-side code/header work */
  float ms_host_call, ms_host_codes, ms_host_layout;
  /* device time of the fused front kernel alone (XYB + ACS + DCT + quant);
   * ms_front also covers the masking quant field and the merge stage */
  float ms_front_kernel;
  /* device time of the masking quant field kernel (JXG_FLAG_AQ_MASKING; 0 otherwise) */
  float ms_aq;
} jxg_stats;

const char* jxg_status_str(jxg_status s);
jxg_status jxg_create(const jxg_params* params, jxg_ctx** ctx);
void jxg_destroy(jxg_ctx* ctx);
/* the caller's stream (hipStream_t) that produces device inputs; NULL: none
 * (writes complete before each call) -- see the conventions above */
jxg_status jxg_set_input_stream(jxg_ctx* ctx, void* stream);

/* host RGB8 (interleaved, row_stride bytes per row) -> codestream */
jxg_status jxg_encode_rgb8(jxg_ctx* ctx, const uint8_t* rgb, uint32_t xsize, uint32_t ysize,
                           size_t row_stride, jxg_buffer* out);
/* device-resident RGB8 (same layout, device pointer) -> codestream */
jxg_status jxg_encode_rgb8_device(jxg_ctx* ctx, const void* d_rgb, uint32_t xsize,
                                  uint32_t ysize, size_t row_stride, jxg_buffer* out);
/* Forced encode: the caller's AC-strategy map instead of the search
 * (DESIGN.md 3.19).  `acs` is [ysize_blocks][xsize_blocks] u8 in the layout of
 * jxg_stats.ac_strategy / jxg_decode_maps: a varblock's first block holds its
 * raw id, every other block it covers 0x80 | id.  Accepted ids:
 *   - the 8x8 class (0, 1, 2, 3, 12, 13);
 *   - the nine merged shapes up to 64 px (4, 5, 6, 7, 10, 11, 18, 19, 20), at
 *     any block position inside one 64x64 tile and the frame's blocks (the
 *     decoder's tile rule), not only at the multiples of their size the search
 *     produces;
 *   - the six kinds of 128 / 256 px, as (rows, columns) of blocks 21 = 16x16,
 *     22 = 16x8, 23 = 8x16, 24 = 32x32, 25 = 32x16, 26 = 16x32, on the shape's
 *     own grid alone: block row a multiple of its blocks down, block column a
 *     multiple of its blocks across, inside the frame's blocks.  There a
 *     varblock never crosses a 256x256 pass group.  A decoder reads some other
 *     placements of these kinds; this encoder has no transform path for them.
 *
 * jxg_check_strategy_map (host only, no context) says whether a map is
 * accepted.  A first block is judged in this order: claimed by another
 * varblock, id and placement supported, fits the frame (up to 64 px: and the
 * tile).  JXG_ERR_UNSUPPORTED for a first block's id without a shape here
 * (AFV 8, 9; 32X8 / 8X32 14 - 17; ids >= 27) and for an id 21 - 26 off its own
 * grid; JXG_ERR_INVALID_ARG for a null map, a size jxg_encode_rgb8 refuses, a
 * varblock reaching past the frame's blocks (ids 21 - 26 on their grid
 * included) or, up to 64 px, across a tile border, a covered byte that is not
 * 0x80 | id of the varblock covering it, a covered byte no varblock covers, a
 * first block inside another varblock, or overlap.  On refusal *bad_block
 * (may be NULL) is the raster index of the first offending block in raster
 * order.
 *
 * The encode calls validate the map before anything is uploaded or launched;
 * a refused map returns the validator's status with *out = {NULL, 0} and
 * leaves the context as it was (jxg_reconstruct_rgb8 still serves the encode
 * before).  `qf` (or NULL) has the same geometry and holds raw - 1 per block
 * as jxg_stats.quant_field; it replaces the adaptive quant field (NULL: the
 * context's own, heuristic or masking).  A merged varblock takes the largest
 * value of the blocks it covers.  Both maps are host memory in both variants.
 * Everything that is not a choice (XYB, Gaborish, DC, chroma from luma, the
 * coder, the filters signalled) is what an effort-7 encode of the context's
 * distance and flags computes; the context's effort and proposals play no
 * part -- a map with ids 21 - 26 is encoded on a context of any effort -- and
 * jxg_stats.homogeneity is NULL.  In every other respect this is
 * jxg_encode_rgb8: JXG_FLAG_KEEP_MAPS, jxg_get_stats, jxg_reconstruct_rgb8 and
 * the reports serve it alike; JXG_ERR_INVALID_ARG for null arguments, a stride
 * under 3 * xsize or streamed frames pending.  There is no batch, streaming,
 * sweep or sharded form. */
jxg_status jxg_check_strategy_map(const uint8_t* acs, uint32_t xsize, uint32_t ysize,
                                  uint32_t* bad_block);
jxg_status jxg_encode_forced_rgb8(jxg_ctx* ctx, const uint8_t* rgb, uint32_t xsize,
                                  uint32_t ysize, size_t row_stride, const uint8_t* acs,
                                  const uint8_t* qf, jxg_buffer* out);
jxg_status jxg_encode_forced_rgb8_device(jxg_ctx* ctx, const void* d_rgb, uint32_t xsize,
                                         uint32_t ysize, size_t row_stride, const uint8_t* acs,
                                         const uint8_t* qf, jxg_buffer* out);
/* Traced encode: a search encode that keeps every estimate its AC-strategy
 * search compared.  jxg_encode_traced_rgb8[_device] is
 * jxg_encode_rgb8[_device] with the context's distance, effort, proposals and
 * flags: the same bytes, jxg_get_stats maps, reconstruction and reports.
 * Effort < 5 has no search: JXG_ERR_UNSUPPORTED, nothing touched (*out =
 * {NULL, 0}; jxg_reconstruct_rgb8 still serves the encode before).
 * JXG_ERR_INVALID_ARG wherever jxg_encode_rgb8 returns it and while streamed
 * frames are pending.  There is no batch, streaming, sharded or forced form;
 * a sweep carries the summary, not the planes, per point
 * (jxg_set_sweep_trace below).
 *
 * jxg_search_trace copies the estimates out; either pointer may be NULL.  It
 * is valid when the context's last use of its buffers was a traced encode,
 * JXG_ERR_INVALID_ARG otherwise (a plain, forced, batch, streamed, sharded or
 * warm-up encode, a decode, no encode at all, frames pending).  It changes
 * nothing the encoder, jxg_reconstruct_rgb8 or the reports read; two calls
 * give the same bits.
 *
 * jxg_trace_maps: caller-owned host planes over the block grid
 * [ysize_blocks][xsize_blocks] (nb blocks), each may be NULL.
 *   cand8_raw, cand8  f32 [6][nb]: the 8x8 scan's six estimates before hook F
 *                     and as compared after it, in scan order DCT8, DCT4X4,
 *                     DCT2X2, DCT4X8, DCT8X4, IDENTITY; every entry a full
 *                     evaluation (a traced job does not prune); equal bit for
 *                     bit without proposals bit 1 (hook F)
 *   scan8             u8 [nb]: raw id of the scan's winner
 *   front8            u8 [nb]: raw id the front kernel wrote (differs from
 *                     scan8 only where hook P overrode a DCT8 win)
 *   qf8               u8 [nb]: raw - 1 of the front kernel, before merged
 *                     varblocks take their maxima
 *   merged            f32 [9][nb], plane order ids 6, 7, 4, 10, 11, 5, 19, 20,
 *                     18: a candidate varblock's estimate as compared (hook F
 *                     applied) at its first block on the shape's own grid; NaN
 *                     everywhere else (not a first block, a candidate that does
 *                     not fit the frame's blocks, a level the effort does not
 *                     search: effort 5 stops at 32 px)
 *   big               f32 [6][nb], plane order ids 22, 23, 21, 25, 26, 24, the
 *                     same rule; all NaN below effort 8; never +inf
 *   chosen            f32 [nb]: the final estimate -- of the chosen varblock at
 *                     its first block, 0 at covered blocks (under hook P the
 *                     scan's best from before the override)
 * jxg_trace_summary: exact integers reduced on the GPU; indices 0..5 are the
 * scan order.
 *   flip[r][s]        blocks by (winner of the scan replayed on cand8_raw,
 *                     scan8): diagonal without hook F
 *   hook_p[t]         overridden blocks by target
 *   merged_over[s]    blocks by scan8 whose final strategy byte is not of the
 *                     8x8 class
 *   margin[s][n]      by scan8; best and second the two lowest of cand8 in the
 *                     scan's order, n = the number of k in 0..6 with
 *                     second >= best * (1.0f + 2^-k) in f32
 *   margin_skipped[s] blocks left out of margin: best not below FLT_MAX, NaN,
 *                     or <= 0 (hook F's factor may be negative) */
typedef struct {
  float* cand8_raw;
  float* cand8;
  uint8_t* scan8;
  uint8_t* front8;
  uint8_t* qf8;
  float* merged;
  float* big;
  float* chosen;
} jxg_trace_maps;
typedef struct {
  uint32_t blocks;
  uint32_t max_px; /* largest level searched: 32 (e5), 64 (e6, e7), 256 (e8+) */
  uint32_t flip[6][6];
  uint32_t hook_p[6];
  uint32_t merged_over[6];
  uint32_t margin[6][8];
  uint32_t margin_skipped[6];
} jxg_trace_summary;
jxg_status jxg_encode_traced_rgb8(jxg_ctx* ctx, const uint8_t* rgb, uint32_t xsize,
                                  uint32_t ysize, size_t row_stride, jxg_buffer* out);
jxg_status jxg_encode_traced_rgb8_device(jxg_ctx* ctx, const void* d_rgb, uint32_t xsize,
                                         uint32_t ysize, size_t row_stride, jxg_buffer* out);
jxg_status jxg_search_trace(jxg_ctx* ctx, jxg_trace_maps* maps, jxg_trace_summary* summary);
/* n frames of equal size (benchmark config 3: 64 x 1080p; the reference's
 * caller encodes every image at 10 distances x 5 efforts, benchmark.rs:
 * 637-642), through the streaming pipeline below (jxg_submit_rgb8 of every
 * frame, codestreams collected as they complete), so the frames' H2D copies,
 * kernels, rANS chains and host-side code construction overlap over the
 * pipeline's lanes.  outs[i] is frame i's codestream (byte-identical to
 * jxg_encode_rgb8 of that frame); on error every output is released.  The
 * context must have no streamed frames pending (JXG_ERR_INVALID_ARG
 * otherwise).  jxg_get_stats then describes the last frame. */
jxg_status jxg_encode_batch_rgb8(jxg_ctx* ctx, const uint8_t* const* rgbs, uint32_t n,
                                 uint32_t xsize, uint32_t ysize, size_t row_stride,
                                 jxg_buffer* outs);
/* the same with device-resident frames */
jxg_status jxg_encode_batch_rgb8_device(jxg_ctx* ctx, const void* const* d_rgbs, uint32_t n,
                                        uint32_t xsize, uint32_t ysize, size_t row_stride,
                                        jxg_buffer* outs);
/* Streaming encode, one host thread: frames are submitted in order and their
 * codestreams received in the same order (byte-identical to jxg_encode_rgb8
 * of each frame).  Internally a software pipeline over this context and up to
 * 11 lanes it creates on first use (same parameters; released by
 * jxg_destroy); the depth D follows the frame size (7 lanes at 8K, 12 at 4K
 * and below; jxg_pipeline_depth), never more than the process's hardware
 * queues - 1 (GPU_MAX_HW_QUEUES, HIP's default 4: raise it, at most 32,
 * before HIP initialises for the full depth -- two lanes on one queue
 * serialise their kernels): a submit finishes the frame submitted D calls earlier if it is
 * still in flight, launches the new frame's front end / merge stage /
 * statistics on a free lane, starts the previous frame's codes on a helper
 * thread and joins the codes of the frame `lag` submits back (1 at 8K, 3 for
 * small frames), whose helper launched its emission -- so the rANS chains
 * (JXG_FLAG_ANS) of earlier frames run under the transform kernels of the
 * next.  Each lane uses its own HIP stream: the process needs that many
 * hardware queues (GPU_MAX_HW_QUEUES=16 set before the HIP runtime starts).
 * jxg_receive blocks until the oldest frame is complete
 * (JXG_ERR_INVALID_ARG if none is pending); jxg_pending counts frames
 * submitted and not yet received.  A device frame must stay unchanged until
 * its codestream is received; a host frame is copied into pinned staging
 * before jxg_submit_rgb8 returns.  jxg_get_stats after jxg_receive describes
 * the received frame.  On an error every frame in flight is dropped. */
jxg_status jxg_submit_rgb8(jxg_ctx* ctx, const uint8_t* rgb, uint32_t xsize, uint32_t ysize,
                           size_t row_stride);
jxg_status jxg_submit_rgb8_device(jxg_ctx* ctx, const void* d_rgb, uint32_t xsize, uint32_t ysize,
                                  size_t row_stride);
jxg_status jxg_receive(jxg_ctx* ctx, jxg_buffer* out);
jxg_status jxg_pending(jxg_ctx* ctx, uint32_t* n);
/* frames the streaming pipeline keeps in flight for frames of this size
 * (world == 1) or for this rank's shard of them (jxg_shard_submit_device):
 * lanes x frames per lane (one batched launch per lane), less what keeps a
 * lane free for the next submit -- (lanes - 1) x batch + 1 */
jxg_status jxg_pipeline_depth(jxg_ctx* ctx, uint32_t xsize, uint32_t ysize, uint32_t rank,
                              uint32_t world, uint32_t* depth);
/* at most `lanes` pipeline lanes (1..12; 0: the default, GPU_MAX_HW_QUEUES - 1)
 * for this context's later streams -- for several contexts streaming on ONE
 * GPU (ranks rehearsed on a shared device), which would otherwise put up to
 * 12 lanes each on the same hardware queues.  JXG_ERR_INVALID_ARG while
 * frames are pending.  jxg_pipeline_depth reflects the cap. */
jxg_status jxg_set_pipeline_lanes(jxg_ctx* ctx, uint32_t lanes);
jxg_status jxg_get_stats(jxg_ctx* ctx, jxg_stats* stats);
void jxg_buffer_free(jxg_buffer* buf);

/* ---- multi-GPU group sharding (one context per rank) ----
 * A frame's 256x256 pass groups are split over `world` ranks (jxg_shard_plan):
 *   kind 0: balanced contiguous raster ranges (rank r: [n*r/world,
 *           n*(r+1)/world)), every LF group (2048x2048) owned by the rank of
 *           most of its pass groups, when that leaves no LF group split over
 *           ranks (16384^2 over 8);
 *   kind 1: else whole LF groups per rank (largest first to the least-loaded
 *           rank) when the largest load is within 5 % of the mean (8K over
 *           2 / 4 / 8): no per-block records move;
 *   kind 2: else the ranges of kind 0 with the record exchange below.
 * The owner of an LF group encodes its LF-group stream.  Per rank:
 *   1. jxg_shard_sizes: words of the AC histogram (132 x 128 counts, then
 *      the rank's varblock count per 128 / 256 px kind, whose sum decides
 *      which quant tables HfGlobal carries) and the byte capacity of the
 *      record send / receive buffers (the largest of any rank);
 *      jxg_shard_exchange: this rank's send and receive bytes per peer;
 *   2. jxg_shard_begin: front end + merge stage + AC token statistics of the
 *      rank's groups; writes the rank's AC histogram to d_hist (u32, device)
 *      and, into d_xbuf (device), the per-block records (strategy, quant
 *      field, quantized DC; 14 KB per pass group) of its groups whose LF group
 *      another rank owns, ordered by destination rank;
 *   -- caller: prefix codes only, all-reduce(sum) d_hist (ANS: nothing, see
 *      below); all_to_all of the records with the jxg_shard_exchange splits
 *      (RCCL over xGMI) into a receive buffer (kinds 0 / 1: all splits 0);
 *   3. jxg_shard_end(d_hist, receive buffer): LF-group streams of its LF
 *      groups, entropy codes, emission of the rank's sections into a payload
 *      kept in device memory (rank 0's also carries LfGlobal, and HfGlobal
 *      with prefix codes); jxg_shard_payload copies it (payload_bytes) to
 *      device or host memory;
 *   -- caller: gather the payloads on rank 0 (RCCL, device to device);
 *   4. jxg_shard_assemble_device (rank 0): payloads in device memory (word
 *      aligned offsets) -> codestream in host memory; or jxg_shard_assemble:
 *      the same from host payloads, host only (no device).
 * Prefix codes (one HF preset from the summed histogram): payload heads of
 * version 1, and the codestream is byte-identical to jxg_encode_rgb8 of the
 * whole frame.  ANS (JXG_FLAG_ANS) with world > 1: every rank clusters its
 * own histogram into its own HF preset, so d_hist needs NO all-reduce; the
 * payload head is version 2 and carries the preset, HfGlobal is written at
 * assembly with num_hf_presets = world, and every pass group selects its
 * rank's preset -- the codestream decodes to exactly the single-GPU image
 * (same coefficients, strategies, quant field, DC, CfL), but its bytes differ
 * from jxg_encode_rgb8's.  The frame needs at least max(2, world) pass groups.
 * Codestreams are released with jxg_buffer_free. */
jxg_status jxg_shard_sizes(uint32_t xsize, uint32_t ysize, uint32_t world, size_t* hist_words,
                           size_t* slot_bytes);
/* the partition: owner rank of every pass group ([num_groups]) and LF group
 * ([num_lf_groups]), and its kind (0 / 1 / 2 above); any pointer may be NULL */
jxg_status jxg_shard_plan(uint32_t xsize, uint32_t ysize, uint32_t world, uint32_t* group_owner,
                          uint32_t* lf_owner, int* kind);
jxg_status jxg_shard_exchange(uint32_t xsize, uint32_t ysize, uint32_t world, uint32_t rank,
                              size_t* send_bytes /* [world] */, size_t* recv_bytes /* [world] */);
jxg_status jxg_shard_begin(jxg_ctx* ctx, const void* d_rgb, uint32_t xsize, uint32_t ysize,
                           size_t row_stride, uint32_t rank, uint32_t world, uint32_t* d_hist,
                           void* d_xbuf);
jxg_status jxg_shard_end(jxg_ctx* ctx, const uint32_t* d_hist, const void* d_xbuf,
                         size_t* payload_bytes);
jxg_status jxg_shard_payload(jxg_ctx* ctx, void* dst, int dst_on_device);
jxg_status jxg_shard_assemble_device(jxg_ctx* ctx, const void* d_payloads, const size_t* offsets,
                                     const size_t* sizes, uint32_t n, jxg_buffer* out);
jxg_status jxg_shard_assemble(const uint8_t* const* payloads, const size_t* sizes, uint32_t n,
                              jxg_buffer* out);

/* Distributed host assembly (instead of the payload gather + rank-0
 * assembly): after jxg_shard_end every rank exports its payload head
 * (jxg_shard_head: a few hundred u32; dst NULL -> *nwords = size), the heads
 * are all-gathered (any collective), and every rank calls
 * jxg_shard_write_host with all heads in rank order: it writes its own
 * sections D2H into `dst` -- one host buffer shared by all ranks (e.g. a
 * /dev/shm mapping, registered with jxg_host_register for DMA) -- at their
 * codestream offsets; rank 0 also writes headers + TOC.  *total = codestream
 * bytes (also returned with JXG_ERR_INVALID_ARG when dst_size is too small).
 * Once every rank has returned (a barrier), dst[0, total) holds the
 * codestream, byte-identical to jxg_shard_assemble_device. */
jxg_status jxg_shard_head(jxg_ctx* ctx, uint32_t* dst, size_t* nwords);
jxg_status jxg_shard_write_host(jxg_ctx* ctx, const uint32_t* const* heads, const size_t* head_words,
                                uint32_t n, void* dst, size_t dst_size, size_t* total);
/* Streaming sharded encode (the multi-GPU pipeline; kinds 0 / 1 with ANS, or
 * world == 1): every rank submits its shard of consecutive frames, in the
 * same order, through the same lanes as jxg_submit_rgb8_device -- front end,
 * merge stage, statistics, codes and rANS chains of several frames overlap,
 * with no collective inside a frame.  For each frame, in submission order:
 *   jxg_shard_next_head: waits until the oldest pending frame's sections are
 *     emitted and exports its payload head (dst NULL -> *nwords = size; the
 *     frame stays pending);
 *   -- caller: all-gather the heads (any collective);
 *   jxg_shard_write_next: as jxg_shard_write_host for that frame (its
 *     sections D2H into the shared host buffer at their codestream offsets,
 *     rank 0 adds headers + TOC), then releases its slot.  The copies are
 *     enqueued and NOT waited for: the call returns once the copies of the
 *     write JXG_SHARD_WRITE_LAG calls back have landed (this rank's part of
 *     frame k is in place when write_next of frame k + JXG_SHARD_WRITE_LAG
 *     returns, or after jxg_shard_write_flush);
 *   jxg_shard_write_flush: waits for every write's copies.
 * A frame's codestream is complete once every rank's part is in place.  At
 * most jxg_pipeline_depth frames may be pending (submit returns
 * JXG_ERR_INVALID_ARG when full; JXG_ERR_UNSUPPORTED for a plan needing the
 * record exchange or, with world > 1, for prefix codes).  The frame's device
 * RGB8 must stay unchanged until its write. */
jxg_status jxg_shard_submit_device(jxg_ctx* ctx, const void* d_rgb, uint32_t xsize, uint32_t ysize,
                                   size_t row_stride, uint32_t rank, uint32_t world);
jxg_status jxg_shard_next_head(jxg_ctx* ctx, uint32_t* dst, size_t* nwords);
jxg_status jxg_shard_write_next(jxg_ctx* ctx, const uint32_t* const* heads, const size_t* head_words,
                                uint32_t n, void* dst, size_t dst_size, size_t* total);
#define JXG_SHARD_WRITE_LAG 2
jxg_status jxg_shard_write_flush(jxg_ctx* ctx);
/* page-lock a host range (e.g. the node-shared /dev/shm codestream buffer of
 * jxg_shard_write_host / jxg_shard_write_next) so the ranks' D2H copies are DMA */
jxg_status jxg_host_register(void* ptr, size_t size);
jxg_status jxg_host_unregister(void* ptr);

/* thesis selector alone over a host XYB frame [3][ysize][xsize] (xsize, ysize
 * multiples of 8): r3 = (r_h, r_v, r_d) per block, type = raw strategy
 * (combined.diff:183-235) */
jxg_status jxg_homogeneity_map(jxg_ctx* ctx, const float* xyb, uint32_t xsize, uint32_t ysize,
                               float distance, uint32_t flags, float* r3, uint8_t* type);

/* ---- decode-side quality: the harness's metrics on the GPU ----
 * Replaces ImageReader::calculate_mse / calculate_psnr
 * (benchmark-jpegxl/src/image_reader.rs:555-606, via metrics.rs:28-53) and
 * calculate_ssim (metrics.rs:55-84, ImageMagick `compare -metric SSIM`).
 * orig / comp: RGB8 interleaved rows (comp = the decoded image).  mse is
 * bit-identical to the reference's sequential f64 sum; ssim is the mean
 * Gaussian-window (11x11, sigma 1.5, K1 0.01, K2 0.03) SSIM over all window
 * positions inside the image and the three channels -- ImageMagick's exact
 * variant is not in the reference (parity unpinned). */
typedef struct {
  uint64_t sse;     /* sum of squared sample differences (exact) */
  uint64_t samples; /* 3 * xsize * ysize */
  double mse;       /* sse / samples */
  double psnr;      /* 10 log10(255^2 / mse); +inf when mse == 0 */
  double ssim;      /* NaN when not requested or the image is under 11x11 */
} jxg_quality;

jxg_status jxg_compare_rgb8(jxg_ctx* ctx, const uint8_t* orig, size_t orig_stride,
                            const uint8_t* comp, size_t comp_stride, uint32_t xsize,
                            uint32_t ysize, int want_ssim, jxg_quality* out);
jxg_status jxg_compare_rgb8_device(jxg_ctx* ctx, const void* d_orig, size_t orig_stride,
                                   const void* d_comp, size_t comp_stride, uint32_t xsize,
                                   uint32_t ysize, int want_ssim, jxg_quality* out);

/* ---- MS-SSIM (Wang, Simoncelli, Bovik 2003) on the GPU ----
 * The harness's column 13, which the reference leaves at 0.0
 * (benchmark.rs:932-933).  Five scales; scale 0 is the two RGB8 images, each
 * channel on its own, and scale j + 1 is the 2 x 2 box mean of scale j (an odd
 * last row or column dropped), so scale j has (xsize >> j) x (ysize >> j)
 * samples, held as exact f32 planes.  At every scale the window, constants and
 * expressions are jxg_quality.ssim's, plus cs = (2 cov + C2) / (var_a + var_b +
 * C2); cs[j] / ssim[j] are the means over all windows and the three channels.
 * ms_ssim = prod_{j<4} max(cs[j], 0)^W[j] * max(ssim[4], 0)^W[4] with W =
 * {0.0448, 0.2856, 0.3001, 0.2363, 0.1333}: 0.0 when a mean is not positive.
 * Deterministic: two calls on the same images give the same bits.
 * JXG_ERR_INVALID_ARG as jxg_compare_rgb8: a null argument, a stride under
 * 3 * xsize, or streamed frames pending.  The pyramid planes (about 8 bytes a
 * pixel) are allocated by the first call and released by jxg_destroy. */
typedef struct {
  double ms_ssim;   /* NaN when min(xsize, ysize) < 176 (then cs / ssim are NaN too) */
  double cs[5];     /* mean contrast-structure term per scale */
  double ssim[5];   /* mean SSIM per scale; ssim[0] is bit-equal to jxg_quality.ssim */
} jxg_msssim;
jxg_status jxg_msssim_rgb8(jxg_ctx* ctx, const uint8_t* orig, size_t orig_stride,
                           const uint8_t* comp, size_t comp_stride, uint32_t xsize,
                           uint32_t ysize, jxg_msssim* out);
jxg_status jxg_msssim_rgb8_device(jxg_ctx* ctx, const void* d_orig, size_t orig_stride,
                                  const void* d_comp, size_t comp_stride, uint32_t xsize,
                                  uint32_t ysize, jxg_msssim* out);

/* ---- decode-side reconstruction: decoded pixels without a decoder ----
 * The decoded image of the frame this context encoded last with
 * jxg_encode_rgb8 / jxg_encode_rgb8_device: what a conforming decoder
 * reconstructs from that codestream (dequantization, inverse transforms,
 * chroma from luma, Gaborish / EPF as signalled, XYB -> sRGB8), computed from
 * the context's device-resident coefficients -- no bitstream parse, no
 * JXG_FLAG_KEEP_MAPS needed, and no buffer the encoder reads is modified (a
 * later encode gives the same bytes).  rgb / d_rgb: xsize x ysize RGB8
 * interleaved, row_stride >= 3 * xsize bytes per row, of which only the first
 * 3 * xsize are written.  Both calls return when the image is complete.  The
 * float planes they need are allocated by the first call and released by
 * jxg_destroy.  Arithmetic is f32: against a double-precision decoder a
 * sample may differ by 1 where a value sits on a rounding boundary.
 * JXG_ERR_INVALID_ARG: null arguments, a stride too small, no frame encoded
 * yet, streamed frames pending, or the context's last encode was not a
 * one-at-a-time encode (or a decode has used the context's buffers since) --
 * the coefficients of batch, streamed and sharded frames (and of jxg_warmup's
 * synthetic frame) live in pipeline lanes or on other ranks: their decoded
 * pixels come from their codestream, through jxg_decode_rgb8 below. */
jxg_status jxg_reconstruct_rgb8(jxg_ctx* ctx, uint8_t* rgb, size_t row_stride);
jxg_status jxg_reconstruct_rgb8_device(jxg_ctx* ctx, void* d_rgb, size_t row_stride);

/* ---- decoder: codestream -> decoded pixels ----
 * Reads exactly what this encoder writes (one-at-a-time, batch, streamed and
 * sharded frames alike): bare codestream, SizeHeader, all-default
 * ImageMetadata, one regular VarDCT frame of one pass with the default LF
 * dequantization / block context map / colour correlation / coefficient
 * orders, Gaborish on or off and 0-3 EPF iterations without custom weights,
 * an unpermuted TOC in either section layout, modular LF groups with local MA
 * trees, prefix-code or 12-bit rANS entropy streams without LZ77, and
 * num_hf_presets >= 1 (sharded ANS streams carry one per rank).  Any other
 * stream returns JXG_ERR_UNSUPPORTED, never a wrong image; a malformed one
 * (truncated, sizes that do not add up, a symbol outside its alphabet, a
 * non-zero count too large or not exhausted, overlapping varblocks, a wrong
 * ANS final state) returns JXG_ERR_INVALID_ARG.  Headers, TOC, LfGlobal,
 * HfGlobal, the decode tables and the LF groups' streams (one task per LF
 * group, at most 8 helper threads) are decoded on the host; the pass groups
 * -- all AC tokens -- on the GPU, one wave per group (csrc/jxg_decode.hip);
 * the pixels by the reconstruction kernels of jxg_reconstruct_rgb8
 * (DESIGN.md 3.12). */
typedef struct {
  uint32_t xsize, ysize, num_groups, num_lf_groups;
  uint32_t global_scale, quant_dc, num_hf_presets;
  uint32_t ans;          /* 1: rANS, 0: prefix codes (the AC stream) */
  uint32_t gaborish, epf_iters;
} jxg_stream_info;

/* host only, no context: headers + TOC + LfGlobal / HfGlobal heads (a frame of
 * one pass group keeps everything in one section, so its LF group is decoded
 * on the way).  JXG_ERR_INVALID_ARG for null arguments or size == 0. */
jxg_status jxg_decode_info(const uint8_t* data, size_t size, jxg_stream_info* info);

/* codestream (host memory) -> decoded RGB8, on the GPU.  rgb / d_rgb as for
 * jxg_reconstruct_rgb8: xsize x ysize interleaved, row_stride >= 3 * xsize, of
 * which only the first 3 * xsize bytes of a row are written; both calls return
 * when the image is complete.  The context's distance / effort / flags play no
 * part.  The decode uses the context's coefficient and map buffers (allocated
 * or grown on first use, like the reconstruction planes), so afterwards
 * jxg_reconstruct_rgb8 returns JXG_ERR_INVALID_ARG until the next one-at-a-time
 * encode; encodes are not affected.  JXG_ERR_INVALID_ARG: null data / rgb,
 * size == 0, a stride under 3 * xsize, or streamed frames pending. */
jxg_status jxg_decode_rgb8(jxg_ctx* ctx, const uint8_t* data, size_t size,
                           uint8_t* rgb, size_t row_stride);
jxg_status jxg_decode_rgb8_device(jxg_ctx* ctx, const uint8_t* data, size_t size,
                                  void* d_rgb, size_t row_stride);

/* the decoded maps in jxg_stats' layouts: acs [blocks] raw strategy, qf [blocks]
 * raw - 1, dc [3][blocks], ac [blocks][3][64], cmap [2][tiles] of int8 chroma
 * from luma factors per 64 x 64 tile (any may be NULL).
 * ctx == NULL: the host path of the same decode core, no device touched;
 * else the pass groups are decoded on the GPU and the maps downloaded (not
 * while streamed frames are pending). */
jxg_status jxg_decode_maps(jxg_ctx* ctx, const uint8_t* data, size_t size, uint8_t* acs,
                           uint8_t* qf, int32_t* dc, int32_t* ac, int8_t* cmap);

/* milliseconds of the context's last jxg_decode_rgb8[_device]: ms[0] host parse
 * of headers / TOC / LfGlobal / HfGlobal and the decode tables, ms[1] the LF
 * groups on the host threads, ms[2] the pass-group kernel and ms[3] the
 * reconstruction chain (device time by events), ms[4] the whole call (host
 * wall clock) */
jxg_status jxg_decode_timings(jxg_ctx* ctx, float* ms /* [5] */);

/* ---- batch decode: n codestreams in one call ----
 * The pass-group kernel of one frame lasts as long as its longest pass group
 * and leaves most of the GPU idle; a batch puts the pass
 * groups of many frames into one launch.  datas[i] / sizes[i]: the codestreams
 * (host memory); rgbs[i] / d_rgbs[i] with row_strides[i]: each frame's output
 * as for jxg_decode_rgb8[_device].  Frames may differ in size, coder, presets
 * and filters.  Every frame is parsed on the host (at most 8 helper threads
 * for all frames' LF groups), frames are taken in consecutive chunks whose
 * device footprint -- per frame blocks * 398 bytes of maps and coefficients,
 * its stream, tables and section bounds -- fits the byte budget of
 * jxg_set_decode_batch_bytes (default 2 GiB: 64 1080p frames of about 13 MB or
 * nine 8K frames of about 206 MB; a frame that alone exceeds it is a chunk of
 * its own, never refused for its size), each chunk's pass groups run in one
 * launch (two when the chunk mixes frames whose symbol tables fit LDS with
 * frames whose tables do not), then each frame's reconstruction chain.
 * Outputs are byte-identical to jxg_decode_rgb8 of each stream.
 * Call-level errors, nothing touched: JXG_ERR_INVALID_ARG for a null ctx /
 * datas / sizes / rgbs / row_strides, n == 0, or streamed frames pending.
 * Otherwise every frame gets its own status in statuses[i] (may be NULL):
 * JXG_ERR_INVALID_ARG for a null or empty stream, a null output or a stride
 * under 3 * xsize, and JXG_ERR_UNSUPPORTED / JXG_ERR_INVALID_ARG as
 * jxg_decode_rgb8 gives them; a refused frame's buffer is not written and the
 * other frames complete.  Returns the first non-OK frame status in index
 * order, or JXG_OK.  JXG_ERR_HIP and JXG_ERR_OOM are call-level and fill every
 * status.  Like jxg_decode_rgb8 the call ends what jxg_reconstruct_rgb8 could
 * read; encodes are not affected. */
jxg_status jxg_decode_batch_rgb8(jxg_ctx* ctx, const uint8_t* const* datas, const size_t* sizes,
                                 uint32_t n, uint8_t* const* rgbs, const size_t* row_strides,
                                 jxg_status* statuses /* [n] or NULL */);
jxg_status jxg_decode_batch_rgb8_device(jxg_ctx* ctx, const uint8_t* const* datas,
                                        const size_t* sizes, uint32_t n, void* const* d_rgbs,
                                        const size_t* row_strides,
                                        jxg_status* statuses /* [n] or NULL */);
/* the device-memory budget of a chunk, bytes; 0: the default (2 GiB).  Not
 * while streamed frames are pending. */
jxg_status jxg_set_decode_batch_bytes(jxg_ctx* ctx, size_t bytes);

/* the context's last jxg_decode_batch_rgb8[_device] */
typedef struct {
  uint32_t frames;           /* n of the call */
  uint32_t chunks;           /* arenas filled, one or two launches each */
  uint32_t items_staged;     /* work items (pass groups) launched with their symbol tables in LDS */
  uint32_t items_unstaged;   /*   and with the tables in memory */
  float ms_parse;            /* host: every frame's parse and LF groups (wall clock) */
  float ms_groups;           /* the pass-group launches, device time by events, summed over chunks */
  float ms_recon;            /* the reconstruction chains, by events, summed over chunks */
  float ms_call;             /* the whole call, host wall clock */
} jxg_decode_batch_stats;
jxg_status jxg_decode_batch_timings(jxg_ctx* ctx, jxg_decode_batch_stats* stats);

/* ---- sweep: one image over many settings in one call ----
 * The reference harness encodes every image at 10 distances x 5 efforts and
 * measures each result (benchmark.rs:637-677).  A sweep uploads the image once
 * (or reads the caller's device copy) and runs the n points through the
 * streaming pipeline's lanes of this one context: a frame carries its point
 * and the lane it lands on encodes with it (a lane's parameters are set at
 * every submit; lanes grow whatever buffers a point needs).  outs[i] is
 * byte-identical to jxg_encode_rgb8 of the image on a context created with
 * points[i].  quality 1 / 2: after a frame's codestream is assembled, its
 * lane runs the reconstruction chain of jxg_reconstruct_rgb8 on its own
 * coefficients and stream, ending in a kernel that converts to sRGB8 and sums
 * the squared error against the original in one pass (the decoded image is
 * stored only when quality == 2, for the SSIM kernels); q[i] is bit-equal to
 * jxg_compare_rgb8_device(original, jxg_reconstruct_rgb8_device) after a
 * one-at-a-time encode with points[i] (ssim NaN with quality 1 or under
 * 11 x 11).  The float planes (24 bytes per block-padded pixel and lane, plus
 * 3 with quality 2) are allocated by the first quality sweep and released by
 * jxg_destroy.  Small frames, which the pipeline batches four to a launch,
 * go one point per launch (a change of point closes the open batch).
 * The context's own distance / effort / proposals / flags play no part and
 * are unchanged afterwards; like a batch encode the call ends what
 * jxg_reconstruct_rgb8 could read.  A device image must stay unchanged until
 * the call returns.
 * Call-level errors, nothing touched: JXG_ERR_INVALID_ARG for a null ctx /
 * rgb / points / outs, n == 0, a size jxg_encode_rgb8 refuses, a stride under
 * 3 * xsize, quality outside 0..2, q non-NULL with quality 0 or NULL
 * otherwise, or streamed frames pending.  Otherwise every point gets its
 * status in statuses[i] (may be NULL): JXG_ERR_INVALID_ARG for a distance,
 * effort or proposals jxg_create refuses, or JXG_FLAG_KEEP_MAPS; a refused
 * point's output is {NULL, 0} (its q[i] zeroed) and the others complete.
 * Returns the first non-OK status in index order.  JXG_ERR_HIP / JXG_ERR_OOM
 * (and any other failure of the pipeline) are call-level: every output is
 * released and every status filled. */
typedef struct {
  float distance; /* (0, 25], computed with max(distance, JXG_MIN_DISTANCE) */
  int effort;
  uint32_t proposals;
  uint32_t flags;
} jxg_sweep_point;
jxg_status jxg_sweep_rgb8(jxg_ctx* ctx, const uint8_t* rgb, uint32_t xsize, uint32_t ysize,
                          size_t row_stride, const jxg_sweep_point* points, uint32_t n,
                          int quality, jxg_buffer* outs /* [n] */,
                          jxg_quality* q /* [n]; NULL iff quality == 0 */,
                          jxg_status* statuses /* [n] or NULL */);
jxg_status jxg_sweep_rgb8_device(jxg_ctx* ctx, const void* d_rgb, uint32_t xsize, uint32_t ysize,
                                 size_t row_stride, const jxg_sweep_point* points, uint32_t n,
                                 int quality, jxg_buffer* outs, jxg_quality* q,
                                 jxg_status* statuses);
/* the context's last jxg_sweep_rgb8[_device] */
typedef struct {
  uint32_t points;   /* points encoded (refused ones not counted) */
  uint32_t lanes;    /* pipeline lanes the frame size gets (jxg_pipeline_depth's lanes) */
  float ms_call;     /* the whole call, host wall clock */
  float ms_upload;   /* host variant: the image's upload (host wall clock) */
  float ms_encode;   /* device time by events, summed over points: frame start -> emission */
  float ms_recon;    /*   reconstruction chain incl. the fused colour + error kernel */
  float ms_metrics;  /*   SSIM (or MS-SSIM) kernels, the strategy reduction, the results' download */
} jxg_sweep_stats;
jxg_status jxg_sweep_timings(jxg_ctx* ctx, jxg_sweep_stats* stats);
/* MS-SSIM in a sweep.  With the switch on (default 0; JXG_ERR_INVALID_ARG
 * while streamed frames are pending) a quality-2 sweep also runs the MS-SSIM
 * kernels for every point on its lane, where the SSIM kernels would run, on
 * the decoded image that quality 2 stores (scale 0's SSIM sum is the SSIM
 * kernels', bit for bit, and fills q[i].ssim); the original's pyramid is built
 * once per sweep.
 * Codestreams and q[] are unchanged, ms_metrics includes the added kernels,
 * and sweeps of other quality levels, or with the switch off, are untouched.
 * jxg_sweep_msssim copies the last sweep's results out in point order, each
 * bit-equal to jxg_msssim_rgb8_device(original, jxg_reconstruct_rgb8_device)
 * after a one-at-a-time encode with that point (NaN fields under 176 pixels,
 * a refused point zero-filled); JXG_ERR_INVALID_ARG when the last sweep did
 * not compute them or n is not that sweep's. */
jxg_status jxg_set_sweep_msssim(jxg_ctx* ctx, int on);
jxg_status jxg_sweep_msssim(jxg_ctx* ctx, jxg_msssim* out, uint32_t n);

/* ---- per-strategy statistics of an encode ----
 * How the frame's area, surviving coefficients, quantizer and squared error
 * split over the AC strategies the encoder chose: one row per raw AcStrategy
 * id.  A block belongs to the strategy of the varblock that covers it (the
 * low 7 bits of its ac_strategy byte; bit 7 marks a covered non-first block).
 * Every field is an exact integer sum, reduced on the GPU from the buffers of
 * the encode (csrc/jxg_report.hip): the rows add up to the frame's blocks,
 * xsize * ysize pixels and jxg_compare_rgb8's sse. */
#define JXG_NUM_STRATEGIES 27            /* raw AcStrategy ids 0..26; AFV 14..17 and
                                            the ids the encoder never emits stay zero */
typedef struct {
  uint64_t varblocks;    /* varblocks of this strategy (first blocks) */
  uint64_t blocks;       /* 8x8 blocks they cover */
  uint64_t pixels;       /* image pixels inside those blocks (edge blocks cropped to xsize, ysize) */
  uint64_t nonzeros[3];  /* non-zero quantized AC coefficients, X / Y / B (entries of jxg_stats' ac) */
  uint64_t qf_sum;       /* sum over covered blocks of the raw quant field (stored value + 1) */
  uint64_t sse;          /* sum of squared RGB8 sample differences, decoded vs original, over `pixels` */
} jxg_strategy_row;      /* 64 bytes */
typedef struct { jxg_strategy_row row[JXG_NUM_STRATEGIES]; } jxg_strategy_report;
/* The report of the context's last one-at-a-time encode against orig / d_orig
 * (xsize x ysize RGB8, rows of orig_stride bytes): the reconstruction chain of
 * jxg_reconstruct_rgb8 runs into scratch and ends in a kernel that compares
 * each decoded pixel -- exactly the pixels jxg_reconstruct_rgb8 returns --
 * with the original's and keeps one sum per 8x8 block; one reduction over the
 * blocks then fills the table.  block_sse (host memory; d_block_sse device
 * memory; may be NULL) receives that map, [ysize_blocks][xsize_blocks] u32:
 * the squared error of the block's image pixels over the three channels.
 * Nothing the encoder reads is modified.  Both calls return when the results
 * are complete.  JXG_ERR_INVALID_ARG where jxg_reconstruct_rgb8 gives it (no
 * one-at-a-time encode was the context's last use of its buffers, streamed
 * frames pending), for a null orig / out and for orig_stride < 3 * xsize. */
jxg_status jxg_strategy_report_rgb8(jxg_ctx* ctx, const uint8_t* orig, size_t orig_stride,
                                    jxg_strategy_report* out, uint32_t* block_sse);
jxg_status jxg_strategy_report_rgb8_device(jxg_ctx* ctx, const void* d_orig, size_t orig_stride,
                                           jxg_strategy_report* out, uint32_t* d_block_sse);
/* Reports in a sweep.  With the switch on (default 0; JXG_ERR_INVALID_ARG
 * while streamed frames are pending) every sweep of quality 1 or 2 also fills
 * one report per point on its lane: the chain ends in the block-map form of
 * the fused colour + error kernel and the reduction follows the metrics.
 * Codestreams, q[] and the MS-SSIM results are unchanged, ms_metrics includes
 * the reduction, and sweeps with the switch off launch what they launched
 * before.  jxg_sweep_report copies the last sweep's reports out in point
 * order, each bit-equal to jxg_strategy_report_rgb8_device after a
 * one-at-a-time encode with that point (a refused point zero-filled; block
 * maps are not kept); JXG_ERR_INVALID_ARG when the last sweep computed none
 * (switch off, or quality 0), when n is not that sweep's, or while streamed
 * frames are pending. */
jxg_status jxg_set_sweep_report(jxg_ctx* ctx, int on);
jxg_status jxg_sweep_report(jxg_ctx* ctx, jxg_strategy_report* out, uint32_t n);

/* ---- coded bits per block and per strategy ----
 * What the tokens of a varblock, and of all varblocks of a strategy, cost in
 * the pass groups' AC streams as written.  Costs are exact integers in units of
 * 1 / JXG_RATE_UNIT bit.  A token costs symbol_cost + JXG_RATE_UNIT * nbits
 * (nbits: its raw bits).  Prefix codes: symbol_cost = JXG_RATE_UNIT * the length
 * of the (cluster, token) code in the frame's final codes.  ANS: symbol_cost =
 * jxg_rate_symbol_cost(f), f (1..4096) the symbol's normalised frequency in the
 * histogram the stream carries.  A varblock's tokens are all tokens of its
 * three channels, the non-zero-count token included, attributed to its first
 * block.  Bound: a varblock has at most 3 x 65536 tokens of at most 7680 units
 * (a symbol is at most 15 bits, raw bits at most 15), 1 509 949 440 < 2^32, so
 * a u32 per block never overflows.
 * Not attributed: the LF groups' streams (DC, strategy / quant-field metadata)
 * and the headers -- they are what stream_bits - ac_bits leaves. */
#define JXG_RATE_UNIT 256u
/* floor(256 * log2(4096.0 / f) + 0.5) in double; 0 for f = 0 or f > 4096.
 * Host only, needs no context.  Over f = 1..4096 the value nearest a rounding
 * tie is 2.4e-4 away (f = 1203), so every libm gives the same table; the
 * largest entry is 3072 (f = 1). */
uint32_t jxg_rate_symbol_cost(uint32_t f);
typedef struct {
  uint64_t tokens[3];   /* X / Y / B */
  uint64_t cost[3];     /* X / Y / B, 1/JXG_RATE_UNIT bit */
} jxg_rate_row;
/* (a struct tag, not a typedef: the report and the call that fills it share
 * the name, which C and C++ allow only for a tag -- write `struct jxg_rate_report`) */
struct jxg_rate_report {
  jxg_rate_row row[JXG_NUM_STRATEGIES];   /* by raw AcStrategy id of the varblock */
  uint64_t ac_bits;      /* exact: sum over pass groups of the bits of their AC streams as emitted
                            (ANS: incl. the 32-bit state), no byte padding */
  uint64_t stream_bits;  /* 8 * codestream bytes */
  uint32_t ans;          /* 1 rANS, 0 prefix codes */
  uint32_t groups;
};
/* The report of the context's last one-at-a-time encode, from what that encode
 * left on the device: the token records, the final code tables and the emit
 * pass's per-group bit counts; one kernel (csrc/jxg_rate.hip) prices every
 * record.  Needs no original image and no reconstruction.  block_cost (host
 * memory; d_block_cost device memory; may be NULL): [ysize_blocks]
 * [xsize_blocks] u32, the geometry of block_sse -- a varblock's first block
 * holds the sum of its three channels' costs, covered blocks 0, every word is
 * written.  Nothing the encoder, jxg_reconstruct_rgb8 or
 * jxg_strategy_report_rgb8 reads is modified: the calls can follow each other
 * in any order, and two calls give the same bits.  Both return when the results
 * are complete.  JXG_ERR_INVALID_ARG for a null ctx / out, where
 * jxg_reconstruct_rgb8 gives it (no encode yet; the last use was a batch,
 * streamed, sharded or warm-up encode, or a decode), and while streamed frames
 * are pending. */
jxg_status jxg_rate_report(jxg_ctx* ctx, struct jxg_rate_report* out, uint32_t* block_cost);
jxg_status jxg_rate_report_device(jxg_ctx* ctx, struct jxg_rate_report* out, uint32_t* d_block_cost);
/* Rate reports in a sweep.  With the switch on (default 0; JXG_ERR_INVALID_ARG
 * while streamed frames are pending) every sweep -- quality 0 included, nothing
 * here needs decoded pixels -- fills one report per point on its lane, after
 * that point's emission.  Codestreams, q[], MS-SSIM results and strategy
 * reports are unchanged, ms_metrics includes the added kernel (quality 1 / 2),
 * and with the switch off a sweep launches what it launched before.
 * jxg_sweep_rates copies the last sweep's reports out in point order, each
 * bit-equal to jxg_rate_report after a one-at-a-time encode with that point (a
 * refused point zero-filled; block maps are not kept); JXG_ERR_INVALID_ARG
 * when the last sweep computed none, when n is not that sweep's, or while
 * streamed frames are pending. */
jxg_status jxg_set_sweep_rates(jxg_ctx* ctx, int on);
jxg_status jxg_sweep_rates(jxg_ctx* ctx, struct jxg_rate_report* out, uint32_t n);

/* ---- A/B report of two encodes: strategy transitions ----
 * Side A and side B are two encodes of the same image, the same xsize x ysize,
 * any parameters.  Everything is counted per 8x8 block of the block grid:
 *   from / to  the raw strategy id of the varblock covering the block in A / in
 *              B (the low 7 bits of the ac_strategy byte);
 *   pixels     the block's image pixels, cropped as jxg_strategy_row.pixels;
 *   sse_a / b  the block's word of that side's block_sse
 *              (jxg_strategy_report_rgb8);
 *   cost_a / b the block's share of its varblock's coded cost, in
 *              1 / JXG_RATE_UNIT bit: a varblock of cost C (its word of
 *              jxg_rate_report's block_cost) covering n = across x down blocks,
 *              numbered k = 0 .. n-1 in raster order inside the varblock, gives
 *              block k  C / n + (k < C % n ? 1 : 0)  in integer arithmetic.
 *              The shares of a varblock add up to C exactly; a share is below
 *              2^31 (C <= 1 509 949 440).
 * The two sides partition the image differently; the shares make a varblock's
 * cost comparable block by block.  Every field is an exact integer sum: summed
 * over `to` the cells give side A's per-strategy blocks, pixels, sse and cost,
 * summed over `from` side B's. */
typedef struct {
  uint64_t blocks, pixels;
  uint64_t sse_a, sse_b;
  uint64_t cost_a, cost_b;      /* 1 / JXG_RATE_UNIT bit */
} jxg_ab_cell;                   /* 48 bytes */
typedef struct {
  jxg_ab_cell cell[JXG_NUM_STRATEGIES][JXG_NUM_STRATEGIES];  /* [from][to] */
} jxg_ab_report;
/* a and b: two contexts on the same HIP device (a == b is allowed and gives a
 * diagonal table), each one's last use a one-at-a-time encode of the same
 * image size; orig / d_orig is that image (RGB8, rows of orig_stride bytes).
 * Each context runs, on its own stream, the reconstruction chain into its block
 * error map, the rate kernel into its cost map and the share pass; the
 * transition kernel (csrc/jxg_ab.hip) runs on b's stream behind a's, without a
 * host wait in between.  Both contexts are used from the calling thread, and
 * the call returns when the results are complete.  block_delta (host memory;
 * d_block_delta device memory; may be NULL): [2][ysize_blocks][xsize_blocks]
 * int32, plane 0 sse_b - sse_a, plane 1 cost_b - cost_a (the shares), every
 * word written.  Nothing the encoder, jxg_reconstruct_rgb8,
 * jxg_strategy_report_rgb8 or jxg_rate_report reads is modified on either
 * context: those calls and this one can follow each other in any order, two
 * calls give the same bits and a re-encode the same bytes.
 * JXG_ERR_INVALID_ARG for a null a, b, orig or out, orig_stride < 3 * xsize,
 * different devices or frame sizes, a context where jxg_reconstruct_rgb8 or
 * jxg_rate_report would give it, and streamed frames pending on either. */
jxg_status jxg_ab_report_rgb8(jxg_ctx* a, jxg_ctx* b, const uint8_t* orig, size_t orig_stride,
                              jxg_ab_report* out, int32_t* block_delta);
jxg_status jxg_ab_report_rgb8_device(jxg_ctx* a, jxg_ctx* b, const void* d_orig, size_t orig_stride,
                                     jxg_ab_report* out, int32_t* d_block_delta);
/* A/B reports in a sweep.  jxg_set_sweep_ab names, for later sweeps of exactly
 * n points, the point each point is compared against: base[i] is -1 (no
 * comparison) or an index < i -- the baseline comes earlier in point order.
 * The array is copied; base == NULL or n == 0 switches it off (the default).
 * JXG_ERR_INVALID_ARG for a base[i] >= i or < -1 and while streamed frames are
 * pending.  With the switch on a sweep of another n is JXG_ERR_INVALID_ARG at
 * call level, nothing touched; a sweep of quality 1 or 2 fills one report for
 * every point with base[i] >= 0, side A point base[i], side B point i (a
 * quality-0 sweep computes none).  The points involved run the block-map form
 * of the fused colour + error kernel and the rate kernel with its map whether
 * or not jxg_set_sweep_report / jxg_set_sweep_rates are on; those switches
 * alone decide whether their reports are returned.  A baseline's block errors,
 * shares and strategy bytes are kept in a snapshot for the call, 9 bytes a
 * block per distinct baseline (4.7 MB at 7680 x 4320).  Codestreams, q[],
 * MS-SSIM results, strategy and rate reports are unchanged, ms_metrics
 * includes the added kernels, and with the switch off a sweep launches and
 * allocates what it did before.
 * jxg_sweep_ab copies the last sweep's reports out in point order, each
 * bit-equal to jxg_ab_report_rgb8_device on two one-at-a-time contexts created
 * with those two points (zero-filled: base[i] = -1, a refused point, a refused
 * baseline); JXG_ERR_INVALID_ARG when the last sweep computed none, when n is
 * not that sweep's, or while streamed frames are pending. */
jxg_status jxg_set_sweep_ab(jxg_ctx* ctx, const int32_t* base, uint32_t n);
jxg_status jxg_sweep_ab(jxg_ctx* ctx, jxg_ab_report* out, uint32_t n);
/* Search-trace summaries in a sweep.  With the switch on
 * (default 0; JXG_ERR_INVALID_ARG for a null ctx and while streamed frames are
 * pending) every sweep -- quality 0 included, nothing here needs decoded pixels
 * -- runs each accepted point whose effort is >= 5 as a traced job on its lane
 * and reduces its jxg_trace_summary there.  A point of effort < 5 has no
 * search: it is encoded exactly as with the switch off and its summary is
 * zero-filled (blocks == 0 marks it), which is no error at point or call
 * level; a refused point's summary is zero-filled too.  The planes
 * (jxg_trace_maps) are not kept.  Codestreams are byte-identical to the same
 * sweep with the switch off, and so to jxg_encode_rgb8 on a context created
 * with the point; q[], MS-SSIM results, strategy, rate and A/B reports are
 * unchanged, and with the switch off a sweep launches and allocates what it
 * did before.  The trace planes, 115 bytes a block (59.6 MB at 7680 x 4320),
 * are allocated per lane by the first traced sweep that reaches the slot and
 * released with the lane.
 * jxg_sweep_trace copies the last sweep's summaries out in point order, each
 * bit-equal to the summary jxg_search_trace gives after jxg_encode_traced_rgb8
 * of the image on a context created with that point; JXG_ERR_INVALID_ARG,
 * nothing written, for a null ctx or out, when the last sweep computed none
 * (the switch was off), when n is not that sweep's, or while streamed frames
 * are pending.  jxg_search_trace after a sweep stays JXG_ERR_INVALID_ARG, as
 * after any sweep. */
jxg_status jxg_set_sweep_trace(jxg_ctx* ctx, int on);
jxg_status jxg_sweep_trace(jxg_ctx* ctx, jxg_trace_summary* out, uint32_t n);

/* Prepares the context for frames of xsize x ysize before the first one
 * arrives: encodes one synthetic frame of that size (device-generated, result
 * discarded), which allocates the size's device buffers and loads every
 * kernel.  Optional -- a caller that creates a context per image (the
 * harness's execute_cjxl pattern, docker_manager.rs:126-136) runs it beside
 * its image decode; jxg_cjxl does.  Not while streamed frames are pending. */
jxg_status jxg_warmup(jxg_ctx* ctx, uint32_t xsize, uint32_t ysize);
/* ---- benchmark input ----
 * The deterministic synthetic RGB8 frame of SURVEY.md §8(d) (64x64 tiles of
 * flat / gradient / stripe / checker / edge / noise content, splitmix64
 * hashes, seed 0x4A584C00 + config index), written into device memory
 * d_out (row_stride bytes per row) on the context's stream; returns when it
 * is complete.  Same bytes as jxg/synth.py synth_rgb8. */
jxg_status jxg_synth_rgb8_device(jxg_ctx* ctx, void* d_out, uint32_t xsize, uint32_t ysize,
                                 size_t row_stride, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif
