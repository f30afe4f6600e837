// jxg_ctx.h -- what the host translation units share: the encoder context
// (Ctx), the state of one encode (Job), device / pinned buffers, and the
// functions that cross files.  Internal: nothing here is exported; the C ABI
// (include/jxg.h) is jxg_abi.cpp.
//
// One encode = one stream-ordered pipeline on the context's HIP stream:
//   front (RGB8 -> ACS/QF/DC/AC)            [jxg_front.hip]
//   ac_hist + lf_hist (token statistics)     [jxg_ac_hist.hip, jxg_entropy.hip]
//   -> D2H histograms; host builds prefix codes, LfGlobal/HfGlobal and the
//      LF-group stream preludes (a few KB of header bits)
//   ac_emit or the rANS chain + ans_emit, lf_code (bit emission into scratch)
//                                 [jxg_ac_emit.hip, jxg_ans.hip, jxg_entropy.hip]
//   -> D2H section sizes; host writes headers + TOC and the piece list
//   concat (bit-exact assembly) -> D2H codestream
// The byte stream equals the CPU oracle's (oracle/encode.c) bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/jxg.h"
#include "jxg_bitstream.h"
#include "jxg_codes.h"
#include "jxg_device.h"
#include "jxg_kernels.h"
#include "jxg_layout.h"
#include "jxg_plan.h"

#pragma GCC visibility push(hidden)
namespace jxg {

#define JXG_HIP(expr)                                                          \
  do {                                                                         \
    hipError_t e_ = (expr);                                                    \
    if (e_ != hipSuccess) {                                                    \
      std::fprintf(stderr, "jxg: %s failed: %s\n", #expr, hipGetErrorString(e_)); \
      return JXG_ERR_HIP;                                                      \
    }                                                                          \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  bool n_grow = false;  // allocated before
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    // a regrowth gets 1/8 headroom: per-frame sizes (bit scratch, output)
    // vary a little between frames, and a reallocation in a streamed frame
    // costs ~0.1 ms of host time (hipFree + hipMalloc)
    size_t want = n_grow ? std::max<size_t>(count + count / 8, 1) : std::max<size_t>(count, 1);
    n_grow = true;
    hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
    if (e == hipSuccess) n = want;
    return e;
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

template <class T>
struct PinBuf {
  T* p = nullptr;
  size_t n = 0;
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
    size_t want = std::max<size_t>(count, 1);
    hipError_t e = hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) n = want;
    return e;
  }
  ~PinBuf() {
    if (p) (void)hipHostFree(p);
  }
};

using Clock = std::chrono::steady_clock;
inline float ms_since(Clock::time_point t0) {
  return std::chrono::duration<float, std::milli>(Clock::now() - t0).count();
}

// the encoder's events of one frame (Ctx::ev), in the order they are recorded
enum EncEvent : int {
  kEvStart = 0,       // frame start
  kEvFrontStart = 9,  // masking quant field done / front kernel start
  kEvFrontDone = 5,   // front kernel done
  kEvMerged = 1,      // transform and merge done
  kEvAcStats = 6,     // AC statistics on the host (stage_download_ac)
  kEvLfStats = 2,     // LF statistics downloaded (stage_download_lf)
  kEvAcEmitted = 7,   // AC emission done and its bit counts on the host
  kEvEmitted = 3,     // emission done
  kEvAcBlock = 8,     // AC block in host memory (stage_concat_split)
  kEvAssembled = 4,   // codestream assembled
  kNumEncEvents = 10
};

// (include/jxg.h: the report shares its name with the call that fills it)
using RateReport = struct ::jxg_rate_report;
// a sweep's riders: the optional per-point results of jxg_sweep_rgb8, each with
// a switch (jxg_set_sweep_*), a getter (jxg_sweep_*) and a slot in Ctx::Sweep
enum Rider { kRiderMsssim, kRiderReport, kRiderRates, kRiderAb, kRiderTrace, kRiders };
// what differs between them besides their enqueue functions (kRiderRules,
// jxg_sweep.cpp): a rider rides on sweeps of quality >= min_quality; a point
// stages `words` pinned 8-byte words, which rider_convert turns into its public
// struct of out_bytes
struct RiderRule {
  int min_quality;
  size_t words, out_bytes;
};
extern const RiderRule kRiderRules[kRiders];
struct Ctx;
struct Job;
struct Pipe;
// batch lanes (jxg_encode_batch_rgb8[_device]): extra contexts of the same
// parameters, each with its own stream and pinned staging, owned by the
// context that ran the batch
struct CtxDeleter {
  void operator()(Ctx* c) const;
};
struct PipeDeleter {  // (Pipe is private to jxg_pipe.cpp)
  void operator()(Pipe* p) const;
};
struct Ctx : EncArenas {
  jxg_params params{};
  std::vector<std::unique_ptr<Ctx, CtxDeleter>> lanes;
  PinBuf<uint8_t> h_stage;  // pinned staging of one host frame (pipeline lanes)
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // AC-block concat + D2H (stage_concat_split)
  hipEvent_t ev[kNumEncEvents] = {};  // by EncEvent
  bool constants_ready = false;
  // device
  DevBuf<uint8_t> rgb, acs, qf, aqf;  // aqf: masking quant field (JXG_FLAG_AQ_MASKING)
  DevBuf<uint8_t> force_acs, force_qf;  // a forced encode's uploaded maps
  DevBuf<float> lut;                   // sRGB8 -> linear (the AQ kernel)
  DevBuf<int8_t> cmap;  // [2][tiles] chroma from luma (front kernel)
  DevBuf<uint16_t> nz, mnat;
  DevBuf<float> ent, mwk, msdk, miwy, xyb_tiles, mcost;
  // merge levels 128 / 256 px (effort >= 8): tables (uploaded once), scratch
  // planes of the persistent workgroups, candidate estimates, chosen list
  DevBuf<float> big_tab, big_scratch, big_cost;
  DevBuf<uint16_t> big_nat;
  DevBuf<uint32_t> big_work;
  bool big_ready = false;
  DevBuf<uint32_t> vb, mwork, xlist;
  DevBuf<uint8_t> lf_mine;  // shard: [nlf] owned LF groups (vb_list)
  DevBuf<int32_t> dc;
  DevBuf<int16_t> ac;
  DevBuf<float> homog, xyb, r3;
  DevBuf<uint8_t> type;
  DevBuf<uint32_t> stream_chunks, scratch, scratch_lf, out;
  DevBuf<uint64_t> lfstatus;  // [nchunks] lf_code look-back words
  // the per-frame statistics, code-table and bit-count arenas (EncArenas:
  // the sections and partial-copy boundaries) and their pinned mirrors
  DevBuf<uint8_t> stat, up, bits;
  PinBuf<uint8_t> h_stat, h_up, h_bits;
  uint32_t* lf_scratch = nullptr;  // LF-stream bit arena (scratch_lf, or in scratch)
  DevBuf<uint32_t> tile_list, glist;  // shard: tile ids, pass groups (non-contiguous plans)
  DevBuf<uint32_t> tokens, tval, ans_state, csum;  // ANS coder
  DevBuf<uint8_t> tlen;
  DevBuf<LfRow> rows;
  DevBuf<LfChunk> lfchunks;
  // decode-side quality (jxg_compare_rgb8; jxg_quality.cpp)
  struct Quality {
    DevBuf<uint8_t> orig, comp;
    DevBuf<uint64_t> sse;
    DevBuf<double> part, ssim;
    bool gauss_ready = false;
    // MS-SSIM (jxg_msssim_rgb8, a sweep's lane): the pyramids of the two
    // images (a sweep's lane fills only pyr_c), per-workgroup partials, the
    // ten window sums; allocated by the first use
    DevBuf<float> pyr_o, pyr_c;
    DevBuf<double> ms_part, ms_out;
    // strategy report (jxg_strategy_report_rgb8, a sweep's lane): the block
    // error map of the chain's last kernel and the 27 x 8 table
    DevBuf<uint32_t> bsse;
    DevBuf<uint64_t> rep;
  } q;
  // decode-side reconstruction (jxg_reconstruct_rgb8; jxg_reconstruct.cpp),
  // allocated by its first call: tables, two sets of three block-padded f32
  // planes, the list of 128 / 256 px varblocks, the host variant's device image
  struct Recon {
    DevBuf<float> tab, pa, pb;
    DevBuf<uint16_t> pos;
    DevBuf<uint32_t> big;
    DevBuf<uint8_t> rgb;
    uint32_t tab_g = 0;  // global scale the EPF sigma table was built for
    // a sweep's chains: pinned staging of the sigma table alone and the event
    // of its last copy
    PinBuf<float> h_sigma;
    hipEvent_t ev_sigma = nullptr;
    // the last encode was jxg_encode_rgb8[_device] of a w x h frame, whose
    // coefficients and maps are still in this context's buffers
    bool ok = false;
    uint32_t w = 0, h = 0;
    // ... and may hold varblocks of 128 / 256 px (Job::big: an effort >= 8
    // search, or a forced map with a big kind on a context of any effort)
    bool has_big = false;
  } rc;
  // rate report (jxg_rate_report, a sweep's lane; jxg_rate.cpp): the symbol
  // cost table (uploaded once), the 27 x 6 table, the device map of the host
  // variant and of an A/B report -- allocated by the first use -- and what the last finished encode of
  // a whole frame left for it (rate_note): its coder, histograms, group count
  // and kernel geometry, the emitted AC bits, the codestream's bits.  The
  // records, code tables and strategy map are the context's own buffers
  // (tokens, codes_ac / ans_tab, bandtok, acs, ac, nz), valid as long as rc.ok
  struct Rate {
    DevBuf<uint16_t> ftab;
    bool ftab_ready = false;
    DevBuf<uint64_t> table;
    DevBuf<uint32_t> map;
    bool have = false, ans = false, whole_group = false;
    uint32_t nhist = 0, groups = 0;
    uint64_t ac_bits = 0, stream_bits = 0;
  } rt;
  // A/B report (jxg_ab_report_rgb8, a sweep's lane; jxg_ab.cpp), allocated by
  // the first use: this side's cost shares, the 27 x 27 x 6 table and the host
  // variant's delta planes (side B's context), the event side A's prepare step
  // ends with
  struct Ab {
    DevBuf<uint32_t> share;
    DevBuf<uint64_t> table;
    DevBuf<int32_t> delta;
    hipEvent_t ev = nullptr;
  } ab;
  // search trace (jxg_encode_traced_rgb8 / jxg_search_trace; jxg_trace.cpp),
  // allocated by the first traced encode: the f32 planes [cand8_raw 6 | cand8 6
  // | merged 9 | big 6 | chosen 1][nb], the u8 planes [scan8 | front8 | qf8][nb]
  // and the summary words.  have: the last one-at-a-time encode was a traced
  // one of a w x h frame (valid as long as rc.ok).  A sweep's lane with
  // jxg_set_sweep_trace uses the same buffers, 115 bytes a block, allocated by
  // the first traced point that lands on the slot and released with it
  struct Trace {
    DevBuf<float> f;
    DevBuf<uint8_t> b;
    DevBuf<uint32_t> sum;
    bool have = false;
    uint32_t w = 0, h = 0;
  } tr;
  // decoder (jxg_decode_rgb8; jxg_decode_dev.cpp), allocated by its first
  // call: the codestream's words, the pass groups' section bounds, the AC
  // stream's decode tables [ctxmap | histograms | prefix or alias tables], the
  // per-group status
  struct Dec {
    DevBuf<uint64_t> stream, sec;
    DevBuf<uint8_t> tab;
    DevBuf<uint32_t> status;
    hipEvent_t ev[3] = {};  // pass-group kernel start / end, reconstruction end
    // last decode: host parse + tables, LF groups, pass-group kernel,
    // reconstruction chain (device), the whole call (host wall); milliseconds
    float ms[5] = {};
  } dec;
  // batch decoder (jxg_decode_batch_rgb8; jxg_decode_batch.cpp), allocated by
  // its first call: one arena for the maps, coefficients, streams and tables
  // of a chunk's frames (jxg_decode_plan.h), the frame descriptors and work
  // lists of the two launches, the per-group status of the chunk
  struct DecBatch {
    DevBuf<uint8_t> arena, desc;
    DevBuf<uint32_t> status;
    hipEvent_t ev[4] = {};  // pass-group launches start / end, reconstruction chains start / end
    size_t budget = 0;      // jxg_set_decode_batch_bytes (0: kDecBatchDefaultBytes)
    jxg_decode_batch_stats stats{};
  } decb;
  // sweep (jxg_sweep_rgb8; jxg_sweep.cpp): the host variant's device image,
  // the points' pinned results [n][2] and events [n][3], the last call's stats,
  // and one slot per rider (the optional per-point results; kRiderRules).
  // MS-SSIM's extras: the original's pyramid, built once per sweep on this
  // context's stream and read by every lane after ev_pyr.  A/B's extras: the
  // base index of every point (empty: off), one snapshot slot [kAbSnapBytes per
  // block] and one event per distinct baseline of the call
  struct Sweep {
    DevBuf<uint8_t> rgb;
    PinBuf<uint64_t> h_q;
    std::vector<hipEvent_t> ev;
    jxg_sweep_stats stats{};
    struct RiderSlot {
      bool on = false;           // the switch (jxg_set_sweep_*)
      PinBuf<uint64_t> h;        // the valid points' pinned words [nv][rule.words]
      std::vector<uint8_t> out;  // the last sweep's public structs [n], in point order
      bool have = false;         // the last sweep computed `out`
    } rider[kRiders];
    DevBuf<float> pyr_o;
    hipEvent_t ev_pyr = nullptr;
    std::vector<int32_t> ab_base;
    std::vector<std::unique_ptr<DevBuf<uint8_t>>> ab_snap;
    std::vector<hipEvent_t> ab_ev;
  } sw;
  // the concat kernel's inputs (stage_concat / stage_concat_split, the shard
  // assemblers)
  struct Concat {
    DevBuf<ConcatPiece> pieces, pieces_ac;
    DevBuf<uint8_t> buf;  // stage_concat: [pieces | chunk words], one upload
    PinBuf<uint8_t> h_buf;
    PinBuf<ConcatPiece> h_pieces_ac;
    DevBuf<uint32_t> chunks, out_ac;
  } cat;
  // host

  // LF row segments cached per frame size and shard
  uint32_t rows_w = 0, rows_h = 0, rows_rank = 0, rows_world = 1;
  std::vector<LfRow> rows_h_cache;
  std::vector<LfChunk> chunks_h_cache;
  std::vector<uint32_t> schunks_cache;
  CtxMapCache ctxmap_cache;  // serialised AC context map of the previous frame
  std::vector<uint8_t> m_acs, m_qf;
  std::vector<int32_t> m_dc, m_ac;
  std::vector<uint32_t> m_ntok;
  std::vector<float> m_homog;
  jxg_stats stats{};
  // ordering of device inputs (jxg_set_input_stream): the caller's stream
  // whose work so far every device-input entry point orders itself after
  hipStream_t in_stream = nullptr;
  hipEvent_t ev_in = nullptr;
  hipEvent_t ev_write = nullptr;  // jxg_shard_write_next: this slot's section copies
  uint32_t lane_cap = 0;          // jxg_set_pipeline_lanes (0: the queues' limit)
  bool owned_lane = false;  // a pipeline / batch lane of another context
  // a pipeline lane's extra slots: contexts with their own buffers that share
  // this context's stream (super-frames: k frames per batched launch)
  std::vector<std::unique_ptr<Ctx, CtxDeleter>> slots;
  bool shared_stream = false;  // `stream` belongs to the lane that owns this slot
  std::unique_ptr<Job> job;                 // sharded encode in flight (begin -> end)
  std::unique_ptr<Pipe, PipeDeleter> pipe;  // streaming encode (jxg_submit_* / jxg_receive)
  std::vector<uint32_t> payload_head;  // last jxg_shard_end: payload head words
  size_t payload_body = 0;             //   and body bytes (in `out`)
};

// state carried between the stages of one encode
struct Job {
  Frame f;
  Plan plan;
  uint32_t w = 0, h = 0;
  size_t stride = 0;
  const uint8_t* d_rgb = nullptr;
  int max_s = 0;
  bool homog = false;
  // forced encode (jxg_encode_forced_rgb8): the caller's validated strategy
  // map on the device, and its quant field or null (the context's own); the
  // job runs as effort 7 without proposals, never in a batch
  const uint8_t* d_force = nullptr;
  const uint8_t* d_force_qf = nullptr;
  // ... and whether the map holds a kind of 128 / 256 px (the validator's mask):
  // the job then runs force_big_list + big_write behind the 64 px write pass
  bool force_big = false;
  // traced encode (jxg_encode_traced_rgb8): a search job whose front kernel,
  // merge stage and 128 / 256 px levels keep every estimate (c->tr); never in
  // a batch
  bool trace = false;
  bool ans = false;  // ANS instead of prefix codes for the AC stream
  uint32_t lf = 0;   // frame header loop-filter code (lf_code: Gaborish / EPF)
  uint32_t nhist_ans = 0, max_tokens = 0;
  uint32_t nrows = 0, nchunks = 0, nstreams = 0;
  AcArgs aa{};
  LfArgs la{};
  // argument blocks of the front / merge / LF-list stages and the rANS coder
  // (build_front, build_emit): the batched launches gather them per frame
  FrontArgs fa{};
  AqArgs qa{};
  MergeArgs ma{};
  BigArgs ba{};
  bool big = false;  // varblocks of 128 / 256 px: the search's levels (effort >= 8) or a forced map's
  VbArgs va{};
  AnsArgs na{};
  bool aq = false;  // masking quant field (aq_kernel before the front kernel)
  // host stage results
  std::vector<BitWriter> preA, preB;
  BitWriter lfglobal, hfglobal;
  // sharded ANS encode with one HF preset per rank: no histogram
  // all-reduce; the rank's clustered histograms travel in its payload head and
  // HfGlobal is written at assembly (build_hf_presets)
  bool presets = false;
  std::vector<uint8_t> pre_ctxmap;   // [kAcCtx] context -> the rank's dense histogram
  std::vector<uint32_t> pre_counts;  // [nhist][kAlpha] clustered counts
  std::vector<uint64_t> gbase, sbase;
  float ms_codes = 0.0f;
  float ms_layout = 0.0f;  // stage_concat_split host layout
  // enc_finish_start -> enc_finish_end: the codestream (pinned pool block,
  // D2H in flight), its size, the host layout time
  uint8_t* host_out = nullptr;
  size_t out_bytes = 0;
  float ms_finish_layout = 0.0f;
};

// ---- jxg_ctx.cpp: context lifetime, constants, the pinned output pool ----
constexpr size_t kOutHdr = 64;  // bytes in front of every output block
uint8_t* out_alloc(size_t bytes);
uint8_t* out_alloc_heap(size_t bytes);  // host-only outputs (no device needed)
void out_set_backref(uint8_t* data, uint8_t* data0);
void out_release(uint8_t* data);
extern std::mutex g_const_mu;  // device __constant__ tables are shared by all contexts
bool lone_context();           // at most one caller-created context is alive
jxg_status ctx_create(const jxg_params& params, Ctx** out);
jxg_status ctx_new_lane(const jxg_params& params, Ctx** out);
void ctx_destroy(Ctx* c);
jxg_status init_constants(Ctx* c);
hipError_t make_event(hipEvent_t* e, unsigned flags);
float elapsed(hipEvent_t a, hipEvent_t b);
uint32_t hw_queues();
jxg_status order_input(Ctx* owner, Ctx* lane);

// ---- jxg_encode.cpp: stages A-H and the phases of one frame ----
uint32_t big_mask(const uint32_t* count);
jxg_status stage_alloc(Ctx* c, Job& J);
jxg_status build_front(Ctx* c, Job& J);
jxg_status stage_download_ac(Ctx* c, Job& J, const uint32_t* hist);
jxg_status launch_transform(Ctx* const* cs, Job* const* js, uint32_t k);
jxg_status launch_lf_stats(Ctx* const* cs, Job* const* js, uint32_t k);
jxg_status launch_stats(Ctx* const* cs, Job* const* js, uint32_t k);
jxg_status stage_codes(Ctx* c, Job& J);
jxg_status launch_emit(Ctx* const* cs, Job* const* js, uint32_t k, bool streamed);
jxg_status stage_emit(Ctx* c, Job& J, bool sync = true);
jxg_status wait_emission(Ctx* c, Job& J);
jxg_status stage_concat(Ctx* c, Job& J, bool full, std::vector<uint32_t>* section_ids,
                        std::vector<uint32_t>* section_bytes, uint8_t** host_out,
                        size_t* out_bytes);
jxg_status enc_prepare(Ctx* c, Job& J, const uint8_t* d_rgb, uint32_t w, uint32_t h,
                       size_t stride, uint32_t rank, uint32_t world);
jxg_status enc_finish_start(Ctx* c, Job& J, bool split);
void enc_stats(Ctx* c, Job& J, size_t out_bytes, float ms_layout, bool assembled,
               const std::vector<int16_t>* m_ac16, Clock::time_point t_call);
jxg_status enc_finish(Ctx* c, Job& J, bool split, jxg_buffer* out, Clock::time_point t_call);
// one frame through the one-at-a-time path, with the bookkeeping of what
// jxg_reconstruct_rgb8 may read afterwards (src: host memory, or device memory
// ordered after the caller's input stream)
// force_acs: a forced encode -- the caller's strategy map (host memory,
// validated by check_strategy_map) and its quant field or null; force_big: the
// validator's mask of the big kinds the map holds
jxg_status encode_one(Ctx* c, const uint8_t* src, bool on_device, uint32_t w, uint32_t h,
                      size_t stride, jxg_buffer* out, Clock::time_point t_call,
                      const uint8_t* force_acs = nullptr, const uint8_t* force_qf = nullptr,
                      bool trace = false, uint32_t force_big = 0);
// jxg_force.cpp (host only): jxg_check_strategy_map, and in *big_kinds (may be
// null) bit k for every big kind k (big_list_kernel's numbering) an accepted map holds
jxg_status check_strategy_map(const uint8_t* acs, uint32_t xsize, uint32_t ysize,
                              uint32_t* bad_block, uint32_t* big_kinds);
jxg_status warmup(Ctx* c, uint32_t w, uint32_t h);

// ---- jxg_pipe.cpp: the streaming pipeline ----
bool pipe_busy(const Ctx* c);
uint32_t pipe_pending(const Ctx* c);
void pipe_abort(Ctx* c);
void pipe_drop_done(Ctx* c);
// a sweep's frame (jxg_sweep.cpp): the point its lane encodes with and, with
// quality != 0, where its reconstruction chain and metrics leave their results
struct SweepReq {
  jxg_params params;
  int quality = 0;         // 0 none, 1 sse, 2 also ssim
  uint64_t* h_q = nullptr;  // pinned [2]: sse, the SSIM sum's bits
  hipEvent_t* ev = nullptr;  // [3]: chain start, chain end, metrics end
  // the riders' pinned slices, null where a rider does not run on this point:
  // [10] window sums behind the SSIM kernels, the [kReportCells] table behind
  // the metrics, [kRateWords] behind the emission, the [kAbWords] table of a
  // comparing point
  uint64_t* h[kRiders] = {};
  // MS-SSIM: the original's pyramid and the event it is complete after
  const float* pyr_o = nullptr;
  hipEvent_t ev_pyr = nullptr;
  // A/B report (jxg_ab.cpp).  ab: the point is a baseline or compares -- its
  // chain writes the block error map and its rate kernel the cost map, whatever
  // the report and rate switches say.  A baseline copies its triple to ab_snap
  // and records ab_ev_snap; a comparing point waits for ab_ev_base and reduces
  // ab_base against its own triple
  bool ab = false;
  uint8_t* ab_snap = nullptr;
  hipEvent_t ab_ev_snap = nullptr;
  const uint8_t* ab_base = nullptr;
  hipEvent_t ab_ev_base = nullptr;
};
jxg_status pipe_submit(Ctx* c, const uint8_t* src, bool on_device, uint32_t w, uint32_t h,
                       size_t stride, uint32_t rank = 0, uint32_t world = 1, bool shard = false,
                       const SweepReq* rq = nullptr);
jxg_status pipe_receive(Ctx* c, jxg_buffer* out);
// a completed frame is worth taking now: its codestream's copy has landed, or
// more than two are waiting
bool pipe_done_ready(Ctx* c);
jxg_status pipe_depth(const Ctx* c, uint32_t w, uint32_t h, uint32_t rank, uint32_t world,
                      uint32_t* depth);
jxg_status batch_encode(Ctx* c, const uint8_t* const* frames, bool on_device, uint32_t n,
                        uint32_t w, uint32_t h, size_t stride, jxg_buffer* outs);
jxg_status shard_next_head(Ctx* c, uint32_t* dst, size_t* nwords);
jxg_status shard_write_next(Ctx* c, const uint32_t* const* heads, const size_t* head_words,
                            uint32_t n, uint8_t* dst, size_t dst_size, size_t* total);
jxg_status shard_write_flush(Ctx* c);

// ---- jxg_sweep.cpp: one image over many settings ----
jxg_status sweep_quality_enqueue(Ctx* lane, const SweepReq& rq, const uint8_t* d_orig, size_t so,
                                 uint32_t w, uint32_t h);
jxg_status sweep(Ctx* c, const uint8_t* src, bool on_device, uint32_t w, uint32_t h, size_t stride,
                 const jxg_sweep_point* points, uint32_t n, int quality, jxg_buffer* outs,
                 jxg_quality* q, jxg_status* statuses);

// ---- jxg_shard_host.cpp: sharded encode and the shard assemblers ----
jxg_status shard_begin(Ctx* c, const uint8_t* d_rgb, uint32_t w, uint32_t h, size_t stride,
                       uint32_t rank, uint32_t world, uint32_t* d_hist, uint8_t* d_xbuf);
jxg_status shard_end(Ctx* c, const uint32_t* d_hist, const uint8_t* d_xbuf, size_t* payload_bytes);
jxg_status shard_finish(Ctx* c, Job& J, size_t* payload_bytes, bool sync = true);
jxg_status shard_payload(Ctx* c, void* dst, bool on_device);
jxg_status shard_head(const Ctx* c, uint32_t* dst, size_t* nwords);
jxg_status shard_assemble_device(Ctx* c, const uint8_t* d_base, const size_t* offsets,
                                 const size_t* psizes, uint32_t n, jxg_buffer* out);
jxg_status shard_write_host(Ctx* c, const uint32_t* const* heads_in, const size_t* words,
                            uint32_t n, uint8_t* dst, size_t dst_size, size_t* total,
                            bool sync = true);
jxg_status shard_assemble(const uint8_t* const* payloads, const size_t* sizes, uint32_t n,
                          jxg_buffer* out);

// ---- jxg_quality.cpp: quality metrics, homogeneity map, synthetic image ----
jxg_status homogeneity_map(Ctx* c, const float* xyb, uint32_t xsize, uint32_t ysize,
                           float distance, uint32_t flags, float* r3, uint8_t* type);
jxg_status synth_device(Ctx* c, uint8_t* d_out, uint32_t w, uint32_t h, size_t stride,
                        uint64_t seed);
jxg_status quality_gauss(Ctx* c);  // the SSIM window's constants, once per context
jxg_status compare_device(Ctx* c, const uint8_t* d_orig, size_t so, const uint8_t* d_comp,
                          size_t sc, uint32_t w, uint32_t h, int want_ssim, jxg_quality* out);
jxg_status compare_host(Ctx* c, const uint8_t* orig, size_t so, const uint8_t* comp, size_t sc,
                        uint32_t w, uint32_t h, int want_ssim, jxg_quality* out);
// MS-SSIM: every field NaN (nothing launched) under kMsMinEdge
jxg_status msssim_device(Ctx* c, const uint8_t* d_orig, size_t so, const uint8_t* d_comp,
                         size_t sc, uint32_t w, uint32_t h, jxg_msssim* out);
jxg_status msssim_host(Ctx* c, const uint8_t* orig, size_t so, const uint8_t* comp, size_t sc,
                       uint32_t w, uint32_t h, jxg_msssim* out);
// the result from the ten window sums (ssim[0 .. 4], cs[0 .. 4]) of a w x h pair
void msssim_result(uint32_t w, uint32_t h, const double* sums, jxg_msssim* out);
void msssim_nan(jxg_msssim* out);

// ---- jxg_reconstruct.cpp ----
// the frame constants of a reconstruction: the encoder fills them from its
// parameters, the decoder from the parsed headers
struct ReconFrame {
  uint32_t w, h;
  uint32_t global_scale, quant_dc;
  uint32_t lf;        // loop-filter code (lf_code: bit 0 Gaborish, bits 1-2 EPF iterations)
  float xmul, bmul;   // x_qm / b_qm multipliers
  bool maybe_big;     // varblocks of 128 / 256 px are possible
};
jxg_status reconstruct_device(Ctx* c, const ReconFrame& R, uint8_t* d_rgb, size_t stride);
// the same from maps and coefficients that are not the context's own buffers
// (the batch decoder's arena slices; layouts of ReconArgs)
struct ReconMaps {
  const uint8_t *acs, *qf;
  const int32_t* dc;
  const int16_t* ac;
  const int8_t* cmap;
};
// q: a sweep's chain on a lane (jxg_sweep.cpp) -- every pass writes planes and
// the fused colour + squared-error kernel ends it (RGB8 stored to d_rgb only
// with q->store); everything is enqueued on c's stream, nothing waited for
struct ReconSse {
  const uint8_t* orig;  // the original, RGB8 rows of orig_stride bytes
  size_t orig_stride;
  uint64_t* sse;        // device, zeroed on the stream before
  bool store;
  uint32_t* block_sse = nullptr;  // device [bys][bxs] squared error per 8x8 block, or null
};
jxg_status reconstruct_device(Ctx* c, const ReconFrame& R, const ReconMaps& M, uint8_t* d_rgb,
                              size_t stride, const ReconSse* q = nullptr);
// the frame constants of a w x h frame encoded with parameters P (a sweep's
// point: big varblocks are possible from effort 8 on)
ReconFrame recon_frame_of_encode(uint32_t w, uint32_t h, const jxg_params& P);
// ... of the last one-at-a-time encode of c (rc.w x rc.h; rc.has_big, not the
// effort, says whether it may hold big varblocks: a forced map may)
ReconFrame recon_frame_of_last(const Ctx* c);
// the last one-at-a-time encode's decoded image, into device / host memory
jxg_status reconstruct_last(Ctx* c, uint8_t* rgb, size_t row_stride, bool on_device);

// the strategy report of the last one-at-a-time encode: the
// chain above with the block-map ending into scratch, then the reduction of
// jxg_report.hip; block_sse (host or device as orig, may be null): the map
jxg_status strategy_report_last(Ctx* c, const uint8_t* orig, size_t orig_stride, bool on_device,
                                jxg_strategy_report* out, uint32_t* block_sse);
// the reduction alone, enqueued on c's stream: c->q.bsse -> c->q.rep (cleared first)
jxg_status strategy_report_enqueue(Ctx* c, uint32_t w, uint32_t h);
// the report's front half, enqueued on c's stream: the original to the device
// (host variant: c->q.orig) and the chain ending in the block-map kernel ->
// c->q.bsse, c->q.sse (JXG_ERR_INVALID_ARG as the report gives it)
jxg_status block_sse_enqueue(Ctx* c, const uint8_t* orig, size_t orig_stride, bool on_device);

// ---- jxg_rate.cpp: coded bits per block and strategy ----
// a pinned result of a sweep's point: the table, then ac_bits, stream_bits,
// ans, groups
constexpr size_t kRateWords = kRateCells + 4;
// the encode of J on c has its emission's bit counts on the host and its
// codestream's size known: keep what the report needs (the Job goes away)
void rate_note(Ctx* c, const Job& J);
// the kernel alone, enqueued on c's stream: c->rt.table (cleared first) and,
// when d_block_cost is not null, the map of the w x h frame c encoded last
jxg_status rate_enqueue(Ctx* c, uint32_t w, uint32_t h, uint32_t* d_block_cost);
// a sweep's point on its lane: the kernel, the table's copy to rq.h[kRiderRates] and
// the scalars beside it
jxg_status sweep_rate_enqueue(Ctx* lane, const SweepReq& rq, uint32_t w, uint32_t h);
// the device map of the host variant and of an A/B report's prepare step
jxg_status rate_map_ensure(Ctx* c, uint32_t w, uint32_t h);
void rate_from_words(const uint64_t* words, RateReport* out);
// the report of the last one-at-a-time encode; block_cost host or device memory, or null
jxg_status rate_report_last(Ctx* c, RateReport* out, uint32_t* block_cost, bool on_device);

// ---- jxg_ab.cpp: A/B report of two encodes ----
// a baseline's snapshot: per block the error word, the share, the strategy
// byte -- [nb] u32 | [nb] u32 | [nb] u8
constexpr size_t kAbSnapBytes = 9;
// the cost-share pass on c's stream: c->rt.map (rate_enqueue with a map) and
// c->acs -> c->ab.share
jxg_status ab_share_enqueue(Ctx* c, uint32_t w, uint32_t h);
// a sweep's point on its lane, behind its chain (block map) and its rate
// kernel (cost map): the share pass, then the snapshot and / or the comparison
jxg_status sweep_ab_enqueue(Ctx* lane, const SweepReq& rq, uint32_t w, uint32_t h);
jxg_status ab_report_pair(Ctx* a, Ctx* b, const uint8_t* orig, size_t orig_stride, bool on_device,
                          jxg_ab_report* out, int32_t* block_delta);

// ---- jxg_trace.cpp: search trace of a traced encode ----
constexpr size_t kTracePlanes = 28, kTraceRaw = 0, kTraceCmp = 6, kTraceMerged = 12,
                 kTraceBig = 21, kTraceChosen = 27;  // f32 planes of Ctx::Trace::f
// the buffers of a w x h frame (before the job's argument blocks are built)
jxg_status trace_alloc(Ctx* c, uint32_t w, uint32_t h);
// the front kernel's trace pointers
void trace_front_args(Ctx* c, FrontArgs& fa);
// on the job's stream: the front kernel's quant field, between it and the merge stage
jxg_status trace_copy_qf(Ctx* c, const Job& J);
// on the job's stream behind the merge stage: the planes and the summary
jxg_status trace_enqueue(Ctx* c, const Job& J);
// a pinned result of a sweep's point: the summary's u32 words
constexpr size_t kTraceWords = kTraceSummaryWords / 2;
// a sweep's traced point on its lane, behind trace_enqueue: the summary's copy
// to rq.h[kRiderTrace]
jxg_status sweep_trace_enqueue(Ctx* lane, const SweepReq& rq);
jxg_status search_trace(Ctx* c, jxg_trace_maps* maps, jxg_trace_summary* summary);

// ---- jxg_decode_dev.cpp ----
jxg_status decode_rgb8(Ctx* c, const uint8_t* data, size_t size, uint8_t* rgb, size_t row_stride,
                       bool on_device);
jxg_status decode_maps_device(Ctx* c, const uint8_t* data, size_t size, uint8_t* acs, uint8_t* qf,
                              int32_t* dc, int32_t* ac, int8_t* cmap);
struct DecFrame;
// what the reconstruction tables cannot honour is refused (JXG_ERR_UNSUPPORTED)
jxg_status decode_recon_frame(const DecFrame& F, ReconFrame* R);

// ---- jxg_decode_batch.cpp ----
jxg_status decode_batch_rgb8(Ctx* c, const uint8_t* const* datas, const size_t* sizes, uint32_t n,
                             uint8_t* const* rgbs, const size_t* row_strides, jxg_status* statuses,
                             bool on_device);

// ---- entry-point helpers (jxg_abi.cpp) ----
// jxg_ctx -> Ctx with its device current; idle: a context whose pipeline
// holds frames is refused (they use it as a lane, and its host state)
inline jxg_status ctx_enter(jxg_ctx* ctx, bool idle, Ctx** c) {
  *c = reinterpret_cast<Ctx*>(ctx);
  if (hipSetDevice((*c)->params.device) != hipSuccess) return JXG_ERR_HIP;
  return idle && pipe_busy(*c) ? JXG_ERR_INVALID_ARG : JXG_OK;
}
template <class F>
jxg_status guarded(F f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return JXG_ERR_OOM;
  } catch (...) {
    return JXG_ERR_INTERNAL;
  }
}

}  // namespace jxg
#pragma GCC visibility pop
