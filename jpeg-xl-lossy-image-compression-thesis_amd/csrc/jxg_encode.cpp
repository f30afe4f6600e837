// jxg_encode.cpp -- the encoder's stages A-H and the phases of one frame
// (jxg_ctx.h has the pipeline's outline); the one-at-a-time entry points'
// bodies.  What a stage does on the GPU is here: buffers, launches, copies,
// events.  What the host computes for it is host-only code next door: the
// frame plan (jxg_plan.cpp), the codes and arena layouts of stage F
// (jxg_codes.cpp), the codestream layout of stage H (jxg_layout.cpp).  The
// streaming pipeline (jxg_pipe.cpp) and the sharded encode
// (jxg_shard_host.cpp) run the same stages.
#include "jxg_ctx.h"

#include <cstdlib>
#include <cstring>

#include "jxg_codes.h"
#include "jxg_tables.h"

namespace jxg {

// LF-group row segments: (lf group, stream, channel, y, x0) in stream order,
// grouped into chunks of one stream (<= kLfChunkSamples samples,
// <= kLfChunkRows segments); only the plan's LF groups get rows (the stream
// table keeps an empty range for the others)
static void build_rows(const Frame& f, const Plan& P, std::vector<LfRow>& rows,
                       std::vector<LfChunk>& chunks, std::vector<uint32_t>& schunks) {
  rows.clear();
  chunks.clear();
  schunks.clear();
  auto add = [&](uint32_t lg, uint16_t stream, uint16_t ch, uint32_t y, uint32_t width) {
    for (uint32_t x0 = 0; x0 < width; x0 += kLfSeg) {
      const uint32_t wseg = std::min(kLfSeg, width - x0);
      const uint32_t sid = lg * 2 + stream;
      if (chunks.empty() || chunks.back().sid != sid || chunks.back().nrows == kLfChunkRows ||
          chunks.back().nsamp + wseg > kLfChunkSamples)
        chunks.push_back({(uint32_t)rows.size(), 0, sid, 0});
      chunks.back().nrows++;
      chunks.back().nsamp += wseg;
      rows.push_back({lg, stream, ch, y, x0, wseg, sid});
    }
  };
  for (uint32_t lg = 0; lg < f.nlf; lg++) {
    const uint32_t bx0 = (lg % f.lfxs) * 256, by0 = (lg / f.lfxs) * 256;
    const uint32_t bw = std::min(256u, f.bxs - bx0), bh = std::min(256u, f.bys - by0);
    const bool own = P.owns_lf(lg);
    schunks.push_back((uint32_t)chunks.size());
    if (own)
      for (uint16_t ch = 0; ch < 3; ch++)
        for (uint32_t y = 0; y < bh; y++) add(lg, 0, ch, y, bw);
    schunks.push_back((uint32_t)chunks.size());
    if (own) {
      const uint32_t cw = (bw + 7) / 8, chh = (bh + 7) / 8;
      for (uint16_t ch = 0; ch < 2; ch++)
        for (uint32_t y = 0; y < chh; y++) add(lg, 1, ch, y, cw);
      for (uint32_t y = 0; y < 2; y++) add(lg, 1, 2, y, bw * bh);
      for (uint32_t y = 0; y < bh; y++) add(lg, 1, 3, y, bw);
    }
  }
  schunks.push_back((uint32_t)chunks.size());
}

// the emission of J on c is done and its bit counts are on the host
jxg_status wait_emission(Ctx* c, Job& J) {
  (void)J;
  JXG_HIP(hipStreamSynchronize(c->stream));
  return JXG_OK;
}

// ---- stage A: buffers for the frame / plan ----
jxg_status stage_alloc(Ctx* c, Job& J) {
  hipStream_t s = c->stream;
  const jxg_params& P = c->params;
  const Frame& f = J.f;
  const size_t nb = (size_t)f.bxs * f.bys;
  // a forced job computes what an effort-7 encode without proposals computes
  const int effort = J.d_force ? 7 : P.effort;
  J.homog = !J.d_force && (P.proposals & 3u) != 0;
  J.ans = (P.flags & JXG_FLAG_ANS) != 0;
  J.lf = lf_code(P.flags, P.distance);
  jxg_status st = init_constants(c);
  if (st) return st;
  JXG_HIP(c->acs.ensure(nb));
  JXG_HIP(c->qf.ensure(nb));
  JXG_HIP(c->nz.ensure(nb * 3));
  JXG_HIP(c->dc.ensure(nb * 3));
  JXG_HIP(c->ac.ensure(nb * 192));
  if (J.homog) JXG_HIP(c->homog.ensure(nb * 3));
  J.max_s = effort >= 6 ? 8 : (effort >= 5 ? 4 : 0);  // merge levels
  const uint32_t ntiles = f.tiles_x * f.tiles_y;
  JXG_HIP(c->cmap.ensure((size_t)ntiles * 2));
  if (J.max_s) {
    JXG_HIP(c->ent.ensure(nb));
    JXG_HIP(c->xyb_tiles.ensure((size_t)ntiles * 3 * 4096));
    JXG_HIP(c->mcost.ensure((size_t)ntiles * kNumShapes * 32));
    JXG_HIP(c->mwork.ensure(merge_work_words(ntiles)));
  }
  // the plan's tile, LF-group and pass-group lists: uploaded when the plan
  // changes (one key for them and the LF row cache below)
  const bool new_plan = c->rows_w != J.w || c->rows_h != J.h || c->rows_rank != J.plan.rank ||
                        c->rows_world != J.plan.world;
  if (!J.plan.tiles.empty()) {
    JXG_HIP(c->tile_list.ensure(J.plan.tiles.size()));
    if (new_plan)
      JXG_HIP(hipMemcpyAsync(c->tile_list.p, J.plan.tiles.data(), J.plan.tiles.size() * 4,
                             hipMemcpyHostToDevice, s));
  }
  if (!J.plan.lf_mine.empty()) {
    JXG_HIP(c->lf_mine.ensure(J.plan.lf_mine.size()));
    if (new_plan)
      JXG_HIP(hipMemcpyAsync(c->lf_mine.p, J.plan.lf_mine.data(), J.plan.lf_mine.size(),
                             hipMemcpyHostToDevice, s));
  }
  JXG_HIP(c->vb.ensure((size_t)f.nlf * 65536));
  J.nstreams = f.nlf * 2;
  {
    // the statistics, code-table and bit-count arenas of this frame, device
    // and pinned side from one layout
    const EncArenas::Layouts L = c->declare(f, J.plan.ng());
    JXG_HIP(c->stat.ensure(c->stat_bytes));
    JXG_HIP(c->h_stat.ensure(c->stat_bytes));
    JXG_HIP(c->up.ensure(c->up_bytes));
    JXG_HIP(c->h_up.ensure(c->up_bytes));
    JXG_HIP(c->bits.ensure(c->bits_bytes));
    JXG_HIP(c->h_bits.ensure(c->bits_bytes));
    L.stat.commit(c->stat.p, c->h_stat.p);
    L.up.commit(c->up.p, c->h_up.p);
    L.bits.commit(c->bits.p, c->h_bits.p);
  }
  if (new_plan) {
    build_rows(f, J.plan, c->rows_h_cache, c->chunks_h_cache, c->schunks_cache);
    c->rows_w = J.w;
    c->rows_h = J.h;
    c->rows_rank = J.plan.rank;
    c->rows_world = J.plan.world;
  }
  J.nrows = (uint32_t)c->rows_h_cache.size();
  J.nchunks = (uint32_t)c->chunks_h_cache.size();
  const uint32_t nstreams = J.nstreams;
  JXG_HIP(c->rows.ensure(J.nrows));
  JXG_HIP(c->lfchunks.ensure(J.nchunks));
  JXG_HIP(c->lfstatus.ensure(J.nchunks));
  JXG_HIP(c->stream_chunks.ensure(nstreams + 1));
  if (new_plan) {
    if (J.nrows)
      JXG_HIP(hipMemcpyAsync(c->rows.p, c->rows_h_cache.data(), J.nrows * sizeof(LfRow),
                             hipMemcpyHostToDevice, s));
    if (J.nchunks)
      JXG_HIP(hipMemcpyAsync(c->lfchunks.p, c->chunks_h_cache.data(), J.nchunks * sizeof(LfChunk),
                             hipMemcpyHostToDevice, s));
    JXG_HIP(hipMemcpyAsync(c->stream_chunks.p, c->schunks_cache.data(),
                           c->schunks_cache.size() * 4, hipMemcpyHostToDevice, s));
  }
  // kernel argument blocks
  AcArgs& aa = J.aa;
  aa = AcArgs{};
  aa.acs = c->acs.p;
  aa.ac = c->ac.p;
  aa.nz = c->nz.p;
  aa.bxs = f.bxs;
  aa.bys = f.bys;
  aa.gxs = f.gxs;
  aa.g0 = J.plan.g0();
  if (!J.plan.contiguous) {
    JXG_HIP(c->glist.ensure(J.plan.ng()));
    if (new_plan)
      JXG_HIP(hipMemcpyAsync(c->glist.p, J.plan.groups.data(), J.plan.ng() * 4,
                             hipMemcpyHostToDevice, s));
    aa.glist = c->glist.p;
  }
  aa.hist = c->hist_ac.d;
  aa.bound = c->bound.d;
  aa.ntok = c->ntok.d;
  aa.bandtok = c->bandtok.d;
  aa.codes = c->codes_ac.d;
  aa.base = c->gbase.d;
  aa.bits = c->gbits.d;
  JXG_HIP(c->tokens.ensure((uint64_t)std::max(1u, J.plan.ng()) * kGroupTokStride));
  aa.tokens = c->tokens.p;
  LfArgs& la = J.la;
  la = LfArgs{};
  la.rows = c->rows.p;
  la.chunks = c->lfchunks.p;
  la.dc = c->dc.p;
  la.acs = c->acs.p;
  la.qf = c->qf.p;
  la.vb = c->vb.p;
  la.vcount = c->vcount.d;
  la.bxs = f.bxs;
  la.bys = f.bys;
  la.lfxs = f.lfxs;
  la.cmap = c->cmap.p;
  la.tiles_x = f.tiles_x;
  la.ntiles_all = f.tiles_x * f.tiles_y;
  la.hist = c->lfhist.d;
  la.sbound = c->sbound.d;
  la.codes = c->lfcodes.d;
  la.status = c->lfstatus.p;
  la.stream_chunks = c->stream_chunks.p;
  la.stream_base = c->stream_base.d;
  la.stream_bits = c->stream_bits.d;
  return JXG_OK;
}

// ---- stage B: argument blocks of the front end, merge stage and LF lists
// over the plan's tiles (launched by launch_stats, batched over frames) ----
jxg_status build_front(Ctx* c, Job& J) {
  const jxg_params& P = c->params;
  const Frame& f = J.f;
  FrontArgs& fa = J.fa;
  fa = FrontArgs{};
  fa.rgb = J.d_rgb;
  fa.w = J.w;
  fa.h = J.h;
  fa.stride = J.stride;
  fa.bxs = f.bxs;
  fa.bys = f.bys;
  fa.xp = f.xp;
  fa.yp = f.yp;
  fa.tiles_x = f.tiles_x;
  fa.distance = P.distance;
  fa.effort = J.d_force ? 7 : P.effort;
  fa.proposals = J.d_force ? 0u : P.proposals;
  fa.h1_int = (P.flags & JXG_FLAG_H1_INT_ABS) ? 1 : 0;
  fa.gab = (P.flags & JXG_FLAG_GABORISH) ? 1 : 0;
  fa.qf_base = f.qf_base;
  fa.inv_g = f.inv_g;
  fa.G = f.G;
  for (int i = 0; i < 3; i++) {
    fa.dc_mul[i] = f.dc_mul[i];
    fa.dc_step[i] = f.dc_step[i];
  }
  fa.acs = c->acs.p;
  fa.qf = c->qf.p;
  fa.dc = c->dc.p;
  fa.ac = c->ac.p;
  fa.nz = c->nz.p;
  fa.homog = J.homog ? c->homog.p : nullptr;
  fa.ent = J.max_s && !J.d_force ? c->ent.p : nullptr;  // (forced: force_list_kernel writes it)
  fa.force = J.d_force;
  if (J.trace) trace_front_args(c, fa);
  fa.xyb_out = J.max_s ? c->xyb_tiles.p : nullptr;
  const bool listed = !J.plan.tiles.empty();
  fa.tile_list = listed ? c->tile_list.p : nullptr;
  fa.cmap = c->cmap.p;
  fa.ntiles_all = f.tiles_x * f.tiles_y;
  // the statistics arena (256-byte aligned sections) is zeroed by the front
  // kernel's workgroups: no memset launch
  fa.zero = reinterpret_cast<uint4*>(c->stat.p);
  fa.zero_quads = (uint32_t)(c->stat_bytes / 16);
  if (J.d_force_qf) {
    // a forced encode's quant field replaces the adaptive one: no aq_kernel
    J.aq = false;
    fa.qf_in = J.d_force_qf;
  } else if (P.flags & JXG_FLAG_AQ_MASKING) {
    // the libjxl-shaped masking quant field of the plan's tiles, before the
    // front kernel (== oracle/aq.c jxo_aq_masking)
    JXG_HIP(c->aqf.ensure((size_t)f.bxs * f.bys));
    J.aq = true;
    AqArgs& q = J.qa;
    q = AqArgs{};
    q.rgb = J.d_rgb;
    q.w = J.w;
    q.h = J.h;
    q.stride = J.stride;
    q.xp = f.xp;
    q.yp = f.yp;
    q.bxs = f.bxs;
    q.bys = f.bys;
    q.tiles_x = f.tiles_x;
    q.lut = c->lut.p;
    aq_erosion_weights(P.distance, q.ew);
    float dampen = 1.0f;
    if (P.distance >= 2.0f) {
      dampen = 1.0f - ((P.distance - 2.0f) / (14.0f - 2.0f));
      if (dampen < 0.0f) dampen = 0.0f;
    }
    q.mul = f.qf_base * dampen;
    q.add = (1.0f - dampen) * (0.48f * f.qf_base);
    q.inv_g = f.inv_g;
    q.qf = c->aqf.p;
    q.tile_list = listed ? c->tile_list.p : nullptr;
    fa.qf_in = c->aqf.p;
  } else {
    J.aq = false;
  }
  if (J.max_s) {
    MergeArgs& ma = J.ma;
    ma = MergeArgs{};
    ma.xyb = c->xyb_tiles.p;
    ma.bxs = f.bxs;
    ma.bys = f.bys;
    ma.tiles_x = f.tiles_x;
    ma.ntiles = listed ? (uint32_t)J.plan.tiles.size() : (J.plan.world == 1 ? f.tiles_x * f.tiles_y : 0);
    ma.tile_list = listed ? c->tile_list.p : nullptr;
    ma.proposals = fa.proposals;
    ma.force = J.d_force;
    ma.max_s = J.max_s;
    ma.G = f.G;
    for (int i = 0; i < 3; i++) {
      ma.dc_mul[i] = f.dc_mul[i];
      ma.dc_step[i] = f.dc_step[i];
    }
    ma.ent = c->ent.p;
    ma.cmap = c->cmap.p;
    ma.ntiles_all = f.tiles_x * f.tiles_y;
    ma.homog = J.homog ? c->homog.p : nullptr;
    ma.acs = c->acs.p;
    ma.qf = c->qf.p;
    ma.dc = c->dc.p;
    ma.ac = c->ac.p;
    ma.nz = c->nz.p;
    ma.cost = c->mcost.p;
    ma.wk = c->mwk.p;
    ma.sdk = c->msdk.p;
    ma.iwy = c->miwy.p;
    ma.nat = c->mnat.p;
    ma.work = c->mwork.p;
    ma.nwrite = 256 * 3 * 4;  // CUs x resident workgroups (3) x 4 rounds
  }
  // the 128 / 256 px levels over the plan's pass groups: the search's from
  // effort 8 on; a forced job's when its map holds a big kind, whatever the
  // context's effort (the tables and buffers below grow on demand)
  J.big = J.max_s && (J.d_force ? J.force_big : P.effort >= 8);
  if (J.big) {
    if (!c->big_ready) {
      static const BigTables bt = build_big_tables();
      JXG_HIP(c->big_tab.ensure(bt.tab.size()));
      JXG_HIP(c->big_nat.ensure(bt.nat.size()));
      JXG_HIP(hipMemcpyAsync(c->big_tab.p, bt.tab.data(), bt.tab.size() * 4, hipMemcpyHostToDevice, c->stream));
      JXG_HIP(hipMemcpyAsync(c->big_nat.p, bt.nat.data(), bt.nat.size() * 2, hipMemcpyHostToDevice, c->stream));
      c->big_ready = true;
    }
    const uint32_t ng = std::max(1u, J.plan.ng());
    // one scratch slot per persistent workgroup; a frame of ng groups has at
    // most 20 ng tasks per level launch (a 512 x 512 frame needs 20
    // slots, not the 512 of an 8K one -- 402 MB per context otherwise)
    const uint32_t slots = std::min<uint32_t>(ng * 20u, kBigSlots);
    JXG_HIP(c->big_scratch.ensure((size_t)slots * kBigPlanes));
    JXG_HIP(c->big_cost.ensure((size_t)ng * 30));  // [group][25 estimates + 5 current sums]
    JXG_HIP(c->big_work.ensure(1 + (size_t)ng * 16));
    BigArgs& ba = J.ba;
    ba = BigArgs{};
    ba.m = J.ma;
    ba.tab = c->big_tab.p;
    ba.nat = c->big_nat.p;
    ba.scratch = c->big_scratch.p;
    ba.slots = slots;
    ba.cost = c->big_cost.p;
    ba.work = c->big_work.p;
    ba.kinds = c->bigcount.d;
    ba.glist = J.plan.contiguous ? nullptr : c->glist.p;
    ba.g0 = J.plan.g0();
    ba.ng = J.plan.ng();
    ba.gxs = f.gxs;
    ba.trace = J.trace ? 1 : 0;
  }
  J.va = VbArgs{c->acs.p, f.bxs, f.bys, f.lfxs, J.plan.world > 1 ? c->lf_mine.p : nullptr, c->vb.p,
                c->vcount.d};
  return JXG_OK;
}

// bit k: the frame (or with a caller's summed histogram, the whole sharded
// frame) holds a varblock of big kind k
uint32_t big_mask(const uint32_t* count) {
  uint32_t m = 0;
  for (int k = 0; k < 4; k++) m |= (count[k] != 0 ? 1u : 0u) << k;
  return m;
}

// ---- stage E: statistics to the host (AC histogram from `hist`) ----
// AC statistics (histogram, bit bounds, token counts) are downloaded as soon as
// ac_hist is done, so the host builds the AC prefix codes while the LF
// statistics kernels still run; the LF statistics follow in stage_download_lf.
jxg_status stage_download_ac(Ctx* c, Job& J, const uint32_t* hist) {
  (void)J;
  hipStream_t s = c->stream;
  if (hist == c->hist_ac.d) {  // [hist_ac | bound | ntok]: one copy
    JXG_HIP(hipMemcpyAsync(c->h_stat.p, c->stat.p, c->stat_lf, hipMemcpyDeviceToHost, s));
  } else {  // a caller's (all-reduced) histogram
    const size_t hb = (size_t)kMaxClusters * kAlpha * 4, ob = (uint8_t*)c->bound.d - c->stat.p;
    JXG_HIP(hipMemcpyAsync(c->hist_ac.h, hist, hb, hipMemcpyDeviceToHost, s));
    JXG_HIP(hipMemcpyAsync(c->h_stat.p + ob, c->stat.p + ob, c->stat_lf - ob, hipMemcpyDeviceToHost, s));
    // the big-kind counts summed with it (jxg_shard_sizes: after the histogram)
    JXG_HIP(hipMemcpyAsync(c->bigcount.h, hist + (size_t)kMaxClusters * kAlpha, 16,
                           hipMemcpyDeviceToHost, s));
  }
  JXG_HIP(hipEventRecord(c->ev[kEvAcStats], s));
  return JXG_OK;
}
static jxg_status stage_download_lf(Ctx* c, Job& J) {
  (void)J;
  hipStream_t s = c->stream;
  // [lfhist | sbound | vcount]: one copy
  JXG_HIP(hipMemcpyAsync(c->h_stat.p + c->stat_lf, c->stat.p + c->stat_lf, c->stat_bytes - c->stat_lf,
                         hipMemcpyDeviceToHost, s));
  JXG_HIP(hipEventRecord(c->ev[kEvLfStats], s));
  return JXG_OK;
}

// ---- stages B-E of k frames of one size and plan whose contexts share one
// stream (a pipeline lane's slots; k = 1 for one-at-a-time encodes): one
// launch of each kernel for all of them, each frame's downloads after it ----
template <class A, class F>
static std::vector<A> gather(Job* const* js, uint32_t k, F f) {
  std::vector<A> v(k);
  for (uint32_t i = 0; i < k; i++) v[i] = f(*js[i]);
  return v;
}
// a batched launch sizes its grid from frame 0 and indexes the argument
// blocks by blockIdx.z: 1..kMaxBatch frames of one geometry and plan, one stream
static bool batch_ok(Ctx* const* cs, Job* const* js, uint32_t k) {
  if (k < 1 || k > kMaxBatch) return false;
  const Job& A = *js[0];
  for (uint32_t i = 0; i < k; i++)
    if ((js[i]->d_force || js[i]->trace) && k > 1) return false;  // a forced or traced job goes alone
  for (uint32_t i = 1; i < k; i++) {
    const Job& B = *js[i];
    if (cs[i]->stream != cs[0]->stream || B.w != A.w || B.h != A.h || B.plan.rank != A.plan.rank ||
        B.plan.world != A.plan.world || B.plan.tiles.size() != A.plan.tiles.size() ||
        B.plan.ng() != A.plan.ng() || B.nchunks != A.nchunks || B.max_s != A.max_s || B.aq != A.aq)
      return false;
  }
  return true;
}
// front end (+ masking quant field), merge stage, AC token statistics
jxg_status launch_transform(Ctx* const* cs, Job* const* js, uint32_t k) {
  if (!batch_ok(cs, js, k)) return JXG_ERR_INTERNAL;
  hipStream_t s = cs[0]->stream;
  const Job& J = *js[0];
  const Frame& f = J.f;
  const bool listed = !J.plan.tiles.empty();
  // a forced or traced job is a whole frame (rank 0 of 1): it has no tile list
  if (listed && (J.d_force || J.trace)) return JXG_ERR_INTERNAL;
  const uint32_t ntiles = listed ? (uint32_t)J.plan.tiles.size() : f.tiles_x * f.tiles_y;
  for (uint32_t i = 0; i < k; i++) JXG_HIP(hipEventRecord(cs[i]->ev[kEvStart], s));
  if (J.aq) {
    const auto q = gather<AqArgs>(js, k, [](Job& j) { return j.qa; });
    launch_aq(q.data(), k, ntiles, s);
  }
  for (uint32_t i = 0; i < k; i++) JXG_HIP(hipEventRecord(cs[i]->ev[kEvFrontStart], s));
  const auto fa = gather<FrontArgs>(js, k, [](Job& j) { return j.fa; });
  if (listed) {
    launch_front_list(fa.data(), k, ntiles, s);
  } else if (J.plan.world == 1) {
    if (J.d_force)  // (batch_ok: k = 1)
      launch_front_forced(fa[0], f.tiles_x, f.tiles_y, s);
    else if (J.trace)
      launch_front_trace(fa[0], f.tiles_x, f.tiles_y, s);
    else
      launch_front(fa.data(), k, f.tiles_x, f.tiles_y, s);
  }
  JXG_HIP(hipGetLastError());
  for (uint32_t i = 0; i < k; i++) JXG_HIP(hipEventRecord(cs[i]->ev[kEvFrontDone], s));  // front kernel alone
  if (J.trace) {  // the front kernel's quant field, before merged varblocks take their maxima
    const jxg_status st = trace_copy_qf(cs[0], J);
    if (st) return st;
  }
  if (J.max_s) {
    const auto ma = gather<MergeArgs>(js, k, [](Job& j) { return j.ma; });
    if (J.d_force)  // the caller's varblocks: no estimates, no resolve
      JXG_HIP(launch_force_merge(J.ma, s));
    else
      JXG_HIP(launch_merge(ma.data(), k, s));
    if (J.big && J.d_force) {  // the map's big varblocks: listed, then big_write
      JXG_HIP(launch_force_big(J.ba, s));
    } else if (J.big) {  // levels 128 / 256 px (effort >= 8)
      const auto ba = gather<BigArgs>(js, k, [](Job& j) { return j.ba; });
      JXG_HIP(launch_big(ba.data(), k, s));
      // test hook: JXG_DEBUG_BIGCOST=path writes frame 0's candidate estimates
      if (const char* dbg = std::getenv("JXG_DEBUG_BIGCOST")) {
        const size_t ngc = std::max(1u, J.plan.ng());
        std::vector<float> h(ngc * 30);
        JXG_HIP(hipMemcpyAsync(h.data(), ba[0].cost, h.size() * 4, hipMemcpyDeviceToHost, s));
        JXG_HIP(hipStreamSynchronize(s));
        if (FILE* fp = std::fopen(dbg, "wb")) {  // the 25 estimates of every group
          for (size_t g = 0; g < ngc; g++) std::fwrite(h.data() + g * 30, 4, 25, fp);
          std::fclose(fp);
        }
      }
    }
  }
  for (uint32_t i = 0; i < k; i++) JXG_HIP(hipEventRecord(cs[i]->ev[kEvMerged], s));
  if (J.trace) {  // the trace's planes and summary, while mcost / big_cost are this encode's
    const jxg_status st = trace_enqueue(cs[0], J);
    if (st) return st;
  }
  // (the statistics arenas were zeroed by the front kernel)
  const auto aa = gather<AcArgs>(js, k, [](Job& j) { return j.aa; });
  launch_ac_hist(aa.data(), k, J.plan.ng(), s, J.big);
  JXG_HIP(hipGetLastError());
  return JXG_OK;
}
// varblock lists, LF-stream histograms, and each frame's LF statistics download
jxg_status launch_lf_stats(Ctx* const* cs, Job* const* js, uint32_t k) {
  if (!batch_ok(cs, js, k)) return JXG_ERR_INTERNAL;
  hipStream_t s = cs[0]->stream;
  const Job& J = *js[0];
  const auto va = gather<VbArgs>(js, k, [](Job& j) { return j.va; });
  launch_vb_list(va.data(), k, J.f.nlf, s);
  const auto la = gather<LfArgs>(js, k, [](Job& j) { return j.la; });
  launch_lf_hist(la.data(), k, J.nchunks, s);
  JXG_HIP(hipGetLastError());
  for (uint32_t i = 0; i < k; i++) {
    const jxg_status st = stage_download_lf(cs[i], *js[i]);
    if (st) return st;
  }
  return JXG_OK;
}
// all of stages B-E (each frame's own AC histogram)
jxg_status launch_stats(Ctx* const* cs, Job* const* js, uint32_t k) {
  jxg_status st = launch_transform(cs, js, k);
  for (uint32_t i = 0; i < k && !st; i++) st = stage_download_ac(cs[i], *js[i], cs[i]->hist_ac.d);
  return st ? st : launch_lf_stats(cs, js, k);
}

// ---- stage F (host): the frame's codes, global sections and arena layouts
// (built by jxg_codes.cpp straight into the pinned upload sections), their
// uploads, and with prefix codes the AC emission ----
jxg_status stage_codes(Ctx* c, Job& J) {
  hipStream_t s = c->stream;
  const Frame& f = J.f;
  JXG_HIP(hipEventSynchronize(c->ev[kEvAcStats]));  // LF kernels may still run
  const Clock::time_point t_codes = Clock::now();
  const AcCodes A = build_ac_codes(c->hist_ac.h, J.ans, c->ans_tab.h, c->codes_ac.h);
  if (J.ans) {
    J.nhist_ans = (uint32_t)A.nhist;
    if (J.presets) {
      J.pre_ctxmap = A.ctxmap;
      J.pre_counts.assign(A.counts.begin(), A.counts.begin() + (size_t)A.nhist * kAlpha);
    }
  }
  // LfGlobal / HfGlobal (rank 0): need the AC codes only
  J.lfglobal = BitWriter();
  J.hfglobal = BitWriter();
  if (J.plan.rank == 0) {
    write_lf_global(J.lfglobal, f.G, f.qdc);
    if (!J.presets) {  // (per-rank presets: HfGlobal at assembly, build_hf_presets)
      const uint32_t mask = J.big ? big_mask(c->bigcount.h) : 0u;
      const BitWriter* cm = &c->ctxmap_cache.get(A.ctxmap, A.nhist);
      if (J.ans)
        write_hf_global(J.hfglobal, mask, f.ngroups, 1, A.ctxmap, A.nhist, A.tables, cm);
      else
        write_hf_global(J.hfglobal, mask, f.ngroups, 1, A.ctxmap, A.nhist, A.codes, cm);
    }
  }
  // AC layout; the pinned upload sources stay valid until the next frame's
  // stage_codes, which runs after this frame's emission has completed
  J.gbase.assign(f.ngroups, 0);
  const uint64_t ac_words = layout_ac(J.plan.groups, c->ntok.h, c->bound.h, J.ans, J.gbase.data());
  if (!J.ans) JXG_HIP(c->scratch.ensure(ac_words));  // (ANS: with the LF arena below)
  std::copy(J.gbase.begin(), J.gbase.end(), c->gbase.h);
  if (J.ans) {
    const uint64_t nrec = (uint64_t)std::max(1u, J.plan.ng()) * kGroupTokStride;
    JXG_HIP(c->tval.ensure(nrec));
    JXG_HIP(c->tlen.ensure(nrec));
    JXG_HIP(c->ans_state.ensure(f.ngroups));
    JXG_HIP(c->csum.ensure((uint64_t)std::max(1u, J.plan.ng()) * kAnsMaxChunks));
    J.max_tokens = ans_chain_order(J.plan, c->ntok.h, c->ans_order.h);
  }
  const float ms_ac_codes = ms_since(t_codes);
  if (!J.ans) {
    // prefix codes: the AC code tables now, so the AC emission runs while the
    // host builds the LF-group codes (ANS: every table in one upload below; the
    // rANS coder -- a long latency-bound chain that hides the LF-code
    // construction anyway -- is launched by stage_emit)
    JXG_HIP(hipMemcpyAsync(c->up.p, c->h_up.p, c->up_ac, hipMemcpyHostToDevice, s));
    J.aa.scratch = c->scratch.p;
    launch_ac_emit(J.aa, J.plan.ng(), s);
    JXG_HIP(hipGetLastError());
    JXG_HIP(hipMemcpyAsync(c->gbits.h, c->gbits.d, f.ngroups * 4, hipMemcpyDeviceToHost, s));
    JXG_HIP(hipEventRecord(c->ev[kEvAcEmitted], s));
  }
  JXG_HIP(hipEventSynchronize(c->ev[kEvLfStats]));  // (stage_download_lf)
  const Clock::time_point t_lf = Clock::now();
  build_lf_codes(f, J.plan, c->lfhist.h, c->vcount.h, J.lf, c->lfcodes.h, J.preA, J.preB);
  J.sbase.assign(J.nstreams, 0);
  const uint64_t lf_words = layout_lf(f, J.plan, c->sbound.h, J.sbase.data());
  std::copy(J.sbase.begin(), J.sbase.end(), c->stream_base.h);
  if (J.ans) {
    // one arena for the AC and LF bits (no fill: the chains clear their
    // ranges, lf_code stores whole words) and every table in one upload
    JXG_HIP(c->scratch.ensure(ac_words + lf_words));
    c->lf_scratch = c->scratch.p + ac_words;
    J.aa.scratch = c->scratch.p;
    JXG_HIP(hipMemcpyAsync(c->up.p + c->up_gbase, c->h_up.p + c->up_gbase,
                           c->up_bytes - c->up_gbase, hipMemcpyHostToDevice, s));
  } else {
    JXG_HIP(c->scratch_lf.ensure(lf_words));
    c->lf_scratch = c->scratch_lf.p;
    JXG_HIP(hipMemcpyAsync(c->up.p + c->up_lf, c->h_up.p + c->up_lf, c->up_bytes - c->up_lf,
                           hipMemcpyHostToDevice, s));
  }
  J.ms_codes = ms_ac_codes + ms_since(t_lf);
  return JXG_OK;
}

// ---- stage G: rANS coder (the prefix-code AC emission was launched by
// stage_codes), LF-stream bit emission, bit counts to the host ----
static void build_emit(Ctx* c, Job& J) {
  J.la.scratch = c->lf_scratch;
  if (!J.ans) return;
  AnsArgs& na = J.na;
  na = AnsArgs{};
  na.tokens = c->tokens.p;
  na.val = c->tval.p;
  na.len = c->tlen.p;
  na.ntok = c->ntok.d;
  na.bandtok = c->bandtok.d;
  na.tab = c->ans_tab.d;
  na.nhist = J.nhist_ans;
  na.state = c->ans_state.p;
  na.base = c->gbase.d;
  na.scratch = c->scratch.p;
  na.bits = c->gbits.d;
  na.g0 = J.plan.g0();
  na.n = J.plan.ng();
  na.glist = J.aa.glist;
  na.order = c->ans_order.d;
  na.csum = c->csum.p;
  na.max_tokens = J.max_tokens;
}
// the emission of k frames sharing a stream (codes built): rANS chains + bit
// placement and LF streams as one launch each, then each frame's bit counts
// to the host.  streamed: frames of the streaming pipeline (launch_ans picks
// the chain kernel by it)
jxg_status launch_emit(Ctx* const* cs, Job* const* js, uint32_t k, bool streamed) {
  if (!batch_ok(cs, js, k)) return JXG_ERR_INTERNAL;
  hipStream_t s = cs[0]->stream;
  const Job& J = *js[0];
  for (uint32_t i = 0; i < k; i++) build_emit(cs[i], *js[i]);
  if (J.ans) {
    const auto na = gather<AnsArgs>(js, k, [](Job& j) { return j.na; });
    launch_ans(na.data(), k, s, streamed);
    JXG_HIP(hipGetLastError());
  }
  const auto la = gather<LfArgs>(js, k, [](Job& j) { return j.la; });
  launch_lf_code(la.data(), k, J.nchunks, s);
  JXG_HIP(hipGetLastError());
  for (uint32_t i = 0; i < k; i++) {
    Ctx* c = cs[i];
    if (J.ans) {  // [gbits | stream_bits]: one copy
      JXG_HIP(hipMemcpyAsync(c->h_bits.p, c->bits.p, c->bits_bytes, hipMemcpyDeviceToHost, s));
      JXG_HIP(hipEventRecord(c->ev[kEvAcEmitted], s));
    } else {
      JXG_HIP(hipMemcpyAsync(c->stream_bits.h, c->stream_bits.d, js[i]->nstreams * 4,
                             hipMemcpyDeviceToHost, s));
    }
    JXG_HIP(hipEventRecord(c->ev[kEvEmitted], s));
  }
  return JXG_OK;
}
jxg_status stage_emit(Ctx* c, Job& J, bool sync) {
  Job* jp = &J;
  jxg_status st = launch_emit(&c, &jp, 1, false);
  if (!st && sync) st = wait_emission(c, J);
  return st;
}

// ---- stage H: concatenation.  Sections are bit-exact piece lists (host
// chunks + device scratch ranges, jxg_layout.h) ----
static JobSections job_sections(const Ctx* c, const Job& J) {
  JobSections j;
  j.nlf = J.f.nlf;
  j.first_rank = J.plan.rank == 0;
  j.presets = J.presets;
  j.rank = J.plan.rank;
  j.world = J.plan.world;
  j.lf_mine = J.plan.world == 1 ? nullptr : J.plan.lf_mine.data();
  j.groups = J.plan.groups.data();
  j.ngroups = J.plan.ng();
  j.lfglobal = &J.lfglobal;
  j.hfglobal = &J.hfglobal;
  j.preA = J.preA.data();
  j.preB = J.preB.data();
  j.sbase = J.sbase.data();
  j.sbits = c->stream_bits.h;
  j.gbase = J.gbase.data();
  j.gbits = c->gbits.h;
  return j;
}
static_assert(sizeof(PlacedPiece) == sizeof(ConcatPiece), "PlacedPiece is what the concat kernel reads");

// Everything on one stream.  full: headers + TOC + all sections into one
// codestream; shard: the plan's sections, each byte-aligned, back to back
// (`section_ids` receives their TOC indices)
jxg_status stage_concat(Ctx* c, Job& J, bool full, std::vector<uint32_t>* section_ids,
                        std::vector<uint32_t>* section_bytes, uint8_t** host_out,
                        size_t* out_bytes) {
  hipStream_t s = c->stream;
  const JobSections js = job_sections(c, J);
  PieceList L;
  L.add_prefix(js);
  L.add_groups(js);
  const bool single = full && J.f.ngroups == 1;
  const std::vector<uint32_t> sizes = L.sizes(single);
  StreamLayout lay;
  if (full) lay = stream_layout(J.w, J.h, J.lf, sizes);
  const size_t nbytes = L.place(full ? &lay.head : nullptr, single);
  const size_t out_words = (nbytes + 3) / 4 + 1;
  const std::vector<PlacedPiece>& cps = L.pieces();
  const std::vector<uint32_t>& chunk_words = L.chunk_words();
  // pieces and chunk words through one pinned staging buffer, one upload
  // (the previous frame of this context has completed: the staging is free)
  const size_t pb = (std::max<size_t>(cps.size(), 1) * sizeof(ConcatPiece) + 255) & ~(size_t)255;
  const size_t wb = chunk_words.size() * 4;
  JXG_HIP(c->cat.buf.ensure(pb + wb));
  JXG_HIP(c->cat.h_buf.ensure(pb + wb));
  JXG_HIP(c->out.ensure(out_words));
  uint8_t* ho = nullptr;
  if (host_out) {  // else the bytes stay in c->out (device)
    ho = out_alloc(out_words * 4);
    if (!ho) return JXG_ERR_OOM;
  }
  if (!cps.empty()) std::memcpy(c->cat.h_buf.p, cps.data(), cps.size() * sizeof(ConcatPiece));
  std::memcpy(c->cat.h_buf.p + pb, chunk_words.data(), wb);
  JXG_HIP(hipMemcpyAsync(c->cat.buf.p, c->cat.h_buf.p, pb + wb, hipMemcpyHostToDevice, s));
  launch_concat(reinterpret_cast<const ConcatPiece*>(c->cat.buf.p), (uint32_t)cps.size(), out_words,
                c->scratch.p, reinterpret_cast<const uint32_t*>(c->cat.buf.p + pb), c->lf_scratch,
                c->out.p, s);
  JXG_HIP(hipGetLastError());
  if (ho && hipMemcpyAsync(ho, c->out.p, out_words * 4, hipMemcpyDeviceToHost, s) != hipSuccess) {
    out_release(ho);
    return JXG_ERR_HIP;
  }
  JXG_HIP(hipEventRecord(c->ev[kEvAssembled], s));
  if (host_out) *host_out = ho;
  *out_bytes = nbytes;
  if (section_ids) *section_ids = L.ids();
  if (section_bytes) *section_bytes = sizes;
  return JXG_OK;
}

// Full codestream of a multi-group frame with the AC block moved early: the
// pass-group sections (the bulk of the bytes) are concatenated on stream2 as
// soon as the AC emission is done and copied to the END region of the host
// block while the LF streams are still being emitted; the prefix (headers,
// TOC, LfGlobal, LF groups, HfGlobal) follows on the main stream and lands
// right before it.  The same PieceList as stage_concat(full), placed in two
// parts.
static jxg_status stage_concat_split(Ctx* c, Job& J, uint8_t** host_out, size_t* out_bytes) {
  if (!c->stream2 && hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess)
    return JXG_ERR_HIP;  // created on first use: only lone contexts take this path
  hipStream_t s = c->stream, s2 = c->stream2;
  const Frame& f = J.f;
  JXG_HIP(hipEventSynchronize(c->ev[kEvAcEmitted]));  // AC emission done, its bit counts on the host
  const JobSections js = job_sections(c, J);  // (one context: all groups)
  PieceList A;
  A.add_groups(js);
  const std::vector<uint32_t> ac_sizes = A.sizes(false);
  const size_t ac_bytes = A.place(nullptr, false);
  const uint32_t np = (uint32_t)A.pieces().size();
  JXG_HIP(c->cat.h_pieces_ac.ensure(std::max<uint32_t>(np, 1)));
  if (np) std::memcpy(c->cat.h_pieces_ac.p, A.pieces().data(), np * sizeof(ConcatPiece));
  // prefix upper bound: chunks + LF stream bounds + headers / TOC + slack for
  // the back reference
  uint64_t pbits = J.lfglobal.bits() + J.hfglobal.bits() + 16;
  for (uint32_t lg = 0; lg < f.nlf; lg++)
    if (J.plan.owns_lf(lg))
      pbits += J.preA[lg].bits() + J.preB[lg].bits() + c->sbound.h[lg * 2] +
               c->sbound.h[lg * 2 + 1] + 8;
  const size_t nsec = 2 + (size_t)f.nlf + f.ngroups;
  size_t pmax = (size_t)(pbits / 8) + 256 + 4 * nsec + 16 + kOutHdr;
  pmax = (pmax + 63) & ~(size_t)63;
  uint8_t* ho = out_alloc(pmax + ac_bytes + 8);
  if (!ho) return JXG_ERR_OOM;
  auto fail = [&](jxg_status e) {
    (void)hipStreamSynchronize(s2);
    (void)hipStreamSynchronize(s);
    out_release(ho);
    return e;
  };
  const size_t ac_words = ac_bytes / 4 + 2;
  if (c->cat.out_ac.ensure(ac_words) != hipSuccess ||
      c->cat.pieces_ac.ensure(std::max<uint32_t>(np, 1)) != hipSuccess)
    return fail(JXG_ERR_HIP);
  if (hipStreamWaitEvent(s2, c->ev[kEvAcEmitted], 0) != hipSuccess ||
      (np && hipMemcpyAsync(c->cat.pieces_ac.p, c->cat.h_pieces_ac.p, np * sizeof(ConcatPiece),
                            hipMemcpyHostToDevice, s2) != hipSuccess))
    return fail(JXG_ERR_HIP);
  launch_concat(c->cat.pieces_ac.p, np, ac_words, c->scratch.p, c->cat.chunks.p, nullptr,
                c->cat.out_ac.p, s2);
  if (hipGetLastError() != hipSuccess ||
      (ac_bytes && hipMemcpyAsync(ho + pmax, c->cat.out_ac.p, ac_bytes, hipMemcpyDeviceToHost, s2) !=
                       hipSuccess) ||
      hipEventRecord(c->ev[kEvAcBlock], s2) != hipSuccess)
    return fail(JXG_ERR_HIP);

  // prefix, after the LF emission (stage_emit without its sync)
  if (hipStreamSynchronize(s) != hipSuccess) return fail(JXG_ERR_HIP);
  const Clock::time_point t_layout = Clock::now();
  PieceList P;
  P.add_prefix(js);
  std::vector<uint32_t> sizes = P.sizes(false);
  sizes.insert(sizes.end(), ac_sizes.begin(), ac_sizes.end());
  const StreamLayout lay = stream_layout(J.w, J.h, J.lf, sizes);
  const size_t pbytes = P.place(&lay.head, false);
  // prefix bound violated (or forced, JXG_FLAG_FORCE_ONE_STREAM): one-stream
  // assembly instead
  if (pbytes + kOutHdr > pmax || (c->params.flags & JXG_FLAG_FORCE_ONE_STREAM)) {
    if (hipStreamSynchronize(s2) != hipSuccess) return fail(JXG_ERR_HIP);
    out_release(ho);
    const jxg_status st = stage_concat(c, J, true, nullptr, nullptr, host_out, out_bytes);
    J.ms_layout = ms_since(t_layout);
    return st;
  }
  const size_t out_words = (pbytes + 3) / 4 + 1;
  const std::vector<PlacedPiece>& cps = P.pieces();
  const std::vector<uint32_t>& chunk_words = P.chunk_words();
  if (c->cat.chunks.ensure(chunk_words.size()) != hipSuccess ||
      c->cat.pieces.ensure(std::max<size_t>(cps.size(), 1)) != hipSuccess ||
      c->out.ensure(out_words) != hipSuccess)
    return fail(JXG_ERR_HIP);
  uint8_t* data = ho + pmax - pbytes;
  if (hipMemcpyAsync(c->cat.chunks.p, chunk_words.data(), chunk_words.size() * 4,
                     hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(c->cat.pieces.p, cps.data(), cps.size() * sizeof(ConcatPiece),
                     hipMemcpyHostToDevice, s) != hipSuccess)
    return fail(JXG_ERR_HIP);
  launch_concat(c->cat.pieces.p, (uint32_t)cps.size(), out_words, c->scratch.p, c->cat.chunks.p,
                c->lf_scratch, c->out.p, s);
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(data, c->out.p, pbytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamWaitEvent(s, c->ev[kEvAcBlock], 0) != hipSuccess ||
      hipEventRecord(c->ev[kEvAssembled], s) != hipSuccess)
    return fail(JXG_ERR_HIP);
  J.ms_layout = ms_since(t_layout);
  out_set_backref(data, ho);
  *host_out = data;
  *out_bytes = pbytes + ac_bytes;
  return JXG_OK;
}

// ---- one frame, in three phases (encode_device runs them back to back; the
// streaming pipeline interleaves the phases of consecutive frames) ----
// phase 1: buffers, front end + merge stage + AC / LF statistics and their
// downloads, all launched asynchronously on the context's stream
// (rank, world): a shard of a frame whose plan needs no record exchange and,
// with world > 1, ANS (one HF preset per rank): no collective before assembly
// the frame's plan, buffers and argument blocks (nothing launched)
jxg_status enc_prepare(Ctx* c, Job& J, const uint8_t* d_rgb, uint32_t w, uint32_t h,
                              size_t stride, uint32_t rank, uint32_t world) {
  J.f = make_frame(w, h, c->params.distance);
  J.plan = make_plan(J.f, rank, world);
  J.w = w;
  J.h = h;
  J.stride = stride;
  J.d_rgb = d_rgb;
  jxg_status st = stage_alloc(c, J);
  if (st) return st;
  J.presets = J.ans && world > 1;
  return build_front(c, J);
}
static jxg_status enc_launch(Ctx* c, Job& J, const uint8_t* d_rgb, uint32_t w, uint32_t h,
                             size_t stride, uint32_t rank = 0, uint32_t world = 1) {
  jxg_status st = enc_prepare(c, J, d_rgb, w, h, stride, rank, world);
  if (st) return st;
  Job* jp = &J;
  return launch_stats(&c, &jp, 1);
}

// phase 2: (host, after the statistics arrive) codes and headers; AC / LF
// emission launched
static jxg_status enc_codes(Ctx* c, Job& J, bool sync) {
  const jxg_status st = stage_codes(c, J);
  if (st) return st;
  return stage_emit(c, J, sync);
}

// phase 3: assembly, the codestream in host memory, stats
// phase 3 in two halves: enc_finish_start (the emission's bit counts on the
// host -> layout, concat and the codestream's D2H enqueued) and enc_finish_end
// (wait for them, stats).  The streaming pipeline starts a frame's assembly
// as soon as its emission is done and ends it when the frame is taken.
jxg_status enc_finish_start(Ctx* c, Job& J, bool split) {
  const Clock::time_point t_layout = Clock::now();
  J.host_out = nullptr;
  J.out_bytes = 0;
  jxg_status st;
  if (split) {
    if ((st = stage_concat_split(c, J, &J.host_out, &J.out_bytes))) return st;
  } else {
    // the emission's bit counts on the host (stage_emit may have returned
    // without waiting)
    if ((st = wait_emission(c, J))) return st;
    if ((st = stage_concat(c, J, true, nullptr, nullptr, &J.host_out, &J.out_bytes))) return st;
  }
  J.ms_finish_layout = split ? J.ms_layout : ms_since(t_layout);
  rate_note(c, J);  // (host bookkeeping: the emission's bit counts are here by now)
  return JXG_OK;
}
// the frame's stats (the lane's jxg_stats); `assembled`: the assembly has
// completed (kEvAssembled), else its time is left out
void enc_stats(Ctx* c, Job& J, size_t out_bytes, float ms_layout, bool assembled,
                      const std::vector<int16_t>* m_ac16, Clock::time_point t_call) {
  const jxg_params& P = c->params;
  const Frame& f = J.f;
  const size_t nb = (size_t)f.bxs * f.bys;
  jxg_stats& S = c->stats;
  S = jxg_stats{};
  S.xsize = J.w;
  S.ysize = J.h;
  S.xsize_blocks = f.bxs;
  S.ysize_blocks = f.bys;
  S.num_groups = f.ngroups;
  S.num_lf_groups = f.nlf;
  S.global_scale = f.G;
  S.quant_dc = f.qdc;
  S.bytes = out_bytes;
  c->m_ntok.assign(c->ntok.h, c->ntok.h + f.ngroups * 3);
  S.ac_tokens = c->m_ntok.data();
  if ((P.flags & JXG_FLAG_KEEP_MAPS) && m_ac16) {
    // coefficients in natural-order slices, widened to int32 for the caller
    for (size_t i = 0; i < nb * 192; i++) c->m_ac[i] = (*m_ac16)[i];
    S.ac_strategy = c->m_acs.data();
    S.quant_field = c->m_qf.data();
    S.dc = c->m_dc.data();
    S.ac = c->m_ac.data();
    S.homogeneity = J.homog ? c->m_homog.data() : nullptr;
  }
  S.ms_front = elapsed(c->ev[kEvStart], c->ev[kEvMerged]);
  S.ms_front_kernel = elapsed(c->ev[kEvFrontStart], c->ev[kEvFrontDone]);
  S.ms_aq = elapsed(c->ev[kEvStart], c->ev[kEvFrontStart]);
  S.ms_histogram = elapsed(c->ev[kEvMerged], c->ev[kEvLfStats]);
  S.ms_emit = elapsed(c->ev[kEvLfStats], c->ev[kEvEmitted]);
  S.ms_assemble = assembled ? elapsed(c->ev[kEvEmitted], c->ev[kEvAssembled]) : 0.0f;
  S.ms_total = elapsed(c->ev[kEvStart], assembled ? c->ev[kEvAssembled] : c->ev[kEvEmitted]);
  S.ms_host_codes = J.ms_codes;
  S.ms_host_layout = ms_layout;
  S.ms_host_call = ms_since(t_call);
}
static jxg_status enc_finish_end(Ctx* c, Job& J, jxg_buffer* out, Clock::time_point t_call) {
  hipStream_t s = c->stream;
  const jxg_params& P = c->params;
  const Frame& f = J.f;
  const size_t nb = (size_t)f.bxs * f.bys;
  uint8_t* host_out = J.host_out;
  const size_t out_bytes = J.out_bytes;
  J.host_out = nullptr;
  std::vector<int16_t> m_ac16_tmp;
  if (P.flags & JXG_FLAG_KEEP_MAPS) {
    c->m_acs.resize(nb);
    c->m_qf.resize(nb);
    c->m_dc.resize(nb * 3);
    c->m_ac.resize(nb * 192);
    JXG_HIP(hipMemcpyAsync(c->m_acs.data(), c->acs.p, nb, hipMemcpyDeviceToHost, s));
    JXG_HIP(hipMemcpyAsync(c->m_qf.data(), c->qf.p, nb, hipMemcpyDeviceToHost, s));
    JXG_HIP(hipMemcpyAsync(c->m_dc.data(), c->dc.p, nb * 12, hipMemcpyDeviceToHost, s));
    m_ac16_tmp.resize(nb * 192);
    JXG_HIP(hipMemcpyAsync(m_ac16_tmp.data(), c->ac.p, nb * 192 * 2, hipMemcpyDeviceToHost, s));
    if (J.homog) {
      c->m_homog.resize(nb * 3);
      JXG_HIP(hipMemcpyAsync(c->m_homog.data(), c->homog.p, nb * 12, hipMemcpyDeviceToHost, s));
    }
  }
  if (hipStreamSynchronize(s) != hipSuccess) {
    out_release(host_out);
    return JXG_ERR_HIP;
  }
  out->data = host_out;
  out->size = out_bytes;
  enc_stats(c, J, out_bytes, J.ms_finish_layout, true, &m_ac16_tmp, t_call);
  return JXG_OK;
}
jxg_status enc_finish(Ctx* c, Job& J, bool split, jxg_buffer* out,
                             Clock::time_point t_call) {
  const jxg_status st = enc_finish_start(c, J, split);
  return st ? st : enc_finish_end(c, J, out, t_call);
}


static jxg_status encode_device(Ctx* c, const uint8_t* d_rgb, uint32_t w, uint32_t h,
                                size_t stride, jxg_buffer* out, Clock::time_point t_call,
                                const uint8_t* force_acs, const uint8_t* force_qf, bool trace,
                                uint32_t force_big) {
  // streamed frames in flight use this context as a lane (and its helper
  // threads its host state): one-at-a-time calls wait until they are received
  if (pipe_busy(c)) return JXG_ERR_INVALID_ARG;
  Job J;
  if (force_acs) {  // the (validated) maps of a forced encode, ahead of the kernels on the stream
    const size_t nb = (size_t)((w + 7) / 8) * ((h + 7) / 8);
    JXG_HIP(c->force_acs.ensure(nb));
    JXG_HIP(hipMemcpyAsync(c->force_acs.p, force_acs, nb, hipMemcpyHostToDevice, c->stream));
    J.d_force = c->force_acs.p;
    J.force_big = force_big != 0;
    if (force_qf) {
      JXG_HIP(c->force_qf.ensure(nb));
      JXG_HIP(hipMemcpyAsync(c->force_qf.p, force_qf, nb, hipMemcpyHostToDevice, c->stream));
      J.d_force_qf = c->force_qf.p;
    }
  }
  jxg_status st;
  if (trace) {  // the trace's buffers, before the argument blocks point into them
    if ((st = trace_alloc(c, w, h))) return st;
    J.trace = true;
  }
  if ((st = enc_launch(c, J, d_rgb, w, h, stride))) return st;
  // split assembly for a single context of a multi-group frame (single-group
  // frames are one section; several contexts keep the one-stream assembly)
  const bool split = J.f.ngroups > 1 && lone_context();
  if ((st = enc_codes(c, J, !split))) return st;
  c->rc.has_big = J.big;
  return enc_finish(c, J, split, out, t_call);
}

jxg_status encode_one(Ctx* c, const uint8_t* src, bool on_device, uint32_t w, uint32_t h,
                      size_t stride, jxg_buffer* out, Clock::time_point t_call,
                      const uint8_t* force_acs, const uint8_t* force_qf, bool trace,
                      uint32_t force_big) {
  c->rc.ok = false;
  c->tr.have = false;
  if (on_device) {
    const jxg_status st = order_input(c, c);
    if (st) return st;
  } else {  // (c->rgb is free: no streamed frame is in flight)
    const size_t bytes = stride * (h - 1) + (size_t)w * 3;
    if (c->rgb.ensure(bytes) != hipSuccess) return JXG_ERR_OOM;
    if (hipMemcpyAsync(c->rgb.p, src, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess)
      return JXG_ERR_HIP;
    src = c->rgb.p;
  }
  const jxg_status st =
      encode_device(c, src, w, h, stride, out, t_call, force_acs, force_qf, trace, force_big);
  if (!st) {
    c->rc.ok = true;
    c->rc.w = w;
    c->rc.h = h;
    c->tr.have = trace;
    c->tr.w = w;
    c->tr.h = h;
  }
  return st;
}

// one synthetic frame of the caller's size through the one-at-a-time path:
// the context's buffers for that size are allocated and every kernel's code
// object is loaded before the caller's first frame (jxg_cjxl runs it beside
// the PNG decode: a new context's first 8K encode took 35 ms against 12 ms)
jxg_status warmup(Ctx* c, uint32_t w, uint32_t h) {
  c->rc.ok = false;
  const size_t stride = (size_t)w * 3;
  if (c->rgb.ensure(stride * h) != hipSuccess) return JXG_ERR_OOM;  // jxg_encode_rgb8's upload buffer
  JXG_HIP(launch_synth(c->rgb.p, w, h, stride, 0x5741524Dull, c->stream));
  jxg_buffer out{nullptr, 0};
  const jxg_status st = encode_one(c, c->rgb.p, true, w, h, stride, &out, Clock::now());
  out_release(out.data);
  c->rc.ok = false;  // (the synthetic frame is not the caller's last encode)
  c->stats = jxg_stats{};
  return st;
}

}  // namespace jxg

