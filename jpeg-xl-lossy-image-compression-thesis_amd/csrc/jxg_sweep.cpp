// jxg_sweep.cpp -- one image over many settings in one call (jxg_sweep_rgb8;
// DESIGN.md §3.14).  The image is uploaded once; every point is a frame of
// the streaming pipeline (jxg_pipe.cpp) that carries its parameters, so the
// points' transform kernels, rANS chains, host-side codes and -- with quality
// -- their reconstruction chains and metrics overlap over the context's lanes.
// A frame's quality is enqueued on its lane's stream right behind its
// codestream's copy (pipe_complete_oldest): the chain of jxg_reconstruct.cpp on
// the lane's own coefficients, ending in the fused colour + squared-error
// kernel, then the SSIM kernels on the stored image when asked for; the two
// result words land in pinned memory before the frame's completion event.
// With jxg_set_sweep_msssim the lane runs, in the SSIM kernels' place, the
// pyramid of its decoded image and the MS-SSIM kernels
// against the original's pyramid, which the context built once on its own
// stream; their scale 0 is the SSIM.
// With jxg_set_sweep_report the chain ends in the kernel that also writes the
// block error map, and the strategy reduction (jxg_report.hip, DESIGN.md
// §3.16) follows the metrics; its table is a third pinned result.
// With jxg_set_sweep_rates every point's lane prices its token records
// (jxg_rate.hip) behind the codestream's copy -- ahead of the
// metrics' end event with quality, alone with quality 0.
// With jxg_set_sweep_ab (quality 1 / 2) a point some later point names as its
// baseline copies its triple -- block errors, cost shares, strategy bytes, 9
// bytes a block -- into a snapshot slot of the sweep (one per distinct
// baseline, kept for the call: 4.7 MB per baseline at 8K) and records an
// event; a comparing point's lane waits for it and reduces the snapshot against
// its own triple (jxg_ab.hip); the table is one more pinned
// result ahead of the metrics' end event.
// With jxg_set_sweep_trace every point of effort >= 5 runs as a traced job on
// its lane (jxg_trace.cpp): the trace instantiations of the
// front kernel and of the 128 / 256 px levels, then the planes and the summary
// behind the merge stage, whose 104 words are copied to pinned memory right
// there -- long before the frame's completion event.  The planes stay in the
// lane's Ctx::Trace (115 bytes a block, kept with the lane) and are not fetched.
#include <cmath>
#include <cstring>

#include "jxg_ctx.h"

namespace jxg {

jxg_status sweep_quality_enqueue(Ctx* S, const SweepReq& rq, const uint8_t* d_orig, size_t so,
                                 uint32_t w, uint32_t h) {
  hipStream_t s = S->stream;
  Ctx::Quality& q = S->q;
  const uint32_t np = ssim_partials(w, h);
  const bool ssim = rq.quality == 2 && np > 0;
  const size_t row = (size_t)w * 3;
  JXG_HIP(q.sse.ensure(1));
  JXG_HIP(q.ssim.ensure(1));
  if (ssim) {
    const jxg_status st = quality_gauss(S);
    if (st) return st;
    JXG_HIP(q.part.ensure(np));
    JXG_HIP(S->rc.rgb.ensure(row * h));
  }
  const bool bmap = rq.h[kRiderReport] || rq.ab;  // the block-map form of the chain's last kernel
  if (bmap) JXG_HIP(q.bsse.ensure((size_t)((w + 7) / 8) * ((h + 7) / 8)));
  JXG_HIP(hipMemsetAsync(q.sse.p, 0, sizeof(uint64_t), s));
  JXG_HIP(hipEventRecord(rq.ev[0], s));
  const ReconSse e{d_orig, so, q.sse.p, ssim, bmap ? q.bsse.p : nullptr};
  const jxg_status st = reconstruct_device(
      S, recon_frame_of_encode(w, h, S->params),
      ReconMaps{S->acs.p, S->qf.p, S->dc.p, S->ac.p, S->cmap.p}, ssim ? S->rc.rgb.p : nullptr, row,
      &e);
  if (st) return st;
  JXG_HIP(hipEventRecord(rq.ev[1], s));
  rq.h_q[1] = 0;
  const bool ms = ssim && rq.h[kRiderMsssim];
  if (ssim && !ms) {
    const MetricArgs a{d_orig, S->rc.rgb.p, so, row, w, h, q.sse.p, q.part.p, q.ssim.p};
    launch_ssim(a, s);
    JXG_HIP(hipGetLastError());
    JXG_HIP(hipMemcpyAsync(rq.h_q + 1, q.ssim.p, sizeof(double), hipMemcpyDeviceToHost, s));
  }
  // MS-SSIM's scale 0 is ssim_kernel's sum bit for bit (ssim_cs_kernel<false>
  // and the reduction order; tests/test_gpu_msssim.py), so the SSIM kernels are
  // not run a second time: the frame's SSIM word is the first of the ten sums
  if (ms) {
    JXG_HIP(q.pyr_c.ensure(ms_pyramid_floats(w, h)));
    JXG_HIP(q.ms_part.ensure(ms_partials(w, h)));
    JXG_HIP(q.ms_out.ensure(2 * kMsScales));
    launch_ms_pyramid(S->rc.rgb.p, row, w, h, q.pyr_c.p, s);
    JXG_HIP(hipStreamWaitEvent(s, rq.ev_pyr, 0));
    const MsArgs a{d_orig, S->rc.rgb.p, so, row, w, h, rq.pyr_o, q.pyr_c.p, q.ms_part.p,
                   q.ms_out.p};
    launch_msssim(a, s);
    JXG_HIP(hipGetLastError());
    JXG_HIP(hipMemcpyAsync(rq.h[kRiderMsssim], q.ms_out.p, 2 * kMsScales * sizeof(double),
                           hipMemcpyDeviceToHost, s));
    JXG_HIP(hipMemcpyAsync(rq.h_q + 1, q.ms_out.p, sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (rq.h[kRiderReport]) {
    const jxg_status sr = strategy_report_enqueue(S, w, h);
    if (sr) return sr;
    JXG_HIP(hipMemcpyAsync(rq.h[kRiderReport], q.rep.p, kReportCells * sizeof(uint64_t),
                           hipMemcpyDeviceToHost, s));
  }
  if (rq.h[kRiderRates] || rq.ab) {
    const jxg_status sr = sweep_rate_enqueue(S, rq, w, h);
    if (sr) return sr;
  }
  if (rq.ab) {
    const jxg_status sr = sweep_ab_enqueue(S, rq, w, h);
    if (sr) return sr;
  }
  JXG_HIP(hipMemcpyAsync(rq.h_q, q.sse.p, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  JXG_HIP(hipEventRecord(rq.ev[2], s));
  return JXG_OK;
}

// the riders' rules (jxg_ctx.h), in the order of enum Rider
static_assert(sizeof(jxg_strategy_report) == kReportCells * 8, "copied as it is staged");
static_assert(sizeof(jxg_ab_report) == kAbWords * 8, "copied as it is staged");
static_assert(sizeof(jxg_trace_summary) == kTraceWords * 8, "copied as it is staged");
const RiderRule kRiderRules[kRiders] = {
    {2, 2 * kMsScales, sizeof(jxg_msssim)},
    {1, kReportCells, sizeof(jxg_strategy_report)},
    {0, kRateWords, sizeof(RateReport)},
    {1, kAbWords, sizeof(jxg_ab_report)},
    {0, kTraceWords, sizeof(jxg_trace_summary)},
};
// a point's staged words to its public struct (words null: MS-SSIM under kMsMinEdge)
static void rider_convert(int r, uint32_t w, uint32_t h, const uint64_t* words, void* out) {
  double sums[2 * kMsScales];  // (the window sums' bits, as h_q[1] carries the SSIM sum's)
  switch (r) {
    case kRiderMsssim:
      if (!words) return msssim_nan(static_cast<jxg_msssim*>(out));
      std::memcpy(sums, words, sizeof(sums));
      return msssim_result(w, h, sums, static_cast<jxg_msssim*>(out));
    case kRiderRates:
      return rate_from_words(words, static_cast<RateReport*>(out));
    default:
      std::memcpy(out, words, kRiderRules[r].out_bytes);
  }
}

static bool point_ok(const jxg_sweep_point& p) {  // as ctx_create checks its parameters
  if (!(p.distance > 0.0f) || p.distance > 25.0f) return false;
  if (p.effort < 1 || p.effort > 10) return false;
  if (p.proposals & ~3u) return false;
  return !(p.flags & JXG_FLAG_KEEP_MAPS);  // (maps are a one-at-a-time context's)
}

jxg_status sweep(Ctx* c, const uint8_t* src, bool on_device, uint32_t w, uint32_t h, size_t stride,
                 const jxg_sweep_point* points, uint32_t n, int quality, jxg_buffer* outs,
                 jxg_quality* q, jxg_status* statuses) {
  const Clock::time_point t0 = Clock::now();
  if (pipe_busy(c)) return JXG_ERR_INVALID_ARG;  // (nothing touched)
  // jxg_set_sweep_ab names the base points of sweeps of exactly its n
  if (!c->sw.ab_base.empty() && c->sw.ab_base.size() != n) return JXG_ERR_INVALID_ARG;
  std::vector<jxg_status> st(n, JXG_OK);
  std::vector<uint32_t> valid;
  jxg_status first = JXG_OK;
  for (uint32_t i = 0; i < n; i++) {
    outs[i] = jxg_buffer{nullptr, 0};
    if (q) q[i] = jxg_quality{};
    if (point_ok(points[i])) {
      valid.push_back(i);
    } else {
      st[i] = JXG_ERR_INVALID_ARG;
      if (!first) first = st[i];
    }
  }
  const uint32_t nv = (uint32_t)valid.size();
  Ctx::Sweep& sw = c->sw;
  sw.stats = jxg_sweep_stats{};
  // which riders ride on this quality (their results exist), and which run:
  // MS-SSIM's kernels only for frames it is defined for, NaN results otherwise
  bool rides[kRiders], runs[kRiders];
  for (int r = 0; r < kRiders; r++) {
    Ctx::Sweep::RiderSlot& sl = sw.rider[r];
    rides[r] = runs[r] = sl.on && quality >= kRiderRules[r].min_quality;
    sl.have = false;
    sl.out.clear();
    if (rides[r]) sl.out.assign((size_t)n * kRiderRules[r].out_bytes, 0);
  }
  const bool ab = rides[kRiderAb];
  const bool ms_run = runs[kRiderMsssim] = rides[kRiderMsssim] && std::min(w, h) >= kMsMinEdge;
  // the context is lane 0 and encodes with its frames' points: its own
  // parameters are put back however the call ends
  const jxg_params saved = c->params;
  struct Restore {
    Ctx* c;
    jxg_params p;
    ~Restore() { c->params = p; }
  } restore{c, saved};
  // a failure of the call: the pipe is aborted by then; drop what it completed, and ours
  auto fail = [&](jxg_status e) {
    pipe_drop_done(c);
    for (uint32_t i = 0; i < n; i++) {
      out_release(outs[i].data);
      outs[i] = jxg_buffer{nullptr, 0};
      if (q) q[i] = jxg_quality{};
      if (statuses) statuses[i] = e;
    }
    sw.stats.ms_call = ms_since(t0);
    for (Ctx::Sweep::RiderSlot& sl : sw.rider) sl.out.clear();
    return e;
  };
  if (nv) {
    const uint8_t* d = src;
    if (!on_device) {  // the one upload every point reads
      const Clock::time_point tu = Clock::now();
      const size_t bytes = stride * (h - 1) + (size_t)w * 3;
      if (sw.rgb.ensure(bytes) != hipSuccess) return fail(JXG_ERR_OOM);
      if (hipMemcpyAsync(sw.rgb.p, src, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
          hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(JXG_ERR_HIP);
      d = sw.rgb.p;
      sw.stats.ms_upload = ms_since(tu);
    }
    if (quality) {
      if (sw.h_q.ensure((size_t)nv * 2) != hipSuccess) return fail(JXG_ERR_OOM);
      while (sw.ev.size() < (size_t)nv * 3) {
        hipEvent_t e = nullptr;
        if (make_event(&e, 0) != hipSuccess) return fail(JXG_ERR_HIP);
        sw.ev.push_back(e);
      }
    }
    for (int r = 0; r < kRiders; r++)
      if (runs[r] && sw.rider[r].h.ensure((size_t)nv * kRiderRules[r].words) != hipSuccess)
        return fail(JXG_ERR_OOM);
    // A/B: the comparisons whose two points are both valid, a snapshot slot and
    // an event per distinct baseline (by its position among the valid points)
    std::vector<int32_t> ab_of, ab_slot;  // per valid point: its baseline's position; its slot
    if (ab) {
      std::vector<int32_t> pos(n, -1);
      for (uint32_t k = 0; k < nv; k++) pos[valid[k]] = (int32_t)k;
      ab_of.assign(nv, -1);
      ab_slot.assign(nv, -1);
      uint32_t nslots = 0;
      for (uint32_t k = 0; k < nv; k++) {
        const int32_t bi = sw.ab_base[valid[k]];
        if (bi < 0 || pos[bi] < 0) continue;  // (a refused baseline: the report stays zero)
        ab_of[k] = pos[bi];
        if (ab_slot[pos[bi]] < 0) ab_slot[pos[bi]] = (int32_t)nslots++;
      }
      const size_t snap = kAbSnapBytes * ((size_t)((w + 7) / 8) * ((h + 7) / 8));
      while (sw.ab_snap.size() < nslots) sw.ab_snap.emplace_back(new DevBuf<uint8_t>());
      for (uint32_t j = 0; j < nslots; j++)
        if (sw.ab_snap[j]->ensure(snap) != hipSuccess) return fail(JXG_ERR_OOM);
      while (sw.ab_ev.size() < nslots) {
        hipEvent_t e = nullptr;
        if (make_event(&e, hipEventDisableTiming) != hipSuccess) return fail(JXG_ERR_HIP);
        sw.ab_ev.push_back(e);
      }
    }
    if (ms_run) {  // the original's pyramid, once: every lane reads it after ev_pyr
      if (sw.pyr_o.ensure(ms_pyramid_floats(w, h)) != hipSuccess) return fail(JXG_ERR_OOM);
      if (!sw.ev_pyr && make_event(&sw.ev_pyr, hipEventDisableTiming) != hipSuccess)
        return fail(JXG_ERR_HIP);
      if (on_device) {
        const jxg_status so = order_input(c, c);
        if (so) return fail(so);
      }
      launch_ms_pyramid(d, stride, w, h, sw.pyr_o.p, c->stream);
      if (hipGetLastError() != hipSuccess || hipEventRecord(sw.ev_pyr, c->stream) != hipSuccess)
        return fail(JXG_ERR_HIP);
    }
    uint32_t got = 0;
    jxg_status e = JXG_OK;
    // point k's slice of rider r's staging
    auto slice = [&](int r, uint32_t k) {
      return sw.rider[r].h.p + (size_t)k * kRiderRules[r].words;
    };
    // valid point k has a result of rider r: A/B only where it compares, the
    // trace only where there is a search (the others' structs stay zero)
    auto has = [&](int r, uint32_t k) {
      if (r == kRiderAb) return ab_of[k] >= 0;
      if (r == kRiderTrace) return points[valid[k]].effort >= 5;
      return true;
    };
    // point valid[got]'s codestream (its completion event covers the quality
    // and riders' results) and its share of the timings
    auto take = [&]() {
      const uint32_t k = got++, i = valid[k];
      if ((e = pipe_receive(c, &outs[i]))) return;
      sw.stats.ms_encode += c->stats.ms_total;
      for (int r = 0; r < kRiders; r++) {
        if (!rides[r] || !has(r, k)) continue;
        rider_convert(r, w, h, runs[r] ? slice(r, k) : nullptr,
                      sw.rider[r].out.data() + (size_t)i * kRiderRules[r].out_bytes);
      }
      if (!quality) return;
      const uint64_t sse = sw.h_q.p[2 * k];
      double ssum;
      std::memcpy(&ssum, &sw.h_q.p[2 * k + 1], sizeof(ssum));
      const bool ssim = quality == 2 && ssim_partials(w, h) > 0;
      jxg_quality& o = q[i];  // (the expressions of compare_device)
      o.sse = sse;
      o.samples = (uint64_t)w * h * 3;
      o.mse = (double)sse / (double)o.samples;
      o.psnr = 10.0 * std::log10((255.0 * 255.0) / o.mse);
      o.ssim = ssim ? ssum / (3.0 * (double)(w - 10) * (double)(h - 10)) : NAN;
      sw.stats.ms_recon += elapsed(sw.ev[3 * k], sw.ev[3 * k + 1]);
      sw.stats.ms_metrics += elapsed(sw.ev[3 * k + 1], sw.ev[3 * k + 2]);
    };
    for (uint32_t k = 0; k < nv && !e; k++) {
      SweepReq rq;
      rq.params = saved;
      rq.params.distance = std::fmax(points[valid[k]].distance, JXG_MIN_DISTANCE);  // as ctx_create
      rq.params.effort = points[valid[k]].effort;
      rq.params.proposals = points[valid[k]].proposals;
      rq.params.flags = points[valid[k]].flags;
      rq.quality = quality;
      if (quality) {
        rq.h_q = sw.h_q.p + 2 * (size_t)k;
        rq.ev = sw.ev.data() + 3 * (size_t)k;
      }
      for (int r = 0; r < kRiders; r++)
        if (runs[r] && has(r, k)) rq.h[r] = slice(r, k);
      if (ms_run) {
        rq.pyr_o = sw.pyr_o.p;
        rq.ev_pyr = sw.ev_pyr;
      }
      if (ab && ab_slot[k] >= 0) {
        rq.ab = true;
        rq.ab_snap = sw.ab_snap[ab_slot[k]]->p;
        rq.ab_ev_snap = sw.ab_ev[ab_slot[k]];
      }
      if (ab && ab_of[k] >= 0) {
        rq.ab = true;
        rq.ab_base = sw.ab_snap[ab_slot[ab_of[k]]]->p;
        rq.ab_ev_base = sw.ab_ev[ab_slot[ab_of[k]]];
      }
      e = pipe_submit(c, d, true, w, h, stride, 0, 1, false, &rq);
      // completed points whose copies have landed (or when more than two wait)
      while (!e && pipe_done_ready(c)) take();
    }
    while (!e && got < nv) take();
    if (e) return fail(e);
  }
  const Frame f = make_frame(w, h, 1.0f);
  sw.stats.points = nv;
  sw.stats.lanes = pipe_shape(f.ngroups, f.tiles_x * f.tiles_y, c->lane_cap, hw_queues()).lanes;
  if (statuses) std::copy(st.begin(), st.end(), statuses);
  for (int r = 0; r < kRiders; r++) sw.rider[r].have = rides[r];
  sw.stats.ms_call = ms_since(t0);
  return first;
}

}  // namespace jxg
