// jxg_trace.cpp -- the search trace of a traced encode (jxg_encode_traced_rgb8
// / jxg_search_trace): the buffers, the launches behind the
// encode's merge stage and the fetch.  A traced job is a search job (Job::trace)
// whose front kernel is the trace instantiation (jxg_front_trace.hip) and whose
// 128 / 256 px level evaluates every candidate in full (BigArgs::trace); what
// the encoder, the reconstruction and the reports read is written exactly as a
// plain encode writes it -- the trace lives in buffers of its own (Ctx::Trace).
#include <cstring>

#include "jxg_ctx.h"

namespace jxg {

static size_t trace_nb(uint32_t w, uint32_t h) {
  return (size_t)((w + 7) / 8) * ((h + 7) / 8);
}

jxg_status trace_alloc(Ctx* c, uint32_t w, uint32_t h) {
  const size_t nb = trace_nb(w, h);
  JXG_HIP(c->tr.f.ensure(nb * kTracePlanes));
  JXG_HIP(c->tr.b.ensure(nb * 3));
  JXG_HIP(c->tr.sum.ensure(kTraceSummaryWords));
  return JXG_OK;
}

void trace_front_args(Ctx* c, FrontArgs& fa) {
  static_assert(kTraceRaw == 0 && kTraceCmp == 6, "tr_est: the raw planes, then the compared ones");
  fa.tr_est = c->tr.f.p;
  fa.tr_ids = c->tr.b.p;  // scan8, front8
}

jxg_status trace_copy_qf(Ctx* c, const Job& J) {
  const size_t nb = (size_t)J.f.bxs * J.f.bys;
  JXG_HIP(hipMemcpyAsync(c->tr.b.p + 2 * nb, c->qf.p, nb, hipMemcpyDeviceToDevice, c->stream));
  return JXG_OK;
}

jxg_status trace_enqueue(Ctx* c, const Job& J) {
  const Frame& f = J.f;
  const size_t nb = (size_t)f.bxs * f.bys;
  // the planes index big_cost by pass group: a traced job is a whole frame
  if (J.big && (J.ba.glist || J.ba.g0 || J.ba.ng != f.gxs * f.gys)) return JXG_ERR_INTERNAL;
  TraceArgs a{};
  a.mcost = J.max_s ? c->mcost.p : nullptr;
  a.big_cost = J.big ? c->big_cost.p : nullptr;
  a.ent = J.max_s ? c->ent.p : nullptr;
  a.acs = c->acs.p;
  a.bxs = f.bxs;
  a.bys = f.bys;
  a.tiles_x = f.tiles_x;
  a.gxs = f.gxs;
  a.ngroups = J.big ? J.ba.ng : 0;
  a.max_s = J.max_s;
  a.max_px = J.big ? 256u : 8u * (uint32_t)J.max_s;
  a.cand8_raw = c->tr.f.p + kTraceRaw * nb;
  a.cand8 = c->tr.f.p + kTraceCmp * nb;
  a.scan8 = c->tr.b.p;
  a.front8 = c->tr.b.p + nb;
  a.merged = c->tr.f.p + kTraceMerged * nb;
  a.big = c->tr.f.p + kTraceBig * nb;
  a.chosen = c->tr.f.p + kTraceChosen * nb;
  a.summary = c->tr.sum.p;
  JXG_HIP(launch_trace(a, c->stream));
  return JXG_OK;
}

// (no host wait: the frame's completion event covers the copy, and the lane's
// next traced frame clears tr.sum behind it in stream order)
jxg_status sweep_trace_enqueue(Ctx* lane, const SweepReq& rq) {
  static_assert(kTraceWords * 8 == sizeof(jxg_trace_summary), "staged as 8-byte words");
  JXG_HIP(hipMemcpyAsync(rq.h[kRiderTrace], lane->tr.sum.p, sizeof(jxg_trace_summary),
                         hipMemcpyDeviceToHost, lane->stream));
  return JXG_OK;
}

jxg_status search_trace(Ctx* c, jxg_trace_maps* maps, jxg_trace_summary* summary) {
  if (!c->rc.ok || !c->tr.have || c->tr.w != c->rc.w || c->tr.h != c->rc.h)
    return JXG_ERR_INVALID_ARG;
  const size_t nb = trace_nb(c->tr.w, c->tr.h);
  hipStream_t s = c->stream;
  auto f32 = [&](float* dst, size_t plane, size_t n) -> hipError_t {
    return dst ? hipMemcpyAsync(dst, c->tr.f.p + plane * nb, n * nb * 4, hipMemcpyDeviceToHost, s)
               : hipSuccess;
  };
  auto u8 = [&](uint8_t* dst, size_t plane) -> hipError_t {
    return dst ? hipMemcpyAsync(dst, c->tr.b.p + plane * nb, nb, hipMemcpyDeviceToHost, s)
               : hipSuccess;
  };
  if (maps) {
    JXG_HIP(f32(maps->cand8_raw, kTraceRaw, 6));
    JXG_HIP(f32(maps->cand8, kTraceCmp, 6));
    JXG_HIP(f32(maps->merged, kTraceMerged, 9));
    JXG_HIP(f32(maps->big, kTraceBig, 6));
    JXG_HIP(f32(maps->chosen, kTraceChosen, 1));
    JXG_HIP(u8(maps->scan8, 0));
    JXG_HIP(u8(maps->front8, 1));
    JXG_HIP(u8(maps->qf8, 2));
  }
  uint32_t words[kTraceSummaryWords];
  if (summary)
    JXG_HIP(hipMemcpyAsync(words, c->tr.sum.p, sizeof(words), hipMemcpyDeviceToHost, s));
  JXG_HIP(hipStreamSynchronize(s));
  if (summary) {
    static_assert(sizeof(jxg_trace_summary) == sizeof(words), "jxg_trace_summary is the kernel's words");
    std::memcpy(summary, words, sizeof(words));
  }
  return JXG_OK;
}

}  // namespace jxg
