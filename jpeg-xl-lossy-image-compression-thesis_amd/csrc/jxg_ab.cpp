// jxg_ab.cpp -- A/B report of two encodes of one image (jxg_ab.hip, DESIGN.md
// §3.18): each side's prepare step on its own stream, the transition kernel on
// side B's stream behind an event of side A's, and a sweep point's part.
#include <cstring>

#include "jxg_ctx.h"

namespace jxg {

static_assert(sizeof(jxg_ab_cell) == kAbCols * sizeof(uint64_t), "cell layout");
static_assert(sizeof(jxg_ab_report) == kAbWords * sizeof(uint64_t), "table layout");
static_assert(JXG_NUM_STRATEGIES == kAbStrategies, "strategy ids");

jxg_status ab_share_enqueue(Ctx* c, uint32_t w, uint32_t h) {
  const Frame f = make_frame(w, h, 1.0f);
  const uint32_t nb = f.bxs * f.bys;
  JXG_HIP(c->ab.share.ensure(nb));
  const AbShareArgs a{c->acs.p, c->rt.map.p, c->ab.share.p, f.bxs, nb};
  JXG_HIP(launch_ab_share(a, c->stream));
  return JXG_OK;
}

// one side of a one-at-a-time report, on c's own stream: the reconstruction
// chain ending in the block-map kernel (c->q.bsse), the rate kernel with its
// map (c->rt.map), the shares (c->ab.share)
static jxg_status ab_prepare(Ctx* c, const uint8_t* orig, size_t orig_stride, bool on_device) {
  jxg_status st = block_sse_enqueue(c, orig, orig_stride, on_device);
  if (!st) st = rate_map_ensure(c, c->rc.w, c->rc.h);
  if (!st) st = rate_enqueue(c, c->rc.w, c->rc.h, c->rt.map.p);
  if (!st) st = ab_share_enqueue(c, c->rc.w, c->rc.h);
  return st;
}

// the reduction on s: the table (cleared first) of `on`, and the delta planes
static jxg_status ab_reduce(Ctx* on, const uint8_t* acs_a, const uint32_t* sse_a,
                            const uint32_t* share_a, uint32_t w, uint32_t h, int32_t* d_delta) {
  const Frame f = make_frame(w, h, 1.0f);
  JXG_HIP(on->ab.table.ensure(kAbWords));
  JXG_HIP(hipMemsetAsync(on->ab.table.p, 0, kAbWords * sizeof(uint64_t), on->stream));
  const AbArgs a{acs_a,    on->acs.p, sse_a,        on->q.bsse.p, share_a, on->ab.share.p,
                 w,        h,         f.bxs,        f.bxs * f.bys, d_delta,
                 reinterpret_cast<unsigned long long*>(on->ab.table.p)};
  JXG_HIP(launch_ab_report(a, on->stream));
  return JXG_OK;
}

jxg_status ab_report_pair(Ctx* a, Ctx* b, const uint8_t* orig, size_t orig_stride, bool on_device,
                          jxg_ab_report* out, int32_t* block_delta) {
  if (a->params.device != b->params.device) return JXG_ERR_INVALID_ARG;
  // (the validity rule of jxg_reconstruct_rgb8 and jxg_rate_report, on both)
  if (!a->rc.ok || !a->rt.have || !b->rc.ok || !b->rt.have) return JXG_ERR_INVALID_ARG;
  const uint32_t w = a->rc.w, h = a->rc.h;
  if (b->rc.w != w || b->rc.h != h || orig_stride < (size_t)w * 3) return JXG_ERR_INVALID_ARG;
  const Frame f = make_frame(w, h, 1.0f);
  const size_t nb = (size_t)f.bxs * f.bys;
  jxg_status st = ab_prepare(a, orig, orig_stride, on_device);
  if (st) return st;
  if (a != b) {
    if ((st = ab_prepare(b, orig, orig_stride, on_device))) return st;
    // side B's stream goes on behind side A's prepare step: no host wait
    if (!a->ab.ev) JXG_HIP(make_event(&a->ab.ev, hipEventDisableTiming));
    JXG_HIP(hipEventRecord(a->ab.ev, a->stream));
    JXG_HIP(hipStreamWaitEvent(b->stream, a->ab.ev, 0));
  }
  int32_t* d_delta = nullptr;
  if (block_delta && on_device) {
    d_delta = block_delta;  // (ordered after the caller's stream by b's prepare step)
  } else if (block_delta) {
    JXG_HIP(b->ab.delta.ensure(2 * nb));
    d_delta = b->ab.delta.p;
  }
  if ((st = ab_reduce(b, a->acs.p, a->q.bsse.p, a->ab.share.p, w, h, d_delta))) return st;
  hipStream_t s = b->stream;
  JXG_HIP(hipMemcpyAsync(out, b->ab.table.p, sizeof(*out), hipMemcpyDeviceToHost, s));
  if (block_delta && !on_device)
    JXG_HIP(hipMemcpyAsync(block_delta, d_delta, 2 * nb * sizeof(int32_t), hipMemcpyDeviceToHost,
                           s));
  // b's stream ends behind a's: both sides' buffers are free again after this
  JXG_HIP(hipStreamSynchronize(s));
  return JXG_OK;
}

jxg_status sweep_ab_enqueue(Ctx* S, const SweepReq& rq, uint32_t w, uint32_t h) {
  hipStream_t s = S->stream;
  const Frame f = make_frame(w, h, 1.0f);
  const size_t nb = (size_t)f.bxs * f.bys;
  const jxg_status st = ab_share_enqueue(S, w, h);
  if (st) return st;
  if (rq.h[kRiderAb]) {
    // The baseline's event has been recorded by now: quality chains are
    // enqueued in submission order (pipe_complete_oldest) and the baseline
    // comes earlier in point order, so this is never a wait for an event
    // without a record (which would not wait at all).
    JXG_HIP(hipStreamWaitEvent(s, rq.ab_ev_base, 0));
    const uint32_t* sse_a = reinterpret_cast<const uint32_t*>(rq.ab_base);
    const jxg_status sr = ab_reduce(S, rq.ab_base + 8 * nb, sse_a, sse_a + nb, w, h, nullptr);
    if (sr) return sr;
    JXG_HIP(hipMemcpyAsync(rq.h[kRiderAb], S->ab.table.p, kAbWords * sizeof(uint64_t),
                           hipMemcpyDeviceToHost, s));
  }
  if (rq.ab_snap) {  // a baseline of later points: the lane's next frame overwrites the triple
    JXG_HIP(hipMemcpyAsync(rq.ab_snap, S->q.bsse.p, nb * 4, hipMemcpyDeviceToDevice, s));
    JXG_HIP(hipMemcpyAsync(rq.ab_snap + 4 * nb, S->ab.share.p, nb * 4, hipMemcpyDeviceToDevice, s));
    JXG_HIP(hipMemcpyAsync(rq.ab_snap + 8 * nb, S->acs.p, nb, hipMemcpyDeviceToDevice, s));
    JXG_HIP(hipEventRecord(rq.ab_ev_snap, s));
  }
  return JXG_OK;
}

}  // namespace jxg
