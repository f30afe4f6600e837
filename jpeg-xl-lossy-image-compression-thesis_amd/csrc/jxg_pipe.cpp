// jxg_pipe.cpp -- streaming encode (jxg_submit_rgb8[_device] / jxg_receive,
// jxg_shard_submit_device / jxg_shard_next_head / jxg_shard_write_next): a
// software pipeline over lanes (the caller's context plus lanes it owns, one
// stream each), driven by the caller's one host thread.  A frame's rANS chains last
// as long as its longest pass group's whatever the frame size, and a lane's
// stream is held by a frame from its front end to its assembly, so the
// frames in flight -- not the GPU's throughput -- bound small frames
// (profiles/r04f: ms per 1080p frame falls as 1 / lanes up to the 12 lanes
// the hardware queues allow).  So a lane carries a SUPER-FRAME: up to
// kMaxBatch frames of one size in slots (contexts with their own buffers
// sharing the lane's stream) that go through every per-frame kernel as one
// batched launch (blockIdx.z = the frame): front end, merge stage,
// statistics, then -- once a helper thread has built the codes of every
// frame of the batch -- rANS chains + bit placement and LF streams.  submit:
//   the frame joins the open batch (a free lane's next slot; completing the
//   oldest frames frees one) -> a full batch (or one of another size) is
//   launched, its codes queued on the helper threads; the last helper to
//   finish launches the batch's emission.
// Frames complete in submission order (deferred finish: layout, concat and
// the codestream's D2H enqueued; jxg_receive waits for the copy).  ~3570 pass
// groups in flight: 8K 7 lanes x 1, 1080p 12 lanes x 4.  Every lane needs
// its own hardware queue (GPU_MAX_HW_QUEUES > lanes, bench.py sets 16).
// The shape (lanes x batch) is pipe_shape, jxg_plan.h.
#include <atomic>
#include <cstring>
#include <deque>
#include <future>

#include "jxg_ctx.h"
#include "jxg_helpers.h"

namespace jxg {

static_assert(kPipeMaxBatch == kMaxBatch, "pipe_shape batches what one launch takes");

// a completed frame: its codestream (pinned host block) and stats; `ev`: the
// codestream's D2H, still in flight when the frame was completed (deferred
// finish) -- jxg_receive waits for it
struct PipeDone {
  jxg_buffer buf;
  jxg_stats stats;
  hipEvent_t ev;
};
struct PipeBatch;
struct PipeFrame {
  Ctx* lane = nullptr;   // the frame's slot (its buffers; the lane's stream)
  Ctx* owner = nullptr;  // the lane
  std::shared_ptr<PipeBatch> batch;
  Job J;
  int phase = 0;  // 0: in the open batch; 1: statistics launched; 2: emission launched
  bool shard = false;
  Clock::time_point t0;
  const uint8_t* src = nullptr;  // the device input (phase 0)
  uint32_t w = 0, h = 0, rank = 0, world = 1;
  size_t stride = 0;
  std::future<jxg_status> codes;  // valid while a helper builds the codes
  bool sweep = false;  // a sweep's frame: its point (the lane's parameters) and quality request
  SweepReq rq;
  bool traced = false;  // a sweep's frame that carries the trace slice: a traced job, alone in its batch
};
// frames launched together on one lane; the last of their codes launches the
// batch's emission
struct PipeBatch {
  Ctx* owner = nullptr;
  uint32_t w = 0, h = 0, rank = 0, world = 1;
  bool shard = false;
  jxg_params params{};  // of every frame of the batch (one distance / effort per launch)
  std::vector<PipeFrame*> frames;
  std::atomic<int> left{0};         // codes not yet built
  std::atomic<int> err{JXG_OK};     // a frame's codes or the emission failed
};
// the codes of frame fr of its batch (a helper thread, or inline); the
// batch's last one launches the emission of all its frames
static jxg_status pipe_codes(PipeFrame* fr) {
  PipeBatch& B = *fr->batch;
  jxg_status st = stage_codes(fr->lane, fr->J);
  if (st) B.err.store(st);
  if (B.left.fetch_sub(1) == 1 && !B.err.load()) {
    std::vector<Ctx*> cs;
    std::vector<Job*> js;
    for (PipeFrame* q : B.frames) {
      cs.push_back(q->lane);
      js.push_back(&q->J);
    }
    const jxg_status e = launch_emit(cs.data(), js.data(), (uint32_t)cs.size(), true);
    if (e) B.err.store(e);
  }
  return st;
}
// the helper's codes of a frame -> phase 2 (on an error the caller aborts)
static jxg_status pipe_join_codes(PipeFrame& fr) {
  jxg_status st = JXG_OK;
  if (fr.codes.valid()) {
    st = fr.codes.get();
    fr.phase = 2;
  }
  if (!st && fr.batch) st = (jxg_status)fr.batch->err.load();
  return st;
}
constexpr int kPipeHelpers = 6;  // codes of a batch (<= kMaxBatch) and the next one's in parallel

struct Pipe {
  std::vector<std::unique_ptr<PipeFrame>> inflight;  // submission order
  std::vector<PipeDone> done;                        // submission order
  std::vector<hipEvent_t> evfree;                    // PipeDone::ev pool
  // shard frames whose sections are emitted and payload head built; each
  // holds its lane (sections in lane->out) until jxg_shard_write_next
  std::vector<std::unique_ptr<PipeFrame>> ready;
  uint64_t submitted = 0;
  int mode = 0;  // 1 whole frames, 2 shards (while any frame is pending)
  uint32_t depth = 0;  // frames in flight (lanes x batch)
  std::shared_ptr<PipeBatch> open;   // frames submitted, not yet launched
  std::deque<hipEvent_t> writes;    // jxg_shard_write_next copies in flight, oldest first
  std::unique_ptr<Helpers> helpers;  // created with the first helper task
  ~Pipe() {
    for (auto& d : done)
      if (d.ev) {
        (void)hipEventSynchronize(d.ev);  // its D2H writes the codestream block
        (void)hipEventDestroy(d.ev);
      }
    for (hipEvent_t e : evfree) (void)hipEventDestroy(e);
  }
};
void PipeDeleter::operator()(Pipe* p) const { delete p; }

// the oldest completed frame's codestream is on the host (its D2H done)
static jxg_status pipe_done_wait(Pipe& p, PipeDone& d) {
  if (!d.ev) return JXG_OK;
  const hipError_t e = hipEventSynchronize(d.ev);
  p.evfree.push_back(d.ev);
  d.ev = nullptr;
  return e == hipSuccess ? JXG_OK : JXG_ERR_HIP;
}
// drop every completed frame (their D2H copies finish first)
void pipe_drop_done(Ctx* c) {
  if (!c->pipe) return;
  Pipe& p = *c->pipe;
  for (auto& d : p.done) {
    (void)pipe_done_wait(p, d);
    out_release(d.buf.data);
  }
  p.done.clear();
}
bool pipe_busy(const Ctx* c) {
  return c->pipe && (!c->pipe->inflight.empty() || !c->pipe->done.empty() ||
                     !c->pipe->ready.empty());
}
uint32_t pipe_pending(const Ctx* c) {
  return c->pipe ? (uint32_t)(c->pipe->inflight.size() + c->pipe->done.size() +
                              c->pipe->ready.size())
                 : 0u;
}

static jxg_status ensure_lanes(Ctx* c, uint32_t extra) {
  while (c->lanes.size() < extra) {
    Ctx* l = nullptr;
    const jxg_status st = ctx_new_lane(c->params, &l);
    if (st) return st;
    c->lanes.emplace_back(l);
  }
  return JXG_OK;
}
// slot i of lane L (0: the lane itself; others share its stream)
static jxg_status ensure_slots(Ctx* L, uint32_t k) {
  while (L->slots.size() + 1 < k) {
    Ctx* q = new (std::nothrow) Ctx();
    if (!q) return JXG_ERR_OOM;
    q->params = L->params;
    q->owned_lane = true;
    q->shared_stream = true;
    q->stream = L->stream;
    L->slots.emplace_back(q);
    for (auto& e : q->ev)
      if (make_event(&e, 0) != hipSuccess) return JXG_ERR_HIP;
  }
  return JXG_OK;
}
static Ctx* lane_slot(Ctx* L, uint32_t i) { return i == 0 ? L : L->slots[i - 1].get(); }

// drop every frame in flight (after an error): wait for the helpers and the
// lanes' streams
void pipe_abort(Ctx* c) {
  Pipe& p = *c->pipe;
  p.open.reset();
  for (auto& fr : p.inflight) (void)pipe_join_codes(*fr);
  for (auto& fr : p.inflight) (void)hipStreamSynchronize(fr->lane->stream);
  for (auto& fr : p.ready) (void)hipStreamSynchronize(fr->lane->stream);
  for (auto& fr : p.inflight)  // codestreams of frames whose assembly had started
    if (fr->J.host_out) {
      out_release(fr->J.host_out);
      fr->J.host_out = nullptr;
    }
  p.inflight.clear();
  p.ready.clear();
}

// a shard frame's stats (its lane's) once its sections are emitted
static void shard_frame_stats(PipeFrame& fr, size_t bytes) {
  jxg_stats& S = fr.lane->stats;
  S = jxg_stats{};
  S.xsize = fr.J.w;
  S.ysize = fr.J.h;
  S.num_groups = fr.J.f.ngroups;
  S.num_lf_groups = fr.J.f.nlf;
  S.bytes = bytes;
  S.ms_front_kernel = elapsed(fr.lane->ev[kEvFrontStart], fr.lane->ev[kEvFrontDone]);
  S.ms_aq = elapsed(fr.lane->ev[kEvStart], fr.lane->ev[kEvFrontStart]);
  S.ms_front = elapsed(fr.lane->ev[kEvStart], fr.lane->ev[kEvMerged]);
  S.ms_host_codes = fr.J.ms_codes;
  S.ms_host_call = ms_since(fr.t0);
}

// the open batch -> launched: every frame's plan and buffers, the batched
// front end / merge / statistics kernels, the frames' codes queued on the
// helper threads (inline without threads: codes, then the emission)
static jxg_status pipe_launch_open(Ctx* c) {
  Pipe& p = *c->pipe;
  std::shared_ptr<PipeBatch> B = std::move(p.open);
  p.open.reset();
  if (!B || B->frames.empty()) return JXG_OK;
  const uint32_t k = (uint32_t)B->frames.size();
  std::vector<Ctx*> cs;
  std::vector<Job*> js;
  for (PipeFrame* fr : B->frames) {
    jxg_status st = JXG_OK;
    // a sweep's traced point (pipe_submit: alone in its batch): the slot's trace
    // buffers, before the argument blocks point into them.  The Job is the
    // frame's own, so every other frame of the slot is a plain one
    if (fr->traced) {
      if ((st = trace_alloc(fr->lane, fr->w, fr->h))) return st;
      fr->J.trace = true;
    }
    st = enc_prepare(fr->lane, fr->J, fr->src, fr->w, fr->h, fr->stride, fr->rank, fr->world);
    if (st) return st;
    cs.push_back(fr->lane);
    js.push_back(&fr->J);
  }
  jxg_status st = launch_stats(cs.data(), js.data(), k);
  if (st) return st;
  for (PipeFrame* fr : B->frames)  // the summary, behind trace_enqueue on the lane's stream
    if (fr->traced && (st = sweep_trace_enqueue(fr->lane, fr->rq))) return st;
  B->left.store((int)k);
  for (PipeFrame* fr : B->frames) fr->phase = 1;
  try {
    if (!p.helpers) p.helpers.reset(new Helpers(c->params.device, kPipeHelpers));
    for (PipeFrame* fr : B->frames) fr->codes = p.helpers->run([fr]() { return pipe_codes(fr); });
  } catch (...) {  // no thread: the codes (and the emission) on this one
    for (PipeFrame* fr : B->frames) {
      if (fr->codes.valid()) continue;
      if ((st = pipe_codes(fr))) return st;
      fr->phase = 2;
    }
  }
  return JXG_OK;
}

// oldest frame in flight -> done (a whole frame: assembled, codestream on
// the host) or ready (a shard: sections emitted, payload head built); on an
// error the caller aborts the pipe
static jxg_status pipe_complete_oldest(Ctx* c) {
  Pipe& p = *c->pipe;
  jxg_status st = JXG_OK;
  if (p.inflight.front()->phase == 0 && (st = pipe_launch_open(c))) return st;
  PipeFrame& fr = *p.inflight.front();
  // every frame of its batch: the last codes launch the batch's emission
  // (the batch's frames are the oldest in flight, consecutive)
  for (size_t i = 0; i < p.inflight.size() && p.inflight[i]->batch == fr.batch; i++) {
    const jxg_status e = pipe_join_codes(*p.inflight[i]);
    if (!st) st = e;
  }
  if (fr.shard) {
    size_t bytes = 0;
    if (!st) st = shard_finish(fr.lane, fr.J, &bytes, false);
    if (st) return st;
    shard_frame_stats(fr, bytes);
    p.ready.push_back(std::move(p.inflight.front()));
    p.inflight.erase(p.inflight.begin());
    return JXG_OK;
  }
  PipeDone d{{nullptr, 0}, {}, nullptr};
  if (fr.lane->params.flags & JXG_FLAG_KEEP_MAPS) {
    if (!st) st = enc_finish(fr.lane, fr.J, false, &d.buf, fr.t0);
  } else if (!st) {
    // deferred finish: layout, concat and the codestream's D2H are enqueued on
    // the lane's stream and the lane is free at once (the next frame's work
    // queues behind them); only jxg_receive waits for the D2H.  Saves this
    // thread one GPU round trip per frame.
    if (p.evfree.empty()) {
      hipEvent_t e = nullptr;
      if (make_event(&e, hipEventDisableTiming) != hipSuccess) return JXG_ERR_HIP;
      p.evfree.push_back(e);
    }
    st = enc_finish_start(fr.lane, fr.J, false);
    // a sweep's quality: the lane's reconstruction chain and metrics behind the
    // codestream's copy, under the other lanes' chains; nothing waited for here
    if (!st && fr.sweep && fr.rq.quality)
      st = sweep_quality_enqueue(fr.lane, fr.rq, fr.J.d_rgb, fr.J.stride, fr.J.w, fr.J.h);
    else if (!st && fr.sweep && fr.rq.h[kRiderRates])  // (with quality: inside, ahead of ev[2])
      st = sweep_rate_enqueue(fr.lane, fr.rq, fr.J.w, fr.J.h);
    if (!st && hipEventRecord(p.evfree.back(), fr.lane->stream) != hipSuccess) st = JXG_ERR_HIP;
    if (st) {
      (void)hipStreamSynchronize(fr.lane->stream);
      out_release(fr.J.host_out);
      fr.J.host_out = nullptr;
      return st;
    }
    d.ev = p.evfree.back();
    p.evfree.pop_back();
    d.buf = jxg_buffer{fr.J.host_out, fr.J.out_bytes};
    fr.J.host_out = nullptr;
    enc_stats(fr.lane, fr.J, d.buf.size, fr.J.ms_finish_layout, false, nullptr, fr.t0);
  }
  if (st) return st;
  d.stats = fr.lane->stats;
  p.done.push_back(d);
  p.inflight.erase(p.inflight.begin());
  return JXG_OK;
}

static Ctx* pipe_lane(Ctx* c, uint32_t li) { return li == 0 ? c : c->lanes[li - 1].get(); }

// submit one frame (world == 1) or this rank's shard of one frame
jxg_status pipe_submit(Ctx* c, const uint8_t* src, bool on_device, uint32_t w, uint32_t h,
                       size_t stride, uint32_t rank, uint32_t world, bool shard,
                       const SweepReq* rq) {
  c->rc.ok = false;  // the lanes' frames overwrite this context's buffers
  if (!c->pipe) c->pipe.reset(new (std::nothrow) Pipe());
  if (!c->pipe) return JXG_ERR_OOM;
  Pipe& p = *c->pipe;
  const int mode = shard ? 2 : 1;
  if (pipe_busy(c) && p.mode != mode) return JXG_ERR_INVALID_ARG;  // one kind at a time
  // the frame's parameters: the context's, or a sweep's point.  The slot the
  // frame lands on is given them below, at every submit -- a slot is free by
  // then, and a sweep (which also uses the context itself as lane 0) puts the
  // context's own back when it ends
  jxg_params prm = c->params;
  if (rq) {
    prm.distance = rq->params.distance;
    prm.effort = rq->params.effort;
    prm.proposals = rq->params.proposals;
    prm.flags = rq->params.flags;
  }
  const Frame f0 = make_frame(w, h, prm.distance);
  uint32_t ngroups = f0.ngroups, ntiles = f0.tiles_x * f0.tiles_y;
  if (shard) {
    if (world < 1 || rank >= world || f0.ngroups < world || (world > 1 && f0.ngroups < 2))
      return JXG_ERR_INVALID_ARG;
    // no collective inside the pipeline: no record exchange, and with more
    // than one rank one HF preset per rank (ANS)
    const Plan P = make_plan(f0, rank, world);
    if (!P.x.send.empty() || !P.x.recv.empty() ||
        (world > 1 && !(prm.flags & JXG_FLAG_ANS)))
      return JXG_ERR_UNSUPPORTED;
    ngroups = P.ng();
    if (!P.tiles.empty()) ntiles = (uint32_t)P.tiles.size();
  }
  const PipeShape shape = pipe_shape(ngroups, ntiles, c->lane_cap, hw_queues());
  jxg_status st = ensure_lanes(c, shape.lanes - 1);
  if (st) return st;
  const Clock::time_point t0 = Clock::now();
  // a shard frame holds its slot until its sections are written: the caller
  // must take one first (jxg_shard_next_head / jxg_shard_write_next)
  if (shard && p.inflight.size() + p.ready.size() >= shape.pending()) return JXG_ERR_INVALID_ARG;
  p.mode = mode;
  p.depth = shape.frames();
  auto fail = [&](jxg_status e) {
    pipe_abort(c);
    return e;
  };
  // an open batch of another size / plan / point, or a full one, goes out
  // first (a batched launch carries one distance and one effort)
  const auto same_point = [](const jxg_params& a, const jxg_params& b) {
    return a.distance == b.distance && a.effort == b.effort && a.proposals == b.proposals &&
           a.flags == b.flags;
  };
  // a sweep's point with the trace slice and a search (effort >= 5) is a traced
  // job, which goes alone (batch_ok): the open batch goes out before it and it
  // is launched as soon as it is in
  const bool traced = rq && rq->h[kRiderTrace] && prm.effort >= 5;
  if (p.open && (p.open->w != w || p.open->h != h || p.open->rank != rank ||
                 p.open->world != world || !same_point(p.open->params, prm) ||
                 p.open->frames.size() >= shape.batch || traced))
    if ((st = pipe_launch_open(c))) return fail(st);
  if (!p.open) {
    // a free lane (no frame in flight or ready on it): complete the oldest
    // frames until one is
    Ctx* L = nullptr;
    for (;;) {
      for (uint32_t li = 0; li < shape.lanes && !L; li++) {
        Ctx* cand = pipe_lane(c, li);
        bool used = false;
        for (auto& q : p.inflight) used = used || q->owner == cand;
        for (auto& q : p.ready) used = used || q->owner == cand;
        if (!used) L = cand;
      }
      if (L) break;
      if (p.inflight.empty()) return shard ? JXG_ERR_INVALID_ARG : fail(JXG_ERR_INTERNAL);
      if ((st = pipe_complete_oldest(c))) return fail(st);
    }
    if ((st = ensure_slots(L, shape.batch))) return fail(st);
    p.open = std::make_shared<PipeBatch>();
    PipeBatch& B = *p.open;
    B.owner = L;
    B.w = w;
    B.h = h;
    B.rank = rank;
    B.world = world;
    B.shard = shard;
    B.params = prm;
  }
  PipeBatch& B = *p.open;
  std::unique_ptr<PipeFrame> fr(new (std::nothrow) PipeFrame());
  if (!fr) return fail(JXG_ERR_OOM);
  Ctx* S = lane_slot(B.owner, (uint32_t)B.frames.size());
  fr->lane = S;
  fr->owner = B.owner;
  fr->batch = p.open;
  fr->t0 = t0;
  fr->shard = shard;
  fr->w = w;
  fr->h = h;
  fr->stride = stride;
  fr->rank = rank;
  fr->world = world;
  if (rq) {
    fr->sweep = true;
    fr->rq = *rq;
    fr->traced = traced;
  }
  S->params = prm;
  if (!on_device) {
    // the slot's previous frame has completed, so its staging is free
    const size_t bytes = stride * (h - 1) + (size_t)w * 3;
    if (S->h_stage.ensure(bytes) != hipSuccess || S->rgb.ensure(bytes) != hipSuccess)
      return fail(JXG_ERR_OOM);
    std::memcpy(S->h_stage.p, src, bytes);
    if (hipMemcpyAsync(S->rgb.p, S->h_stage.p, bytes, hipMemcpyHostToDevice, S->stream) !=
        hipSuccess)
      return fail(JXG_ERR_HIP);
    src = S->rgb.p;
  } else if ((st = order_input(c, S))) {
    return fail(st);
  }
  fr->src = src;
  B.frames.push_back(fr.get());
  p.inflight.push_back(std::move(fr));
  p.submitted++;
  if ((B.frames.size() >= shape.batch || traced) && (st = pipe_launch_open(c))) return fail(st);
  // frames one per lane: this thread waits for the codes of frame j - lag
  // (their emission launched), which paces the launches by the codes and
  // rANS chains instead of filling every lane with transform work at once
  // (8K: +4 %, profiles/r04j); batched small frames are paced by their lanes
  if (shape.batch == 1) {
    const size_t lag = ngroups >= 256 ? 1 : 3;
    if (p.inflight.size() > lag) {
      PipeFrame& fj = *p.inflight[p.inflight.size() - 1 - lag];
      if (fj.phase >= 1 && (st = pipe_join_codes(fj))) return fail(st);
    }
  }
  return JXG_OK;
}

jxg_status pipe_receive(Ctx* c, jxg_buffer* out) {
  if (!c->pipe || c->pipe->mode != 1) return JXG_ERR_INVALID_ARG;
  Pipe& p = *c->pipe;
  if (p.done.empty()) {
    if (p.inflight.empty()) return JXG_ERR_INVALID_ARG;
    const jxg_status st = pipe_complete_oldest(c);
    if (st) {
      pipe_abort(c);
      return st;
    }
  }
  const jxg_status st = pipe_done_wait(p, p.done.front());
  if (st) return st;
  *out = p.done.front().buf;
  c->stats = p.done.front().stats;
  p.done.erase(p.done.begin());
  return JXG_OK;
}

bool pipe_done_ready(Ctx* c) {
  const std::vector<PipeDone>& done = c->pipe->done;
  return !done.empty() && (done.size() > 2 || !done.front().ev ||
                           hipEventQuery(done.front().ev) == hipSuccess);
}

jxg_status pipe_depth(const Ctx* c, uint32_t w, uint32_t h, uint32_t rank, uint32_t world,
                      uint32_t* depth) {
  const Frame f = make_frame(w, h, c->params.distance);
  const Plan P = make_plan(f, rank, world);
  const uint32_t nt = P.tiles.empty() ? f.tiles_x * f.tiles_y : (uint32_t)P.tiles.size();
  *depth = pipe_shape(world > 1 ? P.ng() : f.ngroups, nt, c->lane_cap, hw_queues()).pending();
  return JXG_OK;
}

// Batched encode (BASELINE config 3: 64 x 1080p) through the streaming
// pipeline (pipe_submit / pipe_receive): every frame is
// submitted in order and the codestreams already complete are collected after
// each submit, so the frames' transform kernels, rANS chains, host-side code
// construction (helper threads) and pinned H2D copies overlap over the
// pipeline's lanes.  Outputs are in frame order; the bytes of every frame equal
// jxg_encode_rgb8's.  The context must have no streamed frames pending.
jxg_status batch_encode(Ctx* c, const uint8_t* const* frames, bool on_device, uint32_t n,
                        uint32_t w, uint32_t h, size_t stride, jxg_buffer* outs) {
  for (uint32_t i = 0; i < n; i++) outs[i] = jxg_buffer{nullptr, 0};
  if (pipe_busy(c)) return JXG_ERR_INVALID_ARG;  // would interleave with the caller's stream
  uint32_t got = 0;
  jxg_status st = JXG_OK;
  for (uint32_t i = 0; i < n && !st; i++) {
    st = pipe_submit(c, frames[i], on_device, w, h, stride);
    // take completed frames whose codestream copy has landed (or when more
    // than two are waiting), without waiting on the newest one's
    while (!st && pipe_done_ready(c)) st = pipe_receive(c, &outs[got++]);
  }
  while (!st && got < n) st = pipe_receive(c, &outs[got++]);
  if (st) {  // the pipe is aborted by then; drop what it completed, and ours
    pipe_drop_done(c);
    for (uint32_t i = 0; i < n; i++) {
      out_release(outs[i].data);
      outs[i] = jxg_buffer{nullptr, 0};
    }
  }
  return st;
}

// streaming shards: the oldest pending shard frame, completed if needed
static jxg_status pipe_shard_oldest(Ctx* c, PipeFrame** fr) {
  if (!c->pipe || c->pipe->mode != 2) return JXG_ERR_INVALID_ARG;
  Pipe& p = *c->pipe;
  if (p.ready.empty()) {
    if (p.inflight.empty()) return JXG_ERR_INVALID_ARG;
    const jxg_status st = pipe_complete_oldest(c);
    if (st) {
      pipe_abort(c);
      return st;
    }
  }
  *fr = p.ready.front().get();
  return JXG_OK;
}

jxg_status shard_next_head(Ctx* c, uint32_t* dst, size_t* nwords) {
  PipeFrame* fr = nullptr;
  const jxg_status st = pipe_shard_oldest(c, &fr);
  if (st) return st;
  const std::vector<uint32_t>& hw = fr->lane->payload_head;
  if (dst) {
    if (*nwords < hw.size()) return JXG_ERR_INVALID_ARG;
    std::memcpy(dst, hw.data(), hw.size() * 4);
  }
  *nwords = hw.size();
  c->stats = fr->lane->stats;
  return JXG_OK;
}

jxg_status shard_write_next(Ctx* c, const uint32_t* const* heads, const size_t* head_words,
                            uint32_t n, uint8_t* dst, size_t dst_size, size_t* total) {
  PipeFrame* fr = nullptr;
  jxg_status st = pipe_shard_oldest(c, &fr);
  if (st) return st;
  Ctx* S = fr->lane;
  // the copies are enqueued, not waited for: this call returns once the
  // PREVIOUS frame's copies have landed (jxg_shard_write_flush: the last one's)
  st = shard_write_host(S, heads, head_words, n, dst, dst_size, total, false);
  if (st) return st;  // (too small a buffer: the frame stays, *total tells the size)
  if (!S->ev_write && make_event(&S->ev_write, hipEventDisableTiming) != hipSuccess)
    return JXG_ERR_HIP;
  Pipe& p = *c->pipe;
  // this slot's event may still be queued for an older write of the slot:
  // wait for that write's copies before its record is replaced, so the
  // promise below never rests on an incidental earlier synchronisation
  for (auto it = p.writes.begin(); it != p.writes.end();) {
    if (*it == S->ev_write) {
      JXG_HIP(hipEventSynchronize(*it));
      it = p.writes.erase(it);
    } else {
      ++it;
    }
  }
  JXG_HIP(hipEventRecord(S->ev_write, S->stream));
  p.ready.erase(p.ready.begin());  // its slot is free again (later work queues behind the copies)
  // the copies of the write JXG_SHARD_WRITE_LAG calls back have landed on return
  // (copy kernels queue behind the other lanes' kernels: waiting for the
  // previous frame's held this thread ~0.27 ms per frame, profiles/r04l)
  p.writes.push_back(S->ev_write);
  while (p.writes.size() > JXG_SHARD_WRITE_LAG) {
    const hipEvent_t e = p.writes.front();
    p.writes.pop_front();
    if (e) JXG_HIP(hipEventSynchronize(e));
  }
  return JXG_OK;
}

jxg_status shard_write_flush(Ctx* c) {
  if (c->pipe)
    while (!c->pipe->writes.empty()) {
      const hipEvent_t e = c->pipe->writes.front();
      c->pipe->writes.pop_front();
      if (e) JXG_HIP(hipEventSynchronize(e));
    }
  return JXG_OK;
}

}  // namespace jxg
