// jxg_ctx.cpp -- context lifetime, the shared device constants, the pinned
// output pool, events and the ordering of device inputs (jxg_ctx.h)
#include "jxg_ctx.h"

#include <atomic>
#include <cmath>
#include <cstdlib>

#include "jxg_front_tables.h"
#include "jxg_tables.h"

namespace jxg {

static_assert(kAnsHists == (uint32_t)kAnsMaxHists, "ANS table blob sized for kAnsMaxHists");

// Output codestreams live in pinned host blocks so the final D2H copy lands
// in the caller's buffer directly (no bounce copy, no first-touch page
// faults).  Blocks carry a small header and are recycled through a
// process-wide pool by jxg_buffer_free.
struct OutHeader {
  uint64_t magic;
  size_t cap;     // usable bytes after the header
  uint64_t heap;  // 1: plain heap block (host-only paths), 0: pinned
};
constexpr uint64_t kOutMagic = 0x6a78674f75744275ull;  // "jxgOutBu"
static std::mutex g_pool_mu;
static std::vector<uint8_t*> g_pool;  // free blocks (header addresses)

uint8_t* out_alloc(size_t bytes) {
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    size_t best = g_pool.size();
    for (size_t i = 0; i < g_pool.size(); i++) {
      const size_t cap = reinterpret_cast<OutHeader*>(g_pool[i])->cap;
      if (cap >= bytes && (best == g_pool.size() ||
                           cap < reinterpret_cast<OutHeader*>(g_pool[best])->cap))
        best = i;
    }
    if (best < g_pool.size()) {
      uint8_t* b = g_pool[best];
      g_pool.erase(g_pool.begin() + best);
      return b + kOutHdr;
    }
  }
  const size_t cap = std::max<size_t>(bytes + bytes / 8, 1 << 16);
  void* p = nullptr;
  if (hipHostMalloc(&p, cap + kOutHdr, hipHostMallocDefault) != hipSuccess) return nullptr;
  OutHeader* hd = static_cast<OutHeader*>(p);
  hd->magic = kOutMagic;
  hd->cap = cap;
  hd->heap = 0;
  return static_cast<uint8_t*>(p) + kOutHdr;
}

// host-only outputs (jxg_shard_assemble runs without a device)
uint8_t* out_alloc_heap(size_t bytes) {
  void* p = std::malloc(bytes + kOutHdr);
  if (!p) return nullptr;
  OutHeader* hd = static_cast<OutHeader*>(p);
  hd->magic = kOutMagic;
  hd->cap = bytes;
  hd->heap = 1;
  return static_cast<uint8_t*>(p) + kOutHdr;
}

// A codestream assembled at an offset inside its block (stage_concat_split:
// the AC block is copied first, the prefix lands right before it) carries a
// back reference to the block's data start in the kOutHdr bytes before it.
constexpr uint64_t kOutBackMagic = 0x6a7867426b526566ull;  // "jxgBkRef"
struct OutBackRef {
  uint64_t magic;
  uint8_t* data0;
};
void out_set_backref(uint8_t* data, uint8_t* data0) {
  if (data == data0) return;
  OutBackRef* r = reinterpret_cast<OutBackRef*>(data - kOutHdr);
  r->magic = kOutBackMagic;
  r->data0 = data0;
}

void out_release(uint8_t* data) {
  if (!data) return;
  if (reinterpret_cast<OutBackRef*>(data - kOutHdr)->magic == kOutBackMagic) {
    OutBackRef* r = reinterpret_cast<OutBackRef*>(data - kOutHdr);
    r->magic = 0;
    data = r->data0;
  }
  uint8_t* b = data - kOutHdr;
  if (reinterpret_cast<OutHeader*>(b)->magic != kOutMagic) return;  // not ours
  if (reinterpret_cast<OutHeader*>(b)->heap) {
    reinterpret_cast<OutHeader*>(b)->magic = 0;
    std::free(b);
    return;
  }
  std::lock_guard<std::mutex> lk(g_pool_mu);
  if (g_pool.size() < 8) {
    g_pool.push_back(b);
    return;
  }
  reinterpret_cast<OutHeader*>(b)->magic = 0;
  (void)hipHostFree(b);
}

void CtxDeleter::operator()(Ctx* c) const { ctx_destroy(c); }

std::mutex g_const_mu;
// Live contexts of the process.  A HIP process has 4 hardware queues
// (GPU_MAX_HW_QUEUES); with several contexts their second streams would
// share queues with other contexts' main streams, so the split assembly
// (stage_concat_split, second stream) is used by a lone context only.
static std::atomic<int> g_live_ctx{0};  // caller-created contexts (owned lanes excluded)
bool lone_context() { return g_live_ctx.load() <= 1; }

jxg_status init_constants(Ctx* c) {
  if (c->constants_ready) return JXG_OK;
  std::lock_guard<std::mutex> lock(g_const_mu);
  float lut[256];
  srgb_lut(lut);
  // front_kernel's tables, to each of its three translation units (the static
  // host tables outlive the copies: one synchronisation, below)
  static const FrontTables ft = [&lut] {
    float wts[5][3][64];
    quant_weights(wts);
    return build_front_tables(lut, wts);
  }();
  JXG_HIP(upload_front_tables_search(ft, c->stream));
  JXG_HIP(upload_front_tables_forced(ft, c->stream));
  JXG_HIP(upload_front_tables_trace(ft, c->stream));
  JXG_HIP(c->lut.ensure(256));
  JXG_HIP(hipMemcpyAsync(c->lut.p, lut, sizeof(lut), hipMemcpyHostToDevice, c->stream));
  uint8_t tab[kAcCtx];
  for (int i = 0; i < kAcCtx; i++) tab[i] = (uint8_t)ac_cluster(i);
  JXG_HIP(set_cluster_table(tab, c->stream));
  static const MergeTables mt = build_merge_tables();
  JXG_HIP(set_merge_constants(&mt.llf_p[0][0], &mt.llf_ib[0][0][0], c->stream));
  JXG_HIP(c->mwk.ensure(mt.wk.size()));
  JXG_HIP(c->msdk.ensure(mt.sdk.size()));
  JXG_HIP(c->miwy.ensure(mt.iwy.size()));
  JXG_HIP(c->mnat.ensure(mt.nat.size()));
  JXG_HIP(hipMemcpyAsync(c->mwk.p, mt.wk.data(), mt.wk.size() * 4, hipMemcpyHostToDevice, c->stream));
  JXG_HIP(hipMemcpyAsync(c->msdk.p, mt.sdk.data(), mt.sdk.size() * 4, hipMemcpyHostToDevice, c->stream));
  JXG_HIP(hipMemcpyAsync(c->miwy.p, mt.iwy.data(), mt.iwy.size() * 4, hipMemcpyHostToDevice, c->stream));
  JXG_HIP(hipMemcpyAsync(c->mnat.p, mt.nat.data(), mt.nat.size() * 2, hipMemcpyHostToDevice, c->stream));
  JXG_HIP(hipStreamSynchronize(c->stream));
  JXG_HIP(hipGetLastError());
  c->constants_ready = true;
  return JXG_OK;
}

// Host waits on the library's events (helper threads waiting for statistics,
// emission, codestream copies): JXG_EVENT_BLOCKING=1 makes them blocking-sync
// events (the waiting thread sleeps until the GPU signals) instead of the
// runtime's default active wait -- an A/B switch for the host-CPU budget of
// several ranks per node
hipError_t make_event(hipEvent_t* e, unsigned flags) {
  static const bool blocking = [] {
    const char* v = std::getenv("JXG_EVENT_BLOCKING");
    return v && v[0] == '1';
  }();
  return hipEventCreateWithFlags(e, flags | (blocking ? hipEventBlockingSync : 0u));
}

float elapsed(hipEvent_t a, hipEvent_t b) {
  float ms = 0.0f;
  (void)hipEventElapsedTime(&ms, a, b);
  return ms;
}

// Hardware queues of this process (GPU_MAX_HW_QUEUES as HIP read it at start
// up; HIP's default is 4).  The pipeline's depth never exceeds queues - 1
// (pipe_shape, jxg_plan.h): a caller that wants the full depth raises the
// variable (at most 32) before HIP initialises, as bench.py and
// tests/conftest.py do.
uint32_t hw_queues() {
  const char* e = std::getenv("GPU_MAX_HW_QUEUES");
  const long q = e && *e ? std::strtol(e, nullptr, 10) : 4;
  return (uint32_t)std::min<long>(32, std::max<long>(1, q));
}

// Device inputs (jxg_set_input_stream): `lane`'s stream is ordered after the
// work the caller has submitted to its input stream so far; without an input
// stream the caller's writes must be complete before the call (include/jxg.h).
jxg_status order_input(Ctx* owner, Ctx* lane) {
  if (!owner->in_stream) return JXG_OK;
  if (!lane->ev_in && make_event(&lane->ev_in, hipEventDisableTiming) != hipSuccess)
    return JXG_ERR_HIP;
  JXG_HIP(hipEventRecord(lane->ev_in, owner->in_stream));
  JXG_HIP(hipStreamWaitEvent(lane->stream, lane->ev_in, 0));
  return JXG_OK;
}

// a lane of another context (its own stream); not counted in g_live_ctx
jxg_status ctx_new_lane(const jxg_params& params, Ctx** out) {
  *out = nullptr;
  Ctx* c = new (std::nothrow) Ctx();
  if (!c) return JXG_ERR_OOM;
  c->params = params;
  c->owned_lane = true;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return JXG_ERR_HIP;
  }
  for (auto& e : c->ev)
    if (make_event(&e, 0) != hipSuccess) {
      ctx_destroy(c);
      return JXG_ERR_HIP;
    }
  *out = c;
  return JXG_OK;
}

jxg_status ctx_create(const jxg_params& requested, Ctx** out) {
  *out = nullptr;
  if (!(requested.distance > 0.0f) || requested.distance > 25.0f) return JXG_ERR_INVALID_ARG;
  jxg_params params = requested;  // the effective distance (jxg.h JXG_MIN_DISTANCE)
  params.distance = std::fmax(requested.distance, JXG_MIN_DISTANCE);
  if (params.effort < 1 || params.effort > 10) return JXG_ERR_INVALID_ARG;
  if (params.proposals & ~3u) return JXG_ERR_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return JXG_ERR_NO_DEVICE;
  if (params.device < 0 || params.device >= ndev) return JXG_ERR_INVALID_ARG;
  if (hipSetDevice(params.device) != hipSuccess) return JXG_ERR_HIP;
  const jxg_status st = ctx_new_lane(params, out);
  if (st) return st;
  (*out)->owned_lane = false;
  g_live_ctx++;
  return JXG_OK;
}

void ctx_destroy(Ctx* c) {
  if (!c) return;
  if (c->pipe) {  // frames still in the pipeline (their lanes are released below)
    pipe_abort(c);
    pipe_drop_done(c);
    c->pipe.reset();
  }
  (void)hipSetDevice(c->params.device);
  // written shard frames' section copies may still read a slot's buffers
  (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  c->lanes.clear();  // pipeline lanes (ctx_destroy each)
  c->slots.clear();  // their extra slots (sharing this context's stream)
  if (!c->owned_lane) g_live_ctx--;
#ifdef JXG_MERGE_PROFILE
  dump_merge_profile();
#endif
#ifdef JXG_FRONT_PROFILE
  dump_front_profile();
  dump_hist_profile();
#endif
  for (auto& e : c->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : c->dec.ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : c->decb.ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : c->sw.ev)
    if (e) (void)hipEventDestroy(e);
  if (c->sw.ev_pyr) (void)hipEventDestroy(c->sw.ev_pyr);
  for (auto& e : c->sw.ab_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->ab.ev) (void)hipEventDestroy(c->ab.ev);
  if (c->rc.ev_sigma) (void)hipEventDestroy(c->rc.ev_sigma);
  if (c->ev_in) (void)hipEventDestroy(c->ev_in);
  if (c->ev_write) (void)hipEventDestroy(c->ev_write);
  if (c->stream && !c->shared_stream) (void)hipStreamDestroy(c->stream);
  if (c->stream2) (void)hipStreamDestroy(c->stream2);
  delete c;
}

}  // namespace jxg
