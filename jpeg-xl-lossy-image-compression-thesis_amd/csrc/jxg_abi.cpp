// jxg_abi.cpp -- the C ABI (include/jxg.h): every entry point checks its
// arguments, makes the context's device current (ctx_enter) and calls one
// internal function.  (jxg_decode_info is jxg_decode.cpp's: it needs no device.)
#include <cstring>

#include "jxg_ctx.h"
#include "jxg_decode.h"

using namespace jxg;

// ---- a sweep's riders (kRiderRules): one switch, one getter ----
// a rider's switch (A/B: its base indices, none when off)
static jxg_status sweep_switch(jxg_ctx* ctx, Rider r, bool on, const int32_t* base = nullptr,
                               uint32_t n = 0) {
  if (!ctx) return JXG_ERR_INVALID_ARG;
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (pipe_busy(c)) return JXG_ERR_INVALID_ARG;
  return guarded([&] {
    if (r == kRiderAb) c->sw.ab_base.assign(base, base + (on ? n : 0));
    c->sw.rider[r].on = on;
    return JXG_OK;
  });
}

// a rider's results of the last sweep.  while_pending: jxg_sweep_msssim alone
// answers while frames are pending; the later getters refuse.  The difference
// is the ABI's as it stands and is kept here, not decided
template <class T>
static jxg_status sweep_results(jxg_ctx* ctx, Rider r, T* out, uint32_t n,
                                bool while_pending = false) {
  if (!ctx || !out) return JXG_ERR_INVALID_ARG;
  const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
  const Ctx::Sweep::RiderSlot& sl = c->sw.rider[r];
  if ((!while_pending && pipe_busy(c)) || !sl.have || (size_t)n * sizeof(T) != sl.out.size())
    return JXG_ERR_INVALID_ARG;
  std::memcpy(out, sl.out.data(), sl.out.size());
  return JXG_OK;
}

extern "C" {

const char* jxg_status_str(jxg_status s) {
  switch (s) {
    case JXG_OK: return "ok";
    case JXG_ERR_INVALID_ARG: return "invalid argument";
    case JXG_ERR_NO_DEVICE: return "no HIP device";
    case JXG_ERR_HIP: return "HIP runtime error";
    case JXG_ERR_OOM: return "out of memory";
    case JXG_ERR_UNSUPPORTED: return "unsupported";
    default: return "internal error";
  }
}

jxg_status jxg_create(const jxg_params* params, jxg_ctx** out) {
  if (!params || !out) return JXG_ERR_INVALID_ARG;
  return ctx_create(*params, reinterpret_cast<Ctx**>(out));
}

void jxg_destroy(jxg_ctx* ctx) { ctx_destroy(reinterpret_cast<Ctx*>(ctx)); }

jxg_status jxg_encode_rgb8_device(jxg_ctx* ctx, const void* d_rgb, uint32_t w, uint32_t h,
                                  size_t stride, jxg_buffer* out) {
  if (!ctx || !d_rgb || !out || !frame_args_ok(w, h, stride)) return JXG_ERR_INVALID_ARG;
  const Clock::time_point t0 = Clock::now();
  *out = jxg_buffer{nullptr, 0};
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : encode_one(c, static_cast<const uint8_t*>(d_rgb), true, w, h, stride, out, t0);
}

jxg_status jxg_encode_rgb8(jxg_ctx* ctx, const uint8_t* rgb, uint32_t w, uint32_t h, size_t stride,
                           jxg_buffer* out) {
  if (!ctx || !rgb || !out || !frame_args_ok(w, h, stride)) return JXG_ERR_INVALID_ARG;
  const Clock::time_point t0 = Clock::now();
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);  // (c->rgb may be an in-flight lane's input)
  if (st) return st;
  *out = jxg_buffer{nullptr, 0};
  return encode_one(c, rgb, false, w, h, stride, out, t0);
}

// forced encode: the map is validated (jxg_force.cpp) before the context is
// touched -- a refused map leaves the previous encode's state in place
static jxg_status encode_forced(jxg_ctx* ctx, const void* src, bool on_device, uint32_t w,
                                uint32_t h, size_t stride, const uint8_t* acs, const uint8_t* qf,
                                jxg_buffer* out) {
  if (out) *out = jxg_buffer{nullptr, 0};
  if (!ctx || !src || !acs || !out || !frame_args_ok(w, h, stride)) return JXG_ERR_INVALID_ARG;
  const Clock::time_point t0 = Clock::now();
  Ctx* c;
  jxg_status st = ctx_enter(ctx, true, &c);
  if (st) return st;
  uint32_t big_kinds = 0;  // the map's kinds of 128 / 256 px
  if ((st = check_strategy_map(acs, w, h, nullptr, &big_kinds))) return st;
  return encode_one(c, static_cast<const uint8_t*>(src), on_device, w, h, stride, out, t0, acs, qf,
                    false, big_kinds);
}

jxg_status jxg_encode_forced_rgb8(jxg_ctx* ctx, const uint8_t* rgb, uint32_t w, uint32_t h,
                                  size_t stride, const uint8_t* acs, const uint8_t* qf,
                                  jxg_buffer* out) {
  return encode_forced(ctx, rgb, false, w, h, stride, acs, qf, out);
}

jxg_status jxg_encode_forced_rgb8_device(jxg_ctx* ctx, const void* d_rgb, uint32_t w, uint32_t h,
                                         size_t stride, const uint8_t* acs, const uint8_t* qf,
                                         jxg_buffer* out) {
  return encode_forced(ctx, d_rgb, true, w, h, stride, acs, qf, out);
}

// traced encode (jxg_trace.cpp): a search encode that keeps its estimates;
// without a search (effort < 5) it is refused before the context is touched
static jxg_status encode_traced(jxg_ctx* ctx, const void* src, bool on_device, uint32_t w,
                                uint32_t h, size_t stride, jxg_buffer* out) {
  if (out) *out = jxg_buffer{nullptr, 0};
  if (!ctx || !src || !out || !frame_args_ok(w, h, stride)) return JXG_ERR_INVALID_ARG;
  const Clock::time_point t0 = Clock::now();
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  if (st) return st;
  if (c->params.effort < 5) return JXG_ERR_UNSUPPORTED;
  return encode_one(c, static_cast<const uint8_t*>(src), on_device, w, h, stride, out, t0, nullptr,
                    nullptr, true);
}

jxg_status jxg_encode_traced_rgb8(jxg_ctx* ctx, const uint8_t* rgb, uint32_t w, uint32_t h,
                                  size_t stride, jxg_buffer* out) {
  return encode_traced(ctx, rgb, false, w, h, stride, out);
}

jxg_status jxg_encode_traced_rgb8_device(jxg_ctx* ctx, const void* d_rgb, uint32_t w, uint32_t h,
                                         size_t stride, jxg_buffer* out) {
  return encode_traced(ctx, d_rgb, true, w, h, stride, out);
}

jxg_status jxg_search_trace(jxg_ctx* ctx, jxg_trace_maps* maps, jxg_trace_summary* summary) {
  if (!ctx) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : search_trace(c, maps, summary);
}

jxg_status jxg_encode_batch_rgb8(jxg_ctx* ctx, const uint8_t* const* rgbs, uint32_t n, uint32_t w,
                                 uint32_t h, size_t stride, jxg_buffer* outs) {
  if (!ctx || !rgbs || !outs || !frame_args_ok(w, h, stride)) return JXG_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < n; i++)
    if (!rgbs[i]) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, false, &c);
  return st ? st : batch_encode(c, rgbs, false, n, w, h, stride, outs);
}

jxg_status jxg_encode_batch_rgb8_device(jxg_ctx* ctx, const void* const* d_rgbs, uint32_t n,
                                        uint32_t w, uint32_t h, size_t stride,
                                        jxg_buffer* outs) {
  if (!ctx || !d_rgbs || !outs || !frame_args_ok(w, h, stride)) return JXG_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < n; i++)
    if (!d_rgbs[i]) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, false, &c);
  return st ? st
            : batch_encode(c, reinterpret_cast<const uint8_t* const*>(d_rgbs), true, n, w, h,
                           stride, outs);
}

jxg_status jxg_submit_rgb8_device(jxg_ctx* ctx, const void* d_rgb, uint32_t w, uint32_t h,
                                  size_t stride) {
  if (!ctx || !d_rgb || !frame_args_ok(w, h, stride)) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, false, &c);
  return st ? st : pipe_submit(c, static_cast<const uint8_t*>(d_rgb), true, w, h, stride);
}

jxg_status jxg_submit_rgb8(jxg_ctx* ctx, const uint8_t* rgb, uint32_t w, uint32_t h, size_t stride) {
  if (!ctx || !rgb || !frame_args_ok(w, h, stride)) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, false, &c);
  return st ? st : pipe_submit(c, rgb, false, w, h, stride);
}

jxg_status jxg_receive(jxg_ctx* ctx, jxg_buffer* out) {
  if (!ctx || !out) return JXG_ERR_INVALID_ARG;
  *out = jxg_buffer{nullptr, 0};
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, false, &c);
  return st ? st : pipe_receive(c, out);
}

jxg_status jxg_pending(jxg_ctx* ctx, uint32_t* n) {
  if (!ctx || !n) return JXG_ERR_INVALID_ARG;
  *n = pipe_pending(reinterpret_cast<Ctx*>(ctx));
  return JXG_OK;
}

jxg_status jxg_get_stats(jxg_ctx* ctx, jxg_stats* stats) {
  if (!ctx || !stats) return JXG_ERR_INVALID_ARG;
  *stats = reinterpret_cast<Ctx*>(ctx)->stats;
  return JXG_OK;
}

void jxg_buffer_free(jxg_buffer* buf) {
  if (!buf) return;
  out_release(buf->data);
  *buf = jxg_buffer{nullptr, 0};
}

jxg_status jxg_shard_sizes(uint32_t xsize, uint32_t ysize, uint32_t world, size_t* hist_words,
                           size_t* slot_bytes) {
  if (!hist_words || !slot_bytes || xsize == 0 || ysize == 0 || world == 0)
    return JXG_ERR_INVALID_ARG;
  *hist_words = (size_t)kMaxClusters * kAlpha + 4;  // + the varblocks per big kind
  *slot_bytes = exchange_slot_records(make_frame(xsize, ysize, 1.0f), world) * kGroupRecordBytes;
  return JXG_OK;
}

jxg_status jxg_shard_exchange(uint32_t xsize, uint32_t ysize, uint32_t world, uint32_t rank,
                              size_t* send_bytes, size_t* recv_bytes) {
  if (!send_bytes || !recv_bytes || xsize == 0 || ysize == 0 || world == 0 || rank >= world)
    return JXG_ERR_INVALID_ARG;
  const Frame f = make_frame(xsize, ysize, 1.0f);
  const Exchange X = make_exchange(f, make_partition(f, world), rank, world);
  for (uint32_t p = 0; p < world; p++) {
    send_bytes[p] = (size_t)X.nsend[p] * kGroupRecordBytes;
    recv_bytes[p] = (size_t)X.nrecv[p] * kGroupRecordBytes;
  }
  return JXG_OK;
}

jxg_status jxg_shard_begin(jxg_ctx* ctx, const void* d_rgb, uint32_t w, uint32_t h, size_t stride,
                           uint32_t rank, uint32_t world, uint32_t* d_hist, void* d_xbuf) {
  if (!ctx || !d_rgb || !d_hist || !d_xbuf || !frame_args_ok(w, h, stride))
    return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st
            : shard_begin(c, static_cast<const uint8_t*>(d_rgb), w, h, stride, rank, world, d_hist,
                          static_cast<uint8_t*>(d_xbuf));
}

jxg_status jxg_shard_end(jxg_ctx* ctx, const uint32_t* d_hist, const void* d_xbuf,
                         size_t* payload_bytes) {
  if (!ctx || !d_hist || !d_xbuf || !payload_bytes) return JXG_ERR_INVALID_ARG;
  *payload_bytes = 0;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : shard_end(c, d_hist, static_cast<const uint8_t*>(d_xbuf), payload_bytes);
}

jxg_status jxg_shard_payload(jxg_ctx* ctx, void* dst, int dst_on_device) {
  if (!ctx || !dst) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : shard_payload(c, dst, dst_on_device != 0);
}

jxg_status jxg_shard_assemble_device(jxg_ctx* ctx, const void* d_payloads, const size_t* offsets,
                                     const size_t* sizes, uint32_t n, jxg_buffer* out) {
  if (!ctx || !d_payloads || !offsets || !sizes || !out || n == 0) return JXG_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < n; i++)
    if (offsets[i] % 4) return JXG_ERR_INVALID_ARG;
  *out = jxg_buffer{nullptr, 0};
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st
            : shard_assemble_device(c, static_cast<const uint8_t*>(d_payloads), offsets, sizes, n,
                                    out);
}

jxg_status jxg_shard_head(jxg_ctx* ctx, uint32_t* dst, size_t* nwords) {
  if (!ctx || !nwords) return JXG_ERR_INVALID_ARG;
  return shard_head(reinterpret_cast<Ctx*>(ctx), dst, nwords);
}

jxg_status jxg_shard_write_host(jxg_ctx* ctx, const uint32_t* const* heads, const size_t* head_words,
                                uint32_t n, void* dst, size_t dst_size, size_t* total) {
  if (!ctx || !heads || !head_words || !total || n == 0) return JXG_ERR_INVALID_ARG;
  *total = 0;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st
            : shard_write_host(c, heads, head_words, n, static_cast<uint8_t*>(dst), dst_size, total);
}

jxg_status jxg_host_register(void* ptr, size_t size) {
  if (!ptr || size == 0) return JXG_ERR_INVALID_ARG;
  return hipHostRegister(ptr, size, hipHostRegisterDefault) == hipSuccess ? JXG_OK : JXG_ERR_HIP;
}

jxg_status jxg_host_unregister(void* ptr) {
  if (!ptr) return JXG_ERR_INVALID_ARG;
  return hipHostUnregister(ptr) == hipSuccess ? JXG_OK : JXG_ERR_HIP;
}

jxg_status jxg_shard_assemble(const uint8_t* const* payloads, const size_t* sizes, uint32_t n,
                              jxg_buffer* out) {
  if (!out) return JXG_ERR_INVALID_ARG;
  *out = jxg_buffer{nullptr, 0};
  return shard_assemble(payloads, sizes, n, out);
}

jxg_status jxg_shard_plan(uint32_t xsize, uint32_t ysize, uint32_t world, uint32_t* group_owner,
                          uint32_t* lf_owner, int* kind) {
  if (world == 0 || !frame_args_ok(xsize, ysize, (size_t)xsize * 3)) return JXG_ERR_INVALID_ARG;
  const Frame f = make_frame(xsize, ysize, 1.0f);
  const Partition part = make_partition(f, world);
  if (group_owner) std::copy(part.group.begin(), part.group.end(), group_owner);
  if (lf_owner) std::copy(part.lf.begin(), part.lf.end(), lf_owner);
  if (kind) *kind = part.kind;
  return JXG_OK;
}

jxg_status jxg_set_input_stream(jxg_ctx* ctx, void* stream) {
  if (!ctx) return JXG_ERR_INVALID_ARG;
  reinterpret_cast<Ctx*>(ctx)->in_stream = static_cast<hipStream_t>(stream);
  return JXG_OK;
}

jxg_status jxg_pipeline_depth(jxg_ctx* ctx, uint32_t xsize, uint32_t ysize, uint32_t rank,
                              uint32_t world, uint32_t* depth) {
  if (!ctx || !depth || xsize == 0 || ysize == 0 || world == 0 || rank >= world)
    return JXG_ERR_INVALID_ARG;
  return pipe_depth(reinterpret_cast<Ctx*>(ctx), xsize, ysize, rank, world, depth);
}

jxg_status jxg_set_pipeline_lanes(jxg_ctx* ctx, uint32_t lanes) {
  if (!ctx || lanes > kPipeMaxLanes) return JXG_ERR_INVALID_ARG;
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (pipe_busy(c)) return JXG_ERR_INVALID_ARG;
  c->lane_cap = lanes;
  return JXG_OK;
}

jxg_status jxg_shard_submit_device(jxg_ctx* ctx, const void* d_rgb, uint32_t w, uint32_t h,
                                   size_t stride, uint32_t rank, uint32_t world) {
  if (!ctx || !d_rgb || !frame_args_ok(w, h, stride)) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, false, &c);
  return st ? st
            : pipe_submit(c, static_cast<const uint8_t*>(d_rgb), true, w, h, stride, rank, world,
                          true);
}

jxg_status jxg_shard_next_head(jxg_ctx* ctx, uint32_t* dst, size_t* nwords) {
  if (!ctx || !nwords) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, false, &c);
  return st ? st : shard_next_head(c, dst, nwords);
}

jxg_status jxg_shard_write_next(jxg_ctx* ctx, const uint32_t* const* heads, const size_t* head_words,
                                uint32_t n, void* dst, size_t dst_size, size_t* total) {
  if (!ctx || !heads || !head_words || !total || n == 0) return JXG_ERR_INVALID_ARG;
  *total = 0;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, false, &c);
  return st ? st
            : shard_write_next(c, heads, head_words, n, static_cast<uint8_t*>(dst), dst_size, total);
}

jxg_status jxg_shard_write_flush(jxg_ctx* ctx) {
  if (!ctx) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, false, &c);
  return st ? st : shard_write_flush(c);
}

jxg_status jxg_homogeneity_map(jxg_ctx* ctx, const float* xyb, uint32_t xsize, uint32_t ysize,
                               float distance, uint32_t flags, float* r3, uint8_t* type) {
  if (!ctx || !xyb || !r3 || !type || xsize == 0 || ysize == 0 || xsize % 8 || ysize % 8)
    return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : homogeneity_map(c, xyb, xsize, ysize, distance, flags, r3, type);
}

jxg_status jxg_compare_rgb8_device(jxg_ctx* ctx, const void* d_orig, size_t orig_stride,
                                   const void* d_comp, size_t comp_stride, uint32_t xsize,
                                   uint32_t ysize, int want_ssim, jxg_quality* out) {
  if (!ctx || !d_orig || !d_comp || !out || xsize == 0 || ysize == 0 ||
      orig_stride < (size_t)xsize * 3 || comp_stride < (size_t)xsize * 3)
    return JXG_ERR_INVALID_ARG;
  Ctx* c;
  jxg_status st = ctx_enter(ctx, true, &c);
  if (!st) st = order_input(c, c);
  return st ? st
            : compare_device(c, static_cast<const uint8_t*>(d_orig), orig_stride,
                             static_cast<const uint8_t*>(d_comp), comp_stride, xsize, ysize,
                             want_ssim, out);
}

jxg_status jxg_compare_rgb8(jxg_ctx* ctx, const uint8_t* orig, size_t orig_stride,
                            const uint8_t* comp, size_t comp_stride, uint32_t xsize,
                            uint32_t ysize, int want_ssim, jxg_quality* out) {
  if (!ctx || !orig || !comp || !out || xsize == 0 || ysize == 0 ||
      orig_stride < (size_t)xsize * 3 || comp_stride < (size_t)xsize * 3)
    return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st
            : compare_host(c, orig, orig_stride, comp, comp_stride, xsize, ysize, want_ssim, out);
}

jxg_status jxg_msssim_rgb8_device(jxg_ctx* ctx, const void* d_orig, size_t orig_stride,
                                  const void* d_comp, size_t comp_stride, uint32_t xsize,
                                  uint32_t ysize, jxg_msssim* out) {
  if (!ctx || !d_orig || !d_comp || !out || xsize == 0 || ysize == 0 ||
      orig_stride < (size_t)xsize * 3 || comp_stride < (size_t)xsize * 3)
    return JXG_ERR_INVALID_ARG;
  Ctx* c;
  jxg_status st = ctx_enter(ctx, true, &c);
  if (!st) st = order_input(c, c);
  return st ? st
            : msssim_device(c, static_cast<const uint8_t*>(d_orig), orig_stride,
                            static_cast<const uint8_t*>(d_comp), comp_stride, xsize, ysize, out);
}

jxg_status jxg_msssim_rgb8(jxg_ctx* ctx, const uint8_t* orig, size_t orig_stride,
                           const uint8_t* comp, size_t comp_stride, uint32_t xsize,
                           uint32_t ysize, jxg_msssim* out) {
  if (!ctx || !orig || !comp || !out || xsize == 0 || ysize == 0 ||
      orig_stride < (size_t)xsize * 3 || comp_stride < (size_t)xsize * 3)
    return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : msssim_host(c, orig, orig_stride, comp, comp_stride, xsize, ysize, out);
}

jxg_status jxg_reconstruct_rgb8_device(jxg_ctx* ctx, void* d_rgb, size_t row_stride) {
  if (!ctx || !d_rgb) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : reconstruct_last(c, static_cast<uint8_t*>(d_rgb), row_stride, true);
}

jxg_status jxg_reconstruct_rgb8(jxg_ctx* ctx, uint8_t* rgb, size_t row_stride) {
  if (!ctx || !rgb) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : reconstruct_last(c, rgb, row_stride, false);
}

jxg_status jxg_decode_rgb8_device(jxg_ctx* ctx, const uint8_t* data, size_t size, void* d_rgb,
                                  size_t row_stride) {
  if (!ctx || !data || !d_rgb || size == 0) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : decode_rgb8(c, data, size, static_cast<uint8_t*>(d_rgb), row_stride, true);
}

jxg_status jxg_decode_rgb8(jxg_ctx* ctx, const uint8_t* data, size_t size, uint8_t* rgb,
                           size_t row_stride) {
  if (!ctx || !data || !rgb || size == 0) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : decode_rgb8(c, data, size, rgb, row_stride, false);
}

jxg_status jxg_decode_maps(jxg_ctx* ctx, const uint8_t* data, size_t size, uint8_t* acs,
                           uint8_t* qf, int32_t* dc, int32_t* ac, int8_t* cmap) {
  if (!data || size == 0) return JXG_ERR_INVALID_ARG;
  if (!ctx) return (jxg_status)decode_maps_host(data, size, acs, qf, dc, ac, cmap);
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : guarded([&] { return decode_maps_device(c, data, size, acs, qf, dc, ac, cmap); });
}

jxg_status jxg_decode_timings(jxg_ctx* ctx, float* ms) {
  if (!ctx || !ms) return JXG_ERR_INVALID_ARG;
  std::memcpy(ms, reinterpret_cast<const Ctx*>(ctx)->dec.ms, sizeof(float) * 5);
  return JXG_OK;
}

jxg_status jxg_decode_batch_rgb8(jxg_ctx* ctx, const uint8_t* const* datas, const size_t* sizes,
                                 uint32_t n, uint8_t* const* rgbs, const size_t* row_strides,
                                 jxg_status* statuses) {
  if (!ctx || !datas || !sizes || !rgbs || !row_strides || n == 0) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : decode_batch_rgb8(c, datas, sizes, n, rgbs, row_strides, statuses, false);
}

jxg_status jxg_decode_batch_rgb8_device(jxg_ctx* ctx, const uint8_t* const* datas,
                                        const size_t* sizes, uint32_t n, void* const* d_rgbs,
                                        const size_t* row_strides, jxg_status* statuses) {
  if (!ctx || !datas || !sizes || !d_rgbs || !row_strides || n == 0) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st
            : decode_batch_rgb8(c, datas, sizes, n, reinterpret_cast<uint8_t* const*>(d_rgbs),
                                row_strides, statuses, true);
}

jxg_status jxg_set_decode_batch_bytes(jxg_ctx* ctx, size_t bytes) {
  if (!ctx) return JXG_ERR_INVALID_ARG;
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (pipe_busy(c)) return JXG_ERR_INVALID_ARG;
  c->decb.budget = bytes;
  return JXG_OK;
}

jxg_status jxg_decode_batch_timings(jxg_ctx* ctx, jxg_decode_batch_stats* stats) {
  if (!ctx || !stats) return JXG_ERR_INVALID_ARG;
  *stats = reinterpret_cast<const Ctx*>(ctx)->decb.stats;
  return JXG_OK;
}

// the call-level checks of a sweep (everything that needs no device)
static bool sweep_args_ok(jxg_ctx* ctx, const void* rgb, uint32_t w, uint32_t h, size_t stride,
                          const jxg_sweep_point* points, uint32_t n, int quality,
                          const jxg_buffer* outs, const jxg_quality* q) {
  return ctx && rgb && points && outs && n != 0 && frame_args_ok(w, h, stride) && quality >= 0 &&
         quality <= 2 && (quality != 0) == (q != nullptr);
}

jxg_status jxg_sweep_rgb8(jxg_ctx* ctx, const uint8_t* rgb, uint32_t w, uint32_t h, size_t stride,
                          const jxg_sweep_point* points, uint32_t n, int quality, jxg_buffer* outs,
                          jxg_quality* q, jxg_status* statuses) {
  if (!sweep_args_ok(ctx, rgb, w, h, stride, points, n, quality, outs, q))
    return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : guarded([&] {
    return sweep(c, rgb, false, w, h, stride, points, n, quality, outs, q, statuses);
  });
}

jxg_status jxg_sweep_rgb8_device(jxg_ctx* ctx, const void* d_rgb, uint32_t w, uint32_t h,
                                 size_t stride, const jxg_sweep_point* points, uint32_t n,
                                 int quality, jxg_buffer* outs, jxg_quality* q,
                                 jxg_status* statuses) {
  if (!sweep_args_ok(ctx, d_rgb, w, h, stride, points, n, quality, outs, q))
    return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : guarded([&] {
    return sweep(c, static_cast<const uint8_t*>(d_rgb), true, w, h, stride, points, n, quality,
                 outs, q, statuses);
  });
}

jxg_status jxg_sweep_timings(jxg_ctx* ctx, jxg_sweep_stats* stats) {
  if (!ctx || !stats) return JXG_ERR_INVALID_ARG;
  *stats = reinterpret_cast<const Ctx*>(ctx)->sw.stats;
  return JXG_OK;
}

jxg_status jxg_set_sweep_msssim(jxg_ctx* ctx, int on) {
  return sweep_switch(ctx, kRiderMsssim, on != 0);
}
jxg_status jxg_sweep_msssim(jxg_ctx* ctx, jxg_msssim* out, uint32_t n) {
  return sweep_results(ctx, kRiderMsssim, out, n, /*while_pending=*/true);
}
jxg_status jxg_set_sweep_report(jxg_ctx* ctx, int on) {
  return sweep_switch(ctx, kRiderReport, on != 0);
}
jxg_status jxg_sweep_report(jxg_ctx* ctx, jxg_strategy_report* out, uint32_t n) {
  return sweep_results(ctx, kRiderReport, out, n);
}
jxg_status jxg_set_sweep_rates(jxg_ctx* ctx, int on) {
  return sweep_switch(ctx, kRiderRates, on != 0);
}
jxg_status jxg_sweep_rates(jxg_ctx* ctx, struct jxg_rate_report* out, uint32_t n) {
  return sweep_results(ctx, kRiderRates, out, n);
}
// a base index is -1 or that of an earlier point; null or no indices: off
jxg_status jxg_set_sweep_ab(jxg_ctx* ctx, const int32_t* base, uint32_t n) {
  if (!base) n = 0;
  for (uint32_t i = 0; i < n; i++)
    if (base[i] < -1 || base[i] >= (int32_t)i) return JXG_ERR_INVALID_ARG;
  return sweep_switch(ctx, kRiderAb, n != 0, base, n);
}
jxg_status jxg_sweep_ab(jxg_ctx* ctx, jxg_ab_report* out, uint32_t n) {
  return sweep_results(ctx, kRiderAb, out, n);
}
jxg_status jxg_set_sweep_trace(jxg_ctx* ctx, int on) {
  return sweep_switch(ctx, kRiderTrace, on != 0);
}
jxg_status jxg_sweep_trace(jxg_ctx* ctx, jxg_trace_summary* out, uint32_t n) {
  return sweep_results(ctx, kRiderTrace, out, n);
}

jxg_status jxg_strategy_report_rgb8(jxg_ctx* ctx, const uint8_t* orig, size_t orig_stride,
                                    jxg_strategy_report* out, uint32_t* block_sse) {
  if (!ctx || !orig || !out) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : strategy_report_last(c, orig, orig_stride, false, out, block_sse);
}

jxg_status jxg_strategy_report_rgb8_device(jxg_ctx* ctx, const void* d_orig, size_t orig_stride,
                                           jxg_strategy_report* out, uint32_t* d_block_sse) {
  if (!ctx || !d_orig || !out) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st
            : strategy_report_last(c, static_cast<const uint8_t*>(d_orig), orig_stride, true, out,
                                   d_block_sse);
}

jxg_status jxg_rate_report(jxg_ctx* ctx, struct jxg_rate_report* out, uint32_t* block_cost) {
  if (!ctx || !out) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : rate_report_last(c, out, block_cost, false);
}

jxg_status jxg_rate_report_device(jxg_ctx* ctx, struct jxg_rate_report* out, uint32_t* d_block_cost) {
  if (!ctx || !out) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : rate_report_last(c, out, d_block_cost, true);
}

static jxg_status ab_report_entry(jxg_ctx* a, jxg_ctx* b, const void* orig, size_t orig_stride,
                                  bool on_device, jxg_ab_report* out, int32_t* block_delta) {
  if (!a || !b || !orig || !out) return JXG_ERR_INVALID_ARG;
  Ctx *ca, *cb;
  jxg_status st = ctx_enter(a, true, &ca);
  if (!st) st = ctx_enter(b, true, &cb);
  if (st) return st;
  return guarded([&] {
    return ab_report_pair(ca, cb, static_cast<const uint8_t*>(orig), orig_stride, on_device, out,
                          block_delta);
  });
}

jxg_status jxg_ab_report_rgb8(jxg_ctx* a, jxg_ctx* b, const uint8_t* orig, size_t orig_stride,
                              jxg_ab_report* out, int32_t* block_delta) {
  return ab_report_entry(a, b, orig, orig_stride, false, out, block_delta);
}

jxg_status jxg_ab_report_rgb8_device(jxg_ctx* a, jxg_ctx* b, const void* d_orig, size_t orig_stride,
                                     jxg_ab_report* out, int32_t* d_block_delta) {
  return ab_report_entry(a, b, d_orig, orig_stride, true, out, d_block_delta);
}

jxg_status jxg_warmup(jxg_ctx* ctx, uint32_t xsize, uint32_t ysize) {
  if (!ctx || !frame_args_ok(xsize, ysize, (size_t)xsize * 3)) return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, true, &c);
  return st ? st : warmup(c, xsize, ysize);
}

jxg_status jxg_synth_rgb8_device(jxg_ctx* ctx, void* d_out, uint32_t xsize, uint32_t ysize,
                                 size_t row_stride, uint64_t seed) {
  if (!ctx || !d_out || xsize == 0 || ysize == 0 || row_stride < (size_t)xsize * 3)
    return JXG_ERR_INVALID_ARG;
  Ctx* c;
  const jxg_status st = ctx_enter(ctx, false, &c);
  return st ? st : synth_device(c, static_cast<uint8_t*>(d_out), xsize, ysize, row_stride, seed);
}

}  // extern "C"
