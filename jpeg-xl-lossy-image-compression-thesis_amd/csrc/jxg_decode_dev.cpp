// jxg_decode_dev.cpp -- the decoder's device side (jxg_decode.cpp /
// jxg_decode.hip).  Host: headers, TOC, LfGlobal, LF groups
// (helper threads), HfGlobal, decode tables.  Device: the maps are uploaded
// into the context's own acs / qf / dc / cmap buffers, the pass-group kernel
// fills ac, and the reconstruction chain (jxg_reconstruct.cpp) turns them into
// pixels.  The last encode can no longer be reconstructed from those buffers.
#include <cmath>
#include <cstring>

#include "jxg_ctx.h"
#include "jxg_decode.h"
#include "jxg_tables.h"

namespace jxg {

// F: the parsed stream (decode_parse with its LF groups); nothing of the
// context is touched before the caller has checked its arguments against it
static jxg_status decode_to_device(Ctx* c, const DecFrame* F) {
  hipStream_t s = c->stream;
  Ctx::Dec& D = c->dec;
  c->rc.ok = false;
  const size_t nb = (size_t)F->bxs * F->bys;
  const size_t ntiles = (size_t)F->tiles_x * F->tiles_y;
  const uint32_t ng = F->info.num_groups;
  JXG_HIP(c->acs.ensure(nb));
  JXG_HIP(c->qf.ensure(nb));
  JXG_HIP(c->dc.ensure(nb * 3));
  JXG_HIP(c->ac.ensure(nb * 192));
  JXG_HIP(c->cmap.ensure(ntiles * 2));
  JXG_HIP(D.stream.ensure(F->words.size()));
  JXG_HIP(D.sec.ensure(F->sec.size()));
  JXG_HIP(D.status.ensure(ng));
  // decode tables, one upload: [hist | atab or ptab | ctxmap], 8-byte aligned parts
  const DecEntropy& E = F->hf;
  const DecTableBlob B = decode_table_blob(E);
  const std::vector<uint8_t>& blob = B.bytes;
  const size_t o_atab = B.o_atab, o_ptab = B.o_ptab, o_map = B.o_map;
  JXG_HIP(D.tab.ensure(blob.size()));
  for (hipEvent_t& e : D.ev)
    if (!e && make_event(&e, hipEventDefault) != hipSuccess) return JXG_ERR_HIP;
  JXG_HIP(hipMemcpyAsync(c->acs.p, F->acs.data(), nb, hipMemcpyHostToDevice, s));
  JXG_HIP(hipMemcpyAsync(c->qf.p, F->qf.data(), nb, hipMemcpyHostToDevice, s));
  JXG_HIP(hipMemcpyAsync(c->dc.p, F->dc.data(), nb * 12, hipMemcpyHostToDevice, s));
  JXG_HIP(hipMemcpyAsync(c->cmap.p, F->cmap.data(), ntiles * 2, hipMemcpyHostToDevice, s));
  JXG_HIP(hipMemcpyAsync(D.stream.p, F->words.data(), F->words.size() * 8,
                         hipMemcpyHostToDevice, s));
  JXG_HIP(hipMemcpyAsync(D.sec.p, F->sec.data(), F->sec.size() * 8, hipMemcpyHostToDevice, s));
  JXG_HIP(hipMemcpyAsync(D.tab.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
  DecodeArgs a{};
  a.stream = D.stream.p;
  a.sec = D.sec.p;
  a.sym.hist = reinterpret_cast<const dec::HistDesc*>(D.tab.p);
  a.sym.atab = reinterpret_cast<const dec::AnsEntry*>(D.tab.p + o_atab);
  a.sym.ptab = reinterpret_cast<const uint16_t*>(D.tab.p + o_ptab);
  a.sym.ctxmap = D.tab.p + o_map;
  a.sym.nctx = (uint32_t)E.ctxmap.size();
  a.sym.prefix = E.prefix;
  a.sym.log_alpha = E.log_alpha;
  a.npresets = F->info.num_hf_presets;
  a.preset_bits = F->preset_bits;
  a.acs = c->acs.p;
  a.ac = c->ac.p;
  a.status = D.status.p;
  a.bxs = F->bxs;
  a.bys = F->bys;
  a.gxs = F->gxs;
  a.nhist = (uint32_t)E.hist.size();
  a.tab_bytes = B.tab_bytes;
  JXG_HIP(hipEventRecord(D.ev[0], s));
  JXG_HIP(launch_decode_groups(a, ng, s));
  JXG_HIP(hipEventRecord(D.ev[1], s));
  std::vector<uint32_t> status(ng, 0);
  JXG_HIP(hipMemcpyAsync(status.data(), D.status.p, (size_t)ng * 4, hipMemcpyDeviceToHost, s));
  JXG_HIP(hipStreamSynchronize(s));  // (also: the uploads' host vectors may go)
  for (uint32_t g = 0; g < ng; g++)
    if (status[g]) return status[g] == (uint32_t)dec::kUnsupported ? JXG_ERR_UNSUPPORTED : JXG_ERR_INVALID_ARG;
  float ms = 0.0f;
  (void)hipEventElapsedTime(&ms, D.ev[0], D.ev[1]);
  D.ms[0] = F->ms_head;
  D.ms[1] = F->ms_lf;
  D.ms[2] = ms;
  D.ms[3] = 0.0f;
  return JXG_OK;
}

// what the reconstruction tables cannot honour is refused: a 128 / 256 px
// varblock whose quant table is not the one this encoder writes in DCT mode,
// x_qm / b_qm scales outside the header's range
jxg_status decode_recon_frame(const DecFrame& F, ReconFrame* R) {
  for (int k = 0; k < 4; k++) {
    const bool present = F.qm_mask >> k & 1u;
    if (present && !dequant_params_match(k, F.qm_bits[k])) return JXG_ERR_UNSUPPORTED;
    if ((F.big_used >> k & 1u) && !present) return JXG_ERR_UNSUPPORTED;
  }
  if (F.info.global_scale == 0 || F.info.quant_dc == 0) return JXG_ERR_INVALID_ARG;
  R->w = F.info.xsize;
  R->h = F.info.ysize;
  R->global_scale = F.info.global_scale;
  R->quant_dc = F.info.quant_dc;
  R->lf = (F.info.gaborish ? 1u : 0u) | F.info.epf_iters << 1;
  R->xmul = (float)std::pow(1.25, 2.0 - (double)F.x_qm);
  R->bmul = (float)std::pow(1.25, 2.0 - (double)F.b_qm);
  R->maybe_big = F.big_used != 0;
  return JXG_OK;
}

// tight: into the context's own image (rows of 3 * xsize bytes), for the host
// variant, whose stride `row_stride` is still checked
static jxg_status decode_rgb8_device(Ctx* c, const uint8_t* data, size_t size, uint8_t* d_rgb,
                                     size_t row_stride, bool tight, uint32_t* w, uint32_t* h) {
  const Clock::time_point t0 = Clock::now();
  DecFrame F;
  jxg_status st = (jxg_status)decode_parse(data, size, true, &F);
  if (st) return st;
  if (row_stride < (size_t)F.info.xsize * 3) return JXG_ERR_INVALID_ARG;
  ReconFrame R{};
  st = decode_recon_frame(F, &R);
  if (st) return st;
  st = decode_to_device(c, &F);
  if (st) return st;
  *w = R.w;
  *h = R.h;
  if (tight) {
    row_stride = (size_t)R.w * 3;
    JXG_HIP(c->rc.rgb.ensure(row_stride * R.h));
    d_rgb = c->rc.rgb.p;
  }
  st = reconstruct_device(c, R, d_rgb, row_stride);
  if (st) return st;
  JXG_HIP(hipEventRecord(c->dec.ev[2], c->stream));
  JXG_HIP(hipStreamSynchronize(c->stream));
  (void)hipEventElapsedTime(&c->dec.ms[3], c->dec.ev[1], c->dec.ev[2]);
  c->dec.ms[4] = ms_since(t0);
  return JXG_OK;
}

jxg_status decode_rgb8(Ctx* c, const uint8_t* data, size_t size, uint8_t* rgb, size_t row_stride,
                       bool on_device) {
  uint32_t w = 0, h = 0;
  if (on_device) {
    const jxg_status st = order_input(c, c);  // the caller's earlier use of rgb
    if (st) return st;
    return guarded([&] { return decode_rgb8_device(c, data, size, rgb, row_stride, false, &w, &h); });
  }
  const jxg_status st =
      guarded([&] { return decode_rgb8_device(c, data, size, nullptr, row_stride, true, &w, &h); });
  if (st) return st;
  const size_t row = (size_t)w * 3;
  JXG_HIP(hipMemcpy2DAsync(rgb, row_stride, c->rc.rgb.p, row, row, h, hipMemcpyDeviceToHost,
                           c->stream));
  JXG_HIP(hipStreamSynchronize(c->stream));
  return JXG_OK;
}

jxg_status decode_maps_device(Ctx* c, const uint8_t* data, size_t size, uint8_t* acs, uint8_t* qf,
                              int32_t* dc, int32_t* ac, int8_t* cmap) {
  DecFrame F;
  jxg_status st = (jxg_status)decode_parse(data, size, true, &F);
  if (st) return st;
  st = decode_to_device(c, &F);
  if (st) return st;
  const size_t nb = (size_t)F.bxs * F.bys;
  if (acs) std::memcpy(acs, F.acs.data(), nb);
  if (qf) std::memcpy(qf, F.qf.data(), nb);
  if (dc) std::memcpy(dc, F.dc.data(), nb * 12);
  if (cmap) std::memcpy(cmap, F.cmap.data(), F.cmap.size());
  if (ac) {
    std::vector<int16_t> ac16(nb * 192);
    JXG_HIP(hipMemcpyAsync(ac16.data(), c->ac.p, nb * 192 * 2, hipMemcpyDeviceToHost, c->stream));
    JXG_HIP(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < nb * 192; i++) ac[i] = ac16[i];
  }
  return JXG_OK;
}

}  // namespace jxg
