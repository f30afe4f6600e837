// jxg_reconstruct.cpp -- decode-side reconstruction (jxg_recon.hip, DESIGN.md
// §3.11).  The decoded image of the last one-at-a-time encode, from the
// context's coefficient and map buffers (read only): tile transform kernel
// (+ the 128 / 256 px varblocks where the encode may hold them), Gaborish and EPF passes as
// the frame header signals them; the last kernel of the chain writes RGB8.
// The decoder (jxg_decode_dev.cpp) runs the same chain on what it parsed.
#include <cmath>

#include "jxg_ctx.h"
#include "jxg_tables.h"

namespace jxg {

ReconFrame recon_frame_of_encode(uint32_t w, uint32_t h, const jxg_params& P) {
  const Frame f = make_frame(w, h, P.distance);
  return ReconFrame{w, h, f.G, f.qdc, lf_code(P.flags, P.distance), 1.0f, 1.0f, P.effort >= 8};
}
ReconFrame recon_frame_of_last(const Ctx* c) {
  ReconFrame R = recon_frame_of_encode(c->rc.w, c->rc.h, c->params);
  R.maybe_big = c->rc.has_big;
  return R;
}

jxg_status reconstruct_device(Ctx* c, const ReconFrame& R, uint8_t* d_rgb, size_t stride) {
  return reconstruct_device(c, R, ReconMaps{c->acs.p, c->qf.p, c->dc.p, c->ac.p, c->cmap.p}, d_rgb,
                            stride);
}

jxg_status reconstruct_device(Ctx* c, const ReconFrame& R, const ReconMaps& M, uint8_t* d_rgb,
                              size_t stride, const ReconSse* q) {
  hipStream_t s = c->stream;
  Ctx::Recon& rc = c->rc;
  Frame f = make_frame(R.w, R.h, 1.0f);
  set_frame_scales(f, R.global_scale, R.quant_dc);
  if (q && rc.tab.p && rc.tab_g != f.G) {
    // a sweep changes the global scale with every point: only the EPF's sigma
    // table depends on it.  It goes through the slot's pinned staging, so the
    // copy is asynchronous whatever the runtime does with pageable sources;
    // the staging's previous copy (the slot's previous chain, long queued) has
    // been read before it is rewritten
    JXG_HIP(rc.h_sigma.ensure(256));
    if (!rc.ev_sigma)
      JXG_HIP(make_event(&rc.ev_sigma, hipEventDisableTiming));
    else
      JXG_HIP(hipEventSynchronize(rc.ev_sigma));
    recon_sigma_table(f.G, rc.h_sigma.p);
    JXG_HIP(hipMemcpyAsync(rc.tab.p + kRcTabSigma, rc.h_sigma.p, 256 * sizeof(float),
                           hipMemcpyHostToDevice, s));
    JXG_HIP(hipEventRecord(rc.ev_sigma, s));
    rc.tab_g = f.G;
  }
  if (!rc.tab.p || rc.tab_g != f.G) {
    const ReconTables T = build_recon_tables(f.G);
    JXG_HIP(rc.tab.ensure(T.tab.size()));
    JXG_HIP(rc.pos.ensure(T.pos.size()));
    JXG_HIP(hipMemcpyAsync(rc.tab.p, T.tab.data(), T.tab.size() * 4, hipMemcpyHostToDevice, s));
    JXG_HIP(hipMemcpyAsync(rc.pos.p, T.pos.data(), T.pos.size() * 2, hipMemcpyHostToDevice, s));
    JXG_HIP(hipStreamSynchronize(s));
    rc.tab_g = f.G;
  }
  const size_t plane = (size_t)f.xp * f.yp;
  const uint32_t ntiles = f.tiles_x * f.tiles_y;
  const uint32_t lf = R.lf;
  const bool gab = lf & 1u;
  const uint32_t epf = (lf >> 1) & 3u;
  const bool big = R.maybe_big;  // the tile kernel may list varblocks of 128 / 256 px
  int passes[4], np = 0;           // -1: Gaborish, else the EPF pass
  if (gab) passes[np++] = -1;
  if (epf >= 3) passes[np++] = 0;
  if (epf >= 1) passes[np++] = 1;
  if (epf >= 2) passes[np++] = 2;
  // q: every pass writes planes and the fused colour + error kernel ends the chain
  const bool to_rgb = np == 0 && !big && !q;
  if (!to_rgb) JXG_HIP(rc.pa.ensure(3 * plane));
  if (np || big) JXG_HIP(rc.pb.ensure(3 * plane));
  const uint32_t bigcap = ntiles / 2 + 1;
  JXG_HIP(rc.big.ensure(1 + (size_t)bigcap));
  JXG_HIP(hipMemsetAsync(rc.big.p, 0, sizeof(uint32_t), s));
  ReconArgs a{};
  a.acs = M.acs;
  a.qf = M.qf;
  a.dc = M.dc;
  a.ac = M.ac;
  a.cmap = M.cmap;
  a.w = f.w;
  a.h = f.h;
  a.bxs = f.bxs;
  a.bys = f.bys;
  a.xp = f.xp;
  a.yp = f.yp;
  a.tiles_x = f.tiles_x;
  a.ntiles_all = ntiles;
  a.inv_g = f.inv_g;
  for (int i = 0; i < 3; i++) a.dc_step[i] = f.dc_step[i];
  a.bias[0] = (float)(1.0 - 0.05465007330715401);
  a.bias[1] = (float)(1.0 - 0.07005449891748593);
  a.bias[2] = (float)(1.0 - 0.049935103337343655);
  a.bias[3] = 0.145f;
  a.tab = rc.tab.p;
  a.pos = rc.pos.p;
  a.pa = rc.pa.p;
  a.pb = rc.pb.p;
  a.biglist = rc.big.p;
  a.bigcap = bigcap;
  a.rgb = d_rgb;
  a.stride = stride;
  // XYB -> linear sRGB: the inverse of the opsin absorbance matrix (double)
  {
    const double bias = 0.0037930732552754493;
    const double m[3][3] = {{0.30, 0.622, 0.078},
                            {0.23, 0.692, 0.078},
                            {0.24342268924547819, 0.20476744424496821, 0.55180986650955360}};
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) -
                       m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
        a.cm[i * 3 + j] = (float)((m[r0][c0] * m[r1][c1] - m[r0][c1] * m[r1][c0]) / det);
      }
    a.cbias = (float)std::cbrt(bias);
    a.obias = (float)bias;
  }
  a.xmul = R.xmul;
  a.bmul = R.bmul;
  JXG_HIP(launch_recon_tiles(a, to_rgb, s));
  if (big && q) {
    // no host round trip for the count: a workgroup per list slot, those past
    // the count return at once
    JXG_HIP(launch_recon_big(a, bigcap, s));
  } else if (big) {
    uint32_t nbig = 0;
    JXG_HIP(hipMemcpyAsync(&nbig, rc.big.p, sizeof(nbig), hipMemcpyDeviceToHost, s));
    JXG_HIP(hipStreamSynchronize(s));
    JXG_HIP(launch_recon_big(a, std::min(nbig, bigcap), s));
  }
  if (!to_rgb && np == 0 && !q) JXG_HIP(launch_recon_colour(a, a.pa, s));
  float *src = a.pa, *dst = a.pb;
  for (int i = 0; i < np; i++) {
    const bool last = i + 1 == np && !q;
    if (passes[i] < 0)
      JXG_HIP(launch_recon_gab(a, src, dst, last, s));
    else
      JXG_HIP(launch_recon_epf(a, passes[i], src, dst, last, s));
    std::swap(src, dst);
  }
  if (q) {  // (enqueued only: the caller orders itself after the stream)
    JXG_HIP(launch_recon_colour_sse(a, src, q->orig, q->orig_stride, q->sse, q->store, s,
                                    q->block_sse));
    return JXG_OK;
  }
  JXG_HIP(hipStreamSynchronize(s));
  return JXG_OK;
}

jxg_status reconstruct_last(Ctx* c, uint8_t* rgb, size_t row_stride, bool on_device) {
  if (!c->rc.ok || row_stride < (size_t)c->rc.w * 3) return JXG_ERR_INVALID_ARG;
  if (on_device) {
    const jxg_status st = order_input(c, c);  // the caller's earlier use of rgb
    if (st) return st;
    return reconstruct_device(c, recon_frame_of_last(c), rgb, row_stride);
  }
  const size_t row = (size_t)c->rc.w * 3;
  JXG_HIP(c->rc.rgb.ensure(row * c->rc.h));
  const jxg_status st = reconstruct_device(c, recon_frame_of_last(c), c->rc.rgb.p, row);
  if (st) return st;
  JXG_HIP(hipMemcpy2DAsync(rgb, row_stride, c->rc.rgb.p, row, row, c->rc.h,
                           hipMemcpyDeviceToHost, c->stream));
  JXG_HIP(hipStreamSynchronize(c->stream));
  return JXG_OK;
}

jxg_status strategy_report_enqueue(Ctx* c, uint32_t w, uint32_t h) {
  const Frame f = make_frame(w, h, 1.0f);
  JXG_HIP(c->q.rep.ensure(kReportCells));
  JXG_HIP(hipMemsetAsync(c->q.rep.p, 0, kReportCells * sizeof(uint64_t), c->stream));
  const ReportArgs a{c->acs.p, c->qf.p, c->ac.p, c->q.bsse.p, w, h, f.bxs, f.bxs * f.bys,
                     reinterpret_cast<unsigned long long*>(c->q.rep.p)};
  JXG_HIP(launch_strategy_report(a, c->stream));
  return JXG_OK;
}

jxg_status block_sse_enqueue(Ctx* c, const uint8_t* orig, size_t orig_stride, bool on_device) {
  const uint32_t w = c->rc.w, h = c->rc.h;
  if (!c->rc.ok || orig_stride < (size_t)w * 3) return JXG_ERR_INVALID_ARG;
  hipStream_t s = c->stream;
  const Frame f = make_frame(w, h, 1.0f);
  const size_t nb = (size_t)f.bxs * f.bys;
  const uint8_t* d_orig = orig;
  size_t so = orig_stride;
  if (on_device) {
    const jxg_status st = order_input(c, c);
    if (st) return st;
  } else {
    so = (size_t)w * 3;
    JXG_HIP(c->q.orig.ensure(so * h));
    JXG_HIP(hipMemcpy2DAsync(c->q.orig.p, so, orig, orig_stride, so, h, hipMemcpyHostToDevice, s));
    d_orig = c->q.orig.p;
  }
  JXG_HIP(c->q.sse.ensure(1));
  JXG_HIP(c->q.bsse.ensure(nb));
  JXG_HIP(hipMemsetAsync(c->q.sse.p, 0, sizeof(uint64_t), s));
  const ReconSse e{d_orig, so, c->q.sse.p, false, c->q.bsse.p};
  return reconstruct_device(c, recon_frame_of_last(c),
                            ReconMaps{c->acs.p, c->qf.p, c->dc.p, c->ac.p, c->cmap.p}, nullptr, so,
                            &e);
}

jxg_status strategy_report_last(Ctx* c, const uint8_t* orig, size_t orig_stride, bool on_device,
                                jxg_strategy_report* out, uint32_t* block_sse) {
  jxg_status st = block_sse_enqueue(c, orig, orig_stride, on_device);
  if (!st) st = strategy_report_enqueue(c, c->rc.w, c->rc.h);
  if (st) return st;
  const uint32_t w = c->rc.w, h = c->rc.h;
  hipStream_t s = c->stream;
  const Frame f = make_frame(w, h, 1.0f);
  const size_t nb = (size_t)f.bxs * f.bys;
  static_assert(sizeof(jxg_strategy_report) == kReportCells * sizeof(uint64_t), "table layout");
  JXG_HIP(hipMemcpyAsync(out, c->q.rep.p, sizeof(*out), hipMemcpyDeviceToHost, s));
  if (block_sse)
    JXG_HIP(hipMemcpyAsync(block_sse, c->q.bsse.p, nb * sizeof(uint32_t),
                           on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
  JXG_HIP(hipStreamSynchronize(s));
  return JXG_OK;
}

}  // namespace jxg
