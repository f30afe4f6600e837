// jxg_quality.cpp -- measurements beside the encoder: decode-side quality
// (jxg_compare_rgb8, jxg_metrics.hip; benchmark-jpegxl image_reader.rs:555-606),
// the stand-alone homogeneity map and the synthetic test image.
#include <cmath>

#include "jxg_ctx.h"

namespace jxg {

// Gaussian window of the SSIM: exp(-(k-5)^2 / 4.5), normalized by the sum taken
// in k order (== oracle/metrics.py gaussian_window, libm exp on both sides)
static void gauss_window(double g[11]) {
  double sum = 0.0;
  for (int k = 0; k < 11; k++) {
    const double d = (double)(k - 5);
    g[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  for (int k = 0; k < 11; k++) g[k] /= sum;
}

jxg_status quality_gauss(Ctx* c) {
  if (c->q.gauss_ready) return JXG_OK;
  std::lock_guard<std::mutex> lock(g_const_mu);
  double g[11];
  gauss_window(g);
  JXG_HIP(set_gauss_table(g, c->stream));
  JXG_HIP(hipGetLastError());
  c->q.gauss_ready = true;
  return JXG_OK;
}

jxg_status compare_device(Ctx* c, const uint8_t* d_orig, size_t so, const uint8_t* d_comp,
                          size_t sc, uint32_t w, uint32_t h, int want_ssim, jxg_quality* out) {
  hipStream_t s = c->stream;
  Ctx::Quality& q = c->q;
  const jxg_status gs = quality_gauss(c);
  if (gs) return gs;
  const uint32_t np = ssim_partials(w, h);
  const bool ssim = want_ssim && np > 0;
  JXG_HIP(q.sse.ensure(1));
  JXG_HIP(q.ssim.ensure(1));
  if (ssim) JXG_HIP(q.part.ensure(np));
  JXG_HIP(hipMemsetAsync(q.sse.p, 0, sizeof(uint64_t), s));
  MetricArgs a{d_orig, d_comp, so, sc, w, h, q.sse.p, ssim ? q.part.p : nullptr,
               ssim ? q.ssim.p : nullptr};
  launch_metrics(a, s);
  JXG_HIP(hipGetLastError());
  uint64_t sse = 0;
  double ssum = 0.0;
  JXG_HIP(hipMemcpyAsync(&sse, q.sse.p, sizeof(sse), hipMemcpyDeviceToHost, s));
  if (ssim) JXG_HIP(hipMemcpyAsync(&ssum, q.ssim.p, sizeof(ssum), hipMemcpyDeviceToHost, s));
  JXG_HIP(hipStreamSynchronize(s));
  out->sse = sse;
  out->samples = (uint64_t)w * h * 3;
  out->mse = (double)sse / (double)out->samples;
  out->psnr = 10.0 * std::log10((255.0 * 255.0) / out->mse);  // mse 0 -> +inf (as f64 in Rust)
  out->ssim = ssim ? ssum / (3.0 * (double)(w - 10) * (double)(h - 10)) : NAN;
  return JXG_OK;
}

jxg_status compare_host(Ctx* c, const uint8_t* orig, size_t so, const uint8_t* comp, size_t sc,
                        uint32_t w, uint32_t h, int want_ssim, jxg_quality* out) {
  const size_t row = (size_t)w * 3, n = row * h;
  JXG_HIP(c->q.orig.ensure(n));
  JXG_HIP(c->q.comp.ensure(n));
  hipStream_t s = c->stream;
  JXG_HIP(hipMemcpy2DAsync(c->q.orig.p, row, orig, so, row, h, hipMemcpyHostToDevice, s));
  JXG_HIP(hipMemcpy2DAsync(c->q.comp.p, row, comp, sc, row, h, hipMemcpyHostToDevice, s));
  return compare_device(c, c->q.orig.p, row, c->q.comp.p, row, w, h, want_ssim, out);
}

// MS-SSIM of Wang, Simoncelli, Bovik 2003: the per-scale
// means pool like the SSIM above; the product runs in ascending scale from 1.0
void msssim_result(uint32_t w, uint32_t h, const double* sums, jxg_msssim* out) {
  static const double kW[kMsScales] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  for (int j = 0; j < kMsScales; j++) {
    const double n = 3.0 * (double)((w >> j) - 10) * (double)((h >> j) - 10);
    out->ssim[j] = sums[j] / n;
    out->cs[j] = sums[kMsScales + j] / n;
  }
  double v = 1.0;
  for (int j = 0; j < kMsScales; j++) {
    const double m = j < kMsScales - 1 ? out->cs[j] : out->ssim[j];
    v *= std::pow(m > 0.0 ? m : 0.0, kW[j]);
  }
  out->ms_ssim = v;
}

void msssim_nan(jxg_msssim* out) {
  out->ms_ssim = NAN;
  for (int j = 0; j < kMsScales; j++) out->cs[j] = out->ssim[j] = NAN;
}

jxg_status msssim_device(Ctx* c, const uint8_t* d_orig, size_t so, const uint8_t* d_comp,
                         size_t sc, uint32_t w, uint32_t h, jxg_msssim* out) {
  if (std::min(w, h) < kMsMinEdge) {
    msssim_nan(out);
    return JXG_OK;
  }
  hipStream_t s = c->stream;
  Ctx::Quality& q = c->q;
  const jxg_status gs = quality_gauss(c);
  if (gs) return gs;
  const size_t nf = ms_pyramid_floats(w, h);
  JXG_HIP(q.pyr_o.ensure(nf));
  JXG_HIP(q.pyr_c.ensure(nf));
  JXG_HIP(q.ms_part.ensure(ms_partials(w, h)));
  JXG_HIP(q.ms_out.ensure(2 * kMsScales));
  launch_ms_pyramid(d_orig, so, w, h, q.pyr_o.p, s);
  launch_ms_pyramid(d_comp, sc, w, h, q.pyr_c.p, s);
  const MsArgs a{d_orig, d_comp, so, sc, w, h, q.pyr_o.p, q.pyr_c.p, q.ms_part.p, q.ms_out.p};
  launch_msssim(a, s);
  JXG_HIP(hipGetLastError());
  double sums[2 * kMsScales];
  JXG_HIP(hipMemcpyAsync(sums, q.ms_out.p, sizeof(sums), hipMemcpyDeviceToHost, s));
  JXG_HIP(hipStreamSynchronize(s));
  msssim_result(w, h, sums, out);
  return JXG_OK;
}

jxg_status msssim_host(Ctx* c, const uint8_t* orig, size_t so, const uint8_t* comp, size_t sc,
                       uint32_t w, uint32_t h, jxg_msssim* out) {
  if (std::min(w, h) < kMsMinEdge) {
    msssim_nan(out);
    return JXG_OK;
  }
  const size_t row = (size_t)w * 3, n = row * h;
  JXG_HIP(c->q.orig.ensure(n));
  JXG_HIP(c->q.comp.ensure(n));
  hipStream_t s = c->stream;
  JXG_HIP(hipMemcpy2DAsync(c->q.orig.p, row, orig, so, row, h, hipMemcpyHostToDevice, s));
  JXG_HIP(hipMemcpy2DAsync(c->q.comp.p, row, comp, sc, row, h, hipMemcpyHostToDevice, s));
  return msssim_device(c, c->q.orig.p, row, c->q.comp.p, row, w, h, out);
}

jxg_status homogeneity_map(Ctx* c, const float* xyb, uint32_t xsize, uint32_t ysize,
                           float distance, uint32_t flags, float* r3, uint8_t* type) {
  const size_t plane = (size_t)xsize * ysize, nb = plane / 64;
  JXG_HIP(c->xyb.ensure(plane * 3));
  JXG_HIP(c->r3.ensure(nb * 3));
  JXG_HIP(c->type.ensure(nb));
  hipStream_t s = c->stream;
  JXG_HIP(hipMemcpyAsync(c->xyb.p, xyb, plane * 12, hipMemcpyHostToDevice, s));
  HomogArgs a{c->xyb.p, xsize, ysize, xsize, plane, distance,
              (flags & JXG_FLAG_H1_INT_ABS) ? 1 : 0, c->r3.p, c->type.p};
  launch_homog(a, (xsize / 8 + 7) / 8, (ysize / 8 + 7) / 8, s);
  JXG_HIP(hipGetLastError());
  JXG_HIP(hipMemcpyAsync(r3, c->r3.p, nb * 12, hipMemcpyDeviceToHost, s));
  JXG_HIP(hipMemcpyAsync(type, c->type.p, nb, hipMemcpyDeviceToHost, s));
  JXG_HIP(hipStreamSynchronize(s));
  return JXG_OK;
}

jxg_status synth_device(Ctx* c, uint8_t* d_out, uint32_t w, uint32_t h, size_t stride,
                        uint64_t seed) {
  JXG_HIP(launch_synth(d_out, w, h, stride, seed, c->stream));
  JXG_HIP(hipStreamSynchronize(c->stream));
  return JXG_OK;
}

}  // namespace jxg
