// jxg_rate.cpp -- coded bits per block and per strategy (jxg_rate.hip,
// DESIGN.md §3.17): what an encode leaves for the report, the kernel's launch
// on the context's own buffers, the one-at-a-time report and a sweep point's.
#include <cmath>
#include <cstring>

#include "jxg_ctx.h"

extern "C" uint32_t jxg_rate_symbol_cost(uint32_t f) {
  if (f == 0 || f > 4096) return 0;
  return (uint32_t)std::floor(256.0 * std::log2(4096.0 / (double)f) + 0.5);
}

namespace jxg {

void rate_note(Ctx* c, const Job& J) {
  Ctx::Rate& rt = c->rt;
  rt.have = false;
  if (J.plan.world != 1 || J.presets) return;  // whole frames of one preset only
  rt.ans = J.ans;
  rt.whole_group = J.big;
  rt.nhist = J.nhist_ans;
  rt.groups = J.f.ngroups;
  rt.ac_bits = 0;
  for (uint32_t g = 0; g < J.f.ngroups; g++) rt.ac_bits += c->gbits.h[g];
  rt.stream_bits = 8ull * J.out_bytes;
  rt.have = true;
}

jxg_status rate_enqueue(Ctx* c, uint32_t w, uint32_t h, uint32_t* d_block_cost) {
  Ctx::Rate& rt = c->rt;
  if (!rt.have) return JXG_ERR_INTERNAL;
  hipStream_t s = c->stream;
  const Frame f = make_frame(w, h, 1.0f);
  if (f.ngroups != rt.groups) return JXG_ERR_INTERNAL;
  if (!rt.ftab_ready) {
    static const std::vector<uint16_t> tab = [] {
      std::vector<uint16_t> t(kRateFreqs);
      for (uint32_t i = 0; i < kRateFreqs; i++) t[i] = (uint16_t)jxg_rate_symbol_cost(i);
      return t;
    }();
    JXG_HIP(rt.ftab.ensure(kRateFreqs));
    JXG_HIP(hipMemcpyAsync(rt.ftab.p, tab.data(), kRateFreqs * sizeof(uint16_t),
                           hipMemcpyHostToDevice, s));
    rt.ftab_ready = true;
  }
  JXG_HIP(rt.table.ensure(kRateCells));
  JXG_HIP(hipMemsetAsync(rt.table.p, 0, kRateCells * sizeof(uint64_t), s));
  RateArgs a{};
  a.ac.acs = c->acs.p;
  a.ac.ac = c->ac.p;
  a.ac.nz = c->nz.p;
  a.ac.bxs = f.bxs;
  a.ac.bys = f.bys;
  a.ac.gxs = f.gxs;
  a.ac.g0 = 0;
  a.ac.glist = nullptr;
  a.ac.codes = c->codes_ac.d;
  a.ac.tokens = c->tokens.p;
  a.ans_tab = rt.ans ? c->ans_tab.d : nullptr;
  a.nhist = rt.nhist;
  a.ftab = rt.ftab.p;
  a.block_cost = d_block_cost;
  a.table = reinterpret_cast<unsigned long long*>(rt.table.p);
  JXG_HIP(launch_rate(a, f.ngroups, rt.whole_group, s));
  return JXG_OK;
}

static_assert(sizeof(jxg_rate_row) == kRateCols * sizeof(uint64_t), "row layout");
static_assert(sizeof(RateReport) == kRateWords * sizeof(uint64_t) - sizeof(uint64_t),
              "table, two u64 and two u32");

void rate_from_words(const uint64_t* words, RateReport* out) {
  std::memcpy(out->row, words, kRateCells * sizeof(uint64_t));
  out->ac_bits = words[kRateCells];
  out->stream_bits = words[kRateCells + 1];
  out->ans = (uint32_t)words[kRateCells + 2];
  out->groups = (uint32_t)words[kRateCells + 3];
}

jxg_status rate_map_ensure(Ctx* c, uint32_t w, uint32_t h) {
  const Frame f = make_frame(w, h, 1.0f);
  JXG_HIP(c->rt.map.ensure((size_t)f.bxs * f.bys));
  return JXG_OK;
}

jxg_status sweep_rate_enqueue(Ctx* S, const SweepReq& rq, uint32_t w, uint32_t h) {
  // a point of an A/B comparison (jxg_ab.cpp) also needs the cost map, and
  // runs the kernel whether or not the rate report is returned
  jxg_status st = rq.ab ? rate_map_ensure(S, w, h) : JXG_OK;
  if (!st) st = rate_enqueue(S, w, h, rq.ab ? S->rt.map.p : nullptr);
  if (st || !rq.h[kRiderRates]) return st;
  JXG_HIP(hipMemcpyAsync(rq.h[kRiderRates], S->rt.table.p, kRateCells * sizeof(uint64_t),
                         hipMemcpyDeviceToHost, S->stream));
  rq.h[kRiderRates][kRateCells] = S->rt.ac_bits;
  rq.h[kRiderRates][kRateCells + 1] = S->rt.stream_bits;
  rq.h[kRiderRates][kRateCells + 2] = S->rt.ans ? 1 : 0;
  rq.h[kRiderRates][kRateCells + 3] = S->rt.groups;
  return JXG_OK;
}

jxg_status rate_report_last(Ctx* c, RateReport* out, uint32_t* block_cost, bool on_device) {
  if (!c->rc.ok || !c->rt.have) return JXG_ERR_INVALID_ARG;
  const uint32_t w = c->rc.w, h = c->rc.h;
  hipStream_t s = c->stream;
  const Frame f = make_frame(w, h, 1.0f);
  const size_t nb = (size_t)f.bxs * f.bys;
  uint32_t* d_map = nullptr;
  if (block_cost && on_device) {
    const jxg_status st = order_input(c, c);  // the caller's earlier use of the buffer
    if (st) return st;
    d_map = block_cost;
  } else if (block_cost) {
    const jxg_status st = rate_map_ensure(c, w, h);
    if (st) return st;
    d_map = c->rt.map.p;
  }
  const jxg_status st = rate_enqueue(c, w, h, d_map);
  if (st) return st;
  uint64_t words[kRateWords] = {};
  JXG_HIP(hipMemcpyAsync(words, c->rt.table.p, kRateCells * sizeof(uint64_t),
                         hipMemcpyDeviceToHost, s));
  if (block_cost && !on_device)
    JXG_HIP(hipMemcpyAsync(block_cost, d_map, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  JXG_HIP(hipStreamSynchronize(s));
  words[kRateCells] = c->rt.ac_bits;
  words[kRateCells + 1] = c->rt.stream_bits;
  words[kRateCells + 2] = c->rt.ans ? 1 : 0;
  words[kRateCells + 3] = c->rt.groups;
  rate_from_words(words, out);
  return JXG_OK;
}

}  // namespace jxg
