// jxg_decode_plan.cpp -- the batch decoder's plan (jxg_decode_plan.h): chunks
// by device footprint, arena slices, and the pass-group kernels' work lists by
// launch class, longest section first.  Host only (no HIP include).
#include "jxg_decode_plan.h"

#include <algorithm>

namespace jxg {

uint32_t decode_lds_bytes(uint32_t nhist, uint32_t tab_bytes, bool* staged) {
  // (64 bits: a count from a parsed stream must not wrap the comparison)
  const uint64_t base = (uint64_t)kDecPlanNzs + kDecPlanMap +
                        (((uint64_t)nhist * kDecPlanHistBytes + 7) & ~(uint64_t)7);
  const bool st = tab_bytes && base <= kDecPlanLdsMax && tab_bytes <= kDecPlanLdsMax - base;
  if (staged) *staged = st;
  return (uint32_t)(base + (st ? (tab_bytes + 7) & ~7u : 0u));
}

DecSliceBytes decode_slice_bytes(const DecPlanFrame& f) {
  const size_t nb = (size_t)f.bxs * f.bys;
  return DecSliceBytes{nb,     nb,
                       nb * 12,  // dc: [3][nb] int32
                       nb * 384, // ac: [nb][3][64] int16
                       (size_t)f.ntiles * 2,
                       f.stream_words * 8,
                       (size_t)f.ngroups * 16,
                       f.table_bytes};
}

static size_t align_up(size_t v) { return (v + kDecArenaAlign - 1) & ~(kDecArenaAlign - 1); }

// lays the frame's slices out from `at`; returns the end
static size_t place(const DecPlanFrame& f, size_t at, DecSlices* s) {
  const DecSliceBytes b = decode_slice_bytes(f);
  const size_t bytes[8] = {b.acs, b.qf, b.dc, b.ac, b.cmap, b.stream, b.sec, b.tab};
  size_t* off[8] = {&s->acs, &s->qf, &s->dc, &s->ac, &s->cmap, &s->stream, &s->sec, &s->tab};
  for (int i = 0; i < 8; i++) {
    *off[i] = at;
    at += align_up(bytes[i]);
  }
  s->end = at;
  return at;
}

size_t decode_footprint(const DecPlanFrame& f) {
  DecSlices s;
  return place(f, 0, &s);
}

static uint64_t section_bits(const DecPlanFrame& f, uint32_t g) {
  const uint64_t a = f.sec[2 * (size_t)g], b = f.sec[2 * (size_t)g + 1];
  return b > a ? b - a : 0;
}

std::vector<DecChunk> plan_decode_batch(const std::vector<DecPlanFrame>& frames, size_t budget) {
  if (budget == 0) budget = kDecBatchDefaultBytes;
  std::vector<DecChunk> chunks;
  const uint32_t n = (uint32_t)frames.size();
  for (uint32_t i = 0; i < n;) {
    DecChunk c;
    c.first = i;
    size_t bytes = 0;
    while (i < n) {
      const size_t fp = decode_footprint(frames[i]);
      // the first frame is taken whatever its size: never refused for size
      if (i > c.first && (fp > budget || bytes > budget - fp)) break;
      DecSlices s;
      bytes = place(frames[i], bytes, &s);
      c.at.push_back(s);
      c.status_base.push_back(c.nstatus);
      c.nstatus += frames[i].ngroups;
      i++;
    }
    c.end = i;
    c.bytes = bytes;
    // work lists: (section bits, frame, group), bits descending
    struct Item {
      uint64_t bits;
      DecWork w;
    };
    std::vector<Item> items[2];
    for (uint32_t f = c.first; f < c.end; f++) {
      const DecPlanFrame& F = frames[f];
      bool staged = false;
      const uint32_t lds = decode_lds_bytes(F.nhist, F.tab_bytes, &staged);
      if (F.ngroups == 0 || !F.sec) continue;
      uint32_t& top = staged ? c.lds_staged : c.lds_unstaged;
      top = std::max(top, lds);
      for (uint32_t g = 0; g < F.ngroups; g++)
        items[staged ? 0 : 1].push_back(Item{section_bits(F, g), DecWork{f, g}});
    }
    for (int k = 0; k < 2; k++) {
      std::sort(items[k].begin(), items[k].end(), [](const Item& a, const Item& b) {
        if (a.bits != b.bits) return a.bits > b.bits;
        if (a.w.frame != b.w.frame) return a.w.frame < b.w.frame;
        return a.w.group < b.w.group;
      });
      std::vector<DecWork>& out = k == 0 ? c.staged : c.unstaged;
      out.reserve(items[k].size());
      for (const Item& it : items[k]) out.push_back(it.w);
    }
    chunks.push_back(std::move(c));
  }
  return chunks;
}

}  // namespace jxg
