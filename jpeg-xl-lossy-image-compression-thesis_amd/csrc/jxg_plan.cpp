// jxg_plan.cpp -- frame geometry, shard plan, pipeline shape (jxg_plan.h)
#include "jxg_plan.h"

#include <algorithm>
#include <cmath>

namespace jxg {

void set_frame_scales(Frame& f, uint32_t G, uint32_t qdc) {
  f.G = G;
  f.inv_g = (float)(65536.0 / (double)G);
  f.qdc = qdc;
  const double m_lf[3] = {1.0 / 4096.0, 1.0 / 512.0, 1.0 / 256.0};
  for (int c = 0; c < 3; c++) {
    f.dc_mul[c] = (float)((double)G * (double)qdc / 65536.0 / m_lf[c]);
    f.dc_step[c] = (float)(65536.0 / (double)G / (double)qdc * m_lf[c]);
  }
}

Frame make_frame(uint32_t w, uint32_t h, float distance) {
  Frame f{};
  f.w = w;
  f.h = h;
  f.bxs = (w + 7) / 8;
  f.bys = (h + 7) / 8;
  f.xp = f.bxs * 8;
  f.yp = f.bys * 8;
  f.tiles_x = (f.bxs + 7) / 8;
  f.tiles_y = (f.bys + 7) / 8;
  f.gxs = (w + 255) / 256;
  f.gys = (h + 255) / 256;
  f.ngroups = f.gxs * f.gys;
  f.lfxs = (w + 2047) / 2048;
  f.lfys = (h + 2047) / 2048;
  f.nlf = f.lfxs * f.lfys;
  const double d = distance;
  const double qfb = 0.79 / d;
  f.qf_base = (float)qfb;
  long G = (long)std::floor(qfb * 1024.0 + 0.5);
  G = std::min<long>(std::max<long>(G, 1), 73727);
  double t = 0.3 * std::pow(d / 0.3, 0.66);
  if (t > d) t = d;
  if (t < 0.5 * d) t = 0.5 * d;
  double qdc_f = 1.12 / t;
  if (qdc_f > 50.0) qdc_f = 50.0;
  long qdc = (long)std::floor(qdc_f * 65536.0 / (double)G + 0.5);
  qdc = std::min<long>(std::max<long>(qdc, 1), 65536);
  set_frame_scales(f, (uint32_t)G, (uint32_t)qdc);
  return f;
}

uint32_t shard_g0(uint32_t ngroups, uint32_t r, uint32_t world) {
  return (uint32_t)(((uint64_t)ngroups * r) / world);
}
uint32_t shard_of(uint32_t ngroups, uint32_t g, uint32_t world) {
  uint32_t r = (uint32_t)(((uint64_t)g * world) / ngroups);  // then correct the rounding
  while (r + 1 < world && shard_g0(ngroups, r + 1, world) <= g) r++;
  while (r > 0 && shard_g0(ngroups, r, world) > g) r--;
  return r;
}
uint32_t lf_of_group(const Frame& f, uint32_t g) {
  return ((g / f.gxs) / 8) * f.lfxs + (g % f.gxs) / 8;
}
std::vector<uint32_t> lf_owners_ranges(const Frame& f, uint32_t world) {
  std::vector<uint32_t> own(f.nlf, 0), nassigned(world, 0), cnt(world);
  if (world == 1) return own;
  for (uint32_t lg = 0; lg < f.nlf; lg++) {
    std::fill(cnt.begin(), cnt.end(), 0u);
    const uint32_t lx = lg % f.lfxs, ly = lg / f.lfxs;
    for (uint32_t gy = ly * 8; gy < std::min(ly * 8 + 8, f.gys); gy++)
      for (uint32_t gx = lx * 8; gx < std::min(lx * 8 + 8, f.gxs); gx++)
        cnt[shard_of(f.ngroups, gy * f.gxs + gx, world)]++;
    int best = -1;
    long bs = 0;
    for (uint32_t r = 0; r < world; r++) {
      if (!cnt[r]) continue;
      const long sc = (long)cnt[r] - 16 * (long)nassigned[r];
      if (best < 0 || sc > bs) {
        best = (int)r;
        bs = sc;
      }
    }
    own[lg] = (uint32_t)best;
    nassigned[best]++;
  }
  return own;
}

Partition make_partition(const Frame& f, uint32_t world) {
  Partition P;
  P.group.assign(f.ngroups, 0);
  P.lf.assign(f.nlf, 0);
  if (world <= 1) return P;
  for (uint32_t g = 0; g < f.ngroups; g++) P.group[g] = shard_of(f.ngroups, g, world);
  P.lf = lf_owners_ranges(f, world);
  bool exchange = false;
  for (uint32_t g = 0; g < f.ngroups && !exchange; g++)
    exchange = P.lf[lf_of_group(f, g)] != P.group[g];
  if (!exchange) return P;
  if (f.nlf >= world) {
    // whole LF groups, largest first (pixel area; ties: lower index) to the
    // least-loaded rank (ties: lower rank)
    std::vector<uint64_t> area(f.nlf);
    uint64_t total = 0;
    for (uint32_t lg = 0; lg < f.nlf; lg++) {
      const uint64_t x0 = (uint64_t)(lg % f.lfxs) * 2048, y0 = (uint64_t)(lg / f.lfxs) * 2048;
      area[lg] = std::min<uint64_t>(2048, f.w - x0) * std::min<uint64_t>(2048, f.h - y0);
      total += area[lg];
    }
    std::vector<uint32_t> order(f.nlf);
    for (uint32_t i = 0; i < f.nlf; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return area[a] > area[b]; });
    std::vector<uint64_t> load(world, 0);
    std::vector<uint32_t> lfo(f.nlf, 0);
    for (uint32_t lg : order) {
      uint32_t r = 0;
      for (uint32_t q = 1; q < world; q++)
        if (load[q] < load[r]) r = q;
      lfo[lg] = r;
      load[r] += area[lg];
    }
    const uint64_t most = *std::max_element(load.begin(), load.end());
    const uint64_t least = *std::min_element(load.begin(), load.end());
    if (least > 0 && most * 100 * world <= total * 105) {
      P.lf = lfo;
      for (uint32_t g = 0; g < f.ngroups; g++) P.group[g] = lfo[lf_of_group(f, g)];
      P.kind = 1;
      return P;
    }
  }
  P.kind = 2;
  return P;
}

Exchange make_exchange(const Frame& f, const Partition& part, uint32_t rank, uint32_t world) {
  Exchange X;
  X.nsend.assign(world, 0);
  X.nrecv.assign(world, 0);
  for (uint32_t p = 0; p < world; p++) {
    if (p == rank) continue;
    for (uint32_t g = 0; g < f.ngroups; g++) {
      const uint32_t lo = part.lf[lf_of_group(f, g)];
      if (part.group[g] == rank && lo == p) {
        X.send.push_back(g);
        X.nsend[p]++;
      }
      if (part.group[g] == p && lo == rank) {
        X.recv.push_back(g);
        X.nrecv[p]++;
      }
    }
  }
  return X;
}

size_t exchange_slot_records(const Frame& f, uint32_t world) {
  const Partition part = make_partition(f, world);
  size_t most = 1;
  for (uint32_t r = 0; r < world && world > 1; r++) {
    const Exchange X = make_exchange(f, part, r, world);
    most = std::max(most, std::max(X.send.size(), X.recv.size()));
  }
  return most;
}

Plan make_plan(const Frame& f, uint32_t rank, uint32_t world) {
  Plan P;
  P.rank = rank;
  P.world = world;
  if (world <= 1) {
    P.groups.resize(f.ngroups);
    for (uint32_t g = 0; g < f.ngroups; g++) P.groups[g] = g;
    return P;
  }
  const Partition part = make_partition(f, world);
  for (uint32_t g = 0; g < f.ngroups; g++)
    if (part.group[g] == rank) P.groups.push_back(g);
  P.contiguous = P.groups.empty() || P.groups.back() - P.groups.front() + 1 == P.groups.size();
  for (uint32_t g : P.groups) {
    const uint32_t gx = g % f.gxs, gy = g / f.gxs;
    for (uint32_t ty = gy * 4; ty < std::min(gy * 4 + 4, f.tiles_y); ty++)
      for (uint32_t tx = gx * 4; tx < std::min(gx * 4 + 4, f.tiles_x); tx++)
        P.tiles.push_back(ty * f.tiles_x + tx);
  }
  P.lf_mine.resize(f.nlf);
  for (uint32_t lg = 0; lg < f.nlf; lg++) P.lf_mine[lg] = part.lf[lg] == rank;
  P.x = make_exchange(f, part, rank, world);
  return P;
}

PipeShape pipe_shape(uint32_t ngroups, uint32_t ntiles, uint32_t cap, uint32_t queues) {
  const uint32_t want = (kPipeChainGroups + ngroups - 1) / std::max(1u, ngroups);  // frames
  uint32_t lmax = std::max(2u, std::min(kPipeMaxLanes, queues - 1));
  if (cap) lmax = std::min(lmax, cap);
  const uint32_t kt = ntiles <= kPipeBatchTiles ? kPipeMaxBatch : 1u;
  const uint32_t k = std::min(kt, std::max(1u, (want + lmax - 1) / lmax));
  const uint32_t lanes = std::min(lmax, std::max(std::min(kPipeMinLanes, lmax), (want + k - 1) / k));
  return PipeShape{lanes, k};
}

}  // namespace jxg
