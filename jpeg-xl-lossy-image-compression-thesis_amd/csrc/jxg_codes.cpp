// jxg_codes.cpp -- the entropy codes, global sections and arena layouts of one
// frame (jxg_codes.h); host only
#include "jxg_codes.h"

#include <algorithm>
#include <cstring>
#include <utility>

#include "jxg_dequant.h"

namespace jxg {

EncArenas::Layouts EncArenas::declare(const Frame& f, uint32_t plan_groups) {
  const size_t ns = (size_t)f.nlf * 2;  // LF streams
  Layouts L;
  L.stat.add(hist_ac, (size_t)kMaxClusters * kAlpha);
  L.stat.add(bound, f.ngroups);
  L.stat.add(ntok, (size_t)f.ngroups * 3);
  L.stat.add(bandtok, (size_t)f.ngroups * 4);
  L.stat.add(bigcount, 4);  // varblocks per big kind (big_list_kernel)
  stat_lf = L.stat.mark();
  L.stat.add(lfhist, ns * 4 * kAlpha);
  L.stat.add(sbound, ns);
  L.stat.add(vcount, f.nlf);
  stat_bytes = L.stat.bytes();
  L.up.add(codes_ac, (size_t)kMaxClusters * kAlpha);
  up_gbase = L.up.mark();
  L.up.add(gbase, f.ngroups);
  up_ac = L.up.mark();
  L.up.add(ans_order, std::max(1u, plan_groups));
  L.up.add(ans_tab, kAnsTabBytes);
  up_lf = L.up.mark();
  L.up.add(lfcodes, ns * 4 * kAlpha);
  L.up.add(stream_base, ns);
  up_bytes = L.up.bytes();
  L.bits.add(gbits, f.ngroups);
  L.bits.add(stream_bits, ns);
  bits_bytes = L.bits.bytes();
  return L;
}

AcCodes build_ac_codes(const uint32_t* hist, bool ans, uint8_t* ans_blob_out, uint32_t* packed_out) {
  AcCodes A;
  int group[kMaxClusters];
  if (ans) {
    cluster_ans_histograms(hist, kMaxClusters, group);
  } else {
    int ng = 0;
    for (int cl = 0; cl < kMaxClusters; cl++) {
      uint64_t tot = 0;
      for (int k = 0; k < kAlpha; k++) tot += hist[cl * kAlpha + k];
      group[cl] = tot ? ng++ : -1;
    }
  }
  int dense[kMaxClusters];
  std::fill(dense, dense + kMaxClusters, -1);
  int nhist = 0;
  A.ctxmap.resize(kAcCtx);
  uint8_t* ctxmap = A.ctxmap.data();  // (a local: byte stores may alias A's own members)
  for (int ctx = 0; ctx < kAcCtx; ctx++) {
    const int gr = group[ac_cluster(ctx)];
    if (gr >= 0 && dense[gr] < 0) dense[gr] = nhist++;
    ctxmap[ctx] = (uint8_t)(gr < 0 ? 0 : dense[gr]);
  }
  // no token at all (no frame has none: every varblock codes its non-zero
  // counts): one empty histogram, which is what a decoder reads for a map of
  // zeros -- with none the section would not parse
  if (nhist == 0) nhist = 1;
  A.nhist = nhist;
  std::fill(packed_out, packed_out + (size_t)kMaxClusters * kAlpha, 0u);
  if (ans) {
    A.tables.resize(nhist);
    // (a local vector: the compiler knows its storage aliases nothing and
    // vectorizes the sums; moved into A below)
    std::vector<uint32_t> dh((size_t)nhist * kAlpha, 0);
    for (int cl = 0; cl < kMaxClusters; cl++)
      if (group[cl] >= 0)
        for (int k = 0; k < kAlpha; k++) dh[dense[group[cl]] * kAlpha + k] += hist[cl * kAlpha + k];
    // device table blob (AnsArgs::tab): freq | cum << 16, alias inverses,
    // static cluster -> dense histogram
    uint8_t* blob = ans_blob_out;
    std::memset(blob, 0, kAnsTabBytes);
    uint32_t* sym = reinterpret_cast<uint32_t*>(blob);
    uint16_t* inv = reinterpret_cast<uint16_t*>(blob + kAnsInvOff);
    for (int h = 0; h < nhist; h++) {
      AnsTable& t = A.tables[h];
      t = build_ans_table(dh.data() + h * kAlpha);
      std::copy(t.inv.begin(), t.inv.end(), inv + (size_t)h * 4096);
      for (int k = 0; k < 128; k++) {
        const uint32_t f = t.freq[k];
        if (!f) continue;
        sym[h * 128 + k] = (f - 1) | (uint32_t)t.cum[k] << 12;
      }
    }
    for (int cl = 0; cl < kMaxClusters; cl++)
      blob[kAnsMapOff + cl] = (uint8_t)(group[cl] >= 0 ? dense[group[cl]] : 0);
    A.counts = std::move(dh);
  } else {
    A.codes.resize(nhist);
    for (int cl = 0; cl < kMaxClusters; cl++) {
      if (group[cl] < 0) continue;
      const int h = dense[group[cl]];
      A.codes[h] = build_prefix_code(hist + cl * kAlpha, kAlpha);
      for (int k = 0; k < kAlpha; k++) packed_out[cl * kAlpha + k] = A.codes[h].packed(k);
    }
  }
  return A;
}

void write_lf_global(BitWriter& w, uint32_t G, uint32_t qdc) {
  w.put(1, 1);  // LfChannelDequantization.all_default
  if (G <= 2048)
    write_u32_sel(w, 0, 11, G - 1);
  else if (G <= 4096)
    write_u32_sel(w, 1, 11, G - 2049);
  else if (G <= 8192)
    write_u32_sel(w, 2, 12, G - 4097);
  else
    write_u32_sel(w, 3, 16, G - 8193);
  if (qdc == 16)
    w.put(2, 0);
  else if (qdc <= 32)
    write_u32_sel(w, 1, 5, qdc - 1);
  else if (qdc <= 256)
    write_u32_sel(w, 2, 8, qdc - 1);
  else
    write_u32_sel(w, 3, 16, qdc - 1);
  w.put(1, 1);  // BlockCtxMap default
  w.put(1, 1);  // colour correlation default
  w.put(1, 0);  // GlobalModular: no tree, no channels
}

// the quant tables of the 128 / 256 px kinds the frame uses (e >= 8), the
// preset count, no coefficient orders
static void write_hf_head(BitWriter& w, uint32_t big_mask, uint32_t ngroups, uint32_t npresets) {
  write_dequant_matrices(w, big_mask);
  w.put(ceil_log2(ngroups), npresets - 1);  // num_hf_presets - 1
  write_u32_sel(w, 2, 0, 0);                // used_orders = 0
}
void write_hf_global(BitWriter& w, uint32_t big_mask, uint32_t ngroups, uint32_t npresets,
                     const std::vector<uint8_t>& ctxmap, int nhist,
                     const std::vector<PrefixCode>& codes, const BitWriter* cm_bits) {
  write_hf_head(w, big_mask, ngroups, npresets);
  write_histograms(w, ctxmap, nhist, codes, kCfg420, cm_bits);
}
void write_hf_global(BitWriter& w, uint32_t big_mask, uint32_t ngroups, uint32_t npresets,
                     const std::vector<uint8_t>& ctxmap, int nhist,
                     const std::vector<AnsTable>& tables, const BitWriter* cm_bits) {
  write_hf_head(w, big_mask, ngroups, npresets);
  write_ans_histograms(w, ctxmap, nhist, tables, kCfg420, cm_bits);
}

const BitWriter& CtxMapCache::get(const std::vector<uint8_t>& ctxmap, int nh) {
  if (nh != nhist || ctxmap != last) {
    bits = BitWriter();
    write_context_map(bits, ctxmap, nh);
    last = ctxmap;
    nhist = nh;
    writes++;
  }
  return bits;
}

static inline uint64_t group_tokens(const uint32_t* ntok, uint32_t g) {
  return (uint64_t)ntok[g * 3] + ntok[g * 3 + 1] + ntok[g * 3 + 2];
}

uint64_t layout_ac(const std::vector<uint32_t>& groups, const uint32_t* ntok,
                   const uint32_t* bound, bool ans, uint64_t* gbase_out) {
  uint64_t cursor = 0;
  for (uint32_t g : groups) {
    gbase_out[g] = cursor;
    // ANS: <= 16 + raw bits per token (prefix: <= 15 + raw) and the 32-bit state
    const uint64_t b = (uint64_t)bound[g] + (ans ? group_tokens(ntok, g) + 32 : 0);
    cursor += (b + 63) & ~31ull;
  }
  return (cursor / 32 + 2 + 63) & ~63ull;
}

uint64_t layout_lf(const Frame& f, const Plan& plan, const uint32_t* sbound, uint64_t* sbase_out) {
  uint64_t cursor = 0;
  for (uint32_t i = 0; i < f.nlf * 2; i++) {
    sbase_out[i] = cursor;
    if (plan.owns_lf(i / 2)) cursor += ((uint64_t)sbound[i] + 63) & ~31ull;
  }
  return cursor / 32 + 2;
}

// the 64 lanes of a chain workgroup hold groups of similar length, and the
// workgroups of short groups give their CUs (and their LDS, 139.5 KB each in
// the streamed form, 68 KB in the one-frame form) back early -- the kernel
// still lasts as long as the longest group
uint32_t ans_chain_order(const Plan& plan, const uint32_t* ntok, uint32_t* order_out) {
  const uint32_t ng = plan.ng();
  for (uint32_t i = 0; i < ng; i++) order_out[i] = i;  // launch slots
  const uint32_t* nt = ntok;
  const uint32_t* gl = plan.groups.data();
  std::stable_sort(order_out, order_out + ng, [nt, gl](uint32_t x, uint32_t y) {
    const uint32_t gx = gl[x], gy = gl[y];
    return nt[gx * 3] + nt[gx * 3 + 1] + nt[gx * 3 + 2] > nt[gy * 3] + nt[gy * 3 + 1] + nt[gy * 3 + 2];
  });
  uint32_t max_tokens = 0;
  for (uint32_t g : plan.groups)
    max_tokens = std::max(max_tokens, nt[g * 3] + nt[g * 3 + 1] + nt[g * 3 + 2]);
  return max_tokens;
}

void build_lf_codes(const Frame& f, const Plan& plan, const uint32_t* lfhist,
                    const uint32_t* vcount, uint32_t lf_code, uint32_t* lfpacked_out,
                    std::vector<BitWriter>& preA, std::vector<BitWriter>& preB) {
  std::fill(lfpacked_out, lfpacked_out + (size_t)f.nlf * 2 * 4 * kAlpha, 0u);
  preA.assign(f.nlf, BitWriter());
  preB.assign(f.nlf, BitWriter());
  for (uint32_t lg = 0; lg < f.nlf; lg++) {
    if (!plan.owns_lf(lg)) continue;
    const uint32_t bx0 = (lg % f.lfxs) * 256, by0 = (lg / f.lfxs) * 256;
    const uint32_t bw = std::min(256u, f.bxs - bx0), bh = std::min(256u, f.bys - by0);
    for (int sidx = 0; sidx < 2; sidx++) {
      const uint32_t sid = lg * 2 + sidx;
      const int nleaves = sidx == 0 ? 3 : 4;
      std::vector<PrefixCode> lc(nleaves);
      for (int l = 0; l < nleaves; l++) {
        lc[l] = build_prefix_code(lfhist + ((size_t)sid * 4 + l) * kAlpha, kAlpha);
        for (int k = 0; k < kAlpha; k++) lfpacked_out[((size_t)sid * 4 + l) * kAlpha + k] = lc[l].packed(k);
      }
      if (sidx == 0) {
        preA[lg].put(2, 0);  // extra_precision
        write_modular_prelude(preA[lg], kDcTree, 5, 3, lc);
      } else {
        preB[lg].put(ceil_log2(bw * bh), vcount[lg] - 1);  // varblock count - 1
        write_modular_prelude(preB[lg], (lf_code >> 1) ? kMetaTreeEpf : kMetaTree, 7, 4, lc);
      }
    }
  }
}

}  // namespace jxg
