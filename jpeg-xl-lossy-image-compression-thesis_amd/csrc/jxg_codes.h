// jxg_codes.h -- what the host builds between a frame's statistics and its
// emission (stage F): the AC stream's context map and prefix codes / ANS
// tables, LfGlobal and HfGlobal, the bit layout of the pass groups and LF
// streams in their arenas, the rANS chain order, the LF-group codes and
// Modular preludes.  Host only (no HIP include): statistics in, tables out
// through the caller's pointers (stage_codes passes its pinned upload
// sections, tests/native/codes_host.cpp plain vectors).
#pragma once
#include <cstdint>
#include <vector>

#include "jxg_acmodel.h"
#include "jxg_bitstream.h"
#include "jxg_layout.h"
#include "jxg_plan.h"

#pragma GCC visibility push(hidden)
namespace jxg {

// The three per-frame arenas that exist in device memory and in a pinned host
// mirror, each section declared once (stage_alloc allocates and commits them).
struct EncArenas {
  // Statistics, zeroed by the front kernel and downloaded by two copies (AC
  // part, LF part): [hist_ac | bound | ntok | bandtok | bigcount][lfhist |
  // sbound | vcount].  bandtok is read on the device only.
  Mirror<uint32_t> hist_ac, bound, ntok, bandtok, bigcount, lfhist, sbound, vcount;
  size_t stat_lf = 0, stat_bytes = 0;  // byte offset of the LF part, total
  // Code tables, uploaded by one copy (ANS) or two (prefix codes: the AC part
  // ahead of the AC emission): [codes_ac | gbase | ans_order | ans_tab]
  // [lfcodes | stream_base]
  Mirror<uint32_t> codes_ac, ans_order, lfcodes;
  Mirror<uint64_t> gbase, stream_base;
  Mirror<uint8_t> ans_tab;
  size_t up_gbase = 0, up_ac = 0, up_lf = 0, up_bytes = 0;
  // emitted bit counts, one download: [gbits | stream_bits]
  Mirror<uint32_t> gbits, stream_bits;
  size_t bits_bytes = 0;

  struct Layouts {
    ArenaLayout stat, up, bits;
  };
  // the sections of a frame whose plan has plan_groups pass groups
  Layouts declare(const Frame& f, uint32_t plan_groups);
};

// The AC stream's entropy code.  Prefix codes: one histogram per used static
// cluster; ANS: the static clusters clustered again into <= kAnsMaxHists
// groups (the alias inverses must fit the encoder's LDS).  Dense histogram ids
// in order of first appearance over the contexts (oracle/encode.c).
struct AcCodes {
  std::vector<uint8_t> ctxmap;     // [kAcCtx] context -> dense histogram
  int nhist = 0;                   // histograms (>= 1: an empty one when no token at all)
  std::vector<PrefixCode> codes;   // prefix codes: [nhist]
  std::vector<AnsTable> tables;    // ANS: [nhist]
  std::vector<uint32_t> counts;    // ANS: [nhist][kAlpha] clustered counts
};
// hist: [kMaxClusters][kAlpha].  packed_out: [kMaxClusters][kAlpha] device
// prefix codes (code | len << 16; zeros with ANS).  ans_blob_out (ANS only):
// the kAnsTabBytes table blob of jxg_acmodel.h.
AcCodes build_ac_codes(const uint32_t* hist, bool ans, uint8_t* ans_blob_out, uint32_t* packed_out);

// LfGlobal of a VarDCT frame: default LF dequantization, the quantizer's global
// scale and DC quantizer, default block context map and colour correlation,
// an empty GlobalModular
void write_lf_global(BitWriter& w, uint32_t G, uint32_t qdc);

// HfGlobal: DequantMatrices of the big kinds in big_mask, num_hf_presets, no
// coefficient orders, then the histograms of all presets' contexts
// (ctxmap: [npresets][kAcCtx]).  cm_bits: the serialised context map, or null
// to write it here.
void write_hf_global(BitWriter& w, uint32_t big_mask, uint32_t ngroups, uint32_t npresets,
                     const std::vector<uint8_t>& ctxmap, int nhist,
                     const std::vector<PrefixCode>& codes, const BitWriter* cm_bits);
void write_hf_global(BitWriter& w, uint32_t big_mask, uint32_t ngroups, uint32_t npresets,
                     const std::vector<uint8_t>& ctxmap, int nhist,
                     const std::vector<AnsTable>& tables, const BitWriter* cm_bits);

// the serialised AC context map of the previous frame, reused while the map
// and its histogram count stay equal
struct CtxMapCache {
  std::vector<uint8_t> last;
  int nhist = -1;
  BitWriter bits;
  uint32_t writes = 0;  // serialisations so far
  const BitWriter& get(const std::vector<uint8_t>& ctxmap, int nh);
};

// AC layout: the plan's groups back to back in the bit arena, 32-bit aligned.
// ntok: [ngroups][3], bound: [ngroups] bit upper bounds; gbase_out: [ngroups],
// written for the plan's groups only.  Returns the arena's 32-bit words.
uint64_t layout_ac(const std::vector<uint32_t>& groups, const uint32_t* ntok,
                   const uint32_t* bound, bool ans, uint64_t* gbase_out);
// LF layout: the streams of the plan's LF groups (sbase_out: [2 nlf], all
// written).  Returns the arena's 32-bit words.
uint64_t layout_lf(const Frame& f, const Plan& plan, const uint32_t* sbound, uint64_t* sbase_out);
// rANS chain order: the plan's launch slots by token count, longest first
// (stable), into order_out[plan.ng()].  Returns the most tokens of any group.
uint32_t ans_chain_order(const Plan& plan, const uint32_t* ntok, uint32_t* order_out);

// LF-group stream codes and preludes of the plan's LF groups.  lfhist:
// [2 nlf][4 leaves][kAlpha], vcount: [nlf] varblocks; lfpacked_out: the same
// shape as lfhist (code | len << 16, zero where unused); preA / preB: [nlf]
// GroupHeader + tree + leaf codes of the DC stream / of the varblock count and
// the metadata stream.
void build_lf_codes(const Frame& f, const Plan& plan, const uint32_t* lfhist,
                    const uint32_t* vcount, uint32_t lf_code, uint32_t* lfpacked_out,
                    std::vector<BitWriter>& preA, std::vector<BitWriter>& preB);

}  // namespace jxg
#pragma GCC visibility pop
