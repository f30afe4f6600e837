// jxg_decode.cpp -- host side of the decoder: headers, TOC, LfGlobal, the LF
// groups' modular streams, HfGlobal, histogram -> decode-table construction,
// and a host loop over the pass groups.  Plain C++ (no HIP): builds with g++
// alone for the CPU tests and tests/native/decode_mutate.cpp.  The grammar is
// the one oracle/jxl_decode.py decode() accepts ([ext] ISO/IEC 18181-1
// restricted to what this encoder writes); anything else is
// JXG_ERR_UNSUPPORTED, a malformed stream JXG_ERR_INVALID_ARG.
#include "jxg_decode.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <future>
#include <new>
#include <system_error>

namespace jxg {
namespace {

using dec::AnsEntry;
using dec::BitReader;
using dec::br_peek;
using dec::br_read;
using dec::br_skip;
using dec::HistDesc;

constexpr int kInv = JXG_ERR_INVALID_ARG, kUns = JXG_ERR_UNSUPPORTED;
#define DEC_TRY(expr)          \
  do {                         \
    const int st_ = (expr);    \
    if (st_) return st_;       \
  } while (0)
#define DEC_BITS(br) \
  do {               \
    if ((br).err) return kInv; \
  } while (0)

uint32_t ceil_log2(uint32_t x) {
  uint32_t n = 0;
  while (n < 32 && (1ull << n) < x) n++;
  return n;
}

// U32(d0, d1, d2, d3): bits < 0 means the constant `add`
struct U32Dist {
  int bits;
  uint32_t add;
};
uint32_t read_u32(BitReader& br, const U32Dist (&d)[4]) {
  const U32Dist& s = d[br_read(br, 2)];
  return s.bits < 0 ? s.add : br_read(br, (uint32_t)s.bits) + s.add;
}
uint64_t read_u64(BitReader& br) {
  const uint32_t sel = br_read(br, 2);
  if (sel == 0) return 0;
  if (sel == 1) return 1 + br_read(br, 4);
  if (sel == 2) return 17 + br_read(br, 8);
  uint64_t v = br_read(br, 12);
  uint32_t shift = 12;
  while (!br.err && br_read(br, 1)) {
    if (shift == 60) {
      v |= (uint64_t)br_read(br, 4) << 60;
      break;
    }
    v |= (uint64_t)br_read(br, 8) << shift;
    shift += 8;
  }
  return v;
}
uint32_t read_varlen(BitReader& br, uint32_t nb) {  // varlen u8 (nb 3) / u16 (nb 4)
  if (!br_read(br, 1)) return 0;
  const uint32_t n = br_read(br, nb);
  return n == 0 ? 1u : br_read(br, n) + (1u << n);
}

// ---- prefix codes (Brotli style, read LSB first) ----
constexpr uint32_t kMaxPrefixAlphabet = 256;  // what this encoder's codes span

// lengths[alphabet] -> one histogram's table in the pool
int build_prefix_table(const uint8_t* lengths, uint32_t alphabet, DecEntropy* E, HistDesc* h) {
  uint32_t count[16] = {};
  uint32_t maxlen = 0, used = 0;
  for (uint32_t s = 0; s < alphabet; s++)
    if (lengths[s]) {
      count[lengths[s]]++;
      used++;
      maxlen = std::max<uint32_t>(maxlen, lengths[s]);
    }
  h->maxlen = 0;
  h->single = 0;
  if (used == 0) return 0;  // the single symbol 0
  // One used symbol with a non-zero length (a complex-coded code of one
  // symbol, which the format reads in zero bits): this encoder writes such a
  // code in the simple form, and the grammar this decoder follows
  // (oracle/jxl_decode.py PrefixCode) does not accept it -- outside the subset
  if (used == 1) return kUns;
  uint64_t kraft = 0;
  for (uint32_t l = 1; l < 16; l++) kraft += (uint64_t)count[l] << (15 - l);
  if (kraft != (1u << 15)) return kInv;  // incomplete or over-subscribed
  uint32_t next[16] = {};
  uint32_t code = 0;
  for (uint32_t l = 1; l < 16; l++) {
    code = (code + count[l - 1]) << 1;
    next[l] = code;
  }
  h->maxlen = (uint8_t)maxlen;
  h->off = (uint32_t)E->ptab.size();
  E->ptab.resize(E->ptab.size() + ((size_t)1 << maxlen), 0);
  uint16_t* tab = E->ptab.data() + h->off;
  for (uint32_t s = 0; s < alphabet; s++) {
    const uint32_t l = lengths[s];
    if (!l) continue;
    const uint32_t c = next[l]++;
    uint32_t rev = 0;
    for (uint32_t b = 0; b < l; b++) rev |= ((c >> b) & 1u) << (l - 1 - b);
    for (uint32_t i = rev; i < (1u << maxlen); i += 1u << l) tab[i] = (uint16_t)(l << 8 | s);
  }
  return 0;
}

void single_symbol(HistDesc* h, uint32_t sym) {
  h->maxlen = 0;
  h->single = (uint16_t)sym;
}

int read_simple_prefix(BitReader& br, uint32_t alphabet, DecEntropy* E, HistDesc* h) {
  uint32_t max_bits = 0;
  while ((1u << max_bits) < alphabet) max_bits++;
  const uint32_t nsym = br_read(br, 2) + 1;
  uint32_t syms[4];
  for (uint32_t i = 0; i < nsym; i++) {
    syms[i] = br_read(br, max_bits);
    if (syms[i] >= alphabet) return kInv;
    for (uint32_t j = 0; j < i; j++)
      if (syms[j] == syms[i]) return kInv;
  }
  DEC_BITS(br);
  if (nsym == 1) {
    single_symbol(h, syms[0]);
    return 0;
  }
  uint8_t lengths[kMaxPrefixAlphabet] = {};
  if (nsym == 2) {
    lengths[syms[0]] = lengths[syms[1]] = 1;
  } else if (nsym == 3) {
    lengths[syms[0]] = 1;
    lengths[syms[1]] = lengths[syms[2]] = 2;
  } else if (br_read(br, 1)) {
    lengths[syms[0]] = 1;
    lengths[syms[1]] = 2;
    lengths[syms[2]] = lengths[syms[3]] = 3;
  } else {
    for (uint32_t i = 0; i < 4; i++) lengths[syms[i]] = 2;
  }
  DEC_BITS(br);
  return build_prefix_table(lengths, alphabet, E, h);
}

int read_prefix_code(BitReader& br, uint32_t alphabet, DecEntropy* E, HistDesc* h) {
  static const uint8_t kClOrder[18] = {1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15};
  // static code of the code-length code lengths: 4-bit peek -> (bits, value)
  static const uint8_t kClcl[16][2] = {{2, 0}, {2, 4}, {2, 3}, {3, 2}, {2, 0}, {2, 4},
                                       {2, 3}, {4, 1}, {2, 0}, {2, 4}, {2, 3}, {3, 2},
                                       {2, 0}, {2, 4}, {2, 3}, {4, 5}};
  if (alphabet == 1) {
    single_symbol(h, 0);
    return 0;
  }
  if (alphabet > kMaxPrefixAlphabet) return kUns;
  const uint32_t hskip = br_read(br, 2);
  if (hskip == 1) return read_simple_prefix(br, alphabet, E, h);
  uint8_t cl[18] = {};
  int space = 32;
  uint32_t ncodes = 0;
  for (uint32_t i = hskip; i < 18 && space > 0; i++) {
    const uint8_t* e = kClcl[br_peek(br) & 15];
    br_skip(br, e[0]);
    cl[kClOrder[i]] = e[1];
    if (e[1]) {
      space -= 32 >> e[1];
      ncodes++;
    }
  }
  DEC_BITS(br);
  if (!(ncodes == 1 || space == 0)) return kInv;
  // the code-length code: an 18-symbol prefix code (5-bit table) or one symbol
  uint8_t cl_tab[32][2] = {};
  uint32_t cl_only = 0;
  if (ncodes == 1) {
    for (uint32_t s = 0; s < 18; s++)
      if (cl[s]) cl_only = s;
  } else {
    uint32_t count[6] = {}, next[6] = {}, code = 0;
    for (uint32_t s = 0; s < 18; s++) count[cl[s]]++;
    count[0] = 0;
    for (uint32_t l = 1; l < 6; l++) {
      code = (code + count[l - 1]) << 1;
      next[l] = code;
    }
    for (uint32_t s = 0; s < 18; s++) {
      const uint32_t l = cl[s];
      if (!l) continue;
      const uint32_t c = next[l]++;
      uint32_t rev = 0;
      for (uint32_t b = 0; b < l; b++) rev |= ((c >> b) & 1u) << (l - 1 - b);
      for (uint32_t i = rev; i < 32; i += 1u << l) {
        cl_tab[i][0] = (uint8_t)l;
        cl_tab[i][1] = (uint8_t)s;
      }
    }
  }
  uint8_t lengths[kMaxPrefixAlphabet] = {};
  uint32_t sym = 0, prev_len = 8, repeat = 0, repeat_len = 0;
  int space15 = 32768;
  while (sym < alphabet && space15 > 0) {
    uint32_t v = cl_only;
    if (ncodes != 1) {
      const uint8_t* e = cl_tab[br_peek(br) & 31];
      br_skip(br, e[0]);
      v = e[1];
    }
    DEC_BITS(br);
    if (v < 16) {
      repeat = 0;
      lengths[sym++] = (uint8_t)v;
      if (v) {
        prev_len = v;
        space15 -= 32768 >> v;
      }
    } else {
      const uint32_t extra = v == 16 ? 2 : 3;
      const uint32_t new_len = v == 16 ? prev_len : 0;
      if (repeat_len != new_len) {
        repeat = 0;
        repeat_len = new_len;
      }
      const uint32_t old = repeat;
      if (repeat > 0) repeat = (repeat - 2) << extra;
      repeat += br_read(br, extra) + 3;
      const uint32_t delta = repeat - old;
      if (sym + delta > alphabet) return kInv;
      for (uint32_t k = 0; k < delta; k++) lengths[sym + k] = (uint8_t)repeat_len;
      sym += delta;
      if (repeat_len) space15 -= (int)(delta << (15 - repeat_len));
    }
  }
  DEC_BITS(br);
  if (space15 != 0) return kInv;
  return build_prefix_table(lengths, alphabet, E, h);
}

// ---- ANS: 12-bit precision, alias tables ----
struct LogCountTable {
  uint8_t len[128], sym[128];
  LogCountTable() {
    static const uint8_t k[14][2] = {{5, 17}, {4, 11}, {4, 15}, {4, 3}, {4, 9},  {4, 7},  {3, 4},
                                     {3, 2},  {3, 5},  {3, 6},  {3, 0}, {6, 33}, {7, 1},  {7, 65}};
    std::memset(len, 0, sizeof(len));
    std::memset(sym, 0, sizeof(sym));
    for (int s = 0; s < 14; s++)
      for (int hi = 0; hi < (1 << (7 - k[s][0])); hi++) {
        len[k[s][1] | (hi << k[s][0])] = k[s][0];
        sym[k[s][1] | (hi << k[s][0])] = (uint8_t)s;
      }
  }
};

// counts[n] (n <= 258), summing to 4096
int read_ans_histogram(BitReader& br, std::vector<int>* counts) {
  static const LogCountTable kLog;
  const int total = 1 << 12;
  counts->clear();
  if (br_read(br, 1)) {  // simple
    const uint32_t nsym = br_read(br, 1) + 1;
    uint32_t syms[2] = {0, 0};
    for (uint32_t i = 0; i < nsym; i++) syms[i] = read_varlen(br, 3);
    counts->assign(std::max(syms[0], syms[1]) + 1, 0);
    if (nsym == 1) {
      (*counts)[syms[0]] = total;
    } else {
      if (syms[0] == syms[1]) return kInv;
      (*counts)[syms[0]] = (int)br_read(br, 12);
      (*counts)[syms[1]] = total - (*counts)[syms[0]];
    }
    DEC_BITS(br);
    return 0;
  }
  if (br_read(br, 1)) {  // flat
    const int alpha = (int)read_varlen(br, 3) + 1;
    DEC_BITS(br);
    counts->assign(alpha, total / alpha);
    for (int i = 0; i < total % alpha; i++) (*counts)[i]++;
    return 0;
  }
  uint32_t log = 0;
  while (log < 3 && br_read(br, 1)) log++;
  const int shift = (int)((br_read(br, log) | (1u << log)) - 1);
  if (shift > 13) return kInv;
  const int length = (int)read_varlen(br, 3) + 3;
  DEC_BITS(br);
  int logcounts[260] = {}, same[260] = {};
  int omit_log = -1, omit_pos = -1;
  for (int i = 0; i < length;) {
    const uint32_t p = (uint32_t)br_peek(br) & 127;
    if (!kLog.len[p]) return kInv;
    br_skip(br, kLog.len[p]);
    const int v = kLog.sym[p];
    logcounts[i] = v;
    if (v == 13) {
      const int rle = (int)read_varlen(br, 3);
      same[i] = rle + 5;
      i += rle + 4;
      continue;
    }
    if (v > omit_log) {
      omit_log = v;
      omit_pos = i;
    }
    i++;
  }
  DEC_BITS(br);
  if (omit_pos < 0) return kInv;
  if (omit_pos + 1 < length && logcounts[omit_pos + 1] == 13) return kInv;
  counts->assign(length, 0);
  int prev = 0, numsame = 0, tot = 0;
  for (int i = 0; i < length; i++) {
    int& cnt = (*counts)[i];
    if (same[i]) {
      numsame = same[i] - 1;
      prev = i > 0 ? (*counts)[i - 1] : 0;
    }
    if (numsame > 0) {
      cnt = prev;
      numsame--;
    } else {
      const int code = logcounts[i];
      if (i == omit_pos || code == 0) continue;
      if (code == 1) {
        cnt = 1;
      } else {
        int bc = std::min(code - 1, shift - ((12 - (code - 1)) >> 1));
        bc = std::max(bc, 0);
        cnt = (1 << (code - 1)) + (int)(br_read(br, (uint32_t)bc) << (code - 1 - bc));
      }
    }
    tot += cnt;
    if (tot > total) return kInv;
  }
  DEC_BITS(br);
  (*counts)[omit_pos] = total - tot;
  if ((*counts)[omit_pos] <= 0) return kInv;
  return 0;
}

// counts (sum 4096) -> 1 << log_alpha alias entries
int build_alias_table(const std::vector<int>& counts_in, uint32_t log_alpha, AnsEntry* out) {
  const int table_size = 1 << log_alpha, entry = 4096 >> log_alpha;
  if ((int)counts_in.size() > table_size) return kInv;
  std::vector<int> counts(counts_in);
  counts.resize(table_size, 0);
  int nz = 0, last = 0, sum = 0;
  for (int i = 0; i < table_size; i++) {
    if (counts[i] < 0) return kInv;
    sum += counts[i];
    if (counts[i]) {
      nz++;
      last = i;
    }
  }
  if (sum != 4096 || nz == 0) return kInv;
  std::vector<int> cutoff(table_size, 0), right(table_size, 0), offset(table_size, 0);
  if (nz == 1) {
    for (int i = 0; i < table_size; i++) {
      right[i] = last;
      offset[i] = i * entry;
    }
  } else {
    std::vector<int> cut(counts), under, over;
    for (int i = 0; i < table_size; i++) {
      if (cut[i] > entry)
        over.push_back(i);
      else if (cut[i] < entry)
        under.push_back(i);
    }
    while (!over.empty()) {
      if (under.empty()) return kInv;
      const int o = over.back(), u = under.back();
      under.pop_back();
      const int by = entry - cut[u];
      cut[o] -= by;
      right[u] = o;
      offset[u] = cut[o];
      if (cut[o] < entry) {
        over.pop_back();
        under.push_back(o);
      } else if (cut[o] == entry) {
        over.pop_back();
      }
    }
    for (int i = 0; i < table_size; i++) {
      if (cut[i] == entry) {
        right[i] = i;
        offset[i] = 0;
        cutoff[i] = 0;
      } else {
        offset[i] -= cut[i];
        cutoff[i] = cut[i];
      }
    }
  }
  for (int i = 0; i < table_size; i++) {
    out[i].cutoff = (uint16_t)cutoff[i];
    out[i].right = (uint16_t)right[i];
    out[i].freq0 = (uint16_t)counts[i];
    out[i].freq1 = (uint16_t)counts[right[i]];
    out[i].offset = offset[i];
  }
  return 0;
}

int read_uint_config(BitReader& br, uint32_t log_alpha, HistDesc* h) {
  const uint32_t split_exp = br_read(br, ceil_log2(log_alpha + 1));
  uint32_t msb = 0, lsb = 0;
  if (split_exp > log_alpha) return kInv;
  if (split_exp != log_alpha) {
    msb = br_read(br, ceil_log2(split_exp + 1));
    if (msb > split_exp) return kInv;
    lsb = br_read(br, ceil_log2(split_exp - msb + 1));
    if (msb + lsb > split_exp) return kInv;
  }
  DEC_BITS(br);
  h->split_exp = (uint8_t)split_exp;
  h->msb = (uint8_t)msb;
  h->lsb = (uint8_t)lsb;
  return 0;
}

int read_entropy(BitReader& br, uint32_t nctx, DecEntropy* E);

int read_context_map(BitReader& br, uint32_t n, std::vector<uint8_t>* cm) {
  cm->assign(n, 0);
  if (br_read(br, 1)) {  // simple
    const uint32_t bits = br_read(br, 2);
    for (uint32_t i = 0; i < n; i++) (*cm)[i] = (uint8_t)br_read(br, bits);
    DEC_BITS(br);
  } else {
    const uint32_t use_mtf = br_read(br, 1);
    DecEntropy es;
    DEC_TRY(read_entropy(br, 1, &es));
    const dec::SymReader S = es.view();
    uint32_t state = es.prefix ? 0u : br_read(br, 32);
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t v = dec::read_ctx(br, S, 0, state);
      DEC_BITS(br);
      if (v > 255) return kInv;
      (*cm)[i] = (uint8_t)v;
    }
    if (!es.prefix && state != dec::kAnsFinalState) return kInv;
    if (use_mtf) {
      uint8_t mtf[256];
      for (int i = 0; i < 256; i++) mtf[i] = (uint8_t)i;
      for (uint32_t i = 0; i < n; i++) {
        const uint8_t v = (*cm)[i], s = mtf[v];
        (*cm)[i] = s;
        if (v) {
          std::memmove(mtf + 1, mtf, v);
          mtf[0] = s;
        }
      }
    }
  }
  bool seen[256] = {};
  uint32_t mx = 0, distinct = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (!seen[(*cm)[i]]) {
      seen[(*cm)[i]] = true;
      distinct++;
    }
    mx = std::max<uint32_t>(mx, (*cm)[i]);
  }
  if (distinct != mx + 1) return kInv;
  return 0;
}

// DecodeHistograms: LZ77 bit, context map, coder, uint configs, codes
int read_entropy(BitReader& br, uint32_t nctx, DecEntropy* E) {
  if (br_read(br, 1)) return br.err ? kInv : kUns;  // LZ77
  if (nctx > 1)
    DEC_TRY(read_context_map(br, nctx, &E->ctxmap));
  else
    E->ctxmap.assign(1, 0);
  const uint32_t nh = *std::max_element(E->ctxmap.begin(), E->ctxmap.end()) + 1u;
  E->prefix = br_read(br, 1);
  E->log_alpha = E->prefix ? 15 : 5 + br_read(br, 2);
  DEC_BITS(br);
  E->hist.assign(nh, HistDesc{});
  for (uint32_t i = 0; i < nh; i++) DEC_TRY(read_uint_config(br, E->log_alpha, &E->hist[i]));
  if (E->prefix) {
    std::vector<uint32_t> alphas(nh);
    for (uint32_t i = 0; i < nh; i++) alphas[i] = read_varlen(br, 4) + 1;
    DEC_BITS(br);
    for (uint32_t i = 0; i < nh; i++) DEC_TRY(read_prefix_code(br, alphas[i], E, &E->hist[i]));
    if (E->ptab.empty()) E->ptab.assign(1, 0);
  } else {
    const size_t ts = (size_t)1 << E->log_alpha;
    E->atab.assign(nh * ts, AnsEntry{});
    std::vector<int> counts;
    for (uint32_t i = 0; i < nh; i++) {
      DEC_TRY(read_ans_histogram(br, &counts));
      E->hist[i].off = (uint32_t)(i * ts);
      DEC_TRY(build_alias_table(counts, E->log_alpha, E->atab.data() + i * ts));
    }
  }
  return 0;
}

// ---- modular sub-streams of the LF groups ----
struct TreeNode {
  int prop;  // < 0: leaf
  int32_t splitval;
  uint32_t lchild, rchild;  // value > splitval: lchild
  uint32_t leaf, pred;
  int64_t offset, mul;
};
constexpr size_t kMaxTreeNodes = 1u << 14;

int read_tree(BitReader& br, std::vector<TreeNode>* nodes, uint32_t* nleaves) {
  DecEntropy es;
  DEC_TRY(read_entropy(br, 6, &es));
  const dec::SymReader S = es.view();
  uint32_t state = es.prefix ? 0u : br_read(br, 32);
  nodes->clear();
  uint64_t to_decode = 1;
  uint32_t leaf_id = 0;
  while (to_decode > 0) {
    to_decode--;
    if (nodes->size() >= kMaxTreeNodes) return kUns;
    const uint32_t prop = dec::read_ctx(br, S, 1, state);
    DEC_BITS(br);
    if (prop > 256) return kInv;
    TreeNode n{};
    if (prop == 0) {
      const uint32_t pred = dec::read_ctx(br, S, 2, state);
      const int32_t off = dec::unpack_signed(dec::read_ctx(br, S, 3, state));
      const uint32_t mlog = dec::read_ctx(br, S, 4, state);
      const uint32_t mbits = dec::read_ctx(br, S, 5, state);
      DEC_BITS(br);
      if (pred > 13) return kInv;
      if (!(pred <= 3 || pred == 5 || pred == 8)) return kUns;
      if (mlog > 30 || (((uint64_t)mbits + 1) << mlog) > 0x7FFFFFFFull) return kUns;
      n.prop = -1;
      n.leaf = leaf_id++;
      n.pred = pred;
      n.offset = off;
      n.mul = (int64_t)(((uint64_t)mbits + 1) << mlog);
    } else {
      const int32_t sv = dec::unpack_signed(dec::read_ctx(br, S, 0, state));
      DEC_BITS(br);
      if (!(prop - 1 == 0 || prop - 1 == 2 || prop - 1 == 3)) return kUns;
      n.prop = (int)prop - 1;
      n.splitval = sv;
      n.lchild = (uint32_t)(nodes->size() + to_decode + 1);
      n.rchild = (uint32_t)(nodes->size() + to_decode + 2);
      to_decode += 2;
    }
    nodes->push_back(n);
  }
  if (!es.prefix && state != dec::kAnsFinalState) return kInv;
  for (const TreeNode& n : *nodes)
    if (n.prop >= 0 && (n.lchild >= nodes->size() || n.rchild >= nodes->size())) return kInv;
  *nleaves = leaf_id;
  return 0;
}

struct Channel {
  uint32_t w, h;
  std::vector<int32_t> v;
};

int read_modular(BitReader& br, std::vector<Channel>* chans) {
  if (br_read(br, 1)) return br.err ? kInv : kUns;   // global tree
  if (!br_read(br, 1)) return br.err ? kInv : kUns;  // custom weighted-predictor header
  static const U32Dist kNtr[4] = {{-1, 0}, {-1, 1}, {4, 2}, {8, 18}};
  if (read_u32(br, kNtr)) return br.err ? kInv : kUns;  // transforms
  DEC_BITS(br);
  std::vector<TreeNode> nodes;
  uint32_t nleaves = 0;
  DEC_TRY(read_tree(br, &nodes, &nleaves));
  DecEntropy es;
  DEC_TRY(read_entropy(br, nleaves, &es));
  const dec::SymReader S = es.view();
  uint32_t state = es.prefix ? 0u : br_read(br, 32);
  for (size_t ci = 0; ci < chans->size(); ci++) {
    Channel& ch = (*chans)[ci];
    const uint32_t w = ch.w, h = ch.h;
    ch.v.assign((size_t)w * h, 0);
    for (uint32_t y = 0; y < h; y++) {
      int32_t* row = ch.v.data() + (size_t)y * w;
      const int32_t* up = y ? row - w : nullptr;
      for (uint32_t x = 0; x < w; x++) {
        const TreeNode* n = &nodes[0];
        while (n->prop >= 0) {
          const int64_t v = n->prop == 0 ? (int64_t)ci : (n->prop == 2 ? (int64_t)y : (int64_t)x);
          n = &nodes[v > n->splitval ? n->lchild : n->rchild];
        }
        const int64_t r = dec::unpack_signed(dec::read_ctx(br, S, n->leaf, state));
        DEC_BITS(br);
        int64_t p = 0;
        if (n->pred) {
          const int64_t W = x ? row[x - 1] : (up ? up[x] : 0);
          const int64_t N = up ? up[x] : W;
          const int64_t NW = (x && up) ? up[x - 1] : W;
          switch (n->pred) {
            case 1: p = W; break;
            case 2: p = N; break;
            case 3: p = (W + N) >> 1; break;  // floor, as the oracle's //
            case 5: {
              const int64_t g = W + N - NW, lo = std::min(W, N), hi = std::max(W, N);
              p = std::min(std::max(g, lo), hi);
              break;
            }
            default: p = NW; break;  // 8
          }
        }
        const int64_t val = r * n->mul + n->offset + p;
        if (val < INT32_MIN || val > INT32_MAX) return kInv;
        row[x] = (int32_t)val;
      }
    }
  }
  if (!es.prefix && state != dec::kAnsFinalState) return kInv;
  return 0;
}

// one LF group: DC (Y, X, B), then CfL, strategy / quant-field rows and the
// EPF sharpness; the varblock placement is rebuilt from the strategy list
int decode_lf_group(BitReader& s, DecFrame* F, uint32_t lg, uint32_t* big_used) {
  const uint32_t lgx = lg % F->lfxs, lgy = lg / F->lfxs;
  const uint32_t bx0 = lgx * 256, by0 = lgy * 256;
  const uint32_t bw = std::min(256u, F->bxs - bx0), bh = std::min(256u, F->bys - by0);
  const size_t nb = (size_t)F->bxs * F->bys;
  if (br_read(s, 2)) return s.err ? kInv : kUns;  // extra_precision
  std::vector<Channel> ch(3);
  for (Channel& c : ch) {
    c.w = bw;
    c.h = bh;
  }
  DEC_TRY(read_modular(s, &ch));
  static const int kChan[3] = {1, 0, 2};
  for (int mi = 0; mi < 3; mi++)
    for (uint32_t y = 0; y < bh; y++)
      std::memcpy(&F->dc[kChan[mi] * nb + (size_t)(by0 + y) * F->bxs + bx0],
                  &ch[mi].v[(size_t)y * bw], bw * sizeof(int32_t));
  const uint32_t count = br_read(s, ceil_log2(bw * bh)) + 1;
  DEC_BITS(s);
  if (count > bw * bh) return kInv;
  const uint32_t cw = (bw + 7) / 8, chh = (bh + 7) / 8;
  std::vector<Channel> meta(4);
  meta[0].w = meta[1].w = cw;
  meta[0].h = meta[1].h = chh;
  meta[2].w = count;
  meta[2].h = 2;
  meta[3].w = bw;
  meta[3].h = bh;
  DEC_TRY(read_modular(s, &meta));
  const size_t ntiles = (size_t)F->tiles_x * F->tiles_y;
  for (int i = 0; i < 2; i++)
    for (uint32_t y = 0; y < chh; y++)
      for (uint32_t x = 0; x < cw; x++) {
        const int32_t m = meta[i].v[(size_t)y * cw + x];
        if (m < -128 || m > 127) return kInv;
        F->cmap[i * ntiles + (size_t)(by0 / 8 + y) * F->tiles_x + bx0 / 8 + x] = (int8_t)m;
      }
  for (int32_t sh : meta[3].v) {
    if (sh < 0 || sh > 7) return kInv;
    // the reconstruction's EPF sigma table is built for one sharpness
    if (F->info.epf_iters && sh != 4) return kUns;
  }
  std::vector<uint8_t> covered((size_t)bw * bh, 0);
  uint32_t k = 0;
  for (uint32_t y = 0; y < bh; y++)
    for (uint32_t x = 0; x < bw; x++) {
      if (covered[(size_t)y * bw + x]) continue;
      if (k >= count) return kInv;
      const int32_t t = meta[2].v[k];
      const uint32_t shape = t < 0 ? 0u : dec::strategy_shape((uint32_t)t);
      if (!shape) return (t >= 0 && t < 27) ? kUns : kInv;
      const uint32_t cy = shape & 0xFF, cx = shape >> 8;
      if (y + cy > bh || x + cx > bw) return kInv;
      // the kernels handle a varblock inside one 64 x 64 tile (<= 64 px) or
      // one pass group (128 / 256 px), which is where this encoder puts them
      const uint32_t cell = t >= 21 ? 32u : 8u;
      if (x % cell + cx > cell || y % cell + cy > cell) return kUns;
      if (t >= 21) *big_used |= t == 21 ? 2u : (t == 24 ? 8u : (t <= 23 ? 1u : 4u));
      const int32_t q = std::min(std::max(meta[2].v[(size_t)count + k], 0), 255);
      for (uint32_t iy = 0; iy < cy; iy++)
        for (uint32_t ix = 0; ix < cx; ix++) {
          if (covered[(size_t)(y + iy) * bw + x + ix]) return kInv;  // overlapping
          covered[(size_t)(y + iy) * bw + x + ix] = 1;
          const size_t b = (size_t)(by0 + y + iy) * F->bxs + bx0 + x + ix;
          F->acs[b] = (uint8_t)(t | ((iy || ix) ? 0x80 : 0));
          F->qf[b] = (uint8_t)q;
        }
      k++;
    }
  if (k != count) return kInv;
  return 0;
}

int read_dequant_matrices(BitReader& br, DecFrame* F) {
  // table of the format's order -> the encoder's 128 / 256 px kind, or -1
  static const int kTableBig[17] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 1, 0, 3, 2};
  if (br_read(br, 1)) return 0;  // all_default
  for (int t = 0; t < 17; t++) {
    const uint32_t mode = br_read(br, 3);
    DEC_BITS(br);
    if (mode == 0) continue;  // Library
    if (mode != 6 || kTableBig[t] < 0) return kUns;
    const uint32_t nbands = br_read(br, 4) + 1;
    if (nbands != 8) return br.err ? kInv : kUns;
    const int k = kTableBig[t];
    for (int i = 0; i < 24; i++) {
      const uint32_t bits = br_read(br, 16);
      if (((bits >> 10) & 31) == 31) return kInv;  // inf / NaN
      F->qm_bits[k][i] = (uint16_t)bits;
    }
    DEC_BITS(br);
    F->qm_mask |= 1u << k;
  }
  return 0;
}

using WallClock = std::chrono::steady_clock;
float ms_between(WallClock::time_point a, WallClock::time_point b) {
  return std::chrono::duration<float, std::milli>(b - a).count();
}

int parse(const uint8_t* data, size_t size, bool want_lf, DecFrame* F, uint32_t lf_threads = 8) {
  const auto t0 = WallClock::now();
  if (!data || size == 0 || size > ((size_t)1 << 40)) return kInv;
  F->words.assign(size / 8 + dec::kStreamPadWords, 0);
  std::memcpy(F->words.data(), data, size);
  BitReader br{F->words.data(), 0, (uint64_t)size * 8, 0, 0, 0};
  if (br_read(br, 16) != 0x0AFF) return kInv;
  static const U32Dist kSize[4] = {{9, 1}, {13, 1}, {18, 1}, {30, 1}};
  uint32_t xs, ys;
  if (br_read(br, 1)) {
    ys = (br_read(br, 5) + 1) * 8;
    if (br_read(br, 3)) return br.err ? kInv : kUns;  // ratio
    xs = (br_read(br, 5) + 1) * 8;
  } else {
    ys = read_u32(br, kSize);
    if (br_read(br, 3)) return br.err ? kInv : kUns;
    xs = read_u32(br, kSize);
  }
  DEC_BITS(br);
  if (xs > (1u << 18) || ys > (1u << 18)) return kUns;  // the encoder's limit
  if (!br_read(br, 1)) return br.err ? kInv : kUns;     // ImageMetadata all_default
  dec::br_align_byte(br);
  // FrameHeader
  if (br_read(br, 1)) return br.err ? kInv : kUns;  // all_default
  const uint32_t ftype = br_read(br, 2), enc = br_read(br, 1);
  const uint64_t flags = read_u64(br);
  DEC_BITS(br);
  if (ftype != 0 || enc != 0 || flags != 128) return kUns;
  static const U32Dist kUps[4] = {{-1, 1}, {-1, 2}, {-1, 4}, {-1, 8}};
  if (read_u32(br, kUps) != 1) return br.err ? kInv : kUns;
  F->x_qm = br_read(br, 3);
  F->b_qm = br_read(br, 3);
  static const U32Dist kPasses[4] = {{-1, 1}, {-1, 2}, {-1, 3}, {3, 4}};
  if (read_u32(br, kPasses) != 1) return br.err ? kInv : kUns;
  if (br_read(br, 1)) return br.err ? kInv : kUns;  // crop
  static const U32Dist kBlend[4] = {{-1, 0}, {-1, 1}, {-1, 2}, {2, 3}};
  if (read_u32(br, kBlend) != 0) return br.err ? kInv : kUns;
  if (!br_read(br, 1)) return br.err ? kInv : kUns;  // is_last
  static const U32Dist kName[4] = {{-1, 0}, {4, 0}, {5, 16}, {10, 48}};
  const uint32_t nlen = read_u32(br, kName);
  br_skip(br, 8 * nlen);
  uint32_t gab = 1, epf = 1;  // LoopFilter all_default
  if (!br_read(br, 1)) {
    gab = br_read(br, 1);
    if (gab && br_read(br, 1)) return br.err ? kInv : kUns;  // custom Gaborish weights
    epf = br_read(br, 2);
    if (epf)
      for (int i = 0; i < 3; i++)  // custom sharpness LUT / channel scales / sigmas
        if (br_read(br, 1)) return br.err ? kInv : kUns;
    if (read_u64(br)) return br.err ? kInv : kUns;  // loop filter extensions
  }
  if (read_u64(br)) return br.err ? kInv : kUns;  // frame extensions
  DEC_BITS(br);
  F->bxs = (xs + 7) / 8;
  F->bys = (ys + 7) / 8;
  F->tiles_x = (F->bxs + 7) / 8;
  F->tiles_y = (F->bys + 7) / 8;
  F->gxs = (xs + 255) / 256;
  F->gys = (ys + 255) / 256;
  F->lfxs = (xs + 2047) / 2048;
  F->lfys = (ys + 2047) / 2048;
  const uint32_t ng = F->gxs * F->gys, nlf = F->lfxs * F->lfys;
  jxg_stream_info& I = F->info;
  I.xsize = xs;
  I.ysize = ys;
  I.num_groups = ng;
  I.num_lf_groups = nlf;
  I.gaborish = gab;
  I.epf_iters = epf;
  // TOC
  if (br_read(br, 1)) return br.err ? kInv : kUns;  // permuted
  dec::br_align_byte(br);
  const size_t nent = ng == 1 ? 1 : 2 + (size_t)nlf + ng;
  if (br.pos + nent * 12 > br.end) return kInv;  // an entry takes 12 bits at least
  static const U32Dist kToc[4] = {{10, 0}, {14, 1024}, {22, 17408}, {30, 4211712}};
  std::vector<uint64_t> offs(nent + 1);
  std::vector<uint32_t> sizes(nent);
  for (size_t i = 0; i < nent; i++) sizes[i] = read_u32(br, kToc);
  DEC_BITS(br);
  dec::br_align_byte(br);
  offs[0] = br.pos >> 3;
  for (size_t i = 0; i < nent; i++) offs[i + 1] = offs[i] + sizes[i];
  if (br.pos > br.end || offs[nent] > size) return kInv;  // truncated
  auto section = [&](size_t i) {
    return BitReader{F->words.data(), offs[i] * 8, offs[i + 1] * 8, 0, 0, 0};
  };
  BitReader shared = section(0);
  const bool one = nent == 1;
  // LfGlobal
  BitReader lfg = section(0);
  BitReader& s0 = one ? shared : lfg;
  if (!br_read(s0, 1)) return s0.err ? kInv : kUns;  // custom LF dequant
  static const U32Dist kGs[4] = {{11, 1}, {11, 2049}, {12, 4097}, {16, 8193}};
  static const U32Dist kQdc[4] = {{-1, 16}, {5, 1}, {8, 1}, {16, 1}};
  I.global_scale = read_u32(s0, kGs);
  I.quant_dc = read_u32(s0, kQdc);
  if (!br_read(s0, 1)) return s0.err ? kInv : kUns;  // custom block context map
  if (!br_read(s0, 1)) return s0.err ? kInv : kUns;  // custom colour correlation
  if (br_read(s0, 1)) return s0.err ? kInv : kUns;   // global tree
  DEC_BITS(s0);
  const auto t1 = WallClock::now();
  // LF groups
  const size_t nb = (size_t)F->bxs * F->bys;
  if (want_lf || one) {
    F->acs.assign(nb, 0);
    F->qf.assign(nb, 0);
    F->dc.assign(nb * 3, 0);
    F->cmap.assign((size_t)F->tiles_x * F->tiles_y * 2, 0);
    if (one) {
      DEC_TRY(decode_lf_group(shared, F, 0, &F->big_used));
    } else {
      // one task per LF group on helper threads, as the encoder's host code
      const uint32_t nthreads = std::min(nlf, std::max(lf_threads, 1u));
      std::vector<int> status(nlf, 0);
      std::vector<uint32_t> used(nlf, 0);
      auto work = [&](uint32_t first) {
        for (uint32_t lg = first; lg < nlf; lg += nthreads) {
          BitReader s = section(1 + lg);
          try {
            status[lg] = decode_lf_group(s, F, lg, &used[lg]);
          } catch (const std::bad_alloc&) {
            status[lg] = JXG_ERR_OOM;
          } catch (...) {
            status[lg] = JXG_ERR_INTERNAL;
          }
        }
      };
      std::vector<std::future<void>> helpers;
      helpers.reserve(nthreads);
      for (uint32_t t = 1; t < nthreads; t++) {
        try {
          helpers.push_back(std::async(std::launch::async, work, t));
        } catch (const std::system_error&) {
          work(t);  // no thread to be had: this one's share runs here
        }
      }
      work(0);
      for (auto& h : helpers) h.get();
      for (uint32_t lg = 0; lg < nlf; lg++) {
        DEC_TRY(status[lg]);
        F->big_used |= used[lg];
      }
    }
    F->have_lf = true;
  }
  const auto t2 = WallClock::now();
  // HfGlobal
  BitReader hfg = section(one ? 0 : 1 + nlf);
  BitReader& s1 = one ? shared : hfg;
  DEC_TRY(read_dequant_matrices(s1, F));
  I.num_hf_presets = br_read(s1, ceil_log2(ng)) + 1;
  // more presets than pass groups could use is not something this encoder
  // writes; the bound also keeps num_hf_presets * 7425 contexts within 32 bits
  if (I.num_hf_presets > ng || (uint64_t)I.num_hf_presets * dec::kAcCtxPerPreset > (1ull << 31))
    return s1.err ? kInv : kUns;
  static const U32Dist kOrders[4] = {{-1, 0x5F}, {-1, 0x13}, {-1, 0}, {13, 0}};
  if (read_u32(s1, kOrders)) return s1.err ? kInv : kUns;  // custom coefficient orders
  DEC_BITS(s1);
  DEC_TRY(read_entropy(s1, I.num_hf_presets * dec::kAcCtxPerPreset, &F->hf));
  I.ans = F->hf.prefix ? 0 : 1;
  F->preset_bits = ceil_log2(I.num_hf_presets);
  F->sec.resize((size_t)ng * 2);
  for (uint32_t g = 0; g < ng; g++) {
    F->sec[2 * g] = one ? shared.pos : offs[2 + nlf + g] * 8;
    F->sec[2 * g + 1] = one ? shared.end : offs[2 + nlf + g + 1] * 8;
  }
  const auto t3 = WallClock::now();
  F->ms_lf = ms_between(t1, t2);
  F->ms_head = ms_between(t0, t1) + ms_between(t2, t3);
  return 0;
}

}  // namespace

int decode_parse(const uint8_t* data, size_t size, bool want_lf, DecFrame* F, uint32_t lf_threads) {
  try {
    return parse(data, size, want_lf, F, lf_threads);
  } catch (const std::bad_alloc&) {
    return JXG_ERR_OOM;
  } catch (...) {  // e.g. std::system_error when a helper thread cannot be started
    return JXG_ERR_INTERNAL;
  }
}

int decode_groups_host(const DecFrame& F, int16_t* ac) {
  if (!F.have_lf) return JXG_ERR_INTERNAL;
  const dec::SymReader S = F.hf.view();
  uint8_t nzs[3 * 1024];
  uint32_t pend[dec::kPendCoefs];
  for (uint32_t g = 0; g < F.info.num_groups; g++) {
    const uint32_t gx = g % F.gxs, gy = g / F.gxs;
    dec::GroupGeom geom{gx * 32, gy * 32, std::min(32u, F.bxs - gx * 32),
                        std::min(32u, F.bys - gy * 32), F.bxs};
    std::memset(nzs, 0, sizeof(nzs));
    BitReader br{F.words.data(), F.sec[2 * g], F.sec[2 * g + 1], 0, 0, 0};
    const int st = dec::decode_pass_group(br, S, F.info.num_hf_presets, F.preset_bits,
                                          F.acs.data(), geom, nzs, pend, ac, 0, 1);
    if (st) return st == dec::kUnsupported ? kUns : kInv;
  }
  return 0;
}

int decode_maps_host(const uint8_t* data, size_t size, uint8_t* acs, uint8_t* qf, int32_t* dc,
                     int32_t* ac, int8_t* cmap) {
  try {
    DecFrame F;
    DEC_TRY(parse(data, size, true, &F));
    const size_t nb = (size_t)F.bxs * F.bys;
    std::vector<int16_t> ac16(nb * 192, 0);
    DEC_TRY(decode_groups_host(F, ac16.data()));
    if (acs) std::memcpy(acs, F.acs.data(), nb);
    if (qf) std::memcpy(qf, F.qf.data(), nb);
    if (dc) std::memcpy(dc, F.dc.data(), nb * 3 * sizeof(int32_t));
    if (cmap) std::memcpy(cmap, F.cmap.data(), F.cmap.size());
    if (ac)
      for (size_t i = 0; i < nb * 192; i++) ac[i] = ac16[i];
    return 0;
  } catch (const std::bad_alloc&) {
    return JXG_ERR_OOM;
  } catch (...) {
    return JXG_ERR_INTERNAL;
  }
}

}  // namespace jxg

extern "C" jxg_status jxg_decode_info(const uint8_t* data, size_t size, jxg_stream_info* info) {
  if (!data || !info || size == 0) return JXG_ERR_INVALID_ARG;
  try {
    jxg::DecFrame F;
    const int st = jxg::decode_parse(data, size, false, &F);
    if (st) return (jxg_status)st;
    *info = F.info;
    return JXG_OK;
  } catch (...) {
    return JXG_ERR_OOM;
  }
}
