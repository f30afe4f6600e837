// jxg_decode_core.h -- the decode core shared by the host path
// (jxg_decode.cpp, plain C++) and the pass-group kernel (jxg_decode.hip): bit
// reader, hybrid-uint reader, prefix / alias-table symbol readers, the AC
// context tables and the pass-group token walk.  Plain inline functions; the
// header includes nothing from HIP (JXG_HD is empty for a host compiler), so
// the one implementation is what the CPU tests, the corrupted-input program
// (tests/native/decode_mutate.cpp) and the GPU run.  Grammar: the subset of
// [ext] ISO/IEC 18181-1 that oracle/jxl_decode.py decode() accepts.
//
// Memory safety: a BitReader never loads outside [0, end) rounded up to the
// stream's zero padding (two 64-bit words past the last byte); a read past
// `end` yields zeros and sets err.  Every table index derived from the stream
// is bounded by construction of the tables (build_* in jxg_decode.cpp) or
// checked before use.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "jxg_acmodel.h"  // JXG_HD; the AC context model

// The includer of the kernel defines JXG_WAVE_SYNC (a workgroup barrier of the
// one-wave workgroup) before including this header: it orders the lanes' LDS
// writes of the non-zero map against the next reads.  Nothing on the host.
#ifndef JXG_WAVE_SYNC
#define JXG_WAVE_SYNC() ((void)0)
#endif

// The kernel also defines JXG_UNIFORM32(x): the value of x in the first active
// lane (readfirstlane).  The walk's state is the same in every lane, but what
// a lane loads from LDS or memory arrives in vector registers; naming the
// loaded values uniform moves them -- and the state computed from them -- to
// scalar registers.  The identity on the host.
#ifndef JXG_UNIFORM32
#define JXG_UNIFORM32(x) (x)
#endif

namespace jxg {
namespace dec {

JXG_HD inline uint32_t uni(uint32_t v) { return (uint32_t)JXG_UNIFORM32(v); }
JXG_HD inline uint64_t uni64(uint64_t v) {
  return (uint64_t)uni((uint32_t)(v >> 32)) << 32 | uni((uint32_t)v);
}

constexpr int kOk = 0, kInvalid = 1, kUnsupported = 2;
constexpr uint32_t kAcCtxPerPreset = 15 * (37 + 458);  // 7425
constexpr uint32_t kAnsFinalState = 0x130000;
constexpr uint32_t kStreamPadWords = 3;  // 64-bit words past the last byte's word

struct BitReader {
  const uint64_t* w;  // the codestream as little-endian 64-bit words, zero padded
  uint64_t pos, end;  // bits
  uint32_t err;
  // window: the low nbuf bits of buf are the stream's bits from pos on (bits at
  // or past `end` zero), refilled from memory when fewer than 32 are left -- a
  // peek or read takes at most 32 bits, so most of them touch no memory
  uint32_t nbuf;
  uint64_t buf;
};

// the next bits, at least 32 of them valid (bits at or past `end` are zero)
JXG_HD inline uint64_t br_peek(BitReader& r) {
  if (r.nbuf >= 32) return r.buf;
  uint64_t v = 0;
  if (r.pos < r.end) {
    const uint64_t i = r.pos >> 6;
    const uint32_t s = (uint32_t)(r.pos & 63);
    v = uni64(r.w[i]) >> s;
    if (s) v |= uni64(r.w[i + 1]) << (64 - s);
    const uint64_t avail = r.end - r.pos;
    if (avail < 64) v &= (1ull << avail) - 1;
  }
  r.buf = v;
  r.nbuf = 64;
  return v;
}
JXG_HD inline void br_skip(BitReader& r, uint32_t n) {
  r.pos += n;
  if (n < r.nbuf) {
    r.buf >>= n;
    r.nbuf -= n;
  } else {
    r.buf = 0;
    r.nbuf = 0;
  }
  if (r.pos > r.end) {
    r.pos = r.end;
    r.nbuf = 0;
    r.err = 1;
  }
}
JXG_HD inline void br_align_byte(BitReader& r) {
  r.pos = (r.pos + 7) & ~(uint64_t)7;
  r.nbuf = 0;
}
JXG_HD inline uint32_t br_read(BitReader& r, uint32_t n) {  // n <= 32
  if (n == 0) return 0;
  const uint64_t v = br_peek(r) & ((1ull << n) - 1);
  br_skip(r, n);
  return r.err ? 0u : (uint32_t)v;
}

JXG_HD inline int32_t unpack_signed(uint32_t u) { return (int32_t)(u >> 1) ^ -(int32_t)(u & 1); }

// one clustered histogram of an entropy stream: its hybrid-uint config and
// where its decode table starts.  Prefix codes: `off` indexes the u16 table
// pool, 1 << maxlen entries of (length << 8 | symbol); maxlen 0: the code has
// the single symbol `single` and reads no bits.  ANS: `off` indexes the alias
// entries, 1 << log_alpha per histogram.
struct HistDesc {
  uint32_t off;
  uint16_t single;
  uint8_t maxlen, split_exp, msb, lsb;
  uint8_t pad[2];
};
struct AnsEntry {
  uint16_t cutoff, right;  // positions below cutoff: the entry's own symbol
  uint16_t freq0, freq1;   // frequency of the own / the right symbol
  int32_t offset;          // of the right symbol's slice
};
struct SymReader {
  const uint8_t* ctxmap;  // [nctx - ctx_bias] -> histogram, of contexts ctx_bias and up
  const HistDesc* hist;
  const uint16_t* ptab;
  const AnsEntry* atab;
  uint32_t nctx, prefix, log_alpha;
  uint32_t ctx_bias;  // 0, or the first context of the one HF preset the kernel staged
};

// The readers and the walk are templates over the table struct (SymReader's
// members) and the scratch pointers, so that the kernel can instantiate them
// with LDS-qualified pointers: a read through a generic pointer is a flat load,
// which waits on both memory counters; through an LDS pointer it is a ds_read.
template <class SR>
JXG_HD inline uint32_t read_symbol(BitReader& br, const SR& S, const HistDesc& h,
                                   uint32_t& state) {
  if (S.prefix) {
    if (h.maxlen == 0) return h.single;
    const uint32_t idx = (uint32_t)br_peek(br) & ((1u << h.maxlen) - 1);
    const uint32_t e = uni(S.ptab[h.off + idx]);
    br_skip(br, e >> 8);
    return e & 0xFF;
  }
  const uint32_t shift = 12 - S.log_alpha;
  const uint32_t res = state & 0xFFF;
  const uint32_t i = res >> shift, pos = res & ((1u << shift) - 1);
  const auto& e = S.atab[h.off + i];
  uint32_t sym, f;
  int32_t off;
  if (pos >= uni(e.cutoff)) {
    sym = uni(e.right);
    off = (int32_t)uni((uint32_t)e.offset) + (int32_t)pos;
    f = uni(e.freq1);
  } else {
    sym = i;
    off = (int32_t)pos;
    f = uni(e.freq0);
  }
  state = f * (state >> 12) + (uint32_t)off;
  if (state < (1u << 16)) state = (state << 16) | br_read(br, 16);
  return sym;
}

// token -> value; a value that needs more than 32 bits is malformed
JXG_HD inline uint32_t read_hybrid(BitReader& br, const HistDesc& h, uint32_t token) {
  const uint32_t split = 1u << h.split_exp;
  if (token < split) return token;
  const uint32_t ml = (uint32_t)h.msb + h.lsb;
  const uint32_t nbits = h.split_exp - ml + ((token - split) >> ml);
  if (nbits + h.msb + 1 + h.lsb > 32) {
    br.err = 1;
    return 0;
  }
  const uint32_t low = token & ((1u << h.lsb) - 1);
  token >>= h.lsb;
  const uint32_t bits = br_read(br, nbits);
  const uint32_t hi = (token & ((1u << h.msb) - 1)) | (1u << h.msb);
  return (((hi << nbits) | bits) << h.lsb) | low;
}

template <class SR>
JXG_HD inline uint32_t read_ctx(BitReader& br, const SR& S, uint32_t ctx, uint32_t& state) {
  const auto& d = S.hist[uni(S.ctxmap[ctx - S.ctx_bias])];
  HistDesc h;
  h.off = uni(d.off);
  h.single = (uint16_t)uni(d.single);
  h.maxlen = (uint8_t)uni(d.maxlen);
  h.split_exp = (uint8_t)uni(d.split_exp);
  h.msb = (uint8_t)uni(d.msb);
  h.lsb = (uint8_t)uni(d.lsb);
  const uint32_t tok = read_symbol(br, S, h, state);
  return read_hybrid(br, h, tok);
}

// the format's AC context model (jxg_acmodel.h), the expression forms the
// walk's token chain was tuned with
using jxg::block_ctx;
using jxg::freq_ctx;
using jxg::nnz_ctx;
using jxg::strategy_order;
using jxg::strategy_shape;

struct GroupGeom {
  uint32_t bx0, by0, gw, gh, bxs;  // first block, blocks across / down, frame blocks per row
};

// One pass group: preset index, then per varblock and channel (Y, X, B) the
// non-zero count with its predicted context and the coefficients in natural
// order from position covered_blocks on.  Every value the walk depends on is
// the same in all callers' lanes (reader position, ANS state, left, k, the
// previous-token flag); `lane` of `nlanes` only splits the fill of the
// non-zero map and the write-out of the collected coefficients.
//   acs: the frame's strategy map ([bys][bxs], bit 7 on covered blocks)
//   nzs: [3][32 * 32] scratch (LDS in the kernel), contents irrelevant on entry
//   ac:  the frame's coefficients [block][3][64] int16 natural-order slices,
//        the group's blocks zeroed by the caller; only non-zeros are stored
//   pend: [kPendCoefs] scratch (LDS in the kernel).  Non-zero coefficients are
//        collected there as (position << 16 | value) and written out by all
//        lanes together when it is full or a channel ends: a store per token
//        from the chain itself would put the store's completion into every
//        token's step (the next table load waits for outstanding memory
//        operations), and the lanes' stores go out in parallel.
constexpr uint32_t kPendCoefs = 512;

template <class PendP>
JXG_HD inline void flush_coefs(PendP pend, uint32_t n, int16_t* ac, const GroupGeom& g,
                               uint32_t by, uint32_t bx, uint32_t cx, uint32_t c, uint32_t lane,
                               uint32_t nlanes) {
  JXG_WAVE_SYNC();  // the entries are written
  for (uint32_t i = lane; i < n; i += nlanes) {
    const uint32_t e = pend[i], k = e >> 16, sl = k >> 6;
    const size_t blk = (size_t)(g.by0 + by + sl / cx) * g.bxs + g.bx0 + bx + sl % cx;
    ac[blk * 192 + c * 64 + (k & 63)] = (int16_t)(e & 0xFFFF);
  }
  JXG_WAVE_SYNC();  // and read, before the next ones overwrite them
}

template <class SR, class NzP, class PendP>
JXG_HD inline int decode_pass_group(BitReader& br, const SR& S, uint32_t npresets,
                                    uint32_t preset_bits, const uint8_t* acs, const GroupGeom g,
                                    NzP nzs, PendP pend, int16_t* ac, uint32_t lane,
                                    uint32_t nlanes) {
  const uint32_t preset = br_read(br, preset_bits);
  if (br.err || preset >= npresets) return kInvalid;
  if (((uint64_t)preset + 1) * kAcCtxPerPreset > S.nctx) return kInvalid;  // (no 32-bit wrap)
  const uint32_t off = preset * kAcCtxPerPreset;
  uint32_t state = S.prefix ? 0u : br_read(br, 32);
  for (uint32_t by = 0; by < g.gh; by++) {
    for (uint32_t bx = 0; bx < g.gw; bx++) {
      const uint32_t t = uni(acs[(size_t)(g.by0 + by) * g.bxs + g.bx0 + bx]);
      if (t & 0x80) continue;
      const uint32_t shape = strategy_shape(t);
      const uint32_t cy = shape & 0xFF, cx = shape >> 8;
      if (!shape || bx + cx > g.gw || by + cy > g.gh) return kInvalid;
      const uint32_t cb = cy * cx;
      uint32_t lcb = 0;
      while ((1u << lcb) < cb) lcb++;
      const uint32_t size = 64 * cb;
      const uint32_t ordi = strategy_order(t);
      for (uint32_t ci = 0; ci < 3; ci++) {
        const uint32_t c = ci == 0 ? 1u : (ci == 1 ? 0u : 2u);
        NzP nz_c = nzs + c * 1024;
        uint32_t pred;
        if (bx == 0)
          pred = by == 0 ? 32u : uni(nz_c[(by - 1) * 32 + bx]);
        else if (by == 0)
          pred = uni(nz_c[by * 32 + bx - 1]);
        else
          pred = (uni(nz_c[(by - 1) * 32 + bx]) + uni(nz_c[by * 32 + bx - 1]) + 1) >> 1;
        const uint32_t bctx = block_ctx((c < 2 ? c ^ 1 : 2) * 13 + ordi);
        // nz_bucket(pred) in the walk's unsigned form (calling it moves 4
        // instructions of the kernels; tests/test_ac_model.py pins the two equal)
        const uint32_t pp = pred < 64 ? pred : 64;
        const uint32_t bucket = pp < 8 ? pp : 4 + pp / 2;
        const uint32_t nz = read_ctx(br, S, off + bucket * 15 + bctx, state);
        if (br.err || nz > size - cb) return kInvalid;
        const uint8_t fill = (uint8_t)((nz + cb - 1) >> lcb);
        for (uint32_t i = lane; i < cb; i += nlanes) nz_c[(by + i / cx) * 32 + bx + i % cx] = fill;
        JXG_WAVE_SYNC();
        const uint32_t zoff = off + 15 * 37 + 458 * bctx;
        uint32_t prev = nz > size / 16 ? 0u : 1u;
        uint32_t k = cb, left = nz, npend = 0;
        while (k < size && left > 0) {
          // more non-zeros left than positions: malformed.  Checked before the
          // context is formed: with left <= size - k the two buckets sum to at
          // most 64 and the zero-density context stays below 458; without it a
          // run of zeros would walk the context past the preset's slice
          if (left > size - k) return kInvalid;
          const uint32_t ctx =
              zoff + (nnz_ctx((left + cb - 1) >> lcb) + freq_ctx(k >> lcb)) * 2 + prev;
          const uint32_t u = read_ctx(br, S, ctx, state);
          if (br.err) return kInvalid;
          if (u) {
            const int32_t v = unpack_signed(u);
            if (v < -32768 || v > 32767) return kInvalid;  // the coefficient planes are int16
            pend[npend++] = k << 16 | ((uint32_t)v & 0xFFFF);  // k < 65536; every lane, same value
            if (npend == kPendCoefs) {
              flush_coefs(pend, npend, ac, g, by, bx, cx, c, lane, nlanes);
              npend = 0;
            }
            prev = 1;
            left--;
          } else {
            prev = 0;
          }
          k++;
        }
        if (left) return kInvalid;  // nzeros not exhausted
        if (npend) flush_coefs(pend, npend, ac, g, by, bx, cx, c, lane, nlanes);
      }
    }
  }
  if (br.err) return kInvalid;
  if (!S.prefix && state != kAnsFinalState) return kInvalid;
  return kOk;
}

}  // namespace dec
}  // namespace jxg
