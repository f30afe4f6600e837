// jxg_decode.h -- host side of the decoder (jxg_decode.cpp; plain C++, no
// HIP): headers, TOC, LfGlobal, the LF groups' modular streams, HfGlobal and
// the entropy decode tables, and a host loop over the pass groups through the
// walk of jxg_decode_core.h.  jxg_decode_dev.cpp uploads what this produces and runs
// the pass groups on the GPU (jxg_decode.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "../../include/jxg.h"
#include "jxg_decode_core.h"

namespace jxg {

// an entropy stream's decode tables (DecodeHistograms of the format)
struct DecEntropy {
  std::vector<uint8_t> ctxmap;
  std::vector<dec::HistDesc> hist;
  std::vector<uint16_t> ptab;
  std::vector<dec::AnsEntry> atab;
  uint32_t prefix = 0, log_alpha = 0;
  dec::SymReader view() const {
    return dec::SymReader{ctxmap.data(), hist.data(), ptab.data(), atab.data(),
                          (uint32_t)ctxmap.size(), prefix, log_alpha, 0u};
  }
};

// the decode tables as the pass-group kernels take them, one upload: [hist |
// atab or ptab | ctxmap], 8-byte aligned parts; tab_bytes: the symbol tables'
// (DecodeArgs.tab_bytes)
struct DecTableBlob {
  std::vector<uint8_t> bytes;
  size_t o_atab = 0, o_ptab = 0, o_map = 0;
  uint32_t tab_bytes = 0;
};
inline DecTableBlob decode_table_blob(const DecEntropy& E) {
  DecTableBlob B;
  const size_t b_hist = E.hist.size() * sizeof(dec::HistDesc);
  const size_t b_atab = E.atab.size() * sizeof(dec::AnsEntry);
  const size_t b_ptab = E.ptab.size() * sizeof(uint16_t);
  B.o_atab = (b_hist + 7) & ~(size_t)7;
  B.o_ptab = (B.o_atab + b_atab + 7) & ~(size_t)7;
  B.o_map = (B.o_ptab + b_ptab + 7) & ~(size_t)7;
  B.bytes.assign(B.o_map + E.ctxmap.size(), 0);
  std::memcpy(B.bytes.data(), E.hist.data(), b_hist);
  if (b_atab) std::memcpy(B.bytes.data() + B.o_atab, E.atab.data(), b_atab);
  if (b_ptab) std::memcpy(B.bytes.data() + B.o_ptab, E.ptab.data(), b_ptab);
  std::memcpy(B.bytes.data() + B.o_map, E.ctxmap.data(), E.ctxmap.size());
  B.tab_bytes = (uint32_t)(E.prefix ? b_ptab : b_atab);
  return B;
}

struct DecFrame {
  jxg_stream_info info{};
  uint32_t x_qm = 2, b_qm = 2;
  uint32_t bxs = 0, bys = 0, gxs = 0, gys = 0, lfxs = 0, lfys = 0, tiles_x = 0, tiles_y = 0;
  std::vector<uint64_t> words;  // the codestream, zero padded (dec::kStreamPadWords)
  std::vector<uint64_t> sec;    // [num_groups][2] first / end bit of every pass group
  // the LF groups' maps in the device layouts of the encoder (jxg_kernels.h
  // ReconArgs): acs raw strategy with bit 7 on covered blocks, qf raw - 1,
  // dc [3][blocks] (X, Y, B), cmap [2][tiles]
  bool have_lf = false;
  std::vector<uint8_t> acs, qf;
  std::vector<int32_t> dc;
  std::vector<int8_t> cmap;
  DecEntropy hf;  // the AC stream: num_hf_presets * 7425 contexts
  uint32_t preset_bits = 0;
  // DequantMatrices: tables 13..16 of the format's order (DCT128X128,
  // DCT128X64, DCT256X256, DCT256X128) written in DCT mode, as the encoder's
  // kinds 0 128X64, 1 128X128, 2 256X128, 3 256X256: mask and the binary16
  // words [channel][band]; big_used: the kinds some varblock uses
  uint32_t qm_mask = 0, big_used = 0;
  uint16_t qm_bits[4][24] = {};
  float ms_head = 0, ms_lf = 0;  // host wall time: parse + tables, LF groups
};

// want_lf false: the LF groups are skipped where the layout allows it (frames
// of several sections) -- enough for jxg_decode_info.  JXG_OK or a negative
// jxg_status.  lf_threads: the most threads the frame's LF groups may take (this
// one included); the batch decoder, which parses several frames at a time,
// shares the 8 between them.
int decode_parse(const uint8_t* data, size_t size, bool want_lf, DecFrame* F,
                 uint32_t lf_threads = 8);
// the pass groups on the host; ac: [blocks][3][64] int16, zeroed by the caller
int decode_groups_host(const DecFrame& F, int16_t* ac);
// jxg_decode_maps with ctx == NULL
int decode_maps_host(const uint8_t* data, size_t size, uint8_t* acs, uint8_t* qf, int32_t* dc,
                     int32_t* ac, int8_t* cmap);

}  // namespace jxg
