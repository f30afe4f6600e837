// jxg_payload.h -- a rank's payload head (group sharding, include/jxg.h
// jxg_shard_payload): parsing and validation of every rank's heads into the
// frame's section table, the HfGlobal of per-rank HF presets.  Host only;
// the heads are built by jxg_shard_host.cpp shard_finish.
// payload: "JXGS" | version | rank (| loop-filter code << 16) | world | xsize | ysize | nsections |
//          nsections x (TOC index, bytes) [| version 2: the rank's HF preset]
//          | section bytes back to back
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/jxg.h"
#include "jxg_layout.h"

namespace jxg {

constexpr uint32_t kPayloadMagic = 0x5347584Au;  // "JXGS"

// for each TOC index of the frame: (payload, byte offset inside it, size)
struct SectionRef {
  uint32_t payload;
  uint64_t off;
  uint32_t size;
};

// words of a payload head from its first words (avail of them; 0: malformed
// or more words needed to tell -- version 2 needs 7 + 2 nsections + 1)
size_t head_words(const uint32_t* hw, size_t avail);
// every rank's head (psizes: whole payload bytes) -> frame size, loop-filter
// code, section table; with version-2 heads also the generated HfGlobal
// (`hf`; its SectionRef names payload n = "generated"; hf_bytes false: its
// size only, `hf` left empty)
jxg_status parse_payload_heads(const std::vector<std::vector<uint32_t>>& heads,
                               const std::vector<size_t>& psizes, uint32_t* w, uint32_t* h,
                               std::vector<SectionRef>& secs, std::vector<uint8_t>& hf,
                               uint32_t* lf, bool hf_bytes = true);
// The head at the start of a payload of `size` bytes, wherever it lives:
// fetch(nwords, dst) copies the payload's first nwords words (host memory:
// read_head; device memory: jxg_shard_host.cpp) and returns a status.
template <class Fetch>
jxg_status read_head_from(size_t size, Fetch fetch, std::vector<uint32_t>& hw) {
  if (size < 28) return JXG_ERR_INVALID_ARG;
  hw.resize(7);
  jxg_status st = fetch((size_t)7, hw.data());
  if (st) return st;
  const size_t base = 7 + 2 * (size_t)hw[6];
  if (hw[1] == 2) {  // version 2: read up to the preset block's length
    if (size < (base + 1) * 4) return JXG_ERR_INVALID_ARG;
    hw.resize(base + 1);
    if ((st = fetch(base + 1, hw.data()))) return st;
  }
  const size_t words = head_words(hw.data(), hw.size());
  if (!words || size < words * 4) return JXG_ERR_INVALID_ARG;
  hw.resize(words);
  return fetch(words, hw.data());
}
// the head at the start of a payload in host memory (empty: malformed)
std::vector<uint32_t> read_head(const uint8_t* p, size_t size);

// every rank's head -> the frame: its section table, the generated HfGlobal
// (parse_payload_heads) and the codestream's headers, TOC and section offsets
#pragma GCC visibility push(hidden)
struct ShardFrame {
  std::vector<SectionRef> secs;
  std::vector<uint8_t> hf;
  StreamLayout lay;
};
jxg_status frame_of_heads(const std::vector<std::vector<uint32_t>>& heads,
                          const std::vector<size_t>& psizes, bool hf_bytes, ShardFrame* F);
#pragma GCC visibility pop

}  // namespace jxg
