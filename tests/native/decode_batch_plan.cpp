// decode_batch_plan -- prints what the batch decoder's host-only planner
// computes, for tests/test_decode_batch_plan.py (built by g++ from
// csrc/jxg_decode_plan.cpp alone, under ASan + UBSan where the compiler has
// them):
//   decode_batch_plan FRAMES BUDGET
// FRAMES: a text file, one frame per line:
//   bxs bys ntiles stream_words table_bytes nhist tab_bytes ngroups bits...
// with `ngroups` section lengths in bits (the sections are laid end to end from
// bit 64; a frame of no groups passes a null section table).  Prints
//   frame I footprint lds staged  acs qf dc ac cmap stream sec tab   (slice bytes)
//   chunk K first end bytes nstatus lds_staged lds_unstaged
//   at F acs qf dc ac cmap stream sec tab end status_base             (per frame of the chunk)
//   staged F:G ...   /   unstaged F:G ...
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <fstream>
#include <string>

#include "../../jpeg-xl-lossy-image-compression-thesis_amd/csrc/jxg_decode_plan.h"

using namespace jxg;

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: decode_batch_plan FRAMES BUDGET\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  const size_t budget = (size_t)std::strtoull(argv[2], nullptr, 10);
  std::vector<DecPlanFrame> frames;
  std::vector<std::vector<uint64_t>> secs;
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ls(line);
    DecPlanFrame f;
    uint64_t words = 0, table = 0;
    if (!(ls >> f.bxs >> f.bys >> f.ntiles >> words >> table >> f.nhist >> f.tab_bytes >> f.ngroups)) {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
    f.stream_words = (size_t)words;
    f.table_bytes = (size_t)table;
    std::vector<uint64_t> sec;
    uint64_t at = 64;
    for (uint32_t g = 0; g < f.ngroups; g++) {
      uint64_t bits = 0;
      if (!(ls >> bits)) {
        std::fprintf(stderr, "bad line: %s\n", line.c_str());
        return 2;
      }
      sec.push_back(at);
      sec.push_back(at + bits);
      at += bits;
    }
    secs.push_back(std::move(sec));
    frames.push_back(f);
  }
  for (size_t i = 0; i < frames.size(); i++) frames[i].sec = secs[i].empty() ? nullptr : secs[i].data();
  for (size_t i = 0; i < frames.size(); i++) {
    bool staged = false;
    const uint32_t lds = decode_lds_bytes(frames[i].nhist, frames[i].tab_bytes, &staged);
    const DecSliceBytes b = decode_slice_bytes(frames[i]);
    std::printf("frame %zu %zu %u %d %zu %zu %zu %zu %zu %zu %zu %zu\n", i,
                decode_footprint(frames[i]), lds, staged ? 1 : 0, b.acs, b.qf, b.dc, b.ac, b.cmap,
                b.stream, b.sec, b.tab);
  }
  const std::vector<DecChunk> chunks = plan_decode_batch(frames, budget);
  for (size_t k = 0; k < chunks.size(); k++) {
    const DecChunk& c = chunks[k];
    std::printf("chunk %zu %u %u %zu %u %u %u\n", k, c.first, c.end, c.bytes, c.nstatus,
                c.lds_staged, c.lds_unstaged);
    if (c.at.size() != c.end - c.first || c.status_base.size() != c.at.size()) {
      std::fprintf(stderr, "chunk %zu: %zu slices for %u frames\n", k, c.at.size(), c.end - c.first);
      return 1;
    }
    for (size_t i = 0; i < c.at.size(); i++) {
      const DecSlices& s = c.at[i];
      std::printf("at %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u\n", (size_t)c.first + i, s.acs, s.qf,
                  s.dc, s.ac, s.cmap, s.stream, s.sec, s.tab, s.end, c.status_base[i]);
    }
    std::printf("staged");
    for (const DecWork& w : c.staged) std::printf(" %u:%u", w.frame, w.group);
    std::printf("\nunstaged");
    for (const DecWork& w : c.unstaged) std::printf(" %u:%u", w.frame, w.group);
    std::printf("\n");
  }
  return 0;
}
