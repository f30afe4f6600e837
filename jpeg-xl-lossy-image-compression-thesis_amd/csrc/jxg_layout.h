// jxg_layout.h -- the codestream's layout, written once: headers + TOC and
// the byte offset of every section (stream_layout), and the bit-exact piece
// list the concat kernel assembles a codestream or a rank's sections from
// (PieceList).  Host only: plain bit counts, offsets and BitWriters in, no
// HIP include.  Every assembler goes through here (jxg_encode.cpp
// stage_concat / stage_concat_split, jxg_shard_host.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "jxg_bitstream.h"

#pragma GCC visibility push(hidden)
namespace jxg {

// headers + TOC of a frame whose sections have `sizes` bytes (TOC order; a
// single-group frame has one section holding everything), the sections byte
// aligned and back to back after them
struct StreamLayout {
  BitWriter head;             // SizeHeader .. TOC, byte aligned
  std::vector<uint64_t> off;  // byte offset of every section
  uint64_t total = 0;         // bytes of the codestream
};
StreamLayout stream_layout(uint32_t w, uint32_t h, uint32_t lf, const std::vector<uint32_t>& sizes);

// what the concat kernel reads (== ConcatPiece, jxg_kernels.h)
struct PlacedPiece {
  uint64_t src_bit, dst_bit, nbits;
  uint32_t arena, pad;
};
enum PieceArena : uint32_t { kArenaAc = 0, kArenaChunk = 1, kArenaLf = 2 };

// The sections of one Job as plain data: LfGlobal / HfGlobal / LF-group
// preludes (host bit writers), LF streams and pass groups (bit ranges of the
// device arenas).  lf_mine null: every LF group.
struct JobSections {
  uint32_t nlf = 0;
  bool first_rank = true;  // writes LfGlobal, and HfGlobal unless presets
  bool presets = false;    // per-rank HF presets: every pass group starts with its preset index
  uint32_t rank = 0, world = 1;
  const uint8_t* lf_mine = nullptr;  // [nlf]
  const uint32_t* groups = nullptr;  // the plan's pass groups
  uint32_t ngroups = 0;
  const BitWriter *lfglobal = nullptr, *hfglobal = nullptr;
  const BitWriter *preA = nullptr, *preB = nullptr;  // [nlf]
  const uint64_t* sbase = nullptr;                   // [2 nlf] LF streams: arena bit offset
  const uint32_t* sbits = nullptr;                   //   and exact bits
  const uint64_t* gbase = nullptr;                   // [frame's groups] AC arena bit offset
  const uint32_t* gbits = nullptr;                   //   and exact bits
};

class PieceList {
 public:
  struct Piece {
    uint32_t arena;
    uint64_t src, nbits;
  };
  // host bits into the chunk arena (uploaded with the pieces)
  Piece add_chunk(const BitWriter& bw);
  Piece add_chunk(const uint8_t* bytes, size_t n);
  void section(uint32_t toc_id, std::vector<Piece> pieces);
  // LfGlobal, the owned LF groups (preA | LF stream A | preB | LF stream B), HfGlobal
  void add_prefix(const JobSections& j);
  // the plan's pass groups (with the per-rank preset selector)
  void add_groups(const JobSections& j);
  // bytes of every section; single: one section of all the bits
  std::vector<uint32_t> sizes(bool single) const;
  const std::vector<uint32_t>& ids() const { return ids_; }
  // `head` (if any), then every section from bit 0, byte aligned unless
  // single; appends the chunk arena's read-ahead guard word.  Returns bytes.
  size_t place(const BitWriter* head, bool single);
  const std::vector<PlacedPiece>& pieces() const { return placed_; }
  const std::vector<uint32_t>& chunk_words() const { return chunk_words_; }

 private:
  std::vector<std::vector<Piece>> sections_;
  std::vector<uint32_t> ids_, chunk_words_;
  std::vector<PlacedPiece> placed_;
};

// One section of an arena that exists twice, in device memory and in its
// pinned host mirror, at the same byte offset of both: d / h point at the two
// copies of n elements.  A section read on one side only leaves the other
// pointer unused.
template <class T>
struct Mirror {
  T* d = nullptr;
  T* h = nullptr;
  size_t n = 0;
};
// The layout of such an arena, declared once per frame: sections in order,
// each on a 256-byte boundary; commit() points every section's mirror into
// the two allocations, so the two sides cannot disagree.
class ArenaLayout {
 public:
  static constexpr size_t kAlign = 256;
  template <class T>
  void add(Mirror<T>& m, size_t count) {
    m.n = count;
    slots_.push_back({&m, off_, [](void* mp, uint8_t* dev, uint8_t* host) {
                        Mirror<T>* mm = static_cast<Mirror<T>*>(mp);
                        mm->d = reinterpret_cast<T*>(dev);
                        mm->h = reinterpret_cast<T*>(host);
                      }});
    off_ = (off_ + count * sizeof(T) + kAlign - 1) & ~(kAlign - 1);
  }
  size_t mark() const { return off_; }   // byte offset of the next section
  size_t bytes() const { return off_; }  // of the whole arena
  void commit(void* dev_base, void* host_base) const {
    for (const Slot& s : slots_)
      s.set(s.mirror, static_cast<uint8_t*>(dev_base) + s.off, static_cast<uint8_t*>(host_base) + s.off);
  }

 private:
  struct Slot {
    void* mirror;
    size_t off;
    void (*set)(void*, uint8_t*, uint8_t*);
  };
  std::vector<Slot> slots_;
  size_t off_ = 0;
};

}  // namespace jxg
#pragma GCC visibility pop
