// jxg_layout.cpp -- codestream layout and concat piece lists (jxg_layout.h)
#include "jxg_layout.h"

#include <algorithm>

namespace jxg {

StreamLayout stream_layout(uint32_t w, uint32_t h, uint32_t lf, const std::vector<uint32_t>& sizes) {
  StreamLayout L;
  write_headers(L.head, w, h, lf);
  write_toc(L.head, sizes);
  L.head.pad_to_byte();
  L.off.resize(sizes.size());
  uint64_t pos = L.head.bits() / 8;
  for (size_t i = 0; i < sizes.size(); i++) {
    L.off[i] = pos;
    pos += sizes[i];
  }
  L.total = pos;
  return L;
}

PieceList::Piece PieceList::add_chunk(const BitWriter& bw) {
  Piece p{kArenaChunk, (uint64_t)chunk_words_.size() * 32, bw.bits()};
  auto wv = bw.words32();
  chunk_words_.insert(chunk_words_.end(), wv.begin(), wv.end());
  return p;
}

PieceList::Piece PieceList::add_chunk(const uint8_t* bytes, size_t n) {
  Piece p{kArenaChunk, (uint64_t)chunk_words_.size() * 32, (uint64_t)n * 8};
  for (size_t i = 0; i < n; i += 4) {
    uint32_t wv = 0;
    for (size_t b = 0; b < 4 && i + b < n; b++) wv |= (uint32_t)bytes[i + b] << (8 * b);
    chunk_words_.push_back(wv);
  }
  return p;
}

void PieceList::section(uint32_t toc_id, std::vector<Piece> pieces) {
  sections_.push_back(std::move(pieces));
  ids_.push_back(toc_id);
}

void PieceList::add_prefix(const JobSections& j) {
  if (j.first_rank) section(0, {add_chunk(*j.lfglobal)});
  for (uint32_t lg = 0; lg < j.nlf; lg++) {
    if (j.lf_mine && !j.lf_mine[lg]) continue;
    section(1 + lg, {add_chunk(j.preA[lg]), Piece{kArenaLf, j.sbase[lg * 2], j.sbits[lg * 2]},
                     add_chunk(j.preB[lg]),
                     Piece{kArenaLf, j.sbase[lg * 2 + 1], j.sbits[lg * 2 + 1]}});
  }
  if (j.first_rank && !j.presets) section(1 + j.nlf, {add_chunk(*j.hfglobal)});
}

void PieceList::add_groups(const JobSections& j) {
  BitWriter sel;
  if (j.presets) sel.put(ceil_log2(j.world), j.rank);
  for (uint32_t i = 0; i < j.ngroups; i++) {
    const uint32_t g = j.groups[i];
    const Piece ac{kArenaAc, j.gbase[g], j.gbits[g]};
    if (j.presets)
      section(2 + j.nlf + g, {add_chunk(sel), ac});
    else
      section(2 + j.nlf + g, {ac});
  }
}

std::vector<uint32_t> PieceList::sizes(bool single) const {
  std::vector<uint32_t> sz;
  uint64_t total = 0;
  for (auto& sec : sections_) {
    uint64_t t = 0;
    for (auto& p : sec) t += p.nbits;
    total += t;
    if (!single) sz.push_back((uint32_t)((t + 7) / 8));
  }
  if (single) sz.push_back((uint32_t)((total + 7) / 8));
  return sz;
}

size_t PieceList::place(const BitWriter* head, bool single) {
  placed_.clear();
  uint64_t dst = 0;
  auto emit = [&](const Piece& p) {
    if (p.nbits) placed_.push_back({p.src, dst, p.nbits, p.arena, 0});
    dst += p.nbits;
  };
  if (head) {
    emit(add_chunk(*head));
    dst = (dst + 7) & ~7ull;  // (the TOC ends byte aligned)
  }
  for (auto& sec : sections_) {
    for (auto& p : sec) emit(p);
    if (!single) dst = (dst + 7) & ~7ull;
  }
  dst = (dst + 7) & ~7ull;
  chunk_words_.push_back(0);  // read-ahead guard
  return (size_t)(dst / 8);
}

}  // namespace jxg
