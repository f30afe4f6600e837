// jxg_cli_io.h -- file and image I/O of the two command-line tools (jxg_cjxl,
// jxg_djxl): whole files, 8-bit PNG in and out, binary PPM (P6) and PGM (P5).
// Needs zlib and the standard library only.  Every reader takes the file's
// bytes, checks each size before it is used and answers a malformed file with
// false and one message: tests/native/cli_io.cpp runs them over thousands of
// damaged files under the host sanitizers.
#pragma once
#include <zlib.h>

#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace jxg_cli {

// The longest side a reader accepts: jxg_encode_rgb8's own limit (include/jxg.h
// refuses xsize or ysize above 2^18), so no reader hands on a frame the encoder
// would refuse for its size.
constexpr uint32_t kMaxSide = 1u << 18;

// The whole file, read in pieces until end of file (the size the file system
// reports is only the first piece's size, so pipes and growing files read
// too); a read error is an error.
inline bool read_file(const char* path, std::vector<uint8_t>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  long hint = std::fseek(f, 0, SEEK_END) == 0 ? std::ftell(f) : -1;
  if (std::fseek(f, 0, SEEK_SET) != 0 || hint > (1L << 31)) hint = -1;  // (a hint, not trusted)
  out.resize(hint > 0 ? (size_t)hint + 1 : (size_t)1 << 16);
  size_t n = 0;
  for (;;) {
    n += std::fread(out.data() + n, 1, out.size() - n, f);
    if (n < out.size()) break;  // end of file or an error
    out.resize(out.size() * 2);
  }
  const bool ok = !std::ferror(f);
  std::fclose(f);
  out.resize(ok ? n : 0);
  return ok;
}

inline bool write_file(const char* path, const uint8_t* data, size_t size) {
  FILE* f = std::fopen(path, "wb");
  const bool wr = f && std::fwrite(data, 1, size, f) == size;
  return (!f || std::fclose(f) == 0) && wr;
}

// binary PPM / PGM: "P6" (3 bytes a pixel) or "P5" (1), maxval 255
inline bool write_pnm(const char* path, int ch, const uint8_t* px, uint32_t w, uint32_t h) {
  FILE* f = std::fopen(path, "wb");
  const size_t n = (size_t)w * h * ch;
  const bool wr = f && px && std::fprintf(f, "P%d\n%u %u\n255\n", ch == 3 ? 6 : 5, w, h) > 0 &&
                  std::fwrite(px, 1, n, f) == n;
  return (!f || std::fclose(f) == 0) && wr;
}
inline bool write_ppm(const char* path, const uint8_t* rgb, uint32_t w, uint32_t h) {
  return write_pnm(path, 3, rgb, w, h);
}
inline bool write_pgm(const char* path, const uint8_t* map, uint32_t w, uint32_t h) {
  return write_pnm(path, 1, map, w, h);
}

// ---- PNG -------------------------------------------------------------------

constexpr uint8_t kPngSig[8] = {137, 80, 78, 71, 13, 10, 26, 10};

inline uint32_t be32(const uint8_t* p) {
  return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}

struct PngHeader {
  uint32_t w = 0, h = 0;
  int ch = 0;                                            // bytes a pixel: 1, 2, 3, 4
  std::vector<std::pair<const uint8_t*, size_t>> idat;   // the IDAT pieces in place
};

// Everything decode_png relies on, checked before it allocates: the signature;
// IHDR as the first chunk, 13 bytes at least; 8-bit, non-interlaced gray /
// gray+alpha / RGB / RGBA; sides in 1 .. kMaxSide; every chunk inside the file;
// and that the image the header claims can come out of the IDAT bytes there
// are.  Deflate expands at most 1032 : 1 -- a match is at most 258 bytes long
// (zlib.h under deflateGetDictionary: "matches can be up to 258 bytes long";
// RFC 1951 3.2.5) and takes at least one bit for its length and one for its
// distance, so a byte of input gives at most 4 * 258 = 1032 bytes, the limit
// the zlib technical notes state.  The filtered rows, (w * ch + 1) * h bytes, therefore need at least
// 1 / 1032 of that in IDAT bytes; one stored block's 64 KB is allowed on top,
// so no small image depends on the ratio.  A header of 2^18 x 2^18 over a
// 60-byte IDAT is a truncated PNG and allocates nothing.  (Chunk CRCs are not
// checked.)
inline bool png_header(const std::vector<uint8_t>& d, PngHeader& hd, std::string& err) {
  if (d.size() < 8 || std::memcmp(d.data(), kPngSig, 8)) return err = "not a PNG", false;
  hd = PngHeader{};
  int depth = 0, ctype = -1, interlace = 0;
  uint64_t idat_bytes = 0;
  for (size_t p = 8; p + 12 <= d.size();) {
    const uint32_t len = be32(&d[p]);
    const uint8_t* type = &d[p + 4];
    if (p + 12 + (size_t)len > d.size()) return err = "truncated PNG", false;
    const uint8_t* body = &d[p + 8];
    if (p == 8) {
      if (std::memcmp(type, "IHDR", 4) || len < 13)
        return err = "bad PNG header (IHDR comes first and holds 13 bytes)", false;
      hd.w = be32(body);
      hd.h = be32(body + 4);
      depth = body[8];
      ctype = body[9];
      interlace = body[12];
    } else if (!std::memcmp(type, "IDAT", 4)) {
      hd.idat.emplace_back(body, (size_t)len);
      idat_bytes += len;
    } else if (!std::memcmp(type, "IEND", 4)) {
      break;
    }
    p += 12 + (size_t)len;
  }
  if (ctype < 0) return err = "truncated PNG", false;  // (no room for a first chunk)
  if (depth != 8 || interlace || !(ctype == 0 || ctype == 2 || ctype == 4 || ctype == 6))
    return err = "unsupported PNG (need 8-bit, non-interlaced gray/RGB[A])", false;
  if (hd.w == 0 || hd.h == 0 || hd.w > kMaxSide || hd.h > kMaxSide)
    return err = "bad PNG size", false;
  hd.ch = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 4 ? 2 : 4;
  const uint64_t filtered = ((uint64_t)hd.w * hd.ch + 1) * hd.h;  // < 2^39
  if (hd.idat.empty() || filtered > 1032 * idat_bytes + 65536) return err = "truncated PNG", false;
  return true;
}

// PNG: the IDAT stream is inflated in 1 MB pieces and every completed row is
// unfiltered straight into the RGB output (one switch per row, the filter's
// own loop; no whole-image inflate buffer), so the pass over the pixels runs
// while the data is still in cache.  (The first form inflated the whole
// image, then unfiltered byte by byte through a switch: 275 ms of an 8K
// frame's 496 ms process wall time, bench.py single_image, round 6.)
inline bool unfilter_row(uint8_t ft, const uint8_t* src, const uint8_t* prev, uint8_t* row,
                         size_t stride, int ch) {
  switch (ft) {
    case 0:
      std::memcpy(row, src, stride);
      return true;
    case 1:
      for (size_t x = 0; x < stride; x++) row[x] = (uint8_t)(src[x] + (x >= (size_t)ch ? row[x - ch] : 0));
      return true;
    case 2:
      for (size_t x = 0; x < stride; x++) row[x] = (uint8_t)(src[x] + prev[x]);
      return true;
    case 3:
      for (size_t x = 0; x < stride; x++)
        row[x] = (uint8_t)(src[x] + ((x >= (size_t)ch ? row[x - ch] : 0) + prev[x]) / 2);
      return true;
    case 4:
      for (size_t x = 0; x < stride; x++) {
        const int a = x >= (size_t)ch ? row[x - ch] : 0, b = prev[x],
                  c = x >= (size_t)ch ? prev[x - ch] : 0;
        const int pp = a + b - c, pa = std::abs(pp - a), pb = std::abs(pp - b), pc = std::abs(pp - c);
        row[x] = (uint8_t)(src[x] + ((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c)));
      }
      return true;
    default:
      return false;
  }
}

// 8-bit gray / gray+alpha / RGB / RGBA, non-interlaced -> RGB (alpha dropped)
inline bool decode_png(const std::vector<uint8_t>& d, std::vector<uint8_t>& rgb, uint32_t& w,
                       uint32_t& h, std::string& err) {
  PngHeader hd;
  if (!png_header(d, hd, err)) return false;
  w = hd.w;
  h = hd.h;
  const int ch = hd.ch;
  const auto& idat = hd.idat;
  const size_t stride = (size_t)w * ch, rowbytes = stride + 1;
  rgb.resize((size_t)w * h * 3);
  // RGB rows are unfiltered in place in the output; other layouts go through
  // a two-row buffer and are converted per row
  std::vector<uint8_t> tmp(ch == 3 ? 0 : 2 * stride, 0), zero(stride, 0);
  std::vector<uint8_t> buf((size_t)1 << 20);
  if (buf.size() < 2 * rowbytes) buf.resize(2 * rowbytes);
  z_stream zs{};
  if (inflateInit(&zs) != Z_OK) return err = "PNG inflate failed", false;
  size_t have = 0, piece = 0;
  uint32_t y = 0;
  int zr = Z_OK;
  while (y < h) {
    if (zs.avail_in == 0 && piece < idat.size()) {
      zs.next_in = const_cast<Bytef*>(idat[piece].first);
      zs.avail_in = (uInt)idat[piece].second;
      piece++;
    }
    zs.next_out = buf.data() + have;
    zs.avail_out = (uInt)(buf.size() - have);
    zr = inflate(&zs, Z_NO_FLUSH);
    if (zr != Z_OK && zr != Z_STREAM_END && !(zr == Z_BUF_ERROR && zs.avail_in == 0)) break;
    have = buf.size() - zs.avail_out;
    size_t used = 0;
    while (y < h && have - used >= rowbytes) {
      const uint8_t* src = buf.data() + used;
      uint8_t* row = ch == 3 ? &rgb[(size_t)y * stride] : &tmp[(y & 1) * stride];
      const uint8_t* prev = y == 0 ? zero.data() : (ch == 3 ? row - stride : &tmp[((y + 1) & 1) * stride]);
      if (!unfilter_row(src[0], src + 1, prev, row, stride, ch)) {
        inflateEnd(&zs);
        return err = "bad PNG filter", false;
      }
      if (ch != 3) {
        uint8_t* o = &rgb[(size_t)y * w * 3];
        for (uint32_t x = 0; x < w; x++)
          for (int c = 0; c < 3; c++) o[x * 3 + c] = row[x * ch + (ch >= 3 ? c : 0)];
      }
      used += rowbytes;
      y++;
    }
    std::memmove(buf.data(), buf.data() + used, have - used);
    have -= used;
    if (zr == Z_STREAM_END || (zs.avail_in == 0 && piece == idat.size() && zs.avail_out != 0))
      if (y < h && have < rowbytes) break;
  }
  inflateEnd(&zs);
  if (y != h) return err = "PNG inflate failed", false;
  return true;
}

inline void put_be32(std::vector<uint8_t>& o, uint32_t v) {
  for (int s = 24; s >= 0; s -= 8) o.push_back((uint8_t)(v >> s));
}

inline void put_chunk(std::vector<uint8_t>& o, const char* type, const uint8_t* body, size_t len) {
  put_be32(o, (uint32_t)len);
  const size_t at = o.size();
  o.insert(o.end(), type, type + 4);
  o.insert(o.end(), body, body + len);
  put_be32(o, (uint32_t)crc32(0L, o.data() + at, (uInt)(4 + len)));
}

// an 8-bit RGB PNG: filter type 0, zlib level 1, IDAT pieces of 1 MB at most
inline bool encode_png(const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, std::vector<uint8_t>& out) {
  out.assign(kPngSig, kPngSig + 8);
  std::vector<uint8_t> ihdr;
  put_be32(ihdr, w);
  put_be32(ihdr, h);
  const uint8_t tail[5] = {8, 2, 0, 0, 0};  // 8-bit RGB, deflate, adaptive filtering, no interlace
  ihdr.insert(ihdr.end(), tail, tail + 5);
  put_chunk(out, "IHDR", ihdr.data(), ihdr.size());
  const size_t row = (size_t)w * 3;
  std::vector<uint8_t> raw((row + 1) * h);
  for (uint32_t y = 0; y < h; y++) {
    raw[(row + 1) * y] = 0;  // filter type None
    std::memcpy(&raw[(row + 1) * y + 1], &rgb[row * y], row);
  }
  z_stream zs{};
  if (deflateInit(&zs, 1) != Z_OK) return false;
  std::vector<uint8_t> buf((size_t)1 << 20);
  zs.next_in = raw.data();
  size_t left = raw.size();
  int zr = Z_OK;
  while (zr != Z_STREAM_END) {
    const size_t piece = left < ((size_t)1 << 30) ? left : ((size_t)1 << 30);
    zs.avail_in = (uInt)piece;
    left -= piece;
    do {
      zs.next_out = buf.data();
      zs.avail_out = (uInt)buf.size();
      zr = deflate(&zs, left ? Z_NO_FLUSH : Z_FINISH);
      if (zr == Z_STREAM_ERROR) {
        deflateEnd(&zs);
        return false;
      }
      const size_t n = buf.size() - zs.avail_out;
      if (n) put_chunk(out, "IDAT", buf.data(), n);
    } while (zs.avail_out == 0 && zr != Z_STREAM_END);
  }
  deflateEnd(&zs);
  put_chunk(out, "IEND", nullptr, 0);
  return true;
}

// ---- PPM / PGM ---------------------------------------------------------------

// "P6 W H 255" and one whitespace, in the first 64 bytes; sides in
// 1 .. kMaxSide, checked before any product of them is formed; the pixels
// all there.  `off` is where they start.
inline bool ppm_header(const std::vector<uint8_t>& d, uint32_t& w, uint32_t& h, size_t& off,
                       std::string& err) {
  const std::string s(d.begin(), d.begin() + (long)(d.size() < 64 ? d.size() : 64));
  unsigned W = 0, H = 0, M = 0;
  int n = 0;
  if (std::sscanf(s.c_str(), "P6 %u %u %u%n", &W, &H, &M, &n) != 3 || M != 255)
    return err = "unsupported PPM", false;
  if (W == 0 || H == 0 || W > kMaxSide || H > kMaxSide) return err = "bad PPM size", false;
  off = (size_t)n + 1;
  if (d.size() < off + (size_t)W * H * 3) return err = "truncated PPM", false;
  w = W;
  h = H;
  return true;
}

inline bool read_ppm(const std::vector<uint8_t>& d, std::vector<uint8_t>& rgb, uint32_t& w,
                     uint32_t& h, std::string& err) {
  size_t off = 0;
  if (!ppm_header(d, w, h, off, err)) return false;
  rgb.assign(d.begin() + (long)off, d.begin() + (long)(off + (size_t)w * h * 3));
  return true;
}

inline bool is_ppm(const std::vector<uint8_t>& d) {
  return d.size() >= 2 && d[0] == 'P' && d[1] == '6';
}

// the image size a reader will accept for this file, before it is decoded
// (0 x 0 if the header check of its format refuses it)
inline void probe_dims(const std::vector<uint8_t>& d, uint32_t& w, uint32_t& h) {
  std::string err;
  PngHeader hd;
  size_t off = 0;
  w = h = 0;
  if (is_ppm(d))
    (void)ppm_header(d, w, h, off, err);  // (sets the size only when it accepts)
  else if (png_header(d, hd, err))
    w = hd.w, h = hd.h;
}

// a per-block map as a binary PGM (P5, maxval 255): whitespace- and
// #-comment-separated header tokens, then exactly width x height bytes
inline bool read_pgm(const std::vector<uint8_t>& d, std::vector<uint8_t>& map, uint32_t& bw,
                     uint32_t& bh, std::string& err) {
  size_t pos = 0;
  auto token = [&](std::string& t) {
    t.clear();
    while (pos < d.size()) {
      if (d[pos] == '#') {
        while (pos < d.size() && d[pos] != '\n') pos++;
      } else if (std::isspace(d[pos])) {
        pos++;
      } else {
        break;
      }
    }
    while (pos < d.size() && !std::isspace(d[pos])) t.push_back((char)d[pos++]);
    return !t.empty();
  };
  std::string magic, sw, sh, sm;
  if (!token(magic) || magic != "P5" || !token(sw) || !token(sh) || !token(sm) || sm != "255" ||
      sw.size() > 6 || sh.size() > 6 || sw.find_first_not_of("0123456789") != std::string::npos ||
      sh.find_first_not_of("0123456789") != std::string::npos) {
    err = "not a binary PGM (P5) of maxval 255";
    return false;
  }
  bw = (uint32_t)std::atoi(sw.c_str());
  bh = (uint32_t)std::atoi(sh.c_str());
  pos++;  // the single whitespace after maxval
  if (!bw || !bh || pos > d.size() || d.size() - pos != (size_t)bw * bh) {
    err = "the PGM's data is not width x height bytes";
    return false;
  }
  map.assign(d.begin() + (long)pos, d.end());
  return true;
}

}  // namespace jxg_cli
