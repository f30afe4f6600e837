// cli_io -- the command-line tools' file readers (csrc/jxg_cli_io.h) on damaged
// input, built by tests/test_cli_io.py with the host sanitizers where the
// compiler has them.  What a sanitizer finds ends the program with its report.
//
//   cli_io mutate FILE.png IMAGE.rgb NBYTES NTRUNC
//       FILE.png decodes to the raw RGB bytes of IMAGE.rgb; then NBYTES copies
//       with one byte changed -- positions spread evenly over the whole file,
//       values from a fixed-seed generator -- and NTRUNC truncations spread the
//       same way go through probe_dims and decode_png.  Every call must return.
//       Prints how many of the changed files still decoded.
//   cli_io refuse png|ppm|pgm FILE...
//       every file is refused with a message, and probe_dims gives 0 x 0
//   cli_io accept pgm FILE...
//   cli_io roundtrip
//       encode_png, then decode_png, of 1 x 1, 53 x 37 and 1500 x 400 (larger
//       than one inflate window)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../jpeg-xl-lossy-image-compression-thesis_amd/csrc/jxg_cli_io.h"

using namespace jxg_cli;

static uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// exact-size copies, so a read one byte past the input is a heap overflow
static bool decode(const std::vector<uint8_t>& d, std::vector<uint8_t>& rgb, uint32_t& w, uint32_t& h) {
  uint32_t pw = 0, ph = 0;
  probe_dims(d, pw, ph);
  std::string err;
  const bool ok = decode_png(d, rgb, w, h, err);
  if (!ok && err.empty()) {
    std::printf("refused without a message\n");
    std::exit(1);
  }
  if (ok && (pw != w || ph != h)) {  // (what the warm-up thread is given)
    std::printf("probe_dims %u x %u, decoded %u x %u\n", pw, ph, w, h);
    std::exit(1);
  }
  return ok;
}

static int mutate(const char* png_path, const char* rgb_path, int nbytes, int ntrunc) {
  std::vector<uint8_t> data, want, rgb;
  if (!read_file(png_path, data) || data.empty() || !read_file(rgb_path, want)) {
    std::fprintf(stderr, "cannot read %s / %s\n", png_path, rgb_path);
    return 2;
  }
  uint32_t w = 0, h = 0;
  if (!decode(data, rgb, w, h) || rgb != want) {
    std::printf("unmutated: not the source image\n");
    return 1;
  }
  std::printf("unmutated: ok\n");
  uint64_t seed = 0x4A584C44ull;  // fixed: the same mutations in every run
  int decoded = 0, cut_decoded = 0;
  for (int i = 0; i < nbytes; i++) {
    const size_t pos = (size_t)((double)i * (double)data.size() / (double)nbytes);
    std::vector<uint8_t> m(data);
    m[pos] ^= (uint8_t)(1 + splitmix64(seed) % 255);
    decoded += decode(m, rgb, w, h);
  }
  for (int i = 0; i < ntrunc; i++) {
    const size_t n = 1 + (size_t)((double)i * (double)(data.size() - 1) / (double)ntrunc);
    const std::vector<uint8_t> m(data.begin(), data.begin() + (long)n);
    cut_decoded += decode(m, rgb, w, h);
  }
  std::printf("%d byte changes: %d still decoded; %d truncations: %d still decoded\n", nbytes,
              decoded, ntrunc, cut_decoded);
  return 0;
}

static bool read_kind(const std::string& kind, const std::vector<uint8_t>& d, std::string& err,
                      uint32_t& w, uint32_t& h) {
  std::vector<uint8_t> px;
  if (kind == "png") return decode_png(d, px, w, h, err);
  if (kind == "ppm") return read_ppm(d, px, w, h, err);
  return read_pgm(d, px, w, h, err);
}

static int verdicts(bool accept, const std::string& kind, int n, char** files) {
  for (int i = 0; i < n; i++) {
    std::vector<uint8_t> d;
    if (!read_file(files[i], d)) {
      std::fprintf(stderr, "cannot read %s\n", files[i]);
      return 2;
    }
    std::string err;
    uint32_t w = 0, h = 0, pw = 0, ph = 0;
    const bool ok = read_kind(kind, d, err, w, h);
    if (kind != "pgm") probe_dims(d, pw, ph);
    std::printf("%s: %s\n", files[i], ok ? "read" : err.c_str());
    if (ok != accept || (!ok && (err.empty() || pw || ph))) return 1;
  }
  return 0;
}

static int roundtrip() {
  const uint32_t sizes[3][2] = {{1, 1}, {53, 37}, {1500, 400}};
  uint64_t seed = 7;
  for (const auto& s : sizes) {
    std::vector<uint8_t> rgb((size_t)s[0] * s[1] * 3), png, back;
    for (uint8_t& v : rgb) v = (uint8_t)splitmix64(seed);
    for (size_t i = 0; i < rgb.size() / 2; i++) rgb[i] = rgb[i % 7];  // (something to deflate)
    uint32_t w = 0, h = 0;
    std::string err;
    if (!encode_png(rgb, s[0], s[1], png) || !decode_png(png, back, w, h, err) || w != s[0] ||
        h != s[1] || back != rgb) {
      std::printf("%u x %u: no round trip (%s)\n", s[0], s[1], err.c_str());
      return 1;
    }
    std::printf("%u x %u: ok, %zu bytes\n", s[0], s[1], png.size());
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "mutate" && argc == 6)
    return mutate(argv[2], argv[3], std::atoi(argv[4]), std::atoi(argv[5]));
  if ((mode == "refuse" || mode == "accept") && argc > 3)
    return verdicts(mode == "accept", argv[2], argc - 3, argv + 3);
  if (mode == "roundtrip") return roundtrip();
  std::fprintf(stderr, "usage: cli_io mutate FILE.png IMAGE.rgb NBYTES NTRUNC | "
                       "refuse|accept png|ppm|pgm FILE... | roundtrip\n");
  return 2;
}
