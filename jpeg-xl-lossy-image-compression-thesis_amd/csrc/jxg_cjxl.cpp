// jxg_cjxl -- cjxl-argv-compatible command line over the C ABI.
//
// The reference harness runs `cjxl IN OUT --distance=D --effort=E`
// (benchmark-jpegxl/src/docker_manager.rs:126-136) and maps a non-zero exit
// status to "skip" (benchmark.rs:654-677).  This tool accepts the same argv
// shape (plus --proposals=none|P|F|PF and --device=N), reads 8-bit PNG
// (gray / gray+alpha / RGB / RGBA, non-interlaced; alpha dropped) or binary
// PPM, encodes on the GPU and writes the codestream.  Exit 0 on success; a
// message on stderr and exit 1 otherwise.
//
// `jxg_cjxl INPUT OUTDIR --sweep=LIST` encodes INPUT at every `distance effort`
// line of the file LIST in one process and one jxg_sweep_rgb8 call (the other
// flags apply to every point) and writes OUTDIR/<stem>-<distance>-<effort>.jxl,
// the harness's names (benchmark.rs:644-650) -- its per-image loop without a
// process start per setting.
//
// `--jxg_report=`, `--jxg_rates=` and `--jxg_ab=` (not cjxl options) append the
// encode's strategy report, rate report and A/B report against the same encode
// with other proposals as the CSV text of jxg/harness.py.
//
// `--jxg_strategy_in=MAP.pgm [--jxg_qf_in=MAP.pgm]` (not cjxl options) encode
// with the file's AC-strategy map (and quant field) instead of the search
// (jxg_encode_forced_rgb8); `--jxg_strategy_out=` / `--jxg_qf_out=` write the
// maps of whatever was encoded.  One byte per block, binary PGM.  A map of the
// wrong geometry or one the validator refuses: the reason and the block on
// stderr, exit 1.  Not with --sweep.
//
// `--jxg_trace=FILE.csv` (not a cjxl option) makes the encode a traced one
// (jxg_encode_traced_rgb8: the same codestream) and appends the summary of its
// search trace, one row per scan index.  Not with --sweep or --jxg_strategy_in.
//
// `--jxg_sweep_trace=FILE.csv` (not a cjxl option; only with --sweep) appends
// the same rows for every point of the sweep whose effort is >= 5, traced on its
// lane (jxg_set_sweep_trace: the same codestreams); a point without a search
// writes no rows and one line on stderr.
#include <zlib.h>

#include <cctype>
#include <charconv>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/jxg.h"

namespace {

bool read_file(const char* path, std::vector<uint8_t>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  out.resize(n > 0 ? (size_t)n : 0);
  bool ok = n >= 0 && std::fread(out.data(), 1, out.size(), f) == out.size();
  std::fclose(f);
  return ok;
}

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | p[1] << 16 | p[2] << 8 | p[3]; }

// PNG: the IDAT stream is inflated in 1 MB pieces and every completed row is
// unfiltered straight into the RGB output (one switch per row, the filter's
// own loop; no whole-image inflate buffer), so the pass over the pixels runs
// while the data is still in cache.  (The first form inflated the whole
// image, then unfiltered byte by byte through a switch: 275 ms of an 8K
// frame's 496 ms process wall time, bench.py single_image, round 6.)
bool unfilter_row(uint8_t ft, const uint8_t* src, const uint8_t* prev, uint8_t* row,
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

bool decode_png(const std::vector<uint8_t>& d, std::vector<uint8_t>& rgb, uint32_t& w,
                uint32_t& h, std::string& err) {
  static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
  if (d.size() < 8 || std::memcmp(d.data(), sig, 8)) return err = "not a PNG", false;
  size_t p = 8;
  int depth = 0, ctype = -1, interlace = 0;
  std::vector<std::pair<const uint8_t*, size_t>> idat;  // the IDAT pieces in place
  while (p + 12 <= d.size()) {
    const uint32_t len = be32(&d[p]);
    const char* type = (const char*)&d[p + 4];
    if (p + 12 + (size_t)len > d.size()) return err = "truncated PNG", false;
    const uint8_t* body = &d[p + 8];
    if (!std::memcmp(type, "IHDR", 4)) {
      w = be32(body);
      h = be32(body + 4);
      depth = body[8];
      ctype = body[9];
      interlace = body[12];
    } else if (!std::memcmp(type, "IDAT", 4)) {
      idat.emplace_back(body, (size_t)len);
    } else if (!std::memcmp(type, "IEND", 4)) {
      break;
    }
    p += 12 + len;
  }
  if (depth != 8 || interlace || !(ctype == 0 || ctype == 2 || ctype == 4 || ctype == 6))
    return err = "unsupported PNG (need 8-bit, non-interlaced gray/RGB[A])", false;
  if (w == 0 || h == 0 || w > (1u << 20) || h > (1u << 20)) return err = "bad PNG size", false;
  const int ch = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 4 ? 2 : 4;
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

// the image size from the PNG IHDR / PPM header (0 x 0 if unknown)
void probe_dims(const std::vector<uint8_t>& d, uint32_t& w, uint32_t& h) {
  static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
  w = h = 0;
  if (d.size() >= 24 && !std::memcmp(d.data(), sig, 8) && !std::memcmp(&d[12], "IHDR", 4)) {
    w = be32(&d[16]);
    h = be32(&d[20]);
  } else if (d.size() >= 2 && d[0] == 'P' && d[1] == '6') {
    std::string s(d.begin(), d.begin() + std::min<size_t>(d.size(), 64));
    unsigned W = 0, H = 0;
    if (std::sscanf(s.c_str(), "P6 %u %u", &W, &H) == 2) w = W, h = H;
  }
  if (w > (1u << 18) || h > (1u << 18)) w = h = 0;
}

bool decode_ppm(const std::vector<uint8_t>& d, std::vector<uint8_t>& rgb, uint32_t& w,
                uint32_t& h, std::string& err) {
  std::string s(d.begin(), d.begin() + std::min<size_t>(d.size(), 64));
  unsigned W, H, M;
  int off = 0;
  if (std::sscanf(s.c_str(), "P6 %u %u %u%n", &W, &H, &M, &off) != 3 || M != 255)
    return err = "unsupported PPM", false;
  off += 1;
  w = W;
  h = H;
  if (d.size() < (size_t)off + (size_t)W * H * 3) return err = "truncated PPM", false;
  rgb.assign(d.begin() + off, d.begin() + off + (size_t)W * H * 3);
  return true;
}

// Rust's `{}` of an f64 (the harness's file names): the shortest digits that
// round-trip, never an exponent, "1" for 1.0
std::string rust_f64(double v) {
  char buf[400];
  const auto r = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::fixed);
  return std::string(buf, r.ptr);
}

std::string rust_f32(float v) {
  char buf[200];
  const auto r = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::fixed);
  return std::string(buf, r.ptr);
}

// --jxg_report=FILE.csv: the rows of jxg/harness.py strategy_stats /
// write_strategy_stats for one encode -- one per non-empty strategy of the
// report, appended; the header goes only into a missing or empty file
const char* const kStrategyNames[JXG_NUM_STRATEGIES] = {
    "DCT8", "IDENTITY", "DCT2X2", "DCT4X4", "DCT16X16", "DCT32X32", "DCT16X8", "DCT8X16",
    "DCT32X8", "DCT8X32", "DCT32X16", "DCT16X32", "DCT4X8", "DCT8X4", "AFV0", "AFV1", "AFV2",
    "AFV3", "DCT64X64", "DCT64X32", "DCT32X64", "DCT128X128", "DCT128X64", "DCT64X128",
    "DCT256X256", "DCT256X128", "DCT128X256"};
std::string csv_field(const std::string& v) {  // (Python's csv module, minimal quoting)
  if (v.find_first_of(",\"\r\n") == std::string::npos) return v;
  std::string q = "\"";
  for (char ch : v) {
    if (ch == '"') q += '"';
    q += ch;
  }
  return q + "\"";
}
// a report's CSV, opened for appending rows: the header goes only into a
// missing or empty file
FILE* open_csv(const char* path, const char* header) {
  std::error_code ec;
  const auto size = std::filesystem::file_size(path, ec);
  const bool fresh = ec || size == 0;
  FILE* f = std::fopen(path, fresh ? "w" : "a");
  if (f && fresh) std::fputs(header, f);
  return f;
}
// whose rows: the original's name, the compressed name, distance, effort -- the
// columns every row of a report starts with (A/B: the compressed name twice,
// sides A and B)
struct RowKey {
  std::string orig_name, comp_name;
  float distance;
  int effort;
  std::string lead(bool ab = false) const {
    return csv_field(orig_name) + "," + csv_field(comp_name) + "," +
           (ab ? csv_field(comp_name) + "," : "") + rust_f32(distance) + "," +
           std::to_string(effort);
  }
};
bool write_report_rows(const char* path, const RowKey& key, const jxg_strategy_report& rep,
                       uint32_t w, uint32_t h) {
  FILE* f = open_csv(path,
                     "Original Image Name,Compressed Image Name,Distance,Effort,Strategy,Name,"
                     "Varblocks,Blocks,Pixels,Area Share,Nonzeros X,Nonzeros Y,Nonzeros B,"
                     "Mean Quant Field,SSE,MSE\n");
  if (!f) return false;
  const std::string lead = key.lead();
  for (int i = 0; i < JXG_NUM_STRATEGIES; i++) {
    const jxg_strategy_row& r = rep.row[i];
    if (!r.blocks) continue;
    std::fprintf(f, "%s,%d,%s,%llu,%llu,%llu,%s,%llu,%llu,%llu,%s,%llu,%s\n", lead.c_str(), i,
                 kStrategyNames[i], (unsigned long long)r.varblocks, (unsigned long long)r.blocks,
                 (unsigned long long)r.pixels,
                 rust_f64((double)r.pixels / ((double)w * (double)h)).c_str(),
                 (unsigned long long)r.nonzeros[0], (unsigned long long)r.nonzeros[1],
                 (unsigned long long)r.nonzeros[2],
                 rust_f64((double)r.qf_sum / (double)r.blocks).c_str(),
                 (unsigned long long)r.sse,
                 rust_f64((double)r.sse / (3.0 * (double)r.pixels)).c_str());
  }
  return std::fclose(f) == 0;
}

// --jxg_rates=FILE.csv: the rows of jxg/harness.py rate_stats / write_rate_stats
// for one encode -- one per strategy of the rate report that holds tokens
bool write_rate_rows(const char* path, const RowKey& key, const struct jxg_rate_report& rep) {
  FILE* f = open_csv(path,
                     "Original Image Name,Compressed Image Name,Distance,Effort,Strategy,Name,"
                     "Tokens X,Tokens Y,Tokens B,Bits X,Bits Y,Bits B,AC Bits,Stream Bits\n");
  if (!f) return false;
  const std::string lead = key.lead();
  for (int i = 0; i < JXG_NUM_STRATEGIES; i++) {
    const jxg_rate_row& r = rep.row[i];
    if (!(r.tokens[0] + r.tokens[1] + r.tokens[2])) continue;
    std::fprintf(f, "%s,%d,%s,%llu,%llu,%llu,%s,%s,%s,%llu,%llu\n", lead.c_str(), i,
                 kStrategyNames[i], (unsigned long long)r.tokens[0],
                 (unsigned long long)r.tokens[1],
                 (unsigned long long)r.tokens[2],
                 rust_f64((double)r.cost[0] / (double)JXG_RATE_UNIT).c_str(),
                 rust_f64((double)r.cost[1] / (double)JXG_RATE_UNIT).c_str(),
                 rust_f64((double)r.cost[2] / (double)JXG_RATE_UNIT).c_str(),
                 (unsigned long long)rep.ac_bits, (unsigned long long)rep.stream_bits);
  }
  return std::fclose(f) == 0;
}

// --jxg_trace=FILE.csv: the summary of the encode's search trace
// (jxg_search_trace), one row per scan index s: the blocks the 8x8 scan gave to
// s, of them by the winner of the scan without hook F (flip[r][s]), the hook-P
// overrides with target s, the blocks merged over, the margin histogram
bool write_trace_rows(const char* path, const RowKey& key, const jxg_trace_summary& t) {
  static const int kScanIds[6] = {0, 3, 2, 12, 13, 1};
  FILE* f = open_csv(path,
                     "Original Image Name,Compressed Image Name,Distance,Effort,Scan Index,Strategy,"
                     "Name,Blocks,Max Px,Scan Wins,Raw DCT8,Raw DCT4X4,Raw DCT2X2,Raw DCT4X8,"
                     "Raw DCT8X4,Raw IDENTITY,Hook P,Merged Over,Margin 0,Margin 1,Margin 2,"
                     "Margin 3,Margin 4,Margin 5,Margin 6,Margin 7,Margin Skipped\n");
  if (!f) return false;
  const std::string lead = key.lead();
  for (int s = 0; s < 6; s++) {
    unsigned long long wins = 0;
    for (int r = 0; r < 6; r++) wins += t.flip[r][s];
    std::fprintf(f, "%s,%d,%d,%s,%u,%u,%llu", lead.c_str(), s, kScanIds[s],
                 kStrategyNames[kScanIds[s]], t.blocks, t.max_px, wins);
    for (int r = 0; r < 6; r++) std::fprintf(f, ",%u", t.flip[r][s]);
    std::fprintf(f, ",%u,%u", t.hook_p[s], t.merged_over[s]);
    for (int k = 0; k < 8; k++) std::fprintf(f, ",%u", t.margin[s][k]);
    std::fprintf(f, ",%u\n", t.margin_skipped[s]);
  }
  return std::fclose(f) == 0;
}

// --jxg_ab=FILE.csv: the rows of jxg/harness.py ab_stats / write_ab_stats for
// one pair of encodes -- one per non-empty cell of the A/B report
bool write_ab_rows(const char* path, const RowKey& key, const jxg_ab_report& rep, uint32_t w,
                   uint32_t h) {
  FILE* f = open_csv(path,
                     "Original Image Name,Compressed Image Name A,Compressed Image Name B,Distance,"
                     "Effort,From,From Name,To,To Name,Blocks,Pixels,Area Share,SSE A,SSE B,Bits A,"
                     "Bits B,Diff SSE,Diff Bits\n");
  if (!f) return false;
  const std::string lead = key.lead(true);
  for (int i = 0; i < JXG_NUM_STRATEGIES; i++)
    for (int j = 0; j < JXG_NUM_STRATEGIES; j++) {
      const jxg_ab_cell& c = rep.cell[i][j];
      if (!c.blocks) continue;
      std::fprintf(f, "%s,%d,%s,%d,%s,%llu,%llu,%s,%llu,%llu,%s,%s,%lld,%s\n", lead.c_str(), i,
                   kStrategyNames[i], j, kStrategyNames[j], (unsigned long long)c.blocks,
                   (unsigned long long)c.pixels,
                   rust_f64((double)c.pixels / ((double)w * (double)h)).c_str(),
                   (unsigned long long)c.sse_a, (unsigned long long)c.sse_b,
                   rust_f64((double)c.cost_a / (double)JXG_RATE_UNIT).c_str(),
                   rust_f64((double)c.cost_b / (double)JXG_RATE_UNIT).c_str(),
                   (long long)c.sse_b - (long long)c.sse_a,
                   rust_f64((double)((long long)c.cost_b - (long long)c.cost_a) /
                            (double)JXG_RATE_UNIT).c_str());
    }
  return std::fclose(f) == 0;
}

struct SweepLine {
  double distance;
  int effort;
};
bool read_sweep_list(const char* path, std::vector<SweepLine>& out) {
  FILE* f = std::fopen(path, "r");
  if (!f) return false;
  char line[256];
  bool ok = true;
  while (ok && std::fgets(line, sizeof(line), f)) {
    const char* s = line + std::strspn(line, " \t\r\n");
    if (!*s || *s == '#') continue;
    SweepLine l{};
    ok = std::sscanf(s, "%lf %d", &l.distance, &l.effort) == 2;
    if (ok) out.push_back(l);
  }
  std::fclose(f);
  return ok && !out.empty();
}

// INPUT at every point of the list -> OUTDIR/<stem>-<distance>-<effort>.jxl
int run_sweep(jxg_ctx* ctx, const jxg_params& p, const char* input, const char* outdir,
              const std::vector<SweepLine>& list, const std::vector<uint8_t>& rgb, uint32_t w,
              uint32_t h, const char* report_path, const char* rates_path, const char* ab_path,
              uint32_t ab_base, const char* sweep_trace_path) {
  // with --jxg_ab the list's points with the base proposals go in front: point
  // m + i is the command line's own and is compared with point i
  const size_t m = list.size(), o = ab_path ? m : 0, n = m + o;
  std::vector<jxg_sweep_point> pts(n);
  std::vector<int32_t> base(n, -1);
  for (size_t i = 0; i < m; i++) {
    pts[o + i] = jxg_sweep_point{(float)list[i].distance, list[i].effort, p.proposals, p.flags};
    if (ab_path) {
      pts[i] = jxg_sweep_point{(float)list[i].distance, list[i].effort, ab_base, p.flags};
      base[o + i] = (int32_t)i;
    }
  }
  const bool chain = report_path || ab_path;  // the points' chains run (quality 1)
  std::vector<jxg_buffer> outs(n, jxg_buffer{nullptr, 0});
  std::vector<jxg_status> sts(n, JXG_OK);
  // with a report the points' chains run (quality 1) and end in the reduction
  std::vector<jxg_quality> qs(chain ? n : 0);
  // the report kinds that ride on the sweep (the rate reports need no chain:
  // they follow each point's emission): file, name in messages, switch, getter,
  // the rows of point i
  std::vector<jxg_strategy_report> reps(report_path ? n : 0);
  std::vector<struct jxg_rate_report> rates(rates_path ? n : 0);
  std::vector<jxg_ab_report> abs(ab_path ? n : 0);
  std::vector<jxg_trace_summary> traces(sweep_trace_path ? n : 0);
  const std::string orig_name = std::filesystem::path(input).filename().string();
  const uint32_t un = (uint32_t)n;
  struct Rider {
    const char *path, *what;
    std::function<jxg_status()> set, fetch;
    std::function<bool(const RowKey&, size_t)> write;
  };
  const Rider riders[] = {
      {report_path, "report", [&] { return jxg_set_sweep_report(ctx, 1); },
       [&] { return jxg_sweep_report(ctx, reps.data(), un); },
       [&](const RowKey& k, size_t i) { return write_report_rows(report_path, k, reps[i], w, h); }},
      {rates_path, "rates", [&] { return jxg_set_sweep_rates(ctx, 1); },
       [&] { return jxg_sweep_rates(ctx, rates.data(), un); },
       [&](const RowKey& k, size_t i) { return write_rate_rows(rates_path, k, rates[i]); }},
      {ab_path, "A/B reports", [&] { return jxg_set_sweep_ab(ctx, base.data(), un); },
       [&] { return jxg_sweep_ab(ctx, abs.data(), un); },
       [&](const RowKey& k, size_t i) { return write_ab_rows(ab_path, k, abs[i], w, h); }},
      // (a point without a search, effort < 5, has the zero summary: no rows)
      {sweep_trace_path, "traces", [&] { return jxg_set_sweep_trace(ctx, 1); },
       [&] { return jxg_sweep_trace(ctx, traces.data(), un); },
       [&](const RowKey& k, size_t i) {
         if (traces[i].blocks) return write_trace_rows(sweep_trace_path, k, traces[i]);
         std::fprintf(stderr, "distance %s effort %d: no search to trace, no rows\n",
                      rust_f64(k.distance).c_str(), k.effort);
         return true;
       }},
  };
  for (const Rider& r : riders)
    if (r.path && r.set() != JXG_OK) return 1;
  const auto t0 = std::chrono::steady_clock::now();
  const jxg_status st =
      jxg_sweep_rgb8(ctx, rgb.data(), w, h, (size_t)w * 3, pts.data(), (uint32_t)n,
                     chain ? 1 : 0, outs.data(), chain ? qs.data() : nullptr, sts.data());
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  bool any = false;
  for (size_t i = o; i < n; i++) any = any || outs[i].data;
  if (st != JXG_OK && !any) {
    std::fprintf(stderr, "sweep failed: %s\n", jxg_status_str(st));
    return 1;
  }
  for (const Rider& r : riders)
    if (r.path && r.fetch() != JXG_OK) {
      std::fprintf(stderr, "sweep %s failed\n", r.what);
      return 1;
    }
  std::error_code ec;
  std::filesystem::create_directories(outdir, ec);
  const std::string stem = std::filesystem::path(input).stem().string();
  int rc = 0;
  for (size_t i = o; i < n; i++) {
    const SweepLine& l = list[i - o];
    if (!outs[i].data) {  // a refused point: the harness skips it
      std::fprintf(stderr, "distance %s effort %d: %s\n", rust_f64(l.distance).c_str(), l.effort,
                   jxg_status_str(sts[i]));
      rc = 1;
      continue;
    }
    const std::string name =
        stem + "-" + rust_f64(l.distance) + "-" + std::to_string(l.effort) + ".jxl";
    const std::string path = (std::filesystem::path(outdir) / name).string();
    const RowKey key{orig_name, name, pts[i].distance, pts[i].effort};
    for (const Rider& r : riders)
      if (r.path && !r.write(key, i)) {
        std::fprintf(stderr, "cannot write %s\n", r.path);
        rc = 1;
      }
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(outs[i].data, 1, outs[i].size, f) != outs[i].size) {
      std::fprintf(stderr, "cannot write %s\n", path.c_str());
      rc = 1;
    }
    if (f) std::fclose(f);
    std::printf("Encoding [VarDCT, d%.3f, effort: %d], %u x %u, %zu bytes, %.3f bpp\n",
                pts[i].distance, pts[i].effort, w, h, outs[i].size,
                outs[i].size * 8.0 / ((double)w * h));
  }
  std::printf("Sweep of %zu points, %u x %u, %.2f MP/s\n", n, w, h,
              (double)n * w * h / 1e6 / sec);
  for (size_t i = 0; i < o; i++) jxg_buffer_free(&outs[i]);  // (the base points' streams)
  return rc;
}

// --jxg_strategy_in / _out, --jxg_qf_in / _out: a per-block map as a binary
// PGM (P5, width = xsize_blocks, height = ysize_blocks, maxval 255)
bool read_pgm(const char* path, std::vector<uint8_t>& map, uint32_t& bw, uint32_t& bh,
              std::string& err) {
  std::vector<uint8_t> d;
  if (!read_file(path, d)) {
    err = "cannot read the file";
    return false;
  }
  size_t pos = 0;
  auto token = [&](std::string& t) {  // whitespace- and #-comment-separated header tokens
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
bool write_pgm(const char* path, const uint8_t* map, uint32_t bw, uint32_t bh) {
  FILE* f = std::fopen(path, "wb");
  const bool ok = f && map && std::fprintf(f, "P5\n%u %u\n255\n", bw, bh) > 0 &&
                  std::fwrite(map, 1, (size_t)bw * bh, f) == (size_t)bw * bh;
  if (f) std::fclose(f);
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr,
                 "usage: %s INPUT OUTPUT [--distance=D] [--effort=E] "
                 "[--proposals=none|P|F|PF] [--coder=ans|prefix] [--gaborish=1|0] "
                 "[--epf=-1|0] [--aq=masking|activity] [--device=N] [--jxg_recon=PATH] "
                 "[--jxg_report=FILE.csv] [--jxg_rates=FILE.csv] "
                 "[--jxg_ab=FILE.csv [--jxg_ab_base=none|P|F|PF]] "
                 "[--jxg_strategy_in=MAP.pgm [--jxg_qf_in=MAP.pgm]] "
                 "[--jxg_strategy_out=MAP.pgm] [--jxg_qf_out=MAP.pgm] [--jxg_trace=FILE.csv]\n"
                 "       %s INPUT OUTDIR --sweep=LIST [the same flags, no maps; "
                 "--jxg_sweep_trace=FILE.csv in place of --jxg_trace]   "
                 "(LIST: `distance effort` lines)\n"
                 "defaults: cjxl's (ANS, --gaborish=1, --epf=-1, masking AQ)\n",
                 argv[0], argv[0]);
    return 1;
  }
  // `cjxl IN OUT --distance=D --effort=E` with no other flag (the harness's
  // argv, docker_manager.rs:126-136) gets cjxl's VarDCT defaults [ext]: ANS,
  // Gaborish on, EPF iterations by distance, the masking quant field
  jxg_params p{1.0f, 7, 0, 1, JXG_FLAGS_CJXL_DEFAULTS, 0};
  // --jxg_recon=PATH (not a cjxl option): also write the decoded image of the
  // codestream, reconstructed on the GPU (jxg_reconstruct_rgb8), as a binary PPM
  const char* recon_path = nullptr;
  const char* sweep_path = nullptr;  // --sweep=LIST: OUTPUT is a directory
  // --jxg_report=FILE.csv (not a cjxl option): append the per-strategy
  // statistics of the encode, or of every point of --sweep= (jxg_strategy_report_rgb8)
  const char* report_path = nullptr;
  // --jxg_rates=FILE.csv (not a cjxl option): append the coded bits per strategy
  // of the encode, or of every point of --sweep= (jxg_rate_report)
  const char* rates_path = nullptr;
  // --jxg_ab=FILE.csv [--jxg_ab_base=none|P|F|PF] (not cjxl options): the
  // encode, or every point of --sweep=, is also run with the base proposals
  // (default none) and the A/B report of the two (jxg_ab_report_rgb8; side B is
  // --proposals) is appended; the codestreams written are unchanged
  const char* ab_path = nullptr;
  uint32_t ab_base = 0;
  // --jxg_strategy_in=MAP.pgm [--jxg_qf_in=MAP.pgm] (not cjxl options): the
  // forced encode (jxg_encode_forced_rgb8) with the file's AC-strategy map and
  // quant field; --jxg_strategy_out= / --jxg_qf_out=: the maps of whatever was
  // encoded.  Binary PGMs of xsize_blocks x ysize_blocks, one byte per block
  const char *acs_in = nullptr, *qf_in = nullptr, *acs_out = nullptr, *qf_out = nullptr;
  // --jxg_trace=FILE.csv (not a cjxl option): the encode is a traced one
  // (jxg_encode_traced_rgb8, the same codestream) and its search trace's summary
  // is appended, one row per scan index; not with --sweep or --jxg_strategy_in
  const char* trace_path = nullptr;
  // --jxg_sweep_trace=FILE.csv (not a cjxl option), only with --sweep: every
  // point of effort >= 5 runs traced on its lane (jxg_set_sweep_trace, the same
  // codestreams) and its summary is appended as --jxg_trace writes it
  const char* sweep_trace_path = nullptr;
  for (int i = 3; i < argc; i++) {
    const char* a = argv[i];
    if (!std::strncmp(a, "--distance=", 11) || !std::strncmp(a, "-d=", 3))
      p.distance = (float)std::atof(std::strchr(a, '=') + 1);
    else if (!std::strncmp(a, "--effort=", 9) || !std::strncmp(a, "-e=", 3))
      p.effort = std::atoi(std::strchr(a, '=') + 1);
    else if (!std::strncmp(a, "--proposals=", 12)) {
      const char* v = a + 12;
      p.proposals = (std::strchr(v, 'P') ? JXG_PROPOSAL_P : 0u) | (std::strchr(v, 'F') ? JXG_PROPOSAL_F : 0u);
    } else if (!std::strncmp(a, "--coder=", 8)) {
      if (!std::strcmp(a + 8, "prefix"))
        p.flags &= ~JXG_FLAG_ANS;
      else if (std::strcmp(a + 8, "ans")) {
        std::fprintf(stderr, "unknown coder: %s\n", a + 8);
        return 1;
      }
    } else if (!std::strncmp(a, "--gaborish=", 11)) {  // cjxl --gaborish
      if (!std::strcmp(a + 11, "0"))
        p.flags &= ~JXG_FLAG_GABORISH;
      else if (std::strcmp(a + 11, "1")) {
        std::fprintf(stderr, "unsupported --gaborish: %s\n", a + 11);
        return 1;
      }
    } else if (!std::strncmp(a, "--epf=", 6)) {  // cjxl --epf: -1 = by distance
      if (!std::strcmp(a + 6, "0"))
        p.flags &= ~JXG_FLAG_EPF;
      else if (std::strcmp(a + 6, "-1")) {
        std::fprintf(stderr, "unsupported --epf (-1 or 0): %s\n", a + 6);
        return 1;
      }
    } else if (!std::strncmp(a, "--aq=", 5)) {  // the quant field heuristic
      if (!std::strcmp(a + 5, "activity"))
        p.flags &= ~JXG_FLAG_AQ_MASKING;
      else if (std::strcmp(a + 5, "masking")) {
        std::fprintf(stderr, "unsupported --aq (masking or activity): %s\n", a + 5);
        return 1;
      }
    } else if (!std::strncmp(a, "--device=", 9))
      p.device = std::atoi(a + 9);
    else if (!std::strncmp(a, "--jxg_recon=", 12))
      recon_path = a + 12;
    else if (!std::strncmp(a, "--sweep=", 8))
      sweep_path = a + 8;
    else if (!std::strncmp(a, "--jxg_report=", 13))
      report_path = a + 13;
    else if (!std::strncmp(a, "--jxg_rates=", 12))
      rates_path = a + 12;
    else if (!std::strncmp(a, "--jxg_ab=", 9))
      ab_path = a + 9;
    else if (!std::strncmp(a, "--jxg_ab_base=", 14)) {
      const char* v = a + 14;
      ab_base = (std::strchr(v, 'P') ? JXG_PROPOSAL_P : 0u) | (std::strchr(v, 'F') ? JXG_PROPOSAL_F : 0u);
    } else if (!std::strncmp(a, "--jxg_strategy_in=", 18))
      acs_in = a + 18;
    else if (!std::strncmp(a, "--jxg_qf_in=", 12))
      qf_in = a + 12;
    else if (!std::strncmp(a, "--jxg_strategy_out=", 19))
      acs_out = a + 19;
    else if (!std::strncmp(a, "--jxg_qf_out=", 13))
      qf_out = a + 13;
    else if (!std::strncmp(a, "--jxg_trace=", 12))
      trace_path = a + 12;
    else if (!std::strncmp(a, "--jxg_sweep_trace=", 18))
      sweep_trace_path = a + 18;
    else {
      std::fprintf(stderr, "unknown argument: %s\n", a);
      return 1;
    }
  }
  if ((acs_in || qf_in) && sweep_path) {
    std::fprintf(stderr, "--jxg_strategy_in / --jxg_qf_in: not with --sweep\n");
    return 1;
  }
  if ((acs_out || qf_out) && sweep_path) {
    std::fprintf(stderr, "--jxg_strategy_out / --jxg_qf_out: not with --sweep\n");
    return 1;
  }
  if (trace_path && (sweep_path || acs_in)) {
    std::fprintf(stderr, "--jxg_trace: not with %s (a traced encode is one search encode)\n",
                 sweep_path ? "--sweep" : "--jxg_strategy_in");
    return 1;
  }
  if (sweep_trace_path && !sweep_path) {
    std::fprintf(stderr, "--jxg_sweep_trace: only with --sweep (one encode: --jxg_trace)\n");
    return 1;
  }
  if (qf_in && !acs_in) {
    std::fprintf(stderr, "--jxg_qf_in needs --jxg_strategy_in (the forced encode)\n");
    return 1;
  }
  if (acs_out || qf_out) p.flags |= JXG_FLAG_KEEP_MAPS;  // (the codestream is the same)
  // JXG_CJXL_TIMING=1: the phases of this call as one JSON line on stderr
  // (bench.py's single_image probe: where a per-image process spends its time)
  using Clk = std::chrono::steady_clock;
  const auto ms = [](Clk::time_point a, Clk::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
  };
  const bool timing = std::getenv("JXG_CJXL_TIMING") != nullptr;
  const auto t_start = Clk::now();
  const auto unix_ms = [] {
    return std::chrono::duration<double, std::milli>(
               std::chrono::system_clock::now().time_since_epoch())
        .count();
  };
  const double u_start = unix_ms();  // (the caller's clock brackets main with these)
  jxg_ctx* ctx = nullptr;
  jxg_status st = JXG_OK;
  double ms_create = 0.0;
  // JXG_CJXL_DECODE_ONLY=1 (tests, no GPU): write the decoded image as a
  // binary PPM to OUTPUT instead of encoding it
  const bool decode_only = std::getenv("JXG_CJXL_DECODE_ONLY") != nullptr;
  std::vector<SweepLine> sweep_list;
  if (sweep_path && (recon_path || decode_only || !read_sweep_list(sweep_path, sweep_list))) {
    std::fprintf(stderr, "--sweep: %s\n",
                 recon_path || decode_only ? "not with --jxg_recon / decode only"
                                           : "cannot read the list (`distance effort` lines)");
    return 1;
  }
  std::thread maker;
  auto fail = [&](int code) {
    if (maker.joinable()) maker.join();
    if (ctx) jxg_destroy(ctx);
    return code;
  };
  std::vector<uint8_t> file, rgb;
  if (!read_file(argv[1], file)) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 1;
  }
  // the context (HIP runtime initialisation, device buffers for the image's
  // size, every kernel's code object: jxg_create + jxg_warmup) is made on a
  // second thread while this one decodes the image
  uint32_t pw = 0, ph = 0;
  if (!decode_only) {
    probe_dims(file, pw, ph);
    maker = std::thread([&] {
      const auto t = Clk::now();
      st = jxg_create(&p, &ctx);
      if (st == JXG_OK && pw && ph) (void)jxg_warmup(ctx, pw, ph);  // (best effort)
      ms_create = ms(t, Clk::now());
    });
  }
  uint32_t w = 0, h = 0;
  std::string err;
  const bool ok = file.size() >= 2 && file[0] == 'P' && file[1] == '6'
                      ? decode_ppm(file, rgb, w, h, err)
                      : decode_png(file, rgb, w, h, err);
  if (!ok) {
    std::fprintf(stderr, "%s: %s\n", argv[1], err.c_str());
    return fail(1);
  }
  const auto t_read = Clk::now();
  if (decode_only) {
    FILE* f = std::fopen(argv[2], "wb");
    const bool wr = f && std::fprintf(f, "P6\n%u %u\n255\n", w, h) > 0 &&
                    std::fwrite(rgb.data(), 1, rgb.size(), f) == rgb.size();
    if (f) std::fclose(f);
    if (timing) std::fprintf(stderr, "{\"ms_read_decode\": %.3f}\n", ms(t_start, t_read));
    if (!wr) std::fprintf(stderr, "cannot write %s\n", argv[2]);
    return wr ? 0 : 1;
  }
  maker.join();
  const auto t_create = Clk::now();  // (the wait for the context, if any)
  if (st != JXG_OK) {
    std::fprintf(stderr, "jxg_create: %s\n", jxg_status_str(st));
    return 1;
  }
  if (sweep_path) {
    const int rc = run_sweep(ctx, p, argv[1], argv[2], sweep_list, rgb, w, h, report_path,
                             rates_path, ab_path, ab_base, sweep_trace_path);
    std::fflush(nullptr);
    std::_Exit(rc);  // (as below: no exit-time teardown)
  }
  // the forced encode's maps: the frame's geometry, then the validator's verdict
  const uint32_t mbw = (w + 7) / 8, mbh = (h + 7) / 8;
  std::vector<uint8_t> acs_map, qf_map;
  for (int k = 0; k < 2; k++) {
    const char* path = k ? qf_in : acs_in;
    if (!path) continue;
    uint32_t bw = 0, bh = 0;
    std::string perr;
    if (!read_pgm(path, k ? qf_map : acs_map, bw, bh, perr)) {
      std::fprintf(stderr, "%s: %s\n", path, perr.c_str());
      return fail(1);
    }
    if (bw != mbw || bh != mbh) {
      std::fprintf(stderr, "%s: %u x %u blocks, the image has %u x %u\n", path, bw, bh, mbw, mbh);
      return fail(1);
    }
  }
  if (acs_in) {
    uint32_t bad = 0;
    const jxg_status vs = jxg_check_strategy_map(acs_map.data(), w, h, &bad);
    if (vs != JXG_OK) {
      std::fprintf(stderr, "%s: strategy map refused (%s) at block %u (row %u, column %u)\n", acs_in,
                   vs == JXG_ERR_UNSUPPORTED ? "a strategy the forced encode does not take"
                                             : "not the varblocks of one frame",
                   bad, bad / mbw, bad % mbw);
      return fail(1);
    }
  }
  jxg_buffer out{};
  const auto t0 = std::chrono::steady_clock::now();
  st = acs_in ? jxg_encode_forced_rgb8(ctx, rgb.data(), w, h, (size_t)w * 3, acs_map.data(),
                                       qf_in ? qf_map.data() : nullptr, &out)
       : trace_path ? jxg_encode_traced_rgb8(ctx, rgb.data(), w, h, (size_t)w * 3, &out)
                    : jxg_encode_rgb8(ctx, rgb.data(), w, h, (size_t)w * 3, &out);
  const auto t_enc = Clk::now();
  const double sec = std::chrono::duration<double>(t_enc - t0).count();
  if (st != JXG_OK) {
    std::fprintf(stderr, "encode failed: %s\n", jxg_status_str(st));
    jxg_destroy(ctx);
    return 1;
  }
  FILE* f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data, 1, out.size, f) != out.size) {
    std::fprintf(stderr, "cannot write %s\n", argv[2]);
    if (f) std::fclose(f);
    jxg_buffer_free(&out);
    jxg_destroy(ctx);
    return 1;
  }
  std::fclose(f);
  if (acs_out || qf_out) {
    jxg_stats stats{};
    st = jxg_get_stats(ctx, &stats);
    if (st != JXG_OK || !stats.ac_strategy || !stats.quant_field) {
      std::fprintf(stderr, "no maps to write: %s\n", jxg_status_str(st));
      return fail(1);
    }
    if (acs_out && !write_pgm(acs_out, stats.ac_strategy, mbw, mbh)) {
      std::fprintf(stderr, "cannot write %s\n", acs_out);
      return fail(1);
    }
    if (qf_out && !write_pgm(qf_out, stats.quant_field, mbw, mbh)) {
      std::fprintf(stderr, "cannot write %s\n", qf_out);
      return fail(1);
    }
  }
  if (recon_path) {
    std::vector<uint8_t> rec((size_t)w * h * 3);
    st = jxg_reconstruct_rgb8(ctx, rec.data(), (size_t)w * 3);
    if (st != JXG_OK) {
      std::fprintf(stderr, "reconstruct failed: %s\n", jxg_status_str(st));
      return fail(1);
    }
    FILE* r = std::fopen(recon_path, "wb");
    const bool wr = r && std::fprintf(r, "P6\n%u %u\n255\n", w, h) > 0 &&
                    std::fwrite(rec.data(), 1, rec.size(), r) == rec.size();
    if (r) std::fclose(r);
    if (!wr) {
      std::fprintf(stderr, "cannot write %s\n", recon_path);
      return fail(1);
    }
  }
  const RowKey key{std::filesystem::path(argv[1]).filename().string(),
                   std::filesystem::path(argv[2]).filename().string(), p.distance, p.effort};
  if (trace_path) {
    jxg_trace_summary ts{};
    st = jxg_search_trace(ctx, nullptr, &ts);
    if (st != JXG_OK) {
      std::fprintf(stderr, "search trace failed: %s\n", jxg_status_str(st));
      return fail(1);
    }
    if (!write_trace_rows(trace_path, key, ts)) {
      std::fprintf(stderr, "cannot write %s\n", trace_path);
      return fail(1);
    }
  }
  if (report_path) {
    jxg_strategy_report rep{};
    st = jxg_strategy_report_rgb8(ctx, rgb.data(), (size_t)w * 3, &rep, nullptr);
    if (st != JXG_OK) {
      std::fprintf(stderr, "strategy report failed: %s\n", jxg_status_str(st));
      return fail(1);
    }
    if (!write_report_rows(report_path, key, rep, w, h)) {
      std::fprintf(stderr, "cannot write %s\n", report_path);
      return fail(1);
    }
  }
  if (rates_path) {
    struct jxg_rate_report rates{};
    st = jxg_rate_report(ctx, &rates, nullptr);
    if (st != JXG_OK) {
      std::fprintf(stderr, "rate report failed: %s\n", jxg_status_str(st));
      return fail(1);
    }
    if (!write_rate_rows(rates_path, key, rates)) {
      std::fprintf(stderr, "cannot write %s\n", rates_path);
      return fail(1);
    }
  }
  if (ab_path) {
    jxg_params pa = p;
    pa.proposals = ab_base;
    jxg_ctx* base = nullptr;
    jxg_buffer out_a{};
    jxg_ab_report ab{};
    st = jxg_create(&pa, &base);
    if (st == JXG_OK) st = jxg_encode_rgb8(base, rgb.data(), w, h, (size_t)w * 3, &out_a);
    if (st == JXG_OK) st = jxg_ab_report_rgb8(base, ctx, rgb.data(), (size_t)w * 3, &ab, nullptr);
    if (st != JXG_OK) {
      std::fprintf(stderr, "A/B report failed: %s\n", jxg_status_str(st));
      return fail(1);
    }
    if (!write_ab_rows(ab_path, key, ab, w, h)) {
      std::fprintf(stderr, "cannot write %s\n", ab_path);
      return fail(1);
    }
  }
  const auto t_write = Clk::now();
  std::printf("Encoding [VarDCT, d%.3f, effort: %d], %u x %u, %zu bytes, %.3f bpp, %.2f MP/s\n",
              p.distance, p.effort, w, h, out.size, out.size * 8.0 / ((double)w * h),
              (double)w * h / 1e6 / sec);
  // (no jxg_buffer_free / jxg_destroy: the process ends here, and the
  // driver releases its memory and queues as for any exiting process --
  // destroying the context first cost 10 ms of an 8K call, round 6)
  if (timing) {
    const auto t_end = Clk::now();
    std::fprintf(stderr,
                 "{\"ms_read_decode\": %.3f, \"ms_create_wait\": %.3f, \"ms_encode\": %.3f, "
                 "\"ms_write\": %.3f, \"ms_report\": %.3f, \"ms_create_overlapped\": %.3f, "
                 "\"unix_ms_main\": [%.3f, %.3f]}\n",
                 ms(t_start, t_read), ms(t_read, t_create), sec * 1e3,
                 ms(t_enc, t_write), ms(t_write, t_end), ms_create, u_start, unix_ms());
  }
  // The output is written: leave without the HIP runtime's exit-time
  // teardown (bench.py single_image ms_after_main ≈ 100 -> 83 ms of an 8K
  // call, round 6; what remains is the driver's release of the process's
  // queues and memory).
  std::fflush(nullptr);
  std::_Exit(0);
}
