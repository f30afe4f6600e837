// jxg_cli_csv.h -- the CSV text of jxg/harness.py, written by jxg_cjxl: the
// rows of one encode's strategy report, rate report, A/B report and search-trace
// summary.  Needs the structures of include/jxg.h, no library symbol;
// tests/native/cli_csv.cpp compares the files byte for byte with harness.py's.
#pragma once
#include <charconv>
#include <cstdint>
#include <cstdio>
#include <filesystem>
#include <string>

#include "../../include/jxg.h"

namespace jxg_cli {

// Rust's `{}` of an f64 (the harness's file names): the shortest digits that
// round-trip, never an exponent, "1" for 1.0
inline std::string rust_f64(double v) {
  char buf[400];
  const auto r = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::fixed);
  return std::string(buf, r.ptr);
}

inline std::string rust_f32(float v) {
  char buf[200];
  const auto r = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::fixed);
  return std::string(buf, r.ptr);
}

inline const char* const kStrategyNames[JXG_NUM_STRATEGIES] = {
    "DCT8", "IDENTITY", "DCT2X2", "DCT4X4", "DCT16X16", "DCT32X32", "DCT16X8", "DCT8X16",
    "DCT32X8", "DCT8X32", "DCT32X16", "DCT16X32", "DCT4X8", "DCT8X4", "AFV0", "AFV1", "AFV2",
    "AFV3", "DCT64X64", "DCT64X32", "DCT32X64", "DCT128X128", "DCT128X64", "DCT64X128",
    "DCT256X256", "DCT256X128", "DCT128X256"};

inline std::string csv_field(const std::string& v) {  // (Python's csv module, minimal quoting)
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
inline FILE* open_csv(const char* path, const char* header) {
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

// --jxg_report=FILE.csv: the rows of jxg/harness.py strategy_stats /
// write_strategy_stats for one encode -- one per non-empty strategy of the
// report
inline bool write_report_rows(const char* path, const RowKey& key, const jxg_strategy_report& rep,
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
inline bool write_rate_rows(const char* path, const RowKey& key, const struct jxg_rate_report& rep) {
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

// --jxg_ab=FILE.csv: the rows of jxg/harness.py ab_stats / write_ab_stats for
// one pair of encodes -- one per non-empty cell of the A/B report
inline bool write_ab_rows(const char* path, const RowKey& key, const jxg_ab_report& rep, uint32_t w,
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

// --jxg_trace=FILE.csv: the summary of the encode's search trace
// (jxg_search_trace), one row per scan index s: the blocks the 8x8 scan gave to
// s, of them by the winner of the scan without hook F (flip[r][s]), the hook-P
// overrides with target s, the blocks merged over, the margin histogram
inline bool write_trace_rows(const char* path, const RowKey& key, const jxg_trace_summary& t) {
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

}  // namespace jxg_cli
