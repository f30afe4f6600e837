// cli_csv -- jxg_cjxl's four CSV writers (csrc/jxg_cli_csv.h) on generated
// reports; tests/test_cli_csv.py fills jxg/__init__.py's structures with the
// same generator, writes them through jxg/harness.py and compares the files.
//
//   cli_csv OUTDIR   appends to OUTDIR/{report,rates,ab,trace}.csv
//
// One generator for all four, in this order: s = s * 6364136223846793005 +
// 1442695040888963407 (mod 2^64), value s >> 33, seed 12345, one step per
// word written (zeroed words included).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../jpeg-xl-lossy-image-compression-thesis_amd/csrc/jxg_cli_csv.h"

static uint64_t g_state = 12345;
static uint64_t next() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return g_state >> 33;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: cli_csv OUTDIR\n");
    return 2;
  }
  using namespace jxg_cli;
  const std::string dir = std::string(argv[1]) + "/";
  const RowKey key{"a,b \"q\".png", "a-0.5-7.jxl", 0.5f, 7};
  const uint32_t w = 1000, h = 777;

  // strategy report: every u64 word % 1000003, then blocks = 0 in every fourth row
  static jxg_strategy_report rep;
  uint64_t words[sizeof(rep) / 8];
  for (uint64_t& v : words) v = next() % 1000003;
  std::memcpy(&rep, words, sizeof(rep));
  for (int i = 0; i < JXG_NUM_STRATEGIES; i += 4) rep.row[i].blocks = 0;

  // rate report: the rows' u64 words % 100000007, every fifth word 0, then
  // ac_bits and stream_bits
  static struct jxg_rate_report rates;
  uint64_t rwords[sizeof(rates.row) / 8];
  for (size_t i = 0; i < sizeof(rwords) / 8; i++) {
    const uint64_t v = next() % 100000007;
    rwords[i] = i % 5 == 0 ? 0 : v;
  }
  std::memcpy(rates.row, rwords, sizeof(rates.row));
  rates.ac_bits = next() % 100000007;
  rates.stream_bits = next() % 100000007;

  // A/B report: six u64 words a cell; every seventh cell % 10000019, the rest 0
  static jxg_ab_report ab;
  static uint64_t awords[sizeof(ab) / 8];
  for (size_t i = 0; i < sizeof(awords) / 8; i++) {
    const uint64_t v = next() % 10000019;
    awords[i] = (i / 6) % 7 == 0 ? v : 0;
  }
  std::memcpy(&ab, awords, sizeof(ab));

  // trace summary: every u32 word % 4099
  jxg_trace_summary tr;
  uint32_t twords[sizeof(tr) / 4];
  for (uint32_t& v : twords) v = (uint32_t)(next() % 4099);
  std::memcpy(&tr, twords, sizeof(tr));

  const bool ok = write_report_rows((dir + "report.csv").c_str(), key, rep, w, h) &&
                  write_rate_rows((dir + "rates.csv").c_str(), key, rates) &&
                  write_ab_rows((dir + "ab.csv").c_str(), key, ab, w, h) &&
                  write_trace_rows((dir + "trace.csv").c_str(), key, tr);
  return ok ? 0 : 1;
}
