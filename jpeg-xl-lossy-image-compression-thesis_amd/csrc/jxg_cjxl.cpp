// jxg_cjxl -- cjxl-argv-compatible command line over the C ABI.
//
// The reference harness runs `cjxl IN OUT --distance=D --effort=E`
// (benchmark-jpegxl/src/docker_manager.rs:126-136) and maps a non-zero exit
// status to "skip" (benchmark.rs:654-677).  This tool accepts the same argv
// shape, reads 8-bit PNG (gray / gray+alpha / RGB / RGBA, non-interlaced; alpha
// dropped) or binary PPM (csrc/jxg_cli_io.h), encodes on the GPU and writes the
// codestream.  Exit 0 on success; one message on stderr and exit 1 otherwise.
// Three modes:
//
//   jxg_cjxl INPUT OUTPUT [options]               one image (run_single)
//   jxg_cjxl INPUT OUTDIR --sweep=LIST [options]  INPUT at every `distance
//       effort` line of LIST in one process and one jxg_sweep_rgb8 call, written
//       as OUTDIR/<stem>-<distance>-<effort>.jxl, the harness's names
//       (benchmark.rs:644-650): its per-image loop without a process start per
//       setting (run_sweep)
//   JXG_CJXL_DECODE_ONLY=1 jxg_cjxl INPUT OUTPUT  tests, no GPU: the decoded
//       image as a binary PPM (run_decode_only)
//
// Every option is one row of kOptions below (the usage text is printed from
// it), every combination that is refused one row of kConflicts, and every CSV
// report one row of kReportKinds (the text itself: csrc/jxg_cli_csv.h).
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/jxg.h"
#include "jxg_cli_csv.h"
#include "jxg_cli_io.h"

namespace {

using namespace jxg_cli;

struct Options {
  // `cjxl IN OUT --distance=D --effort=E` with no other flag (the harness's
  // argv, docker_manager.rs:126-136) gets cjxl's VarDCT defaults [ext]: ANS,
  // Gaborish on, EPF iterations by distance, the masking quant field
  jxg_params p{1.0f, 7, 0, 1, JXG_FLAGS_CJXL_DEFAULTS, 0};
  uint32_t ab_base = 0;
  const char *sweep = nullptr, *recon = nullptr, *report = nullptr, *rates = nullptr,
             *ab = nullptr, *acs_in = nullptr, *qf_in = nullptr, *acs_out = nullptr,
             *qf_out = nullptr, *trace = nullptr, *sweep_trace = nullptr;
  bool decode_only = false;  // JXG_CJXL_DECODE_ONLY
};

uint32_t proposal_bits(const char* v) {
  return (std::strchr(v, 'P') ? JXG_PROPOSAL_P : 0u) | (std::strchr(v, 'F') ? JXG_PROPOSAL_F : 0u);
}

// an option over one of cjxl's default flags: `on` keeps it, `off` clears it
bool flag_choice(Options& o, const char* v, const char* on, const char* off, uint32_t flag,
                 const char* complaint) {
  if (!std::strcmp(v, off))
    o.p.flags &= ~flag;
  else if (std::strcmp(v, on)) {
    std::fprintf(stderr, "%s: %s\n", complaint, v);
    return false;
  }
  return true;
}

struct Option {
  const char *name, *alias;  // with their '='; what follows is the value
  const char *value, *help;
  bool (*set)(Options&, const char*);  // false: refused, the message is printed
};
#define JXG_PATH_OPTION(field) [](Options& o, const char* v) { return o.field = v, true; }
const Option kOptions[] = {
    {"--distance=", "-d=", "D", "Butteraugli distance target, 1 by default (cjxl's)",
     [](Options& o, const char* v) { return o.p.distance = (float)std::atof(v), true; }},
    {"--effort=", "-e=", "E", "effort, 7 by default (cjxl's)",
     [](Options& o, const char* v) { return o.p.effort = std::atoi(v), true; }},
    {"--proposals=", nullptr, "none|P|F|PF", "the thesis's proposals P and F (default none)",
     [](Options& o, const char* v) { return o.p.proposals = proposal_bits(v), true; }},
    {"--coder=", nullptr, "ans|prefix", "entropy coder (default ans, cjxl's)",
     [](Options& o, const char* v) {
       return flag_choice(o, v, "ans", "prefix", JXG_FLAG_ANS, "unknown coder");
     }},
    {"--gaborish=", nullptr, "1|0", "cjxl --gaborish (default 1)",
     [](Options& o, const char* v) {
       return flag_choice(o, v, "1", "0", JXG_FLAG_GABORISH, "unsupported --gaborish");
     }},
    {"--epf=", nullptr, "-1|0", "cjxl --epf: -1 = iterations by distance (default), 0 = off",
     [](Options& o, const char* v) {
       return flag_choice(o, v, "-1", "0", JXG_FLAG_EPF, "unsupported --epf (-1 or 0)");
     }},
    {"--aq=", nullptr, "masking|activity", "the quant field heuristic (default masking, cjxl's)",
     [](Options& o, const char* v) {
       return flag_choice(o, v, "masking", "activity", JXG_FLAG_AQ_MASKING,
                          "unsupported --aq (masking or activity)");
     }},
    {"--device=", nullptr, "N", "HIP device index",
     [](Options& o, const char* v) { return o.p.device = std::atoi(v), true; }},
    {"--sweep=", nullptr, "LIST",
     "OUTPUT is a directory: INPUT at every `distance effort` line of the file LIST, the other "
     "options at every point",
     JXG_PATH_OPTION(sweep)},
    // the rest are not cjxl options
    {"--jxg_recon=", nullptr, "PATH",
     "also write the codestream's decoded image, reconstructed on the GPU "
     "(jxg_reconstruct_rgb8), as a binary PPM; not with --sweep",
     JXG_PATH_OPTION(recon)},
    {"--jxg_report=", nullptr, "FILE.csv",
     "append the per-strategy statistics of the encode, or of every point of --sweep "
     "(jxg_strategy_report_rgb8), as jxg/harness.py's CSV",
     JXG_PATH_OPTION(report)},
    {"--jxg_rates=", nullptr, "FILE.csv",
     "append the coded bits per strategy of the encode, or of every point (jxg_rate_report)",
     JXG_PATH_OPTION(rates)},
    {"--jxg_ab=", nullptr, "FILE.csv",
     "also run the encode, or every point, with the base proposals and append the A/B report of "
     "the two (jxg_ab_report_rgb8; side B is --proposals); the codestreams written are unchanged",
     JXG_PATH_OPTION(ab)},
    {"--jxg_ab_base=", nullptr, "none|P|F|PF", "the base proposals of --jxg_ab (default none)",
     [](Options& o, const char* v) { return o.ab_base = proposal_bits(v), true; }},
    {"--jxg_strategy_in=", nullptr, "MAP.pgm",
     "encode with the file's AC-strategy map instead of the search (jxg_encode_forced_rgb8): "
     "binary PGM of xsize_blocks x ysize_blocks, one byte per block; a map of the wrong geometry "
     "or one the validator refuses: the reason and the block, exit 1; not with --sweep",
     JXG_PATH_OPTION(acs_in)},
    {"--jxg_qf_in=", nullptr, "MAP.pgm", "the forced encode's quant field, the same geometry",
     JXG_PATH_OPTION(qf_in)},
    {"--jxg_strategy_out=", nullptr, "MAP.pgm",
     "write the AC-strategy map of whatever was encoded; not with --sweep",
     JXG_PATH_OPTION(acs_out)},
    {"--jxg_qf_out=", nullptr, "MAP.pgm", "write its quant field; not with --sweep",
     JXG_PATH_OPTION(qf_out)},
    {"--jxg_trace=", nullptr, "FILE.csv",
     "make the encode a traced one (jxg_encode_traced_rgb8: the same codestream) and append the "
     "summary of its search trace, one row per scan index; not with --sweep or --jxg_strategy_in",
     JXG_PATH_OPTION(trace)},
    {"--jxg_sweep_trace=", nullptr, "FILE.csv",
     "only with --sweep: the same rows for every point of effort >= 5, traced on its lane "
     "(jxg_set_sweep_trace: the same codestreams); a point without a search writes no rows and "
     "one line on stderr",
     JXG_PATH_OPTION(sweep_trace)},
};
#undef JXG_PATH_OPTION

int usage(const char* argv0) {
  std::fprintf(stderr,
               "usage: %s INPUT OUTPUT [options]\n"
               "       %s INPUT OUTDIR --sweep=LIST [options]\n"
               "INPUT: 8-bit PNG or binary PPM.  Options:\n",
               argv0, argv0);
  for (const Option& op : kOptions) {
    std::string head = std::string(op.name) + op.value;
    if (op.alias) head += std::string(", ") + op.alias + op.value;
    std::fprintf(stderr, "  %s\n      %s\n", head.c_str(), op.help);
  }
  return 1;
}

bool parse_options(int argc, char** argv, Options& o) {
  for (int i = 3; i < argc; i++) {
    const char* a = argv[i];
    const Option* hit = nullptr;
    const char* value = nullptr;
    for (const Option& op : kOptions)
      for (const char* name : {op.name, op.alias})
        if (!hit && name && !std::strncmp(a, name, std::strlen(name))) {
          hit = &op;
          value = a + std::strlen(name);
        }
    if (!hit) {
      std::fprintf(stderr, "unknown argument: %s\n", a);
      return false;
    }
    if (!hit->set(o, value)) return false;
  }
  o.decode_only = std::getenv("JXG_CJXL_DECODE_ONLY") != nullptr;
  return true;
}

// the combinations that are refused, in the order they are looked at
struct Conflict {
  bool (*when)(const Options&);
  const char* message;
};
const Conflict kConflicts[] = {
    {[](const Options& o) { return (o.acs_in || o.qf_in) && o.sweep; },
     "--jxg_strategy_in / --jxg_qf_in: not with --sweep"},
    {[](const Options& o) { return (o.acs_out || o.qf_out) && o.sweep; },
     "--jxg_strategy_out / --jxg_qf_out: not with --sweep"},
    {[](const Options& o) { return o.trace && o.sweep; },
     "--jxg_trace: not with --sweep (a traced encode is one search encode)"},
    {[](const Options& o) { return o.trace && o.acs_in; },
     "--jxg_trace: not with --jxg_strategy_in (a traced encode is one search encode)"},
    {[](const Options& o) { return o.sweep_trace && !o.sweep; },
     "--jxg_sweep_trace: only with --sweep (one encode: --jxg_trace)"},
    {[](const Options& o) { return o.qf_in && !o.acs_in; },
     "--jxg_qf_in needs --jxg_strategy_in (the forced encode)"},
    {[](const Options& o) { return o.sweep && (o.recon || o.decode_only); },
     "--sweep: not with --jxg_recon / decode only"},
};

using Clk = std::chrono::steady_clock;
double ms(Clk::time_point a, Clk::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}
double unix_ms() {
  return std::chrono::duration<double, std::milli>(
             std::chrono::system_clock::now().time_since_epoch())
      .count();
}
// JXG_CJXL_TIMING=1: the phases of this call as one JSON line on stderr
// (bench.py's single_image probe: where a per-image process spends its time)
struct Timing {
  bool on = std::getenv("JXG_CJXL_TIMING") != nullptr;
  Clk::time_point start = Clk::now(), read, create;
  double unix_start = unix_ms();  // (the caller's clock brackets main with these)
};

struct Image {
  // (the file's bytes stay until the process ends: giving an 8K PNG's 25 MB back
  // before the encode costs 2 ms of page releases)
  std::vector<uint8_t> file, rgb;
  uint32_t w = 0, h = 0;
  size_t stride() const { return (size_t)w * 3; }
};

// What a failing path would have to give back, so every one of them is a plain
// `return 1`: the maker thread (joined), the output buffers, the A/B base
// context and the context.  A maker still running when this is destroyed means
// the input was refused: it is told to skip the warm-up before it is joined, so
// the message does not wait for a synthetic encode of the header's size.
struct Guard {
  std::atomic<bool> abandoned{false};
  jxg_status created = JXG_OK;
  double ms_create = 0.0;
  jxg_ctx *ctx = nullptr, *base = nullptr;
  std::vector<jxg_buffer> outs;
  std::thread maker;

  // the context (HIP runtime initialisation, device buffers for the image's
  // size, every kernel's code object: jxg_create + jxg_warmup) is made on a
  // second thread while the first one decodes the image
  void start(const jxg_params& p, uint32_t pw, uint32_t ph) {
    maker = std::thread([this, &p, pw, ph] {
      const auto t = Clk::now();
      created = jxg_create(&p, &ctx);
      if (created == JXG_OK && pw && ph && !abandoned.load())
        (void)jxg_warmup(ctx, pw, ph);  // (best effort)
      ms_create = ms(t, Clk::now());
    });
  }
  ~Guard() {
    abandoned.store(true);
    if (maker.joinable()) maker.join();
    for (jxg_buffer& b : outs) jxg_buffer_free(&b);
    if (base) jxg_destroy(base);
    if (ctx) jxg_destroy(ctx);
  }
};

// ---- the CSV reports, one row per kind, for both modes --------------------

struct Reports {  // of the one encode, or of every point of the sweep
  std::vector<jxg_trace_summary> trace;
  std::vector<jxg_strategy_report> report;
  std::vector<struct jxg_rate_report> rates;
  std::vector<jxg_ab_report> ab;
};
struct Job {
  const Options& o;
  Guard& g;
  const Image& im;
  std::vector<int32_t> base;  // sweep with --jxg_ab: the point each point is compared with
};
struct ReportKind {
  const char *Options::*path, *Options::*sweep_path;  // the option that names the file
  const char *what, *sweep_what;                      // in messages
  jxg_status (*fetch)(Job&, Reports&);                // one image: after the encode
  jxg_status (*sweep_on)(Job&, uint32_t n);           // sweep: the switch before the call,
  jxg_status (*sweep_get)(Job&, Reports&, uint32_t n);  // every point's report after it
  bool (*write)(const char* path, const RowKey&, const Reports&, size_t i, const Image&);
};
// (the trace comes first: jxg_search_trace is valid only while the traced
// encode is the last use of the context's buffers)
const ReportKind kReportKinds[] = {
    {&Options::trace, &Options::sweep_trace, "search trace", "traces",
     [](Job& j, Reports& r) {
       r.trace.resize(1);
       return jxg_search_trace(j.g.ctx, nullptr, r.trace.data());
     },
     [](Job& j, uint32_t) { return jxg_set_sweep_trace(j.g.ctx, 1); },
     [](Job& j, Reports& r, uint32_t n) {
       r.trace.resize(n);
       return jxg_sweep_trace(j.g.ctx, r.trace.data(), n);
     },
     [](const char* path, const RowKey& k, const Reports& r, size_t i, const Image&) {
       // (a sweep's point without a search, effort < 5, has the zero summary)
       if (r.trace[i].blocks) return write_trace_rows(path, k, r.trace[i]);
       std::fprintf(stderr, "distance %s effort %d: no search to trace, no rows\n",
                    rust_f64(k.distance).c_str(), k.effort);
       return true;
     }},
    {&Options::report, &Options::report, "strategy report", "report",
     [](Job& j, Reports& r) {
       r.report.resize(1);
       return jxg_strategy_report_rgb8(j.g.ctx, j.im.rgb.data(), j.im.stride(), r.report.data(),
                                       nullptr);
     },
     [](Job& j, uint32_t) { return jxg_set_sweep_report(j.g.ctx, 1); },
     [](Job& j, Reports& r, uint32_t n) {
       r.report.resize(n);
       return jxg_sweep_report(j.g.ctx, r.report.data(), n);
     },
     [](const char* path, const RowKey& k, const Reports& r, size_t i, const Image& im) {
       return write_report_rows(path, k, r.report[i], im.w, im.h);
     }},
    // (the rate reports need no chain: they follow each point's emission)
    {&Options::rates, &Options::rates, "rate report", "rates",
     [](Job& j, Reports& r) {
       r.rates.resize(1);
       return jxg_rate_report(j.g.ctx, r.rates.data(), nullptr);
     },
     [](Job& j, uint32_t) { return jxg_set_sweep_rates(j.g.ctx, 1); },
     [](Job& j, Reports& r, uint32_t n) {
       r.rates.resize(n);
       return jxg_sweep_rates(j.g.ctx, r.rates.data(), n);
     },
     [](const char* path, const RowKey& k, const Reports& r, size_t i, const Image&) {
       return write_rate_rows(path, k, r.rates[i]);
     }},
    {&Options::ab, &Options::ab, "A/B report", "A/B reports",
     [](Job& j, Reports& r) {  // side A: the same encode with the base proposals
       jxg_params pa = j.o.p;
       pa.proposals = j.o.ab_base;
       r.ab.resize(1);
       j.g.outs.push_back(jxg_buffer{nullptr, 0});
       jxg_status st = jxg_create(&pa, &j.g.base);
       if (st == JXG_OK)
         st = jxg_encode_rgb8(j.g.base, j.im.rgb.data(), j.im.w, j.im.h, j.im.stride(),
                              &j.g.outs.back());
       if (st == JXG_OK)
         st = jxg_ab_report_rgb8(j.g.base, j.g.ctx, j.im.rgb.data(), j.im.stride(), r.ab.data(),
                                 nullptr);
       return st;
     },
     [](Job& j, uint32_t n) { return jxg_set_sweep_ab(j.g.ctx, j.base.data(), n); },
     [](Job& j, Reports& r, uint32_t n) {
       r.ab.resize(n);
       return jxg_sweep_ab(j.g.ctx, r.ab.data(), n);
     },
     [](const char* path, const RowKey& k, const Reports& r, size_t i, const Image& im) {
       return write_ab_rows(path, k, r.ab[i], im.w, im.h);
     }},
};

// ---- --sweep -------------------------------------------------------------------

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

// the points' streams and rows: OUTDIR/<stem>-<distance>-<effort>.jxl each; 1 if
// any point was refused or any file not written
int write_sweep(Job& job, const Reports& reps, const char* input, const char* outdir,
                const std::vector<SweepLine>& list, const std::vector<jxg_sweep_point>& pts,
                const std::vector<jxg_status>& sts) {
  const Image& im = job.im;
  const std::vector<jxg_buffer>& outs = job.g.outs;
  const size_t o = pts.size() - list.size();
  std::error_code ec;
  std::filesystem::create_directories(outdir, ec);
  const std::string orig_name = std::filesystem::path(input).filename().string();
  const std::string stem = std::filesystem::path(input).stem().string();
  int rc = 0;
  for (size_t i = o; i < pts.size(); i++) {
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
    for (const ReportKind& k : kReportKinds)
      if (job.o.*k.sweep_path && !k.write(job.o.*k.sweep_path, key, reps, i, im)) {
        std::fprintf(stderr, "cannot write %s\n", job.o.*k.sweep_path);
        rc = 1;
      }
    if (!write_file(path.c_str(), outs[i].data, outs[i].size)) {
      std::fprintf(stderr, "cannot write %s\n", path.c_str());
      rc = 1;
    }
    std::printf("Encoding [VarDCT, d%.3f, effort: %d], %u x %u, %zu bytes, %.3f bpp\n",
                pts[i].distance, pts[i].effort, im.w, im.h, outs[i].size,
                outs[i].size * 8.0 / ((double)im.w * im.h));
  }
  return rc;
}

// INPUT at every point of the list -> OUTDIR/<stem>-<distance>-<effort>.jxl
int run_sweep(const Options& opt, Guard& g, const Image& im, const char* input, const char* outdir,
              const std::vector<SweepLine>& list) {
  // with --jxg_ab the list's points with the base proposals go in front: point
  // m + i is the command line's own and is compared with point i
  const size_t m = list.size(), o = opt.ab ? m : 0, n = m + o;
  const jxg_params& p = opt.p;
  std::vector<jxg_sweep_point> pts(n);
  Job job{opt, g, im, std::vector<int32_t>(n, -1)};
  for (size_t i = 0; i < m; i++) {
    pts[o + i] = jxg_sweep_point{(float)list[i].distance, list[i].effort, p.proposals, p.flags};
    if (opt.ab) {
      pts[i] = jxg_sweep_point{(float)list[i].distance, list[i].effort, opt.ab_base, p.flags};
      job.base[o + i] = (int32_t)i;
    }
  }
  // with a report the points' chains run (quality 1) and end in the reduction
  const bool chain = opt.report || opt.ab;
  g.outs.assign(n, jxg_buffer{nullptr, 0});
  std::vector<jxg_status> sts(n, JXG_OK);
  std::vector<jxg_quality> qs(chain ? n : 0);
  for (const ReportKind& k : kReportKinds)
    if (opt.*k.sweep_path && k.sweep_on(job, (uint32_t)n) != JXG_OK) return 1;
  const auto t0 = Clk::now();
  const jxg_status st =
      jxg_sweep_rgb8(g.ctx, im.rgb.data(), im.w, im.h, im.stride(), pts.data(), (uint32_t)n,
                     chain ? 1 : 0, g.outs.data(), chain ? qs.data() : nullptr, sts.data());
  const double sec = std::chrono::duration<double>(Clk::now() - t0).count();
  bool any = false;
  for (size_t i = o; i < n; i++) any = any || g.outs[i].data;
  if (st != JXG_OK && !any) {
    std::fprintf(stderr, "sweep failed: %s\n", jxg_status_str(st));
    return 1;
  }
  Reports reps;
  for (const ReportKind& k : kReportKinds)
    if (opt.*k.sweep_path && k.sweep_get(job, reps, (uint32_t)n) != JXG_OK) {
      std::fprintf(stderr, "sweep %s failed\n", k.sweep_what);
      return 1;
    }
  const int rc = write_sweep(job, reps, input, outdir, list, pts, sts);
  std::printf("Sweep of %zu points, %u x %u, %.2f MP/s\n", n, im.w, im.h,
              (double)n * im.w * im.h / 1e6 / sec);
  std::fflush(nullptr);
  std::_Exit(rc);  // (as at the end of run_single: no exit-time teardown)
}

// ---- one image -------------------------------------------------------------------

// the forced encode's maps: the frame's geometry, then the validator's verdict
bool read_forced_maps(const Options& o, const Image& im, std::vector<uint8_t>& acs_map,
                      std::vector<uint8_t>& qf_map) {
  const uint32_t mbw = (im.w + 7) / 8, mbh = (im.h + 7) / 8;
  for (int k = 0; k < 2; k++) {
    const char* path = k ? o.qf_in : o.acs_in;
    if (!path) continue;
    uint32_t bw = 0, bh = 0;
    std::string perr = "cannot read the file";
    std::vector<uint8_t> file;
    if (!read_file(path, file) || !read_pgm(file, k ? qf_map : acs_map, bw, bh, perr)) {
      std::fprintf(stderr, "%s: %s\n", path, perr.c_str());
      return false;
    }
    if (bw != mbw || bh != mbh) {
      std::fprintf(stderr, "%s: %u x %u blocks, the image has %u x %u\n", path, bw, bh, mbw, mbh);
      return false;
    }
  }
  if (!o.acs_in) return true;
  uint32_t bad = 0;
  const jxg_status vs = jxg_check_strategy_map(acs_map.data(), im.w, im.h, &bad);
  if (vs != JXG_OK)
    std::fprintf(stderr, "%s: strategy map refused (%s) at block %u (row %u, column %u)\n",
                 o.acs_in,
                 vs == JXG_ERR_UNSUPPORTED ? "a strategy the forced encode does not take"
                                           : "not the varblocks of one frame",
                 bad, bad / mbw, bad % mbw);
  return vs == JXG_OK;
}

// --jxg_strategy_out / --jxg_qf_out and --jxg_recon: what else the encode left
bool write_maps_and_recon(const Options& o, Guard& g, const Image& im) {
  if (o.acs_out || o.qf_out) {
    const uint32_t mbw = (im.w + 7) / 8, mbh = (im.h + 7) / 8;
    jxg_stats stats{};
    const jxg_status st = jxg_get_stats(g.ctx, &stats);
    if (st != JXG_OK || !stats.ac_strategy || !stats.quant_field) {
      std::fprintf(stderr, "no maps to write: %s\n", jxg_status_str(st));
      return false;
    }
    if (o.acs_out && !write_pgm(o.acs_out, stats.ac_strategy, mbw, mbh)) {
      std::fprintf(stderr, "cannot write %s\n", o.acs_out);
      return false;
    }
    if (o.qf_out && !write_pgm(o.qf_out, stats.quant_field, mbw, mbh)) {
      std::fprintf(stderr, "cannot write %s\n", o.qf_out);
      return false;
    }
  }
  if (o.recon) {
    std::vector<uint8_t> rec(im.rgb.size());
    const jxg_status st = jxg_reconstruct_rgb8(g.ctx, rec.data(), im.stride());
    if (st != JXG_OK) {
      std::fprintf(stderr, "reconstruct failed: %s\n", jxg_status_str(st));
      return false;
    }
    if (!write_ppm(o.recon, rec.data(), im.w, im.h)) {
      std::fprintf(stderr, "cannot write %s\n", o.recon);
      return false;
    }
  }
  return true;
}

int run_single(const Options& o, Guard& g, const Image& im, const char* input, const char* output,
               const Timing& tm) {
  std::vector<uint8_t> acs_map, qf_map;
  if (!read_forced_maps(o, im, acs_map, qf_map)) return 1;
  g.outs.assign(1, jxg_buffer{nullptr, 0});
  const auto t0 = Clk::now();
  const jxg_status st =
      o.acs_in  ? jxg_encode_forced_rgb8(g.ctx, im.rgb.data(), im.w, im.h, im.stride(),
                                         acs_map.data(), o.qf_in ? qf_map.data() : nullptr,
                                         &g.outs[0])
      : o.trace ? jxg_encode_traced_rgb8(g.ctx, im.rgb.data(), im.w, im.h, im.stride(), &g.outs[0])
                : jxg_encode_rgb8(g.ctx, im.rgb.data(), im.w, im.h, im.stride(), &g.outs[0]);
  const auto t_enc = Clk::now();
  const double sec = std::chrono::duration<double>(t_enc - t0).count();
  if (st != JXG_OK) {
    std::fprintf(stderr, "encode failed: %s\n", jxg_status_str(st));
    return 1;
  }
  const size_t bytes = g.outs[0].size;
  if (!write_file(output, g.outs[0].data, bytes)) {
    std::fprintf(stderr, "cannot write %s\n", output);
    return 1;
  }
  if (!write_maps_and_recon(o, g, im)) return 1;
  const RowKey key{std::filesystem::path(input).filename().string(),
                   std::filesystem::path(output).filename().string(), o.p.distance, o.p.effort};
  Job job{o, g, im, {}};
  Reports reps;
  for (const ReportKind& k : kReportKinds) {
    const char* path = o.*k.path;
    if (!path) continue;
    const jxg_status rs = k.fetch(job, reps);
    if (rs != JXG_OK) {
      std::fprintf(stderr, "%s failed: %s\n", k.what, jxg_status_str(rs));
      return 1;
    }
    if (!k.write(path, key, reps, 0, im)) {
      std::fprintf(stderr, "cannot write %s\n", path);
      return 1;
    }
  }
  const auto t_write = Clk::now();
  std::printf("Encoding [VarDCT, d%.3f, effort: %d], %u x %u, %zu bytes, %.3f bpp, %.2f MP/s\n",
              o.p.distance, o.p.effort, im.w, im.h, bytes, bytes * 8.0 / ((double)im.w * im.h),
              (double)im.w * im.h / 1e6 / sec);
  // (no jxg_buffer_free / jxg_destroy: the process ends here, and the
  // driver releases its memory and queues as for any exiting process --
  // destroying the context first cost 10 ms of an 8K call, round 6)
  if (tm.on) {
    const auto t_end = Clk::now();
    std::fprintf(stderr,
                 "{\"ms_read_decode\": %.3f, \"ms_create_wait\": %.3f, \"ms_encode\": %.3f, "
                 "\"ms_write\": %.3f, \"ms_report\": %.3f, \"ms_create_overlapped\": %.3f, "
                 "\"unix_ms_main\": [%.3f, %.3f]}\n",
                 ms(tm.start, tm.read), ms(tm.read, tm.create), sec * 1e3, ms(t_enc, t_write),
                 ms(t_write, t_end), g.ms_create, tm.unix_start, unix_ms());
  }
  // The output is written: leave without the HIP runtime's exit-time
  // teardown (bench.py single_image ms_after_main ≈ 100 -> 83 ms of an 8K
  // call, round 6; what remains is the driver's release of the process's
  // queues and memory).
  std::fflush(nullptr);
  std::_Exit(0);
}

// JXG_CJXL_DECODE_ONLY=1 (tests, no GPU): the decoded image as a binary PPM
int run_decode_only(const Image& im, const char* output, const Timing& tm) {
  const bool wr = write_ppm(output, im.rgb.data(), im.w, im.h);
  if (tm.on) std::fprintf(stderr, "{\"ms_read_decode\": %.3f}\n", ms(tm.start, tm.read));
  if (!wr) std::fprintf(stderr, "cannot write %s\n", output);
  return wr ? 0 : 1;
}

// INPUT read and decoded, while the guard's second thread makes the context
// for the size its header names
bool load_image(const Options& o, const char* input, Guard& g, Image& im) {
  const std::vector<uint8_t>& file = im.file;
  if (!read_file(input, im.file)) {
    std::fprintf(stderr, "cannot read %s\n", input);
    return false;
  }
  if (!o.decode_only) {
    uint32_t pw = 0, ph = 0;
    probe_dims(file, pw, ph);
    g.start(o.p, pw, ph);
  }
  std::string err;
  const bool ok = is_ppm(file) ? read_ppm(file, im.rgb, im.w, im.h, err)
                               : decode_png(file, im.rgb, im.w, im.h, err);
  if (!ok) std::fprintf(stderr, "%s: %s\n", input, err.c_str());
  return ok;
}

}  // namespace

// parse, check, load the image, dispatch.  A failure is `return 1` and unwinds
// through the Guard; the two successful encodes end in _Exit.
int main(int argc, char** argv) {
  if (argc < 3) return usage(argv[0]);
  try {
    Options o;
    if (!parse_options(argc, argv, o)) return 1;
    for (const Conflict& c : kConflicts)
      if (c.when(o)) {
        std::fprintf(stderr, "%s\n", c.message);
        return 1;
      }
    if (o.acs_out || o.qf_out) o.p.flags |= JXG_FLAG_KEEP_MAPS;  // (the codestream is the same)
    Timing tm;
    std::vector<SweepLine> sweep_list;
    if (o.sweep && !read_sweep_list(o.sweep, sweep_list)) {
      std::fprintf(stderr, "--sweep: cannot read the list (`distance effort` lines)\n");
      return 1;
    }
    Guard g;
    Image im;
    if (!load_image(o, argv[1], g, im)) return 1;
    tm.read = Clk::now();
    if (o.decode_only) return run_decode_only(im, argv[2], tm);
    g.maker.join();
    tm.create = Clk::now();  // (the wait for the context, if any)
    if (g.created != JXG_OK) {
      std::fprintf(stderr, "jxg_create: %s\n", jxg_status_str(g.created));
      return 1;
    }
    return o.sweep ? run_sweep(o, g, im, argv[1], argv[2], sweep_list)
                   : run_single(o, g, im, argv[1], argv[2], tm);
  } catch (const std::bad_alloc&) {
    std::fprintf(stderr, "out of memory\n");
    return 1;
  }
}
