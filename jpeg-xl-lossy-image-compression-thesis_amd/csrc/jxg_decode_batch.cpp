// jxg_decode_batch.cpp -- jxg_decode_batch_rgb8[_device]: many codestreams in
// one call (DESIGN.md §3.12 "Batch decode").  A frame's pass-group kernel lasts
// as long as its longest pass group and occupies a fraction of the GPU, so the
// batch puts the pass groups of many frames into one launch: every frame is
// parsed on the host (jxg_decode.cpp, frames and their LF groups over at most 8
// threads), the planner (jxg_decode_plan.cpp) cuts the frames into chunks by
// device footprint and sorts each chunk's (frame, group) work items longest
// first, a chunk's maps / streams / tables are uploaded into one arena,
// decode_batch_kernel (jxg_decode.hip) runs once per launch class, and the
// reconstruction chain (jxg_reconstruct.cpp) runs per frame from the frame's
// arena slices into the caller's buffer.  The arithmetic is that of
// jxg_decode_rgb8: same walk, same reconstruction kernels.
#include <atomic>
#include <future>
#include <memory>

#include "jxg_ctx.h"
#include "jxg_decode.h"
#include "jxg_decode_plan.h"

namespace jxg {

namespace {

bool frame_status(jxg_status st) { return st == JXG_ERR_INVALID_ARG || st == JXG_ERR_UNSUPPORTED; }

// parses frames `todo` into F (status in st); the frames and their LF groups
// share at most 8 threads, this one included
void parse_frames(const uint8_t* const* datas, const size_t* sizes, const std::vector<uint32_t>& todo,
                  std::vector<std::unique_ptr<DecFrame>>& F, std::vector<jxg_status>& st) {
  const uint32_t nthreads = (uint32_t)std::min<size_t>(todo.size(), 8);
  const uint32_t lf_threads = std::max(1u, 8u / std::max(nthreads, 1u));
  std::atomic<uint32_t> next{0};
  auto work = [&]() {
    for (;;) {
      const uint32_t k = next.fetch_add(1);
      if (k >= todo.size()) return;
      const uint32_t i = todo[k];
      try {
        F[i].reset(new DecFrame);
        st[i] = (jxg_status)decode_parse(datas[i], sizes[i], true, F[i].get(), lf_threads);
      } catch (const std::bad_alloc&) {
        st[i] = JXG_ERR_OOM;
      } catch (...) {
        st[i] = JXG_ERR_INTERNAL;
      }
    }
  };
  std::vector<std::future<void>> helpers;
  helpers.reserve(nthreads);
  for (uint32_t t = 1; t < nthreads; t++) {
    try {
      helpers.push_back(std::async(std::launch::async, work));
    } catch (const std::system_error&) {
      break;  // no thread to be had: the others take its share
    }
  }
  work();
  for (auto& h : helpers) h.get();
}

jxg_status hip_status(hipError_t e) { return e == hipErrorOutOfMemory ? JXG_ERR_OOM : JXG_ERR_HIP; }
#define JXG_HIP_MEM(expr)                        \
  do {                                           \
    const hipError_t e_ = (expr);                \
    if (e_ != hipSuccess) return hip_status(e_); \
  } while (0)

// call-level status; per-frame statuses in st
jxg_status run(Ctx* c, const uint8_t* const* datas, const size_t* sizes, uint32_t n,
               uint8_t* const* rgbs, const size_t* strides, std::vector<jxg_status>& st,
               bool on_device) {
  const Clock::time_point t_call = Clock::now();
  hipStream_t s = c->stream;
  Ctx::DecBatch& B = c->decb;
  jxg_decode_batch_stats stats{};
  stats.frames = n;
  // ---- host: parse every frame that has its arguments
  std::vector<std::unique_ptr<DecFrame>> F(n);
  std::vector<uint32_t> todo;
  for (uint32_t i = 0; i < n; i++) {
    if (!datas[i] || sizes[i] == 0 || !rgbs[i])
      st[i] = JXG_ERR_INVALID_ARG;
    else
      todo.push_back(i);
  }
  parse_frames(datas, sizes, todo, F, st);
  std::vector<ReconFrame> R(n);
  std::vector<uint32_t> good;  // the call's frame of each planned frame
  for (uint32_t i : todo) {
    if (st[i] == JXG_OK && strides[i] < (size_t)F[i]->info.xsize * 3) st[i] = JXG_ERR_INVALID_ARG;
    if (st[i] == JXG_OK) st[i] = decode_recon_frame(*F[i], &R[i]);
    if (st[i] == JXG_OK)
      good.push_back(i);
    else if (!frame_status(st[i]))
      return st[i];  // out of memory, internal: the call's
    else
      F[i].reset();
  }
  stats.ms_parse = ms_since(t_call);
  // ---- plan
  std::vector<DecPlanFrame> P(good.size());
  std::vector<DecTableBlob> blobs(good.size());
  size_t max_plane = 0, max_rgb = 0, max_tiles = 0;
  for (size_t k = 0; k < good.size(); k++) {
    const DecFrame& f = *F[good[k]];
    blobs[k] = decode_table_blob(f.hf);
    DecPlanFrame& p = P[k];
    p.bxs = f.bxs;
    p.bys = f.bys;
    p.ntiles = f.tiles_x * f.tiles_y;
    p.stream_words = f.words.size();
    p.table_bytes = blobs[k].bytes.size();
    p.nhist = (uint32_t)f.hf.hist.size();
    p.tab_bytes = blobs[k].tab_bytes;
    p.ngroups = f.info.num_groups;
    p.sec = f.sec.data();
    const Frame g = make_frame(f.info.xsize, f.info.ysize, 1.0f);
    max_plane = std::max(max_plane, (size_t)g.xp * g.yp);
    max_tiles = std::max(max_tiles, (size_t)g.tiles_x * g.tiles_y);
    max_rgb = std::max(max_rgb, (size_t)f.info.xsize * 3 * f.info.ysize);
  }
  const std::vector<DecChunk> chunks = plan_decode_batch(P, B.budget);
  if (!good.empty()) {
    c->rc.ok = false;
    if (on_device) {
      const jxg_status so = order_input(c, c);  // the caller's earlier use of the outputs
      if (so) return so;
    }
    for (hipEvent_t& e : B.ev)
      if (!e && make_event(&e, hipEventDefault) != hipSuccess) return JXG_ERR_HIP;
    // the reconstruction's planes, sized once for the largest frame of the call
    JXG_HIP_MEM(c->rc.pa.ensure(3 * max_plane));
    JXG_HIP_MEM(c->rc.pb.ensure(3 * max_plane));
    JXG_HIP_MEM(c->rc.big.ensure(1 + (max_tiles / 2 + 1)));
    if (!on_device) JXG_HIP_MEM(c->rc.rgb.ensure(max_rgb));
  }
  // ---- device, chunk by chunk
  for (const DecChunk& C : chunks) {
    const uint32_t nf = C.end - C.first;
    const uint32_t ns = (uint32_t)C.staged.size(), nu = (uint32_t)C.unstaged.size();
    JXG_HIP_MEM(B.arena.ensure(C.bytes));
    JXG_HIP_MEM(B.status.ensure(C.nstatus));
    const size_t desc_bytes = (size_t)nf * sizeof(DecodeArgs);
    static_assert(sizeof(DecodeArgs) % 8 == 0, "the work list follows the descriptors");
    std::vector<uint8_t> h_desc(desc_bytes + ((size_t)ns + nu) * sizeof(DecWork));
    JXG_HIP_MEM(B.desc.ensure(h_desc.size()));
    DecodeArgs* h_args = reinterpret_cast<DecodeArgs*>(h_desc.data());
    DecWork* h_work = reinterpret_cast<DecWork*>(h_desc.data() + desc_bytes);
    uint8_t* const base = B.arena.p;
    for (uint32_t k = 0; k < nf; k++) {
      const DecFrame& f = *F[good[C.first + k]];
      const DecTableBlob& T = blobs[C.first + k];
      const DecSlices& at = C.at[k];
      const DecSliceBytes sz = decode_slice_bytes(P[C.first + k]);
      JXG_HIP(hipMemcpyAsync(base + at.acs, f.acs.data(), sz.acs, hipMemcpyHostToDevice, s));
      JXG_HIP(hipMemcpyAsync(base + at.qf, f.qf.data(), sz.qf, hipMemcpyHostToDevice, s));
      JXG_HIP(hipMemcpyAsync(base + at.dc, f.dc.data(), sz.dc, hipMemcpyHostToDevice, s));
      JXG_HIP(hipMemcpyAsync(base + at.cmap, f.cmap.data(), sz.cmap, hipMemcpyHostToDevice, s));
      JXG_HIP(hipMemcpyAsync(base + at.stream, f.words.data(), sz.stream, hipMemcpyHostToDevice, s));
      JXG_HIP(hipMemcpyAsync(base + at.sec, f.sec.data(), sz.sec, hipMemcpyHostToDevice, s));
      JXG_HIP(hipMemcpyAsync(base + at.tab, T.bytes.data(), sz.tab, hipMemcpyHostToDevice, s));
      DecodeArgs a{};
      a.stream = reinterpret_cast<const uint64_t*>(base + at.stream);
      a.sec = reinterpret_cast<const uint64_t*>(base + at.sec);
      a.sym.hist = reinterpret_cast<const dec::HistDesc*>(base + at.tab);
      a.sym.atab = reinterpret_cast<const dec::AnsEntry*>(base + at.tab + T.o_atab);
      a.sym.ptab = reinterpret_cast<const uint16_t*>(base + at.tab + T.o_ptab);
      a.sym.ctxmap = base + at.tab + T.o_map;
      a.sym.nctx = (uint32_t)f.hf.ctxmap.size();
      a.sym.prefix = f.hf.prefix;
      a.sym.log_alpha = f.hf.log_alpha;
      a.npresets = f.info.num_hf_presets;
      a.preset_bits = f.preset_bits;
      a.acs = base + at.acs;
      a.ac = reinterpret_cast<int16_t*>(base + at.ac);
      a.status = B.status.p + C.status_base[k];
      a.bxs = f.bxs;
      a.bys = f.bys;
      a.gxs = f.gxs;
      a.nhist = P[C.first + k].nhist;
      a.tab_bytes = T.tab_bytes;
      std::memcpy(&h_args[k], &a, sizeof(a));
    }
    // the launches index the chunk's descriptors: frame - C.first
    for (uint32_t i = 0; i < ns + nu; i++) {
      const DecWork& w = i < ns ? C.staged[i] : C.unstaged[i - ns];
      const DecWork rel{w.frame - C.first, w.group};
      std::memcpy(&h_work[i], &rel, sizeof(rel));
    }
    JXG_HIP(hipMemcpyAsync(B.desc.p, h_desc.data(), h_desc.size(), hipMemcpyHostToDevice, s));
    const DecodeArgs* d_args = reinterpret_cast<const DecodeArgs*>(B.desc.p);
    const DecWork* d_work = reinterpret_cast<const DecWork*>(B.desc.p + desc_bytes);
    JXG_HIP(hipEventRecord(B.ev[0], s));
    JXG_HIP(launch_decode_batch(d_args, d_work, ns, true, C.lds_staged, s));
    JXG_HIP(launch_decode_batch(d_args, d_work + ns, nu, false, C.lds_unstaged, s));
    JXG_HIP(hipEventRecord(B.ev[1], s));
    std::vector<uint32_t> status(C.nstatus, 0);
    JXG_HIP(hipMemcpyAsync(status.data(), B.status.p, (size_t)C.nstatus * 4, hipMemcpyDeviceToHost,
                           s));
    JXG_HIP(hipStreamSynchronize(s));  // (also: the uploads' host vectors may go)
    stats.chunks++;
    stats.items_staged += ns;
    stats.items_unstaged += nu;
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, B.ev[0], B.ev[1]);
    stats.ms_groups += ms;
    JXG_HIP(hipEventRecord(B.ev[2], s));
    for (uint32_t k = 0; k < nf; k++) {
      const uint32_t i = good[C.first + k];
      const uint32_t ng = P[C.first + k].ngroups;
      F[i].reset();
      for (uint32_t g = 0; g < ng && st[i] == JXG_OK; g++) {
        const uint32_t v = status[C.status_base[k] + g];
        if (v) st[i] = v == (uint32_t)dec::kUnsupported ? JXG_ERR_UNSUPPORTED : JXG_ERR_INVALID_ARG;
      }
      if (st[i] != JXG_OK) continue;
      const DecSlices& at = C.at[k];
      const ReconMaps M{base + at.acs, base + at.qf, reinterpret_cast<const int32_t*>(base + at.dc),
                        reinterpret_cast<const int16_t*>(base + at.ac),
                        reinterpret_cast<const int8_t*>(base + at.cmap)};
      const size_t row = (size_t)R[i].w * 3;
      jxg_status rs;
      if (on_device) {
        rs = reconstruct_device(c, R[i], M, rgbs[i], strides[i]);
      } else {
        rs = reconstruct_device(c, R[i], M, c->rc.rgb.p, row);
        if (rs == JXG_OK)
          JXG_HIP(hipMemcpy2DAsync(rgbs[i], strides[i], c->rc.rgb.p, row, row, R[i].h,
                                   hipMemcpyDeviceToHost, s));
      }
      if (rs) return rs;
    }
    JXG_HIP(hipEventRecord(B.ev[3], s));
    JXG_HIP(hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&ms, B.ev[2], B.ev[3]);
    stats.ms_recon += ms;
  }
  stats.ms_call = ms_since(t_call);
  B.stats = stats;
  return JXG_OK;
}

}  // namespace

jxg_status decode_batch_rgb8(Ctx* c, const uint8_t* const* datas, const size_t* sizes, uint32_t n,
                             uint8_t* const* rgbs, const size_t* row_strides, jxg_status* statuses,
                             bool on_device) {
  jxg_status call = JXG_OK;
  std::vector<jxg_status> st;
  try {
    st.assign(n, JXG_OK);
    call = run(c, datas, sizes, n, rgbs, row_strides, st, on_device);
  } catch (const std::bad_alloc&) {
    call = JXG_ERR_OOM;
  } catch (...) {
    call = JXG_ERR_INTERNAL;
  }
  if (call != JXG_OK) {
    // a device or memory failure is the call's: no frame's output is vouched for
    (void)hipStreamSynchronize(c->stream);
    if (statuses)
      for (uint32_t i = 0; i < n; i++) statuses[i] = call;
    return call;
  }
  jxg_status first = JXG_OK;
  for (uint32_t i = 0; i < n; i++) {
    if (statuses) statuses[i] = st[i];
    if (first == JXG_OK && st[i] != JXG_OK) first = st[i];
  }
  return first;
}

}  // namespace jxg
