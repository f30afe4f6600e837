// jxg_shard_host.cpp -- sharded encode, one frame at a time (jxg_shard_begin /
// jxg_shard_end, with the caller's collectives in between), a rank's payload,
// and the three assemblers of every rank's payloads into one codestream.  The
// codestream's layout is jxg_layout.h's; the heads are parsed by
// jxg_payload.cpp (frame_of_heads).
#include <cstring>

#include "jxg_ctx.h"
#include "jxg_layout.h"
#include "jxg_payload.h"

namespace jxg {

jxg_status shard_begin(Ctx* c, const uint8_t* d_rgb, uint32_t w, uint32_t h, size_t stride,
                       uint32_t rank, uint32_t world, uint32_t* d_hist, uint8_t* d_xbuf) {
  hipStream_t s = c->stream;
  c->rc.ok = false;
  c->job = std::make_unique<Job>();
  Job& J = *c->job;
  J.f = make_frame(w, h, c->params.distance);
  if (world < 1 || rank >= world || J.f.ngroups < world || J.f.ngroups < 2)
    return JXG_ERR_INVALID_ARG;
  J.plan = make_plan(J.f, rank, world);
  J.w = w;
  J.h = h;
  J.stride = stride;
  J.d_rgb = d_rgb;
  jxg_status st = stage_alloc(c, J);
  if (st) return st;
  // ANS: one HF preset per rank (its own histograms; the caller need not
  // all-reduce d_hist).  Prefix codes keep one preset from the summed
  // histogram (N x 132 clusters would not fit one context map).
  J.presets = J.ans && world > 1;
  if ((st = order_input(c, c))) return st;
  if ((st = build_front(c, J))) return st;
  Job* jp = &J;
  if ((st = launch_transform(&c, &jp, 1))) return st;
  JXG_HIP(hipMemcpyAsync(d_hist, c->hist_ac.d, kMaxClusters * kAlpha * 4, hipMemcpyDeviceToDevice, s));
  JXG_HIP(hipMemcpyAsync(d_hist + (size_t)kMaxClusters * kAlpha, c->bigcount.d, 16,
                         hipMemcpyDeviceToDevice, s));
  // the send list (then the receive list) of the record exchange
  const Exchange& X = J.plan.x;
  JXG_HIP(c->xlist.ensure(X.send.size() + X.recv.size() + 1));
  if (!X.send.empty())
    JXG_HIP(hipMemcpyAsync(c->xlist.p, X.send.data(), X.send.size() * 4, hipMemcpyHostToDevice, s));
  if (!X.recv.empty())
    JXG_HIP(hipMemcpyAsync(c->xlist.p + X.send.size(), X.recv.data(), X.recv.size() * 4,
                           hipMemcpyHostToDevice, s));
  PackArgs pa{c->acs.p, c->qf.p, c->dc.p, J.f.bxs, J.f.bys, J.f.gxs, c->cmap.p, J.f.tiles_x,
              J.f.tiles_y, d_xbuf, c->xlist.p, (uint32_t)X.send.size()};
  launch_pack(pa, s);
  JXG_HIP(hipGetLastError());
  JXG_HIP(hipEventRecord(c->ev[kEvMerged], s));
  JXG_HIP(hipStreamSynchronize(s));
  return JXG_OK;
}

jxg_status shard_end(Ctx* c, const uint32_t* d_hist, const uint8_t* d_xbuf, size_t* payload_bytes) {
  if (!c->job) return JXG_ERR_INVALID_ARG;
  const Clock::time_point t_call = Clock::now();
  Job& J = *c->job;
  hipStream_t s = c->stream;
  const Exchange& X = J.plan.x;
  PackArgs pa{c->acs.p, c->qf.p, c->dc.p, J.f.bxs, J.f.bys, J.f.gxs, c->cmap.p, J.f.tiles_x,
              J.f.tiles_y, const_cast<uint8_t*>(d_xbuf), c->xlist.p + X.send.size(),
              (uint32_t)X.recv.size()};
  launch_unpack(pa, s);
  JXG_HIP(hipGetLastError());
  jxg_status st;
  if ((st = stage_download_ac(c, J, d_hist))) return st;
  Job* jp = &J;
  if ((st = launch_lf_stats(&c, &jp, 1))) return st;
  if ((st = stage_codes(c, J))) return st;
  if ((st = stage_emit(c, J))) return st;
  if ((st = shard_finish(c, J, payload_bytes))) return st;
  c->stats = jxg_stats{};
  c->stats.xsize = J.w;
  c->stats.ysize = J.h;
  c->stats.num_groups = J.f.ngroups;
  c->stats.num_lf_groups = J.f.nlf;
  c->stats.bytes = *payload_bytes;
  c->stats.ms_front = elapsed(c->ev[kEvStart], c->ev[kEvMerged]);
  c->stats.ms_front_kernel = elapsed(c->ev[kEvFrontStart], c->ev[kEvFrontDone]);
  c->stats.ms_aq = elapsed(c->ev[kEvStart], c->ev[kEvFrontStart]);
  c->stats.ms_total = elapsed(c->ev[kEvStart], c->ev[kEvAssembled]);
  c->stats.ms_host_call = ms_since(t_call);
  c->job.reset();
  return JXG_OK;
}

// A rank's sections of a frame (codes built, emission launched) -> payload
// head (host, lane->payload_head) + body (device, lane->out); the stream is
// synchronised.  The payload's format: jxg_payload.h.
// (sync false: the body may still be in flight on the context's stream; the
// streaming path enqueues its D2H behind it -- shard_write_host -- so the head
// goes out one GPU round trip earlier)
jxg_status shard_finish(Ctx* c, Job& J, size_t* payload_bytes, bool sync) {
  hipStream_t s = c->stream;
  jxg_status st0 = wait_emission(c, J);  // the emission's bit counts on the host
  if (st0) return st0;
  std::vector<uint32_t> ids, sizes;
  size_t nbytes = 0;
  jxg_status st;
  if ((st = stage_concat(c, J, false, &ids, &sizes, nullptr, &nbytes))) return st;
  std::vector<uint32_t>& hw = c->payload_head;
  hw.assign(7 + 2 * ids.size(), 0);
  hw[0] = kPayloadMagic;
  hw[1] = J.presets ? 2 : 1;
  // the rank, the frame's loop-filter code, the 128 / 256 px kinds the rank's
  // groups use (their quant tables go into HfGlobal, effort >= 8)
  hw[2] = J.plan.rank | J.lf << 16 | (J.big ? big_mask(c->bigcount.h) : 0u) << 24;
  hw[3] = J.plan.world;
  hw[4] = J.w;
  hw[5] = J.h;
  hw[6] = (uint32_t)ids.size();
  for (size_t i = 0; i < ids.size(); i++) {
    hw[7 + 2 * i] = ids[i];
    hw[8 + 2 * i] = sizes[i];
  }
  if (J.presets) {
    // version 2: the rank's HF preset -- [B][nhist][context map, bytes packed
    // in words][clustered counts nhist x kAlpha], B = words after B
    const uint32_t nh = J.nhist_ans, cw = (kAcCtx + 3) / 4;
    hw.push_back(1 + cw + nh * kAlpha);
    hw.push_back(nh);
    const size_t o = hw.size();
    hw.resize(o + cw, 0);
    std::memcpy(hw.data() + o, J.pre_ctxmap.data(), kAcCtx);
    hw.insert(hw.end(), J.pre_counts.begin(), J.pre_counts.end());
  }
  c->payload_body = nbytes;
  *payload_bytes = hw.size() * 4 + nbytes;
  if (sync) JXG_HIP(hipStreamSynchronize(s));
  return JXG_OK;
}

// copy the payload of the last jxg_shard_end to dst (device or host memory)
jxg_status shard_payload(Ctx* c, void* dst, bool on_device) {
  hipStream_t s = c->stream;
  const size_t head = c->payload_head.size() * 4;
  if (!head) return JXG_ERR_INVALID_ARG;
  uint8_t* d = static_cast<uint8_t*>(dst);
  if (on_device) {
    JXG_HIP(hipMemcpyAsync(d, c->payload_head.data(), head, hipMemcpyHostToDevice, s));
    JXG_HIP(hipMemcpyAsync(d + head, c->out.p, c->payload_body, hipMemcpyDeviceToDevice, s));
  } else {
    std::memcpy(d, c->payload_head.data(), head);
    JXG_HIP(hipMemcpyAsync(d + head, c->out.p, c->payload_body, hipMemcpyDeviceToHost, s));
  }
  JXG_HIP(hipStreamSynchronize(s));
  return JXG_OK;
}

jxg_status shard_head(const Ctx* c, uint32_t* dst, size_t* nwords) {
  const size_t n = c->payload_head.size();
  if (n == 0) return JXG_ERR_INVALID_ARG;
  if (dst) {
    if (*nwords < n) return JXG_ERR_INVALID_ARG;
    std::memcpy(dst, c->payload_head.data(), n * 4);
  }
  *nwords = n;
  return JXG_OK;
}

// device-resident payloads (payload i at d_base + offsets[i]) -> codestream in
// host memory: headers + TOC on the host, every section moved by the concat
// kernel, one D2H of the result
jxg_status shard_assemble_device(Ctx* c, const uint8_t* d_base, const size_t* offsets,
                                 const size_t* psizes, uint32_t n, jxg_buffer* out) {
  hipStream_t s = c->stream;
  // payload heads to the host (a few KB each)
  std::vector<std::vector<uint32_t>> heads(n);
  const std::vector<size_t> ps(psizes, psizes + n);
  for (uint32_t i = 0; i < n; i++) {
    const uint8_t* src = d_base + offsets[i];
    const jxg_status st = read_head_from(ps[i], [src](size_t nwords, uint32_t* dst) {
      JXG_HIP(hipMemcpy(dst, src, nwords * 4, hipMemcpyDeviceToHost));
      return JXG_OK;
    }, heads[i]);
    if (st) return st;
  }
  ShardFrame F;
  const jxg_status st = frame_of_heads(heads, ps, true, &F);
  if (st) return st;
  // payloads are read as one 32-bit-word arena starting at d_base; a
  // generated HfGlobal (per-rank presets) goes through the chunk arena
  PieceList L;
  for (size_t i = 0; i < F.secs.size(); i++) {
    const SectionRef& r = F.secs[i];
    if (r.payload == n)
      L.section((uint32_t)i, {L.add_chunk(F.hf.data(), r.size)});
    else
      L.section((uint32_t)i, {PieceList::Piece{kArenaAc, (offsets[r.payload] + r.off) * 8,
                                               (uint64_t)r.size * 8}});
  }
  const size_t nbytes = L.place(&F.lay.head, false);
  const size_t out_words = (nbytes + 3) / 4 + 1;
  const std::vector<PlacedPiece>& cps = L.pieces();
  const std::vector<uint32_t>& chunk_words = L.chunk_words();
  JXG_HIP(c->cat.chunks.ensure(chunk_words.size()));
  JXG_HIP(c->cat.pieces.ensure(cps.size()));
  JXG_HIP(c->out.ensure(out_words));
  uint8_t* ho = out_alloc(out_words * 4);
  if (!ho) return JXG_ERR_OOM;
  JXG_HIP(hipMemcpyAsync(c->cat.chunks.p, chunk_words.data(), chunk_words.size() * 4, hipMemcpyHostToDevice, s));
  JXG_HIP(hipMemcpyAsync(c->cat.pieces.p, cps.data(), cps.size() * sizeof(ConcatPiece), hipMemcpyHostToDevice, s));
  // arena 0 = the payload base (word aligned: offsets are multiples of 4)
  launch_concat(c->cat.pieces.p, (uint32_t)cps.size(), out_words,
                reinterpret_cast<const uint32_t*>(d_base), c->cat.chunks.p, nullptr, c->out.p, s);
  JXG_HIP(hipGetLastError());
  if (hipMemcpyAsync(ho, c->out.p, out_words * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    out_release(ho);
    return JXG_ERR_HIP;
  }
  out->data = ho;
  out->size = nbytes;
  return JXG_OK;
}

// Distributed host assembly: with every rank's payload head (host), each rank
// writes its own sections straight from its device body into one host buffer
// shared by all ranks (one D2H per contiguous run: its pass groups are one
// run, its LF groups one each); rank 0 also writes headers + TOC.  The layout
// is shard_assemble_device's (frame_of_heads), without the payload gather and
// the serial D2H of the whole codestream on rank 0.
// (sync false: the copies are left in flight on the context's stream)
jxg_status shard_write_host(Ctx* c, const uint32_t* const* heads_in, const size_t* words,
                            uint32_t n, uint8_t* dst, size_t dst_size, size_t* total, bool sync) {
  if (c->payload_head.size() < 7) return JXG_ERR_INVALID_ARG;
  std::vector<std::vector<uint32_t>> heads(n);
  std::vector<size_t> ps(n);
  for (uint32_t i = 0; i < n; i++) {
    if (!heads_in[i] || words[i] < 7) return JXG_ERR_INVALID_ARG;
    heads[i].assign(heads_in[i], heads_in[i] + words[i]);
    if (head_words(heads[i].data(), words[i]) != words[i]) return JXG_ERR_INVALID_ARG;
    size_t body = 0;
    for (uint32_t k = 0; k < heads[i][6]; k++) body += heads[i][8 + 2 * k];
    ps[i] = words[i] * 4 + body;
  }
  const uint32_t me = c->payload_head[2] & 0xFFFFu;
  if (me >= n || heads[me] != c->payload_head) return JXG_ERR_INVALID_ARG;
  // a generated HfGlobal (per-rank presets) is written by rank 0; the others
  // need its size only
  ShardFrame F;
  const jxg_status st = frame_of_heads(heads, ps, me == 0, &F);
  if (st) return st;
  const std::vector<uint64_t>& out_off = F.lay.off;
  *total = (size_t)F.lay.total;
  if (!dst || F.lay.total > dst_size) return JXG_ERR_INVALID_ARG;  // *total tells the size needed
  hipStream_t s = c->stream;
  const std::vector<uint32_t>& hw = c->payload_head;
  // runs of consecutive sections (payload body -> codestream offsets)
  std::vector<ScatterPiece> runs;
  uint64_t body = 0;
  for (uint32_t k = 0; k < hw[6]; k++) {
    const uint32_t id = hw[7 + 2 * k], sz = hw[8 + 2 * k];
    ScatterPiece* r = runs.empty() ? nullptr : &runs.back();
    if (r && r->src + r->len == body && r->dst + r->len == out_off[id])
      r->len += sz;
    else if (sz)
      runs.push_back({body, out_off[id], sz, 0});
    body += sz;
  }
  // one scatter launch through the buffer's device mapping (page-locked with
  // jxg_host_register); D2H copies per run otherwise
  void* dmap = nullptr;
  if (!runs.empty() && runs.size() <= (size_t)kMaxScatterPieces &&
      hipHostGetDevicePointer(&dmap, dst, 0) == hipSuccess && dmap) {
    ScatterArgs sa{};
    sa.src = reinterpret_cast<const uint8_t*>(c->out.p);
    sa.dst = static_cast<uint8_t*>(dmap);
    sa.n = (uint32_t)runs.size();
    uint32_t nwg = 0;
    for (size_t i = 0; i < runs.size(); i++) {
      sa.p[i] = runs[i];
      sa.p[i].wg0 = nwg;
      const uint64_t w0 = runs[i].dst >> 2, w1 = (runs[i].dst + runs[i].len + 3) >> 2;
      nwg += (uint32_t)((w1 - w0 + 1023) / 1024);
    }
    launch_scatter(sa, nwg, s);
    JXG_HIP(hipGetLastError());
  } else {
    (void)hipGetLastError();  // (an unmapped buffer: hipHostGetDevicePointer failed)
    for (const ScatterPiece& r : runs)
      JXG_HIP(hipMemcpyAsync(dst + r.dst, reinterpret_cast<const uint8_t*>(c->out.p) + r.src, r.len,
                             hipMemcpyDeviceToHost, s));
  }
  if (me == 0) {
    const std::vector<uint8_t> hb = F.lay.head.bytes();
    std::memcpy(dst, hb.data(), hb.size());
    for (size_t i = 0; i < F.secs.size(); i++)  // a generated HfGlobal (per-rank presets)
      if (F.secs[i].payload == n && F.secs[i].size)
        std::memcpy(dst + out_off[i], F.hf.data(), F.hf.size());
  }
  if (sync) JXG_HIP(hipStreamSynchronize(s));
  return JXG_OK;
}

// host only: payloads of every rank -> codestream (no device needed)
jxg_status shard_assemble(const uint8_t* const* payloads, const size_t* sizes, uint32_t n,
                          jxg_buffer* out) {
  if (!payloads || !sizes || !out || n == 0) return JXG_ERR_INVALID_ARG;
  std::vector<std::vector<uint32_t>> heads(n);
  const std::vector<size_t> ps(sizes, sizes + n);
  for (uint32_t i = 0; i < n; i++) {
    if (!payloads[i]) return JXG_ERR_INVALID_ARG;
    heads[i] = read_head(payloads[i], sizes[i]);
    if (heads[i].empty()) return JXG_ERR_INVALID_ARG;
  }
  ShardFrame F;
  const jxg_status st = frame_of_heads(heads, ps, true, &F);
  if (st) return st;
  uint8_t* o = out_alloc_heap((size_t)F.lay.total);
  if (!o) return JXG_ERR_OOM;
  const std::vector<uint8_t> hb = F.lay.head.bytes();
  std::memcpy(o, hb.data(), hb.size());
  for (size_t i = 0; i < F.secs.size(); i++) {
    const SectionRef& r = F.secs[i];
    std::memcpy(o + F.lay.off[i], r.payload == n ? F.hf.data() : payloads[r.payload] + r.off, r.size);
  }
  out->data = o;
  out->size = (size_t)F.lay.total;
  return JXG_OK;
}

}  // namespace jxg
