// jxg_plan.h -- what a context encodes, as plain host data: the frame's
// geometry and scales, the shard partition / record exchange / work plan, and
// the streaming pipeline's shape.  Host only (no HIP include): the encoder's
// files launch from these, tests/native/plan_host.cpp prints them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#pragma GCC visibility push(hidden)
namespace jxg {

// frame-level scalars: same formulas as oracle jxo_frame_init (host, double)
struct Frame {
  uint32_t w, h, bxs, bys, xp, yp, tiles_x, tiles_y;
  uint32_t gxs, gys, ngroups, lfxs, lfys, nlf;
  float qf_base, inv_g;
  uint32_t G, qdc;
  float dc_mul[3], dc_step[3];
};
// the frame-argument limits of every entry point that takes a frame
inline bool frame_args_ok(uint32_t w, uint32_t h, size_t stride) {
  return w != 0 && h != 0 && w <= (1u << 18) && h <= (1u << 18) && stride >= (size_t)w * 3;
}
// global scale and DC quantizer -> the dequantization steps (the encoder takes
// the two from the distance, the decoder from LfGlobal)
void set_frame_scales(Frame& f, uint32_t G, uint32_t qdc);
Frame make_frame(uint32_t w, uint32_t h, float distance);

// ---------------------------------------------------------------------------
// Work plan: which tiles, pass groups and LF groups this context encodes.
// world == 1: everything.  Sharded, make_partition:
//   1. balanced contiguous raster ranges of pass groups (rank r: [n*r/world,
//      n*(r+1)/world)), each LF group owned by the rank holding most of its
//      pass groups -- kept when that needs no record exchange (16384^2 over 8
//      ranks: LF-group rows fall on range boundaries);
//   2. otherwise whole LF groups per rank, when they balance: LF groups
//      assigned largest first (pixel area) to the least-loaded rank, kept if
//      the largest rank load is within 5 % of the mean (8K over 2 / 4 / 8
//      ranks: 1.1 %) -- every rank then owns the LF groups of all its pass
//      groups, so no per-block records move between ranks and a rank's frames
//      need no collective until assembly (the streaming shard pipeline);
//   3. else the ranges of 1 with the record exchange.
// ---------------------------------------------------------------------------
uint32_t shard_g0(uint32_t ngroups, uint32_t r, uint32_t world);
uint32_t shard_of(uint32_t ngroups, uint32_t g, uint32_t world);
uint32_t lf_of_group(const Frame& f, uint32_t g);
// LF-group owners under the contiguous ranges: the rank holding the most of
// the LF group's pass groups, less 16 per LF group already assigned to it (so
// near ties -- an LF group split over ranks' row ranges -- spread over ranks
// instead of piling onto one); ties go to the lower rank.
std::vector<uint32_t> lf_owners_ranges(const Frame& f, uint32_t world);
struct Partition {
  std::vector<uint32_t> group;  // [ngroups] owner rank of each pass group
  std::vector<uint32_t> lf;     // [nlf] owner rank of each LF group
  int kind = 0;                 // 0 ranges (no exchange), 1 whole LF groups, 2 ranges + exchange
};
Partition make_partition(const Frame& f, uint32_t world);
// Record exchange of rank `rank`: send = its groups whose LF group another
// rank owns, ordered by (destination rank, group); recv = other ranks' groups
// inside its own LF groups, ordered by (source rank, group).  Counts per peer.
struct Exchange {
  std::vector<uint32_t> send, recv, nsend, nrecv;
};
Exchange make_exchange(const Frame& f, const Partition& part, uint32_t rank, uint32_t world);
// exchange record of one pass group (jxg_shard.hip): acs, qf, 3 x int32 DC
constexpr size_t kGroupRecordBytes = 1024 * 2 + 1024 * 4 * 3 + 32;  // jxg_shard.hip
// records of the largest send or receive buffer of any rank (at least 1)
size_t exchange_slot_records(const Frame& f, uint32_t world);

struct Plan {
  uint32_t rank = 0, world = 1;
  std::vector<uint32_t> groups; // pass groups, ascending (launch slot i = groups[i])
  bool contiguous = true;       // groups == [groups[0], groups[0] + size)
  std::vector<uint32_t> tiles;  // shard: owned tile ids (ty * tiles_x + tx)
  std::vector<uint8_t> lf_mine; // shard: [nlf] 1 = owned LF group
  Exchange x;                   // shard: record exchange
  bool owns_lf(uint32_t lg) const { return world == 1 || lf_mine[lg]; }
  uint32_t g0() const { return groups.empty() ? 0 : groups[0]; }
  uint32_t ng() const { return (uint32_t)groups.size(); }
};
Plan make_plan(const Frame& f, uint32_t rank, uint32_t world);

// ---------------------------------------------------------------------------
// The streaming pipeline's shape (jxg_pipe.cpp): lanes and frames per lane
// (batch) for a frame / shard of `ngroups` pass groups and `ntiles` 64x64
// tiles.  Batches only for frames of at most kPipeBatchTiles tiles (1080p:
// 510, a rank's eighth of 8K: 1080): 4K in batches of 3 fell from 8.1 to
// 4.8 GPix/s (profiles/r04h) -- a frame that fills the chip gains nothing from
// sharing a launch and its lane's latency grows with every frame in the
// batch; the 8K eighth gains 0.63 -> 0.56 ms per frame, a quarter (2160
// tiles) nothing (profiles/r04k).
// ---------------------------------------------------------------------------
#ifndef JXG_PIPE_CHAIN_GROUPS  // (experiment builds override it: tools/build_variant.sh)
#define JXG_PIPE_CHAIN_GROUPS 3570
#endif
#ifndef JXG_PIPE_BATCH_TILES  // (experiment builds override it: tools/build_variant.sh)
#define JXG_PIPE_BATCH_TILES 1280
#endif
constexpr uint32_t kPipeMaxLanes = 12, kPipeMinLanes = 4, kPipeChainGroups = JXG_PIPE_CHAIN_GROUPS;
constexpr uint32_t kPipeBatchTiles = JXG_PIPE_BATCH_TILES;
constexpr uint32_t kPipeMaxBatch = 4;  // == kMaxBatch of the batched launches (jxg_kernels.h)
struct PipeShape {
  uint32_t lanes, batch;
  uint32_t frames() const { return lanes * batch; }
  // shard frames that may be pending with the next submit always accepted:
  // unwritten frames (written oldest first, so only the oldest batch is
  // partly written) leave a lane free while they fill at most lanes - 1
  // batches -- jxg_pipeline_depth
  uint32_t pending() const { return (lanes - 1) * batch + 1; }
};
// cap: jxg_set_pipeline_lanes, 0 = none.  queues: the process's hardware
// queues (hw_queues(), jxg_ctx.cpp); lanes beyond queues - 1 (one is left for
// the caller's own stream) would share a queue with another lane and
// serialise its kernels (5.5 vs 6.7 GPix/s at 8K)
PipeShape pipe_shape(uint32_t ngroups, uint32_t ntiles, uint32_t cap, uint32_t queues);

}  // namespace jxg
#pragma GCC visibility pop
