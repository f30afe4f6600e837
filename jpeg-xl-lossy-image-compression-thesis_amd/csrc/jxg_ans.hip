// jxg_ans.hip -- the rANS coder of the pass groups' AC tokens on gfx950, over
// the token records ac_hist_kernel wrote (jxg_acrec.h): the chains in two
// forms, the per-chunk bit sums, the bit placement.
#include "jxg_device.h"
#include "jxg_kernels.h"
#include "jxg_acrec.h"

namespace jxg {

// ---------------------------------------------------------------------------
// ANS: the token records ac_hist wrote in stream order; one lane per group
// runs the rANS encoder backwards over its records (the stream's only
// sequential dependency), then the group's workgroup places the emitted bits
// in parallel.
// ---------------------------------------------------------------------------
// Two chain kernels share the step: the streaming pipeline's frames run the
// lane-per-chain form below (small footprint beside the other frames'
// kernels), a frame coded by itself the diagonal form after it (shorter span);
// launch_ans chooses.
//
// rANS backwards over each group's records, one LANE per group: workgroup w
// of a frame takes the slots order[64 w .. 64 w + 63] (longest group first,
// so its lanes have similar lengths), and lane c of its chain wave (wave 0)
// runs that slot's chain by itself: at step t the record n_c - 1 - t.  Every
// lane does useful work at every step, so the 510 chains of an 8K frame are
// 8 chain waves instead of 510.
//
// The state recurrence is the stream's only sequential dependency, so the
// per-step latency sets the kernel time (a pass group holds up to ~100K
// tokens).  The state x = k << 12 | v is kept as (k = quotient of the
// previous step, v = its inverse-table entry).  The step's dependent path:
//   emission k >= f << 8 (x >= f << 20) -> the shift sh = 16 or 0,
//   x = k << 12 + v, xs = x >> sh, the quotient floor(xs / f) =
//   trunc((xs + 0.5) * rcp(f)) in f64 (cvt, fma, cvt; exact: one rounding,
//   < 2^-19, while (xs + .5) / f stays >= .5 / f from an integer), the table
//   address base + 2 (xs - q f) (shift-add, 24-bit multiply-add), the u16 read.
// The chain wave touches no global memory (64 lanes walking 64 streams are 64
// cache lines per access, and the CU's memory pipe then sets the step: 8.3 ms
// a frame against 5.6 with the loads and stores in the chain wave, DESIGN.md
// §3.5).  It works from two LDS stages of kAnsBlk steps x 64 lanes, double
// buffered by block:
//   ea : per step and lane the record's stage word: the byte offset of its
//        constants entry (one 16-byte entry per (histogram, token): rcp =
//        1.0 / (double)f computed once per workgroup -- no division in the
//        loop --, -2 f, and the byte offset of the symbol's inverse row; the
//        idle entry, f = 4096 on histogram 0, never emits and keeps any state
//        valid), and beside it the record's raw bits and their count;
//   x  : the state before the step, which the chain wave writes back.
// The helper waves fetch the records of block b + 2, fill ea for block b + 1
// and turn the x and ea of block b - 1 into the records' emitted bits while
// the chain wave runs block b: a helper wave takes one chain at a time, lane =
// step, so its loads and stores are contiguous.  A lane past its record 0
// gets idle entries; the state before the first idle step is the chain's
// final state (an empty chain: the initial state 0x130000), which the helper
// stores.  The stage rows are 65 words so that the chain wave's rows and the
// helpers' columns are both free of bank conflicts.
//
// Synchronisation: one workgroup barrier per block and nothing else.  Every
// wave runs the same number of barriers, NB + 1 with NB taken from the
// workgroup's longest chain before the loop; no wave waits on a flag.
//
// LDS: inverse tables 64 KB + constants 8.02 KB + cluster map 0.5 KB + stages
// 2 x 2 x 16.25 KB = 65 KB + chain parameters 2 KB = 139.5 KB per workgroup
// (142 872 bytes in the kernel descriptor), 8 workgroups per 8K frame (the
// diagonal form: 64 x 68 KB).  20.5 KB of the CU's 160 KB stay free beside a
// chain workgroup: ans_sums (12.1 KB), ans_emit (14.8 KB), lf_code (17.3 KB),
// lf_hist, vb_list, merge_resolve and concat workgroups fit there; front (79
// KB), aq (46 KB), merge_eval (53 KB), merge_write (37 KB) and ac_hist (31 KB) do not,
// so the 8 CUs of a frame's chains are lost to the transform kernels of the
// frames behind it.  The chain wave runs at the highest wave priority.
// Workgroup shape: ONE chain wave per workgroup, not one per SIMD sharing the
// tables: in the form where each chain wave did its own loads and stores, 2
// and 4 chain waves per workgroup ran 1.5x and 2.4x slower;
// that has not been measured again with helpers.  Wave 4 only takes the
// barriers: on the assumption (not measured: no 6-against-7-helper A/B was
// run) that a workgroup's waves go to the SIMDs round robin, it would share
// the chain wave's SIMD.
constexpr int kAnsWgWaves = 8;  // wave 0: the chains; waves 1-3, 5-7: helpers; 4: barriers only
constexpr int kAnsHelpers = 6;
constexpr int kAnsPieces = (64 + kAnsHelpers - 1) / kAnsHelpers;  // chains per helper
constexpr int kAnsBlk = 64;     // steps per stage block
constexpr int kAnsRow = 65;     // stage row stride in words
constexpr uint32_t kAnsIdle = kAnsHists * 64;  // constants entry of the idle step
struct AnsConst {
  double rcp;      // 1.0 / (double)f
  uint32_t nf2;    // -2 f
  uint32_t base2;  // byte offset of the symbol's inverse row
};
struct AnsChainP {  // a lane's chain, for the helpers
  int n;            // records
  uint32_t slot;
  uint32_t c1, c2, c3;  // first stream position of bands 1-3
  uint32_t g;       // pass group; ~0u: no chain in this lane
  uint32_t pad[2];
};
struct AnsLds {
  AnsConst c[kAnsIdle + 1];            // per (histogram, token), then the idle entry
  uint16_t ent[256];                   // cluster byte -> byte offset of its histogram's 64 entries
  uint32_t inv[kAnsHists * 4096 / 2];  // alias inverses, u16 pairs
  uint32_t ea[2][kAnsBlk * kAnsRow];
  uint32_t x[2][kAnsBlk * kAnsRow];
  AnsChainP ch[64];
  int T;                               // steps of the workgroup: its longest chain + 1
};
// blk: the chain workgroup's index within its frame
__device__ __forceinline__ void ans_chain(const AnsArgs& a, uint32_t blk) {
  // (one object, constants first: every table address is an instruction offset)
  __shared__ __attribute__((aligned(16))) AnsLds L;
  const uint32_t c0 = blk * 64;
  if (c0 >= a.n) return;  // the whole workgroup
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tab);
  for (uint32_t i = threadIdx.x; i < a.nhist * 512; i += blockDim.x)
    reinterpret_cast<uint4*>(L.inv)[i] = reinterpret_cast<const uint4*>(src + kAnsInvOff / 4)[i];
  for (uint32_t i = threadIdx.x; i <= kAnsIdle; i += blockDim.x) {
    uint32_t f = 4096, row = 0;  // the idle step; also the histograms not in use
    if (i < a.nhist * 64) {
      const uint32_t e = src[(i >> 6) * 128 + (i & 63)];
      f = (e & 0xFFF) + 1;
      row = (i >> 6) * 4096 + (e >> 12);
    }
    L.c[i].rcp = 1.0 / (double)f;
    L.c[i].nf2 = (uint32_t)(-(int)(2 * f));
    L.c[i].base2 = 2 * row;
  }
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x)
    L.ent[i] = (uint16_t)(i < 136 ? min((uint32_t)a.tab[kAnsMapOff + i], kAnsHists - 1) * 64 * 16
                                  : kAnsIdle * 16);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave == 0) {
    AnsChainP P = {0, 0, 0, 0, 0, ~0u, {0, 0}};
    if (c0 + lane < a.n) {
      P.slot = a.order[c0 + lane];
      P.g = slot_group(a.glist, a.g0, P.slot);
      P.n = (int)group_tokens(a.ntok, P.g);
      P.c1 = a.bandtok[P.g * kBands];
      P.c2 = P.c1 + a.bandtok[P.g * kBands + 1];
      P.c3 = P.c2 + a.bandtok[P.g * kBands + 2];
    }
    L.ch[lane] = P;
    int m = P.n;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, __shfl_xor(m, d, 64));
    if (lane == 0) L.T = m + 1;
  }
  __syncthreads();
  const int NB = (L.T + kAnsBlk - 1) / kAnsBlk;  // blocks: the same in every wave
  const uint8_t* inv = reinterpret_cast<const uint8_t*>(L.inv);
  const uint8_t* cst = reinterpret_cast<const uint8_t*>(L.c);
  // helper h of kAnsHelpers, or none
  const int h = (wave & 3) ? (int)(wave >> 2) * 3 + (int)(wave & 3) - 1 : -1;
  // a helper wave takes one chain at a time, lane = step of the block
  const uint32_t hs = lane;
  // stage word of a record: its constants entry (byte offset, a multiple of
  // 16, < 2^14) | raw-bit count | raw bits << 14
  auto word_of = [&](uint32_t rec) {
    return ((uint32_t)L.ent[rec_cluster(rec)] + rec_token(rec) * 16) | rec_nbits(rec) | rec_bits(rec) << 14;
  };
  auto record = [&](const AnsChainP& P, int i) {  // stream position i of the chain (rec_index)
    const uint32_t u = (uint32_t)i;
    const uint32_t j = (u >= P.c1 ? 1u : 0u) + (u >= P.c2 ? 1u : 0u) + (u >= P.c3 ? 1u : 0u);
    const uint32_t lo = u >= P.c3 ? P.c3 : u >= P.c2 ? P.c2 : u >= P.c1 ? P.c1 : 0u;
    return a.tokens[(uint64_t)P.slot * kGroupTokStride + j * (uint32_t)kBandTokStride + (u - lo)];
  };
  // A helper owns the chains q = h, h + kAnsHelpers, ... (<= kAnsPieces of
  // them): the same lane fills and flushes a stage slot, so its own program
  // order is all the ordering a slot's reuse needs.
  constexpr uint32_t kIdleRec = 0xFFu;  // cluster byte 0xFF -> the idle entry
  // the records of block b, all loads in flight at once
  auto fetch = [&](int b, uint32_t* R) {
#pragma unroll
    for (int j = 0; j < kAnsPieces; j++) {
      const int q = h + kAnsHelpers * j;
      R[j] = kIdleRec;
      if (q < 64) {
        const AnsChainP P = L.ch[q];
        const int i = P.n - 1 - (b * kAnsBlk + (int)hs);
        if (i >= 0) R[j] = record(P, i);
      }
    }
  };
  auto fill = [&](int b, const uint32_t* R) {
#pragma unroll
    for (int j = 0; j < kAnsPieces; j++) {
      const int q = h + kAnsHelpers * j;
      if (q < 64) L.ea[b & 1][hs * kAnsRow + q] = word_of(R[j]);
    }
  };
  // what block b left in the stages: the states and its records' words
  auto unstage = [&](int b, uint32_t* X, uint32_t* RC) {
#pragma unroll
    for (int j = 0; j < kAnsPieces; j++) {
      const int q = h + kAnsHelpers * j;
      X[j] = RC[j] = 0;
      if (q < 64) {
        X[j] = L.x[b & 1][hs * kAnsRow + q];
        RC[j] = L.ea[b & 1][hs * kAnsRow + q];
      }
    }
  };
  auto flush = [&](int b, const uint32_t* X, const uint32_t* RC) {
#pragma unroll
    for (int j = 0; j < kAnsPieces; j++) {
      const int q = h + kAnsHelpers * j;
      if (q < 64) {
        const AnsChainP P = L.ch[q];
        const int i = P.n - 1 - (b * kAnsBlk + (int)hs);
        const uint32_t x = X[j], w = RC[j];
        if (i >= 0) {
          // emitted bits of the record: [16-bit chunk] then its raw bits
          // (their sums per chunk: ans_sums)
          const uint32_t nf2 = reinterpret_cast<const AnsConst*>(cst + (w & 0x3FF0))->nf2;
          const bool em = (x >> 12) >= (uint32_t)__mul24((int)nf2, -128);  // k >= f << 8
          const uint32_t raw = w >> 14, nb = w & 15;
          const uint64_t o = (uint64_t)P.slot * kGroupTokStride + (uint32_t)i;
          a.val[o] = em ? (x & 0xFFFFu) | raw << 16 : raw;
          a.len[o] = (uint8_t)(em ? nb + 16 : nb);
        } else if (i == -1 && P.g != ~0u) {
          a.state[P.g] = x;  // the state after record 0
        }
      }
    }
  };
  uint32_t k = 0x130u, v = 0;  // the initial state x = 0x130000 (chain wave)
  auto chain_block = [&](int b) {
    const uint32_t* eas = L.ea[b & 1] + lane;
    uint32_t* xo = L.x[b & 1] + lane;
    AnsConst Cn = *reinterpret_cast<const AnsConst*>(cst + (eas[0] & 0x3FF0));
#pragma unroll
    for (int s = 0; s < kAnsBlk; s++) {
      const AnsConst C = Cn;  // read one step ahead, off the dependent path
      if (s + 1 < kAnsBlk) Cn = *reinterpret_cast<const AnsConst*>(cst + (eas[(s + 1) * kAnsRow] & 0x3FF0));
      const double hr = 0.5 * C.rcp;
      const uint32_t Fq = (uint32_t)__mul24((int)C.nf2, -128);  // f << 8: emit iff k >= Fq
      // the dependent path: k, v -> x -> xs -> quotient -> address -> read
      const uint32_t sh = k >= Fq ? 16u : 0u;
      const uint32_t x = (k << 12) + v;
      const uint32_t xs = x >> sh;
      const uint32_t kk = (uint32_t)__builtin_fma((double)xs, C.rcp, hr);
      const uint32_t x2 = (xs << 1) + C.base2;
      uint32_t addr;
      asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(addr) : "v"(kk), "v"(C.nf2), "v"(x2));
      v = *reinterpret_cast<const uint16_t*>(inv + addr);
      k = kk;
      xo[s * kAnsRow] = x;
    }
  };
  if (wave == 0) __builtin_amdgcn_s_setprio(3);
  // helpers: the records are fetched two blocks ahead of the chain wave and
  // staged one block ahead, so a block's global latency is never waited for
  uint32_t R[kAnsPieces], X[kAnsPieces], RC[kAnsPieces];
  if (h >= 0) {
    fetch(0, R);
    fill(0, R);
    fetch(1, R);
  }
  __syncthreads();
  for (int b = 0; b < NB; b++) {
    if (wave == 0) {
      chain_block(b);
    } else if (h >= 0) {
      if (b > 0) unstage(b - 1, X, RC);  // before fill(b + 1) reuses block b - 1's ea slots
      fill(b + 1, R);
      fetch(b + 2, R);
      if (b > 0) flush(b - 1, X, RC);
    }
    __syncthreads();
  }
  if (h >= 0) {
    unstage(NB - 1, X, RC);
    flush(NB - 1, X, RC);
  }
}
__global__ __launch_bounds__(kAnsWgWaves * 64) void ans_encode_kernel(Batch<AnsArgs> bt_) {
  ans_chain(bt_.a[blockIdx.z], blockIdx.x);
}
// The latency form, for a frame coded by itself (one-at-a-time encodes: nothing
// else wants the GPU, and the frame waits for its longest chain): one WAVE per
// group "on the diagonal", kAnsDiagWaves groups per workgroup sharing the LDS
// tables (symbols 4 KB + all alias inverses 64 KB = 68 KB).  Lane L holds
// record L's constants in registers and step L is computed in lane L from
// lane L-1's result, which a DPP wave rotation (wave_ror:1, VALU to VALU)
// hands over; the other lanes run the same rANS steps on other (valid)
// states, so every lane's table address stays in range.  The same step
// arithmetic as above in 15 issue slots, with no stage, no barrier and no
// helper in its way: 5.6 ms for an 8K frame's chains against 6.15 ms for the
// lane-per-chain form, but 510 waves on 64 CUs, which is what the streamed
// frames cannot afford.  Per 64 records the lanes decode
// record, f, rcp and table base in parallel (the next 64 records are fetched
// meanwhile) and store the emitted bits of their record with one coalesced
// store.  The lane protocol is pinned by tests/test_ans_lane_model.py.
constexpr int kAnsDiagWaves = 8;
__device__ __forceinline__ uint32_t wave_ror1(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x13C, 0xF, 0xF, false);
}
// blk: the chain workgroup's index within its frame
__device__ __forceinline__ void ans_chain_diag(const AnsArgs& a, uint32_t blk) {
  __shared__ uint32_t sSym[kAnsHists * 128];
  __shared__ uint32_t sInv[kAnsHists * 4096 / 2];  // u16 pairs
  __shared__ uint8_t sMap[136];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tab);
  for (uint32_t i = threadIdx.x; i < a.nhist * 128; i += blockDim.x) sSym[i] = src[i];
  for (uint32_t i = threadIdx.x; i < a.nhist * 2048; i += blockDim.x)
    sInv[i] = src[kAnsInvOff / 4 + i];
  for (uint32_t i = threadIdx.x; i < 136; i += blockDim.x) sMap[i] = a.tab[kAnsMapOff + i];
  __syncthreads();
  const uint8_t* inv = reinterpret_cast<const uint8_t*>(sInv);
  const uint32_t lane = threadIdx.x & 63;
  // the chain's group: groups sorted longest first (host), kAnsDiagWaves per
  // workgroup, so a workgroup's waves finish at about the same time and the
  // workgroups of short groups free their CUs early
  const uint32_t gi = __builtin_amdgcn_readfirstlane(blk * kAnsDiagWaves + (threadIdx.x >> 6));
  if (gi >= a.n) return;
  const uint32_t slot = __builtin_amdgcn_readfirstlane(a.order[gi]);
  const uint32_t g = __builtin_amdgcn_readfirstlane(slot_group(a.glist, a.g0, slot));
  __builtin_amdgcn_s_setprio(3);
  const int n = (int)group_tokens(a.ntok, g);
  const uint64_t b = (uint64_t)slot * kGroupTokStride;
  uint32_t bt[kBands];  // the group's stream = its bands' record spaces, in order
#pragma unroll
  for (int i = 0; i < kBands; i++) bt[i] = a.bandtok[g * kBands + i];
  // every lane starts from the initial state x = 0x130000
  uint32_t k = 0x130u, v = 0;
  uint32_t rec = (int)lane < min(64, n) ? a.tokens[b + rec_index(bt, n - 1 - lane)] : 0u;
  for (int hi = n; hi > 0; hi -= 64) {
    const int cnt = min(64, hi);
    // lane L: record hi - 1 - L.  Lanes past cnt get f = 4096 (a valid
    // never-emitting step on histogram 0).
    uint32_t f = 4096, base2 = 0;
    if ((int)lane < cnt) {
      const uint32_t h = sMap[rec_cluster(rec)], e = sSym[h * 128 + rec_token(rec)];
      f = (e & 0xFFF) + 1;
      base2 = 2 * (h * 4096 + (e >> 12));  // byte offset of the symbol's inverse row
    }
    const uint32_t Fq = f << 8;  // emit iff k >= Fq
    const uint32_t nf2 = (uint32_t)(-(int)(2 * f));
    const double rcp = 1.0 / (double)f, hr = 0.5 * rcp;
    const int hn = hi - 64;
    const uint32_t nrec = (int)lane < min(64, hn) ? a.tokens[b + rec_index(bt, hn - 1 - lane)] : 0u;
    uint32_t X = 0;     // lane L: the state before record L's step
    uint32_t xin = 0;   // the state handed to the previous step
    auto step = [&](int s) {
      // shadow: emission (a shift of 16 drops v: (k << 12 | v) >> 16 = k >> 4),
      // and the previous step's input state into its lane
      const uint32_t kin = wave_ror1(k);
      const uint32_t sh = kin >= Fq ? 16u : 0u;
      if (s > 0)
        asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(X) : "v"(X), "v"(xin), "s"(1ull << (s - 1)));
      __builtin_amdgcn_sched_barrier(0);
      // critical path: v -> x -> xs -> quotient -> address -> next read
      const uint32_t vin = wave_ror1(v);
      const uint32_t x = (kin << 12) + vin;
      const uint32_t xs = x >> sh;
      const uint32_t kk = (uint32_t)__builtin_fma((double)xs, rcp, hr);
      const uint32_t x2 = (xs << 1) + base2;
      uint32_t addr;
      asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(addr) : "v"(kk), "v"(nf2), "v"(x2));
      v = *reinterpret_cast<const uint16_t*>(inv + addr);
      k = kk;
      xin = x;
      __builtin_amdgcn_sched_barrier(0);
    };
    if (cnt == 64) {
#pragma unroll
      for (int s = 0; s < 64; s++) step(s);
      asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(X) : "v"(X), "v"(xin), "s"(1ull << 63));
    } else {
      for (int s = 0; s < cnt; s++) {
        const uint32_t kin = wave_ror1(k);
        const bool emit = kin >= Fq;
        const uint32_t t = (kin << 12) >> (emit ? 16 : 0);
        const double P = __builtin_fma((double)t, rcp, hr);
        const uint32_t C = 2 * t + base2;
        const uint32_t vin = wave_ror1(v);
        X = (int)lane == s ? (kin << 12) + vin : X;
        const uint32_t vv = emit ? 0u : vin;
        const uint32_t kk = (uint32_t)__builtin_fma((double)vv, rcp, P);
        const uint32_t addr = (uint32_t)((int)(2 * vv + C) - (int)(2 * f) * (int)kk);
        v = *reinterpret_cast<const uint16_t*>(inv + addr);
        k = kk;
      }
    }
    if ((int)lane < cnt) {
      // emitted bits of the record: [16-bit chunk] then its raw bits (their
      // sums per chunk: ans_sums, off the chain)
      const bool em = (X >> 20) >= f;
      const uint32_t raw = rec_bits(rec), nb = rec_nbits(rec);
      a.val[b + hi - 1 - lane] = em ? (X & 0xFFFFu) | raw << 16 : raw;
      a.len[b + hi - 1 - lane] = (uint8_t)(em ? nb + 16 : nb);
    }
    rec = nrec;
    if (hi <= 64) {  // the final state: lane cnt - 1's result
      const uint32_t kf = __builtin_amdgcn_readlane(k, cnt - 1);
      const uint32_t vf = __builtin_amdgcn_readlane(v, cnt - 1);
      if (lane == 0) a.state[g] = (kf << 12) + vf;
    }
  }
  if (n == 0 && lane == 0) a.state[g] = 0x130000u;
}
__global__ __launch_bounds__(kAnsDiagWaves * 64) void ans_encode_diag_kernel(Batch<AnsArgs> bt_) {
  ans_chain_diag(bt_.a[blockIdx.z], blockIdx.x);
}
// After the chains, one 256-thread workgroup per group: the emitted bits of
// every 64-record chunk q (stream order; records [n - 64 (K - q), n - 64 (K -
// q - 1)) clipped at 0) into csum[q], from which ans_emit places its
// segments; the section's bit count (the 32-bit state, then every record's
// bits); and the section's scratch words zeroed (ans_emit ORs the two words a
// segment shares with its neighbours; no arena memset).  Round 4 did this
// bookkeeping inside the chain, on its serial path.
constexpr int kSumThreads = 1024;
__global__ __launch_bounds__(kSumThreads) void ans_sums_kernel(Batch<AnsArgs> bt_) {
  __shared__ uint32_t sC[kAnsMaxChunks];
  __shared__ uint32_t sTot[kSumThreads / 64];
  const AnsArgs& a = bt_.a[blockIdx.z];
  const uint32_t slot = blockIdx.x;
  if (slot >= a.n) return;
  const uint32_t g = slot_group(a.glist, a.g0, slot);
  const uint32_t n = group_tokens(a.ntok, g);
  const uint32_t K = (n + 63) / 64;
  const uint64_t b = (uint64_t)slot * kGroupTokStride;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (uint32_t q = threadIdx.x; q < K; q += kSumThreads) sC[q] = 0;
  __syncthreads();
  // chunk q = records [64 q - off, 64 q + 64 - off) clipped at 0 (chunks end
  // at n); 16-byte words of the lengths: a chunk boundary can only fall at
  // byte r = n % 16 of a word (n - 64 (K - q) = r mod 16), so a word's bytes
  // below r go to one chunk and the rest to one chunk (LDS adds)
  const uint32_t off = (64u - (n & 63u)) & 63u, r = n & 15u;
  const uint4* L = reinterpret_cast<const uint4*>(a.len + b);
  for (uint32_t w = threadIdx.x; w < (n + 15) / 16; w += kSumThreads) {
    const uint4 v = L[w];
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
    const uint32_t valid = min(16u, n - 16u * w);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
      const uint32_t x = j < valid ? (d[j >> 2] >> (8 * (j & 3))) & 0xFFu : 0u;
      if (j < r) lo += x;
      else hi += x;
    }
    if (lo) atomicAdd(&sC[(16u * w + off) >> 6], lo);
    if (hi) atomicAdd(&sC[(16u * w + r + off) >> 6], hi);
  }
  __syncthreads();
  uint32_t* csum = a.csum + (uint64_t)slot * kAnsMaxChunks;
  uint32_t tot = 0;
  for (uint32_t q = threadIdx.x; q < K; q += kSumThreads) {
    const uint32_t c = sC[q];
    csum[q] = c;
    tot += c;
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) tot += __shfl_xor(tot, m, 64);
  if (lane == 0) sTot[wv] = tot;
  __syncthreads();
  uint32_t total = 32;
#pragma unroll
  for (int i = 0; i < kSumThreads / 64; i++) total += sTot[i];
  if (threadIdx.x == 0) a.bits[g] = total;
  uint32_t* dst = a.scratch + (a.base[g] >> 5);
  for (uint32_t i = threadIdx.x; i < (total + 31) / 32; i += kSumThreads) dst[i] = 0;
}
// bit placement: the 32-bit state, then every record's bits, in order.  One
// 256-thread workgroup per (group, segment of kSegChunks chunks of 64
// records): the segment's first bit is 32 + the chain's chunk sums before it
// (no pass over the lengths); each wave places whole chunks (their offsets
// from the same sums) with a wave scan of the lengths into an LDS image of
// the segment aligned to the scratch words, then the workgroup stores it --
// plain stores inside the segment, atomic ORs on the two words it may share
// with its neighbours (zeroed by the chain).
constexpr int kSegChunks = 64, kEmitThreads = 256;
constexpr int kSegWords = (kSegChunks * 64 * 29 + 31) / 32 + 2;  // <= 29 bits per record
__global__ __launch_bounds__(kEmitThreads) void ans_emit_kernel(Batch<AnsArgs> bt_) {
  __shared__ __attribute__((aligned(16))) uint32_t sBits[kSegWords];
  __shared__ uint32_t sCs[kSegChunks + 1];
  __shared__ uint32_t sPre[kEmitThreads / 64];
  const AnsArgs& a = bt_.a[blockIdx.z];
  const uint32_t slot = blockIdx.x, seg = blockIdx.y;
  if (slot >= a.n) return;
  const uint32_t g = slot_group(a.glist, a.g0, slot);
  const uint32_t n = group_tokens(a.ntok, g);
  const uint32_t K = (n + 63) / 64, q0 = seg * kSegChunks;
  const uint64_t base = a.base[g];  // word aligned
  if (seg == 0 && threadIdx.x == 0) a.scratch[base >> 5] = a.state[g];
  if (q0 >= K) return;
  const uint32_t q1 = min(K, q0 + kSegChunks);
  const uint32_t* csum = a.csum + (uint64_t)slot * kAnsMaxChunks;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // bits before the segment: 32 + sum of the chunks before q0
  uint32_t pre = 0;
  for (uint32_t q = threadIdx.x; q < q0; q += kEmitThreads) pre += csum[q];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) pre += __shfl_xor(pre, d, 64);
  if (lane == 0) sPre[wv] = pre;
  if (threadIdx.x <= kSegChunks) sCs[threadIdx.x] = q0 + threadIdx.x < q1 ? csum[q0 + threadIdx.x] : 0u;
  for (int i = threadIdx.x; i < kSegWords; i += kEmitThreads) sBits[i] = 0;
  __syncthreads();
  const uint64_t start = base + 32 + sPre[0] + sPre[1] + sPre[2] + sPre[3];  // the segment's first bit
  const uint32_t sh0 = (uint32_t)(start & 31);
  uint32_t segbits = 0;
  for (uint32_t q = 0; q < q1 - q0; q++) segbits += sCs[q];
  // chunk q's records: [chunk_lo(q), chunk_lo(q + 1)), chunk_lo(K) = n
  auto chunk_lo = [&](uint32_t q) { return q == 0 ? 0u : n - 64u * (K - q); };
  const uint64_t b = (uint64_t)slot * kGroupTokStride;
  constexpr int kPerWave = kSegChunks / (kEmitThreads / 64);
  uint32_t run = sh0;  // bit offset inside the LDS image
  for (int i = 0; i < wv * kPerWave; i++) run += sCs[i];
  for (int i = 0; i < kPerWave; i++) {
    const uint32_t q = q0 + (uint32_t)(wv * kPerWave + i);
    if (q >= q1) break;
    const uint32_t lo = chunk_lo(q), hi = chunk_lo(q + 1);
    const uint32_t k = lo + (uint32_t)lane;
    const uint32_t len = k < hi ? a.len[b + k] : 0u;
    const uint32_t val = k < hi ? a.val[b + k] : 0u;
    const uint32_t incl = wave_incl_scan(len);
    if (len) {
      const uint32_t pos = run + incl - len;
      const uint32_t w = pos >> 5, sh = pos & 31;
      atomicOr(&sBits[w], val << sh);
      if (sh + len > 32) atomicOr(&sBits[w + 1], val >> (32 - sh));
    }
    run += sCs[wv * kPerWave + i];
  }
  __syncthreads();
  const uint32_t nw = (sh0 + segbits + 31) / 32;
  uint32_t* dst = a.scratch + (start >> 5);
  for (uint32_t i = threadIdx.x; i < nw; i += kEmitThreads) {
    const uint32_t v = sBits[i];
    if (i == 0 || i == nw - 1) {
      if (v) atomicOr(&dst[i], v);
    } else {
      dst[i] = v;
    }
  }
}

// the chains, then the bit placement, of k frames (same plan: same group
// count; the segment grid covers the longest group of any of them).
// streamed: the frames share the GPU with other frames' kernels -> the
// lane-per-chain kernel (8 workgroups per 8K frame); a frame coded by itself
// -> the diagonal kernel, whose chains finish sooner.  Same val / len / state.
void launch_ans(const AnsArgs* a, uint32_t k, hipStream_t s, bool streamed) {
  if (!k || !a[0].n) return;
  const Batch<AnsArgs> b = make_batch(a, k);
  uint32_t n = 0, maxtok = 0;
  for (uint32_t i = 0; i < k; i++) {
    n = max(n, a[i].n);
    maxtok = max(maxtok, a[i].max_tokens);
  }
  if (streamed)
    hipLaunchKernelGGL(ans_encode_kernel, dim3((n + 63) / 64, 1, k), dim3(kAnsWgWaves * 64), 0, s, b);
  else
    hipLaunchKernelGGL(ans_encode_diag_kernel, dim3((n + kAnsDiagWaves - 1) / kAnsDiagWaves, 1, k),
                       dim3(kAnsDiagWaves * 64), 0, s, b);
  hipLaunchKernelGGL(ans_sums_kernel, dim3(n, 1, k), dim3(kSumThreads), 0, s, b);
  const uint32_t nseg = (maxtok + kSegChunks * 64 - 1) / (kSegChunks * 64);
  if (nseg) hipLaunchKernelGGL(ans_emit_kernel, dim3(n, nseg, k), dim3(kEmitThreads), 0, s, b);
}
}  // namespace jxg
