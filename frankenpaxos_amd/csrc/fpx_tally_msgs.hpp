// fpx_tally_msgs.hpp -- ProxyLeader.handlePhase2b (multipaxos/ProxyLeader.scala:217-258) for a tick of PER-ACCEPTOR
// Phase2b messages, as reference acceptors send them: one message per (acceptor, slot), f + 1 or more per slot, in any
// order, duplicates and several rounds of one slot included.  k_tally (fpx_kernels.hpp) takes one row per (slot, round)
// and needs the slots of a launch pairwise distinct; the host fold that used to build those rows
// (fpx_wire_phase2b_rows, one thread, a hash table) is done here by three launches whose boundaries order the passes:
//
//   k_msgs_claim   thread / message: checks the message's bit, finds the tally entry of (slot, round) with k_tally's own
//                  lookup, and bids for the entry with atomicMin(owner[entry], i) -- the FIRST message of every
//                  (slot, round) ends up its owner, which is where fpx_wire_phase2b_rows + fpx_proxy_phase2b report the
//                  row's outcome
//   k_msgs_gather  thread / message: atomicOr of the message's bit into the owner's row (n x 4 words, zeroed per call)
//   k_msgs_tally   thread / message: the owner runs tally_row -- k_tally's body -- on the gathered row and hands the
//                  entry back (owner[entry] = INT_MAX); every other message reports "nothing chosen"
//   k_msgs_tail    one thread: turns what the claim pass found (a bad bit, an unknown (slot, round)) into the context's
//                  status, lowest message index first
//
// Only integer atomics (min / or / max), so the result does not depend on the order the hardware runs the threads in.
// `owner` ([S][wp] int32, one word per tally entry) is INT_MAX between calls: every entry claimed in a call has exactly
// one message whose index the minimum settled on, and that message resets it in k_msgs_tally -- also when the call
// applies nothing (a bad bit, or the context already in the "apply nothing" state, in which case nothing is claimed).
//
// The per-message bodies (msgs_claim_one, msgs_gather_dst + msgs_or_merged, msgs_tally_one) are device functions: the
// Mencius burst kernels (fpx_mencius_msgs.hpp) run them for the Phase2b's of a mixed burst.
//
// Then the compaction of a tick's newly chosen records in message order (fpx_wire_phase2b_tick): count per workgroup,
// scan of the workgroup counts, emit.
#pragma once
#include <limits.h>

#include "fpx_kernels.hpp"
#include "fpx_scan.hpp"

namespace fpx {

// status words: 0x7fffffff - the lowest offending message index, 0 = none (the encoding of ST_WIRE)
enum { ST_MSG_BAD = 6, ST_MSG_UNKNOWN = 7 };

#ifndef FPX_GATHER_MERGE
#define FPX_GATHER_MERGE 1  // k_msgs_gather: neighbouring lanes with the same destination word merge before the atomic
#endif

struct MsgBatch {
  int32_t n;
  const int32_t* kind;   // null: every message is a Phase2b
  const int32_t* group;  // null: group_index 0
  const int32_t* acceptor;
  const int32_t* slot;
  const int32_t* round;
  int32_t grid_cols;
  int32_t phase2b;       // FPX_WIRE_PHASE2B
  int32_t* owner;        // [S][wp]
  int32_t* entry;        // [n]  the message's tally entry, -1 = contributes nothing
  unsigned long long* row_bits;  // [n][4]
  uint8_t* chosen;
  int32_t* chosen_round;
  int32_t* chosen_value;
};

// the claim of ONE Phase2b message: its tally entry, -1 = contributes nothing (shared with fpx_mencius_msgs.hpp)
__device__ __forceinline__ int msgs_claim_one(const Geom& g, const State& st, const MsgBatch& b, int i) {
  int e = -1;
  const int a = b.acceptor[i], s = b.slot[i], rnd = b.round[i];
  const long long bit = b.grid_cols > 0 ? (long long)(b.group ? b.group[i] : 0) * b.grid_cols + a : a;
  if (bit < 0 || bit >= 256 || a < 0 || (b.grid_cols > 0 && a >= b.grid_cols) || s < 0 || s >= g.S || rnd < 0 ||
      rnd > MAX_ROUND) {
    atomicMax(&st.status[ST_MSG_BAD], 0x7fffffff - i);
  } else if ((g.member[bit >> 6] >> (bit & 63)) & 1ull) {  // a bit outside the member set contributes nothing
    const size_t ps = (size_t)phys_slot(g, s);
    const uint32_t* kr = st.pl_key + ps * g.wp;
    const uint32_t want = (uint32_t)rnd + 1u;
    int way = -1;
    for (int w = 0; w < g.ways; ++w)
      if ((kr[w] & KEY_ROUND_MASK) == want) way = w;
    if (way < 0) {
      atomicMax(&st.status[ST_MSG_UNKNOWN], 0x7fffffff - i);  // :220-225; the message is dropped
    } else {
      e = (int)(ps * g.wp + way);
      atomicMin(&b.owner[e], i);
    }
  }
  return e;
}

__global__ void __launch_bounds__(256) k_msgs_claim(const Geom g, const State st, const MsgBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.n) return;
  int e = -1;
  if (st.status[ST_ABORT] == 0 && (!b.kind || b.kind[i] == b.phase2b)) e = msgs_claim_one(g, st, b, i);
  b.entry[i] = e;
}

// atomicOr(&base[dst], v) for every lane with dst >= 0 (every lane of the wavefront calls this)
__device__ __forceinline__ void msgs_or_merged(unsigned long long* base, long long dst, unsigned long long v) {
#if FPX_GATHER_MERGE
  // The votes of one slot often sit next to each other in a tick: a run of neighbouring lanes with one destination
  // becomes ONE atomic, sent by the run's first lane (a segmented OR towards lower lanes, 6 steps; every lane of the
  // wavefront takes part in the shuffles)
  const int lane = threadIdx.x & 63;
  const long long up = __shfl_up(dst, 1);
  const bool head = lane == 0 || up != dst;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long ov = __shfl_down(v, d);
    const long long od = __shfl_down(dst, d);
    if (lane + d < 64 && od == dst) v |= ov;  // lanes lane .. lane + d hold dst throughout: runs are contiguous
  }
  if (dst >= 0 && head) atomicOr(&base[dst], v);
#else
  if (dst >= 0) atomicOr(&base[dst], v);
#endif
}

// where the bit of Phase2b message i goes: the word of row_bits (-1: nowhere) and the bit within it
__device__ __forceinline__ long long msgs_gather_dst(const MsgBatch& b, int i, int e, unsigned long long* v) {
  if (e < 0) return -1;
  const int bit = b.grid_cols > 0 ? (b.group ? b.group[i] : 0) * b.grid_cols + b.acceptor[i] : b.acceptor[i];
  *v = 1ull << (bit & 63);
  return (long long)b.owner[e] * 4 + (bit >> 6);
}

__global__ void __launch_bounds__(256) k_msgs_gather(const Geom g, const State st, const MsgBatch b) {
  if (st.status[ST_ABORT] != 0 || st.status[ST_MSG_BAD] != 0) return;  // nothing is applied: no row is read
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = i < b.n ? b.entry[i] : -1;
  unsigned long long v = 0;
  const long long dst = msgs_gather_dst(b, i, e, &v);  // the word of row_bits this message's bit goes to
  msgs_or_merged(b.row_bits, dst, v);
}

// the tally of ONE Phase2b message (shared with fpx_mencius_msgs.hpp): the owner of entry e tallies the gathered row
__device__ __forceinline__ void msgs_tally_one(const Geom& g, const State& st, const MsgBatch& b, int i, int e, bool apply,
                                               uint8_t* ch, int* cr, int* cv) {
  if (e >= 0 && b.owner[e] == i) {
    if (apply) {
      uint64_t row[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) row[w] = b.row_bits[(size_t)i * 4 + w];
      tally_row(g, st, i, b.slot[i], b.round[i], row, ch, cr, cv);
    }
    b.owner[e] = INT_MAX;
  }
}

__global__ void __launch_bounds__(256) k_msgs_tally(const Geom g, const State st, const MsgBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.n) return;
  const bool apply = st.status[ST_ABORT] == 0 && st.status[ST_MSG_BAD] == 0;
  uint8_t ch = 0;
  int cr = -1, cv = -1;
  msgs_tally_one(g, st, b, i, b.entry[i], apply, &ch, &cr, &cv);
  if (b.chosen) b.chosen[i] = ch;
  if (b.chosen_round) b.chosen_round[i] = cr;
  if (b.chosen_value) b.chosen_value[i] = cv;
}

__global__ void k_msgs_tail(const State st, const MsgBatch b) {
  const int32_t bad = st.status[ST_MSG_BAD], unk = st.status[ST_MSG_UNKNOWN];
  st.status[ST_MSG_BAD] = 0, st.status[ST_MSG_UNKNOWN] = 0;
  if (bad != 0) {
    const int i = 0x7fffffff - bad;
    report_abort(st, 1 /*FPX_EINVAL*/, i, b.slot[i], b.round[i]);
  } else if (unk != 0) {
    const int i = 0x7fffffff - unk;
    report(st, 2 /*FPX_EFATAL_UNKNOWN_SLOTROUND*/, i, b.slot[i], b.round[i]);
  }
}

// ---- the newly chosen records of a tick, compacted in message order ------------------------------------------------
// out: [3][cap] = slot, round, value of the k-th newly chosen message; totals[0] = how many there are (also when they do
// not fit: FPX_ECAPACITY, a per-call code -- the first `cap` records are written).
struct MsgCompact {
  int32_t n, nblk, cap;
  const uint8_t* chosen;
  const int32_t* slot;
  const int32_t* chosen_round;
  const int32_t* chosen_value;
  int32_t* blk;  // [nblk] workgroup counts, then their exclusive sums
  int32_t *out_slot, *out_round, *out_value;
  int64_t* totals;
};

__global__ void __launch_bounds__(256) k_msgs_count(const State st, const MsgCompact c) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool f = st.status[ST_ABORT] == 0 && i < c.n && c.chosen[i] != 0;
  __shared__ int wsum[4];
  int total;
  (void)block_rank(f, &total, wsum);
  if (threadIdx.x == 0) c.blk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(1024) k_msgs_scan(const State st, const MsgCompact c) {
  __shared__ int lds[SCAN_ARRAY_LDS(1024)];
  const int total = scan_array_excl<ScanSum, 1024, 1>(c.blk, c.nblk, lds);
  if (threadIdx.x == 0) {
    c.totals[0] = total;
    if (total > c.cap) report(st, 5 /*FPX_ECAPACITY*/, -1, -1, -1);
  }
}

__global__ void __launch_bounds__(256) k_msgs_emit(const State st, const MsgCompact c) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool f = st.status[ST_ABORT] == 0 && i < c.n && c.chosen[i] != 0;
  __shared__ int wsum[4];
  int total;
  const int at = c.blk[blockIdx.x] + block_rank(f, &total, wsum);
  if (f && at < c.cap) {
    c.out_slot[at] = c.slot[i];
    c.out_round[at] = c.chosen_round[i];
    c.out_value[at] = c.chosen_value[i];
  }
}

}  // namespace fpx
