// fpx_phase1b_msgs.hpp -- Leader.handlePhase1b (multipaxos/Leader.scala:306-329, 504-577; mencius/Leader.scala:359-385,
// 582-659) for a BURST of Phase1b messages in delivery order, each with its own Phase1b.info run: the consumer of
// fpx_acceptor_phase1b_info_all_dev's records and of the leader-inbound decoder's.  fpx_leader_phase1b_scan reads the vote
// rows of acceptors that live in this context; here the acceptors are anywhere (remote processes, other shards) and all
// the leader has is their messages.  Stateless: the context gives the geometry and keeps the scratch, nothing else.
//
// The handler, message by message: a message of another round is ignored; phase1bs(group)(acceptor) = message (a later
// one replaces an earlier one whole); at the FIRST message k after which the quorum condition holds the leader recovers
// from what it holds and is in Phase 2 -- everything after k is ignored.  The launches, no host read in between:
//
//   k_p1m_headers  thread / message: header checks; first[acceptor] = the lowest index of a counted message (atomicMin)
//   k_p1m_decide   ONE workgroup: the condition is monotone in k (the held set only grows, and it grows at first
//                  occurrences), so k is found by bisection over the index, each probe a pass over the first[] table;
//                  then last[acceptor] = the highest counted index <= k (atomicMax): the message that WINS the acceptor
//   k_p1m_plan     ONE workgroup: the winners in index order, the acceptors used, max_slot from each winner's last
//                  record (runs ascend), the exclusive sums of their work units, the output range
//   k_p1m_clear    zeroes the min(count, cap) words of the bid table
//   k_p1m_bid      a wavefront per P1M_UNIT consecutive records of ONE run (a run ascends in slot, so a wavefront's
//                  destinations ascend too): checks the records, and every record of an output slot of its own group
//                  bids atomicMax(table[j], (vote_round + 1) << 8 | (255 - bit)) -- the highest round, then the lowest bit
//   k_p1m_write    the same walk: the record whose key the maximum settled on writes safe_round / safe_value (one
//                  acceptor has one record per slot, so exactly one record matches)
//   k_p1m_fill     out_slot, and Noop where nobody bid; its first workgroup publishes the result words and the status
//
// Integer atomics only (min / max / or): the result does not depend on the order the hardware runs anything in.
// Nothing reaches the caller's arrays before every check has passed: the bid pass writes the scratch table only.
#pragma once
#include <limits.h>

#include "fpx_kernels.hpp"
#include "fpx_scan.hpp"
#include "fpx_phase1b_plan.hpp"

namespace fpx {

// control block (u64 words)
enum {
  P1M_BAD = 0,     // 0x7fffffff - the lowest message index that fails a check (atomicMax), 0 = none
  P1M_FUTURE = 1,  // the same for msg_round > round (logger.checkLt)
  P1M_STATE = 2,   // P1M_ST_*
  P1M_K = 3,
  P1M_FIRST = 4,   // the first output slot
  P1M_COUNT = 5,
  P1M_LIMIT = 6,   // min(count, cap)
  P1M_MAX = 7,     // max_slot + 1
  P1M_NEXT = 8,
  P1M_NWIN = 9,
  P1M_UNITS = 10
};
enum { P1M_ST_NONE = 0, P1M_ST_INCOMPLETE = 1, P1M_ST_GO = 2, P1M_ST_NOT_OWNED = 3 };
// result words (int64, include/fpx.h FPX_P1B_*)
enum { P1M_R_COMPLETE = 0, P1M_R_DECIDED_AT = 1, P1M_R_COUNT = 2, P1M_R_MAX_SLOT = 3, P1M_R_NEXT_SLOT = 4, P1M_R_WRITTEN = 5 };

struct P1mArgs {
  int32_t n;
  int32_t round, leader_group, recover_slot, watermark;
  int32_t all_rows;   // FPX_P1B_GRID_ALL_ROWS
  int32_t grid_cols;
  int32_t need;       // f + 1 acceptors per group (no grid)
  int32_t phase1b;    // FPX_WIRE_PHASE1B
  int32_t cap;
  const int32_t* kind;   // null: every message is a Phase1b
  const int32_t* msg_round;
  const int32_t* group;  // null: group_index 0
  const int32_t* acceptor;
  const int64_t* offsets;
  const int32_t* info_slot;
  const int32_t* info_round;
  const int32_t* info_value;
  int32_t keys;
  unsigned long long* ctl;
  unsigned long long* held;   // [ngroups][4]
  int64_t* unit0;             // [n + 1]
  int32_t* first;             // [keys]
  int32_t* last;              // [keys]
  int32_t* win;               // [n]
  unsigned long long* table;  // [cap]
  int32_t* out_slot;
  int32_t* safe_round;
  int32_t* safe_value;
  int64_t* result;            // [8]
  uint64_t* held_out;         // [ngroups][4] or null
};

__device__ __forceinline__ bool p1m_is_phase1b(const P1mArgs& a, int i) { return !a.kind || a.kind[i] == a.phase1b; }
__device__ __forceinline__ int p1m_key_of(const Geom& g, const P1mArgs& a, int i) {
  return p1m_key(a.grid_cols, g.num_groups, g.total, a.group ? a.group[i] : 0, a.acceptor[i]);
}
// a message the handler gets past its round check with (its key is known to be in range by then)
__device__ __forceinline__ bool p1m_counted(const P1mArgs& a, int i) { return p1m_is_phase1b(a, i) && a.msg_round[i] == a.round; }

__global__ void __launch_bounds__(256) k_p1m_headers(const Geom g, const State st, const P1mArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n || st.status[ST_ABORT] != 0) return;
  bool bad = a.offsets[i + 1] < a.offsets[i] || (i == 0 && a.offsets[0] != 0);
  if (p1m_is_phase1b(a, i)) {
    const int key = p1m_key_of(g, a, i);
    const int mr = a.msg_round[i];
    if (key < 0) bad = true;
    else if (mr > a.round) atomicMax(&a.ctl[P1M_FUTURE], (unsigned long long)(0x7fffffff - i));  // skipped
    else if (mr == a.round) atomicMin(&a.first[key], i);
  }
  if (bad) atomicMax(&a.ctl[P1M_BAD], (unsigned long long)(0x7fffffff - i));
}

// does the quorum condition hold over the acceptors whose first counted message has an index <= k?  (every thread of
// the workgroup of 1024 calls it, every thread gets the answer)
__device__ __forceinline__ bool p1m_holds(const Geom& g, const P1mArgs& a, int k, int* s_fail, uint64_t* s_held) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) *s_fail = 0;
  __syncthreads();
  if (a.grid_cols > 0) {
    if (t < P1M_KEYS_PER_GROUP) {
      const unsigned long long m = __ballot(t < g.total && a.first[t] <= k);
      if (lane == 0) s_held[wave] = m;
    }
  } else {
    for (int grp = wave; grp < g.num_groups; grp += 16) {
      int cnt = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int bit = q * 64 + lane;
        cnt += __popcll(__ballot(bit < g.total && a.first[grp * P1M_KEYS_PER_GROUP + bit] <= k));
      }
      if (lane == 0 && cnt < a.need) *s_fail = 1;  // phase1bs.exists(_.size < config.f + 1)
    }
  }
  __syncthreads();
  bool ok;
  if (a.grid_cols > 0) {
    const uint64_t x[4] = {s_held[0], s_held[1], s_held[2], s_held[3]};
    ok = is_read_quorum(g, x);  // grid.isReadQuorum(phase1bAcceptors)
  } else {
    ok = *s_fail == 0;
  }
  __syncthreads();
  return ok;
}

__global__ void __launch_bounds__(1024) k_p1m_decide(const Geom g, const State st, const P1mArgs a) {
  __shared__ int s_fail;
  __shared__ uint64_t s_held[4];
  const int t = threadIdx.x;
  if (st.status[ST_ABORT] != 0 || a.ctl[P1M_BAD] != 0) return;  // (state stays P1M_ST_NONE)
  if (a.n == 0 || !p1m_holds(g, a, a.n - 1, &s_fail, s_held)) {
    if (t == 0) a.ctl[P1M_STATE] = P1M_ST_INCOMPLETE;
    return;
  }
  int lo = 0, hi = a.n - 1;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (p1m_holds(g, a, mid, &s_fail, s_held)) hi = mid;
    else lo = mid + 1;
  }
  // the last message of every acceptor at indices <= k
  for (int i = t; i <= lo; i += 1024)
    if (p1m_counted(a, i)) atomicMax(&a.last[p1m_key_of(g, a, i)], i);
  if (t == 0) a.ctl[P1M_K] = (unsigned long long)lo, a.ctl[P1M_STATE] = P1M_ST_GO;
}

__global__ void __launch_bounds__(1024) k_p1m_plan(const Geom g, const P1mArgs a) {
  __shared__ int64_t w_units[16];
  __shared__ int w_win[16], w_max[16];
  __shared__ int64_t c_units;
  __shared__ int c_win;
  if (a.ctl[P1M_STATE] != P1M_ST_GO) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int k = (int)a.ctl[P1M_K];
  const int L = g.num_leader_groups;
  if (t == 0) c_units = 0, c_win = 0;
  __syncthreads();
  int ms = -1;
  for (int base = 0; base <= k; base += 1024) {
    const int i = base + t;
    bool win = false;
    int64_t units = 0;
    if (i <= k && p1m_counted(a, i)) {
      const int key = p1m_key_of(g, a, i);
      if (a.last[key] == i) {
        win = true;
        const int64_t o0 = a.offsets[i], o1 = a.offsets[i + 1];
        units = (o1 - o0 + P1M_UNIT - 1) / P1M_UNIT;
        if (o1 > o0) {
          const int top = a.info_slot[o1 - 1];  // maxPhase1bSlot: the run ascends (checked by the bid pass)
          ms = top > ms ? top : ms;
        }
        const int grp = a.grid_cols > 0 ? 0 : a.leader_group * g.num_groups + key / P1M_KEYS_PER_GROUP;
        const int bit = a.grid_cols > 0 ? key : key % P1M_KEYS_PER_GROUP;
        atomicOr(&a.held[(size_t)grp * 4 + (bit >> 6)], 1ull << (bit & 63));
      }
    }
    // the winners before this one, and their units
    const int wi = wave_incl_scan<ScanSum>(win ? 1 : 0);
    const int64_t ui = wave_incl_scan<ScanSum>(units);
    if (lane == 63) w_win[wave] = wi, w_units[wave] = ui;
    __syncthreads();
    int bw = c_win;
    int64_t bu = c_units;
    for (int w = 0; w < wave; ++w) bw += w_win[w], bu += w_units[w];
    if (win) a.win[bw + wi - 1] = i, a.unit0[bw + wi - 1] = bu + ui - units;
    __syncthreads();
    if (t == 1023) c_win = bw + wi, c_units = bu + ui;
    __syncthreads();
  }
  ms = block_reduce<ScanMax, 1024>(ms, w_max);
  if (t != 0) return;
  a.unit0[c_win] = c_units;
  const int64_t max_slot = ms > a.recover_slot ? ms : a.recover_slot;  // (recover_slot is -1 for MultiPaxos)
  // logger.check(maxSlot == -1 || slotSystem.leader(maxSlot) == groupIndex)
  if (max_slot != -1 && max_slot % L != a.leader_group) {
    a.ctl[P1M_STATE] = P1M_ST_NOT_OWNED, a.ctl[P1M_MAX] = (unsigned long long)(max_slot + 1);
    return;
  }
  const int64_t first = p1m_first_slot(L, a.leader_group, a.watermark);
  const int64_t count = p1m_count(L, first, max_slot);
  a.ctl[P1M_FIRST] = (unsigned long long)first;
  a.ctl[P1M_COUNT] = (unsigned long long)count;
  a.ctl[P1M_LIMIT] = (unsigned long long)(count < a.cap ? count : a.cap);
  a.ctl[P1M_MAX] = (unsigned long long)(max_slot + 1);
  a.ctl[P1M_NEXT] = (unsigned long long)p1m_next_classic_round(L, a.leader_group, max_slot);
  a.ctl[P1M_NWIN] = (unsigned long long)c_win;
  a.ctl[P1M_UNITS] = (unsigned long long)c_units;
}

__global__ void __launch_bounds__(256) k_p1m_clear(const P1mArgs a) {
  if (a.ctl[P1M_STATE] != P1M_ST_GO) return;
  const int64_t limit = (int64_t)a.ctl[P1M_LIMIT];
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < limit; j += (int64_t)gridDim.x * 256) a.table[j] = 0ull;
}

// The walk of the bid and write passes: wavefront / unit of P1M_UNIT records of one winning message.  WRITE = false:
// checks every record and bids; WRITE = true: the record that holds its slot's maximum writes.
template <bool WRITE>
__global__ void __launch_bounds__(256) k_p1m_walk(const Geom g, const P1mArgs a) {
  if (a.ctl[P1M_STATE] != P1M_ST_GO) return;
  if (WRITE && a.ctl[P1M_BAD] != 0) return;  // a bad record: nothing is written
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t units = (int64_t)a.ctl[P1M_UNITS], first = (int64_t)a.ctl[P1M_FIRST], limit = (int64_t)a.ctl[P1M_LIMIT];
  const int64_t max_slot = (int64_t)a.ctl[P1M_MAX] - 1;
  const int nwin = (int)a.ctl[P1M_NWIN];
  const int L = g.num_leader_groups;
  const int rows = a.grid_cols > 0 ? p1m_grid_rows(a.grid_cols, g.total) : 1;
  for (int64_t u = wave; u < units; u += nwaves) {
    // the last winner whose units start at or before u (a winner with an empty run has none and is stepped over)
    int lo = 0, hi = nwin - 1;
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (a.unit0[mid] <= u) lo = mid;
      else hi = mid - 1;
    }
    const int i = a.win[lo];
    const int64_t o0 = a.offsets[i], o1 = a.offsets[i + 1];
    const int64_t r0 = o0 + (u - a.unit0[lo]) * P1M_UNIT;
    const int64_t r1 = r0 + P1M_UNIT < o1 ? r0 + P1M_UNIT : o1;
    const int gi = a.group ? a.group[i] : 0;
    const int bit = a.grid_cols > 0 ? gi * a.grid_cols + a.acceptor[i] : a.acceptor[i];
    for (int64_t r = r0 + lane; r < r1; r += 64) {
      const int s = a.info_slot[r], vr = a.info_round[r];
      if (!WRITE) {
        const int prev = r > o0 ? a.info_slot[r - 1] : -1;
        if (s < 0 || s <= prev || vr < 0 || vr > MAX_ROUND) {
          atomicMax(&a.ctl[P1M_BAD], (unsigned long long)(0x7fffffff - i));
          continue;
        }
      }
      // a record below the watermark, of a slot another leader group owns, or beyond the range entered max_slot only
      if (s < first || s > max_slot) continue;
      const int64_t d = (int64_t)s - first;
      if (d % L != 0) continue;
      const int64_t j = d / L;
      if (j >= limit) continue;
      // phase1bs(slot % numAcceptorGroups) / phase1bs(acceptorGroupIndexBySlot(slot)); a grid: the row, or every row
      const bool mine = a.grid_cols > 0 ? (a.all_rows || gi == s % rows) : (gi == (s / L) % g.num_groups);
      if (!mine) continue;
      const unsigned long long key = ((unsigned long long)(vr + 1) << 8) | (unsigned long long)(255 - bit);
      if (!WRITE) {
        atomicMax(&a.table[j], key);
      } else if (a.table[j] == key) {
        a.safe_round[j] = vr, a.safe_value[j] = a.info_value[r];
      }
    }
  }
}

__global__ void __launch_bounds__(256) k_p1m_fill(const Geom g, const State st, const P1mArgs a) {
  const int state = (int)a.ctl[P1M_STATE];
  const bool bad = a.ctl[P1M_BAD] != 0;
  if (state == P1M_ST_GO && !bad) {
    const int64_t limit = (int64_t)a.ctl[P1M_LIMIT], first = (int64_t)a.ctl[P1M_FIRST];
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < limit; j += (int64_t)gridDim.x * 256) {
      a.out_slot[j] = (int32_t)(first + j * g.num_leader_groups);
      if (a.table[j] == 0ull) a.safe_round[j] = -1, a.safe_value[j] = -1 /*FPX_NOOP*/;
    }
  }
  if (blockIdx.x != 0) return;
  if (state == P1M_ST_GO && !bad && a.held_out)
    for (int w = threadIdx.x; w < g.ngroups * 4; w += 256) a.held_out[w] = a.held[w];
  if (threadIdx.x != 0) return;
  if (st.status[ST_ABORT] != 0) {  // the "apply nothing" state
    a.result[P1M_R_COMPLETE] = 0;
    return;
  }
  if (bad) {
    const int i = 0x7fffffff - (int)a.ctl[P1M_BAD];
    report_abort(st, 1 /*FPX_EINVAL*/, i, -1, a.msg_round[i]);
    return;
  }
  if (a.ctl[P1M_FUTURE] != 0) {
    const int i = 0x7fffffff - (int)a.ctl[P1M_FUTURE];
    report(st, 9 /*FPX_EFATAL_PROTOCOL*/, i, -1, a.msg_round[i]);  // logger.checkLt(phase1b.round, round); the others go on
  }
  if (state == P1M_ST_INCOMPLETE) {
    a.result[P1M_R_COMPLETE] = 0, a.result[P1M_R_DECIDED_AT] = -1;
  } else if (state == P1M_ST_NOT_OWNED) {
    report(st, 9 /*FPX_EFATAL_PROTOCOL*/, -1, (int)((int64_t)a.ctl[P1M_MAX] - 1), a.round);
  } else if (state == P1M_ST_GO) {
    const int64_t count = (int64_t)a.ctl[P1M_COUNT];
    a.result[P1M_R_COMPLETE] = 1, a.result[P1M_R_DECIDED_AT] = (int64_t)a.ctl[P1M_K];
    a.result[P1M_R_COUNT] = count, a.result[P1M_R_MAX_SLOT] = (int64_t)a.ctl[P1M_MAX] - 1;
    a.result[P1M_R_NEXT_SLOT] = (int64_t)a.ctl[P1M_NEXT], a.result[P1M_R_WRITTEN] = (int64_t)a.ctl[P1M_LIMIT];
    if (count > a.cap) report(st, 5 /*FPX_ECAPACITY*/, -1, -1, -1);  // the first cap entries are written all the same
  }
}

}  // namespace fpx
