// fpx_replica_msgs.hpp -- mencius.Replica.handleChosen + handleChosenNoopRange + executeLog (mencius/Replica.scala:402-420,
// 464-485, 331-371) for a BURST of messages in delivery order, Chosens and ChosenNoopRanges interleaved, exactly as if the
// replica had handled them one by one -- without the host reading anything between the passes.
//
// What makes the one-by-one result depend on order: a slot is put by the FIRST message that reaches it; a range stops (and
// does not run executeLog) at the first of its slots that is in the log already -- put before the burst, by an earlier
// Chosen of the burst, or by an earlier range of its residue class mod L that got that far; a redundant Chosen does not
// run executeLog either, so the watermark is the prefix of the log AS IT STOOD after the last message that did.
//
// `claim` ([S] int32, 4 B per slot, INT_MAX between calls, allocated by the first call): the index of the message that
// puts the slot in this burst.  Only slots that are absent before the burst are ever claimed, so afterwards
// claim[s] != INT_MAX  <=>  slot s was put by message claim[s] of this burst.
//
//   k_rm_claim   thread / message: range checks (the lowest bad index goes to the status words; a bad burst applies
//                nothing); a Chosen of an absent slot bids atomicMin(claim[slot], i) -- the lower index wins; the
//                workgroup's number of ranges is left for the compaction
//   k_rm_offsets one workgroup: exclusive sums of those numbers, and the number of ranges m
//   k_rm_list    thread / message: the ranges' message indices in message order (a burst has hundreds, not millions)
//   k_rm_walk    one workgroup per residue class: walks the class's ranges in message order, 1024 positions at a time;
//                range i stops at the first position with log_present || claim < i and puts Noop (claim = i) before it.
//                Earlier ranges of the class are seen through what they put (the workgroup's own stores, behind a
//                barrier); classes share no slot.  A later Chosen's bid is overwritten: that Chosen is then redundant
//   k_rm_apply   grid-stride over the messages: Chosen i puts iff claim[slot] == i; per workgroup the count of puts, the
//                largest key and the largest index of a Chosen that was put (one triple per workgroup, no same-address
//                atomics: fpx_kernels.hpp, k_log_ingest)
//   k_rm_prep    one workgroup: folds the triples and the ranges' results into numChosen, largestKey and j*, the largest
//                index of a message that reached executeLog (a Chosen that was put, a range that ran to its end)
//   k_rm_scan    k_log_scan with "present" = in the log and (not put by this burst, or put by a message <= j*); does
//                nothing when no message reached executeLog
//   k_rm_finish  commits the watermark (only if j* exists), hands the claim words of the burst back (INT_MAX), and turns a
//                bad index into the context's status -- also when nothing was applied
//
// Integer atomics (min / max) only: the result does not depend on the order the hardware runs the threads in.
//
// The class walk reads the log at stride L.  A slot-major sweep for bursts with one range per class (thread <-> slot,
// coalesced) was not built.
#pragma once
#include <limits.h>

#include "fpx_kernels.hpp"
#include "fpx_scan.hpp"
#include "fpx_scratch.hpp"
#include "fpx_tally_msgs.hpp"

namespace fpx {

// words of ReplicaMsgs::hdr
enum { RM_NRANGES = 0, RM_JSTAR = 1, RM_HDR_WORDS = BURST_HDR_WORDS };
constexpr int RM_WALK_THREADS = 1024;

struct ReplicaMsgs {
  int32_t n, nblk, nparts;
  int32_t chosen_kind, range_kind;  // FPX_WIRE_CHOSEN, FPX_WIRE_CHOSEN_NOOP_RANGE
  const int32_t* kind;
  const int32_t* slot;
  const int32_t* slot_end;
  const int32_t* value;
  const uint8_t* mask;  // null = all
  int32_t* claim;       // [S]
  int32_t* hdr;         // [RM_HDR_WORDS]
  int32_t* parts;       // [nparts][3]  count, largest key, largest index put
  int32_t* blk;         // [nblk]  ranges per workgroup of k_rm_claim, then their exclusive sums
  int32_t* list;        // [n]  message index of the q-th range
  int32_t* res;         // [n]  the q-th range: c >= 0: ran to its end after c puts; c < 0: stopped after -1 - c puts
};

__device__ __forceinline__ int rm_kind(const ReplicaMsgs& b, int i) {
  return (!b.mask || b.mask[i]) ? b.kind[i] : -1;
}

__global__ void __launch_bounds__(256) k_rm_claim(const Geom g, const State st, const ReplicaMsgs b) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool range = false;
  if (i < b.n) {
    const int k = rm_kind(b, i);
    range = k == b.range_kind;
    if (st.status[ST_ABORT] == 0) {
      const int s = b.slot[i];
      if (k == b.chosen_kind) {
        if (s < 0 || s >= g.S)
          atomicMax(&st.status[ST_MSG_BAD], 0x7fffffff - i);
        else if (!st.log_present[s])
          atomicMin(&b.claim[s], i);
      } else if (range && (s < 0 || b.slot_end[i] > g.S)) {
        atomicMax(&st.status[ST_MSG_BAD], 0x7fffffff - i);
      }
    }
  }
  __shared__ int wsum[4];
  int total;
  (void)block_rank(range, &total, wsum);
  if (threadIdx.x == 0) b.blk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(1024) k_rm_offsets(const ReplicaMsgs b) {
  __shared__ int lds[SCAN_ARRAY_LDS(1024)];
  const int total = scan_array_excl<ScanSum, 1024, 1>(b.blk, b.nblk, lds);
  if (threadIdx.x == 0) b.hdr[RM_NRANGES] = total, b.hdr[RM_JSTAR] = -1;
}

__global__ void __launch_bounds__(256) k_rm_list(const ReplicaMsgs b) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool range = i < b.n && rm_kind(b, i) == b.range_kind;
  __shared__ int wsum[4];
  int total;
  const int at = b.blk[blockIdx.x] + block_rank(range, &total, wsum);
  if (range) b.list[at] = i, b.res[at] = -1;  // "stopped after 0 puts" until k_rm_walk says otherwise
}

// workgroup c <-> the ranges whose start is congruent to c mod L
__global__ void __launch_bounds__(RM_WALK_THREADS) k_rm_walk(const Geom g, const State st, const ReplicaMsgs b) {
  __shared__ int s_stop[3];
  if (st.status[ST_ABORT] != 0 || st.status[ST_MSG_BAD] != 0) return;
  const int L = g.num_leader_groups, t = threadIdx.x;
  if (t < 3) s_stop[t] = INT_MAX;
  __syncthreads();
  const int m = b.hdr[RM_NRANGES];
  int it = 0;  // which of the three stop words this step uses: the one after next is cleared meanwhile
  for (int q = 0; q < m; ++q) {
    const int i = b.list[q];
    const int start = b.slot[i], end = b.slot_end[i];
    if (start % L != (int)blockIdx.x) continue;
    const int count = start < end ? (int)(((long long)end - start + L - 1) / L) : 0;
    int stop = INT_MAX;
    for (int base = 0; base < count && stop == INT_MAX; base += RM_WALK_THREADS, it = it == 2 ? 0 : it + 1) {
      const int k = base + t;
      const size_t s = (size_t)start + (size_t)k * L;
      if (k < count && (st.log_present[s] || b.claim[s] < i)) atomicMin(&s_stop[it], k);
      __syncthreads();
      stop = s_stop[it];
      if (t == 0) s_stop[it == 0 ? 2 : it - 1] = INT_MAX;
      if (k < count && k < stop) {
        b.claim[s] = i;
        st.log_value[s] = -1;  // Noop
        st.log_present[s] = 1;
      }
    }
    if (t == 0) b.res[q] = stop == INT_MAX ? count : -1 - stop;
    __syncthreads();  // the next range of the class sees what this one put
  }
}

__global__ void __launch_bounds__(256) k_rm_apply(const Geom g, const State st, const ReplicaMsgs b) {
  if (st.status[ST_ABORT] != 0 || st.status[ST_MSG_BAD] != 0) return;
  __shared__ int w_cnt[4], w_top[4], w_idx[4];
  int cnt = 0, top = -1, idx = -1;
  const int step = gridDim.x * 256;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < b.n; i += step) {
    if (rm_kind(b, i) != b.chosen_kind) continue;
    const int s = b.slot[i];
    if (b.claim[s] == i) {
      st.log_value[s] = b.value[i];
      st.log_present[s] = 1;
      ++cnt;
      top = s > top ? s : top;
      idx = i;  // increasing along the loop
    }
  }
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    cnt += __shfl_xor(cnt, k);
    const int o = __shfl_xor(top, k), p = __shfl_xor(idx, k);
    top = o > top ? o : top;
    idx = p > idx ? p : idx;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) w_cnt[w] = cnt, w_top[w] = top, w_idx[w] = idx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 1; j < 4; ++j) {
      cnt += w_cnt[j];
      top = w_top[j] > top ? w_top[j] : top;
      idx = w_idx[j] > idx ? w_idx[j] : idx;
    }
    b.parts[3 * blockIdx.x] = cnt, b.parts[3 * blockIdx.x + 1] = top, b.parts[3 * blockIdx.x + 2] = idx;
  }
}

__global__ void __launch_bounds__(256) k_rm_prep(const Geom g, const State st, const ReplicaMsgs b) {
  __shared__ int s_cnt[256], s_top[256], s_idx[256];
  if (st.status[ST_ABORT] != 0 || st.status[ST_MSG_BAD] != 0) return;
  int c = 0, t = -1, x = -1;
  for (int j = threadIdx.x; j < b.nparts; j += 256) {
    c += b.parts[3 * j];
    const int o = b.parts[3 * j + 1], p = b.parts[3 * j + 2];
    t = o > t ? o : t;
    x = p > x ? p : x;
  }
  const int m = b.hdr[RM_NRANGES], L = g.num_leader_groups;
  for (int q = threadIdx.x; q < m; q += 256) {
    const int r = b.res[q], i = b.list[q];
    const int puts = r >= 0 ? r : -1 - r;
    c += puts;
    if (puts > 0) {
      const int o = b.slot[i] + (puts - 1) * L;  // BufferMap.largestKey
      t = o > t ? o : t;
    }
    if (r >= 0 && i > x) x = i;
  }
  s_cnt[threadIdx.x] = c, s_top[threadIdx.x] = t, s_idx[threadIdx.x] = x;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int j = 1; j < 256; ++j) {
    c += s_cnt[j];
    t = s_top[j] > t ? s_top[j] : t;
    x = s_idx[j] > x ? s_idx[j] : x;
  }
  st.log_scalars[LG_NUM_CHOSEN] += c;
  if (t > st.log_scalars[LG_LARGEST]) st.log_scalars[LG_LARGEST] = t;
  b.hdr[RM_JSTAR] = x;
  const int hi = st.log_scalars[LG_LARGEST] + 1;
  st.log_scalars[LG_FIRST_MISSING] = hi < g.S ? hi : g.S;
}

__global__ void __launch_bounds__(256) k_rm_scan(const Geom g, const State st, const ReplicaMsgs b) {
  if (st.status[ST_ABORT] != 0 || st.status[ST_MSG_BAD] != 0) return;
  const int jstar = b.hdr[RM_JSTAR];
  if (jstar < 0) return;  // no message of the burst reached executeLog
  const int lo = st.log_scalars[LG_WATERMARK];
  const int hi0 = st.log_scalars[LG_LARGEST] + 1;
  const int hi = hi0 < g.S ? hi0 : g.S;
  const int stride = gridDim.x * blockDim.x;
  int mine = 0x7fffffff;
  for (int s = lo + blockIdx.x * blockDim.x + threadIdx.x; s < hi; s += stride) {
    if (s >= __hip_atomic_load(&st.log_scalars[LG_FIRST_MISSING], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    bool there = st.log_present[s] != 0;
    if (there) {
      const int w = b.claim[s];  // put by a message behind j*: not in the log yet when executeLog last ran
      there = w == INT_MAX || w <= jstar;
    }
    if (!there) {
      mine = s;
      break;
    }
  }
  wave_atomic_min(&st.log_scalars[LG_FIRST_MISSING], mine);
}

__global__ void __launch_bounds__(256) k_rm_finish(const Geom g, const State st, const ReplicaMsgs b) {
  const int L = g.num_leader_groups, step = gridDim.x * 256, tid = blockIdx.x * 256 + threadIdx.x;
  // the claim words of the burst: the Chosens' slots (checked again: a bad burst keeps its bad slots) ...
  for (int i = tid; i < b.n; i += step) {
    if (rm_kind(b, i) != b.chosen_kind) continue;
    const int s = b.slot[i];
    if (s >= 0 && s < g.S) b.claim[s] = INT_MAX;
  }
  // ... and what the ranges put (nothing, when k_rm_walk did not run)
  const int m = b.hdr[RM_NRANGES];
  for (int q = 0; q < m; ++q) {
    const int r = b.res[q];
    const int puts = r >= 0 ? r : -1 - r;
    if (puts == 0) continue;
    const int start = b.slot[b.list[q]];
    for (int k = tid; k < puts; k += step) b.claim[(size_t)start + (size_t)k * L] = INT_MAX;
  }
  if (tid != 0) return;
  // (no other thread of this grid reads the status words)
  const int32_t bad = st.status[ST_MSG_BAD];
  st.status[ST_MSG_BAD] = 0;
  if (bad != 0) {
    const int i = 0x7fffffff - bad;
    report_abort(st, 1 /*FPX_EINVAL*/, i, b.slot[i], -1);
  } else if (st.status[ST_ABORT] == 0 && b.hdr[RM_JSTAR] >= 0) {
    const int fm = st.log_scalars[LG_FIRST_MISSING];
    if (fm > st.log_scalars[LG_WATERMARK]) st.log_scalars[LG_WATERMARK] = fm;
  }
}

}  // namespace fpx
