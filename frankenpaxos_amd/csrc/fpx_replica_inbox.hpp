// fpx_replica_inbox.hpp -- multipaxos.Replica's inbox for a BURST of messages in delivery order: handleChosen + executeLog
// (multipaxos/Replica.scala:572-590, 394-413) interleaved with the read path, handleDeferrableRead[s] / handleEventualRead[s]
// / processDeferredReads / executeRead (:455-529, 629-690), exactly as if the replica had handled the messages one by one --
// without the host reading anything between the passes.
//
// The Chosens are ingested as fpx_replica_msgs.hpp ingests them (its claim array and its apply / prep / scan kernels are
// used as they are; a MultiPaxos burst has no ranges).  What a read needs on top is the watermark AS IT STOOD at the read's
// position in the burst, W(i).  The claim word of a slot is "which message put this slot"; the running maximum of those
// words along the slot axis, from the old watermark W0 on, is "which message EXECUTED this slot": slot s runs in the
// executeLog of the last of the messages that put W0 .. s.
//
//   c[s] = -1 if slot s was in the log before the burst, else claim[s]           for s in [W0, W1)
//   M[s] = max(c[W0 .. s])                                                       non-decreasing
//   W(i) = W0 + #{s : M[s] < i}                                                  a binary search in M
//
//   k_ri_claim    thread / message: k_rm_claim without ranges, and the workgroup's number of reads (k_rm_offsets turns
//                 those into exclusive sums: a read's rank among the reads, in index order)
//   k_rm_apply, k_rm_prep, k_rm_scan   (fpx_replica_msgs.hpp) the puts, numChosen, and the first missing slot = W1
//   k_ri_tilemax  workgroup / tile of RI_TILE slots of [W0, W1): the tile's largest c
//   k_ri_tilescan one workgroup, RI_SCAN_THREADS tiles per step with a carry: the exclusive running maximum over the
//                 tiles; also freezes W0, W1 and the number of reads for the kernels behind it
//   k_ri_execby   workgroup / tile: M, written over the claim words of [W0, W1)
//   k_ri_reads    thread / message: exec_count and reply_slot, the sort key of a read (exec_count; num_slots + 1 for a read
//                 that stays deferred) at the read's rank, and the count of reads that ran
//   k_sort_count, k_sort_scan, k_sort_scatter   (fpx_burst_sort.hpp) a stable LSD radix sort of the reads by that key
//   k_ri_finish   hands the claim words back (INT_MAX: the Chosens' slots and all of [W0, W1)), commits the watermark,
//                 writes counts, and turns a bad index into the context's status
//
// Integer atomicMin / atomicMax and one count: no output depends on the order the hardware runs the threads in.
#pragma once
#include <limits.h>

#include "../../include/fpx_wire.h"
#include "fpx_burst_sort.hpp"
#include "fpx_replica_msgs.hpp"

namespace fpx {

constexpr int RI_TILE = BURST_TILE;    // slots per tile of the executed-by scan (one per thread)
constexpr int RI_SCAN_THREADS = 1024;  // tiles per step of k_ri_tilescan: the span's second level is RI_TILE * RI_SCAN_THREADS slots

// words of ReplicaInbox::hdr (RI_M is the sort's length word)
enum { RI_W0 = 0, RI_W1 = 1, RI_M = 2, RI_RAN = 3, RI_OK = 4, RI_HDR_WORDS = BURST_HDR_WORDS };

struct ReplicaInbox {
  int32_t n, S;
  const int32_t* kind;
  const int32_t* slot;
  const uint8_t* mask;  // null = all
  int32_t* claim;       // [S]  (ReplicaMsgs::claim)
  int32_t* mhdr;        // ReplicaMsgs::hdr of the Chosens' kernels: RM_NRANGES = 0, RM_JSTAR
  int32_t* rhdr;        // ReplicaMsgs::hdr of the reads' k_rm_offsets: RM_NRANGES = the number of reads
  int32_t* hdr;         // [RI_HDR_WORDS]
  int32_t* blk;         // [nblk]  reads per workgroup of k_ri_claim, then their exclusive sums
  int32_t* tmax;        // [ceil(S / RI_TILE)]  the tiles' maxima, then their exclusive running maxima
  int32_t *key0, *val0;  // [n]  the sort's input: the reads' keys and message indices, by rank
  int32_t *exec_count, *reply_slot, *order, *counts;
};

// 0: not a read (or masked out), 1: deferrable, 2: eventual
__device__ __forceinline__ int ri_read_class(const ReplicaInbox& b, int i) {
  if (b.mask && !b.mask[i]) return 0;
  switch (b.kind[i]) {
    case FPX_WIRE_READ_REQUEST:
    case FPX_WIRE_SEQUENTIAL_READ_REQUEST:
    case FPX_WIRE_READ_REQUEST_BATCH:
    case FPX_WIRE_SEQUENTIAL_READ_REQUEST_BATCH: return 1;
    case FPX_WIRE_EVENTUAL_READ_REQUEST:
    case FPX_WIRE_EVENTUAL_READ_REQUEST_BATCH: return 2;
    default: return 0;
  }
}

// [W0, W1): the slots this burst executes (empty when nothing is applied).  Valid between k_rm_scan and k_ri_finish.
__device__ __forceinline__ bool ri_span(const State& st, const ReplicaInbox& b, int* w0, int* w1) {
  const bool ok = st.status[ST_ABORT] == 0 && st.status[ST_MSG_BAD] == 0;
  const int lo = st.log_scalars[LG_WATERMARK];
  int hi = lo;
  if (ok && b.mhdr[RM_JSTAR] >= 0) {
    const int fm = st.log_scalars[LG_FIRST_MISSING];
    hi = fm > lo ? fm : lo;
  }
  *w0 = lo, *w1 = hi;
  return ok;
}

__global__ void __launch_bounds__(256) k_ri_claim(const Geom g, const State st, const ReplicaInbox b) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool read = false;
  if (i < b.n) {
    read = ri_read_class(b, i) != 0;
    if (!read && st.status[ST_ABORT] == 0 && (!b.mask || b.mask[i]) && b.kind[i] == FPX_WIRE_CHOSEN) {
      const int s = b.slot[i];
      if (s < 0 || s >= g.S)
        atomicMax(&st.status[ST_MSG_BAD], 0x7fffffff - i);
      else if (!st.log_present[s])
        atomicMin(&b.claim[s], i);
    }
  }
  __shared__ int wsum[4];
  int total;
  (void)block_rank(read, &total, wsum);
  if (threadIdx.x == 0) b.blk[blockIdx.x] = total;
  if (i == 0) b.mhdr[RM_NRANGES] = 0, b.mhdr[RM_JSTAR] = -1, b.hdr[RI_RAN] = 0;
}

__device__ __forceinline__ int ri_c(const ReplicaInbox& b, int s, int w1) {
  if (s >= w1) return -1;
  const int c = b.claim[s];
  return c == INT_MAX ? -1 : c;
}

__global__ void __launch_bounds__(256) k_ri_tilemax(const State st, const ReplicaInbox b) {
  __shared__ int w[4];
  int w0, w1;
  (void)ri_span(st, b, &w0, &w1);
  const int ntiles = (w1 - w0 + RI_TILE - 1) / RI_TILE;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m = block_reduce<ScanMax, 256>(ri_c(b, w0 + tile * RI_TILE + (int)threadIdx.x, w1), w);
    if (threadIdx.x == 0) b.tmax[tile] = m;
  }
}

__global__ void __launch_bounds__(RI_SCAN_THREADS) k_ri_tilescan(const State st, const ReplicaInbox b) {
  __shared__ int lds[SCAN_ARRAY_LDS(RI_SCAN_THREADS)];
  int w0, w1;
  const bool ok = ri_span(st, b, &w0, &w1);
  if (threadIdx.x == 0) {
    b.hdr[RI_W0] = w0, b.hdr[RI_W1] = w1, b.hdr[RI_OK] = ok ? 1 : 0;
    b.hdr[RI_M] = ok && b.order ? b.rhdr[RM_NRANGES] : 0;
  }
  (void)scan_array_excl<ScanMax, RI_SCAN_THREADS, 1>(b.tmax, (w1 - w0 + RI_TILE - 1) / RI_TILE, lds);
}

__global__ void __launch_bounds__(256) k_ri_execby(const ReplicaInbox b) {
  __shared__ int wtot[4];
  const int w0 = b.hdr[RI_W0], w1 = b.hdr[RI_W1];
  const int ntiles = (w1 - w0 + RI_TILE - 1) / RI_TILE;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int s = w0 + tile * RI_TILE + (int)threadIdx.x;
    const int c = ri_c(b, s, w1);
    const int before = block_excl_scan<ScanMax, 256>(c, b.tmax[tile], wtot);
    if (s < w1) b.claim[s] = c > before ? c : before;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_ri_reads(const ReplicaInbox b) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool ok = b.hdr[RI_OK] != 0;
  const int w0 = b.hdr[RI_W0], w1 = b.hdr[RI_W1];
  const int cls = i < b.n && ok ? ri_read_class(b, i) : 0;
  int exec = -2, reply = -2;  // not a read
  if (cls != 0) {
    const int r = cls == 1 ? b.slot[i] : -1;
    bool at_once = r < w0;
    if (!at_once && r < w1) at_once = b.claim[r] < i;  // M[r] < i: slot r ran before message i arrived
    if (at_once) {
      // W(i) = the first slot of [W0, W1) that a message behind i executes (M is non-decreasing)
      int lo = w0, hi = w1;
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (b.claim[mid] < i) lo = mid + 1; else hi = mid;
      }
      exec = lo, reply = lo - 1;
    } else if (r < w1) {
      exec = r + 1, reply = r - 1;  // released inside executeLog, before the watermark moves past r (Replica.scala:405-413, 526)
    } else {
      exec = -1, reply = -1;  // still deferred
    }
  }
  __shared__ int wsum[4];
  int total;
  const int q = b.blk[blockIdx.x] + block_rank(cls != 0, &total, wsum);
  __syncthreads();  // (wsum is used again)
  (void)block_rank(cls != 0 && exec >= 0, &total, wsum);
  if (!ok) return;  // a bad burst writes no output
  if (threadIdx.x == 0 && total != 0) atomicAdd(&b.hdr[RI_RAN], total);
  if (i >= b.n) return;
  b.exec_count[i] = exec, b.reply_slot[i] = reply;
  if (cls != 0) b.key0[q] = exec >= 0 ? exec : b.S + 1, b.val0[q] = i;
}

__global__ void __launch_bounds__(256) k_ri_finish(const Geom g, const State st, const ReplicaInbox b) {
  const int step = gridDim.x * 256, tid = blockIdx.x * 256 + threadIdx.x;
  // the claim words of the burst: the Chosens' slots (checked again: a bad burst keeps its bad slots) ...
  for (int i = tid; i < b.n; i += step) {
    if ((b.mask && !b.mask[i]) || b.kind[i] != FPX_WIRE_CHOSEN) continue;
    const int s = b.slot[i];
    if (s >= 0 && s < g.S) b.claim[s] = INT_MAX;
  }
  // ... and the executed span, which k_ri_execby wrote M over
  const int w0 = b.hdr[RI_W0], w1 = b.hdr[RI_W1];
  for (int s = w0 + tid; s < w1; s += step) b.claim[s] = INT_MAX;
  if (tid != 0) return;
  // (no other thread of this grid reads the status words or the scalars)
  const int32_t bad = st.status[ST_MSG_BAD];
  st.status[ST_MSG_BAD] = 0;
  if (bad != 0) {
    const int i = 0x7fffffff - bad;
    report_abort(st, 1 /*FPX_EINVAL*/, i, b.slot[i], -1);
  } else if (b.hdr[RI_OK] != 0) {
    if (w1 > st.log_scalars[LG_WATERMARK]) st.log_scalars[LG_WATERMARK] = w1;
    b.counts[0] = b.rhdr[RM_NRANGES], b.counts[1] = b.hdr[RI_RAN], b.counts[2] = w0, b.counts[3] = w1;
  }
}

}  // namespace fpx
