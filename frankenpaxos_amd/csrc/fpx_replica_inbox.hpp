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
//   k_ri_hist, k_ri_hscan, k_ri_scatter   a stable LSD radix sort of the reads by that key, RI_RADIX_BITS bits per pass,
//                 in the shape of k_rs_hist / k_rs_scan / k_rs_scatter of fpx_epaxos.hip: per-tile digit counts,
//                 digit-major exclusive sums by one workgroup, and a scatter in which a key's place among the equal digits
//                 of its tile is its rank by position (ballots), never a cursor handed out by an atomic
//   k_ri_finish   hands the claim words back (INT_MAX: the Chosens' slots and all of [W0, W1)), commits the watermark,
//                 writes counts, and turns a bad index into the context's status
//
// Integer atomicMin / atomicMax and one count: no output depends on the order the hardware runs the threads in.
#pragma once
#include <limits.h>

#include "../../include/fpx_wire.h"
#include "fpx_replica_msgs.hpp"

namespace fpx {

constexpr int RI_TILE = 256;           // slots per tile of the executed-by scan (one per thread)
constexpr int RI_SCAN_THREADS = 1024;  // tiles per step of k_ri_tilescan: the span's second level is RI_TILE * RI_SCAN_THREADS slots
constexpr int RI_RADIX_BITS = 4;
constexpr int RI_RADIX = 1 << RI_RADIX_BITS;
constexpr int RI_SORT_TILE = 256;  // reads per tile of the sort (one per thread)

// words of ReplicaInbox::hdr
enum { RI_W0 = 0, RI_W1 = 1, RI_M = 2, RI_RAN = 3, RI_OK = 4, RI_HDR_WORDS = 8 };

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
  int32_t* hist;        // [RI_RADIX][tiles of the sort]
  int32_t* key[2];      // [n] each
  int32_t* val[2];      // [n] each
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
  int total;
  (void)block_rank(read, &total);
  if (threadIdx.x == 0) b.blk[blockIdx.x] = total;
  if (i == 0) b.mhdr[RM_NRANGES] = 0, b.mhdr[RM_JSTAR] = -1, b.hdr[RI_RAN] = 0;
}

// the largest of 256 threads' values, in every thread (one use per barrier pair: `w` is reused by the next call)
__device__ __forceinline__ int ri_block_max(int v, int* w) {
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const int o = __shfl_xor(v, k);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = w[0];
  for (int j = 1; j < 4; ++j) r = w[j] > r ? w[j] : r;
  __syncthreads();
  return r;
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
    const int m = ri_block_max(ri_c(b, w0 + tile * RI_TILE + (int)threadIdx.x, w1), w);
    if (threadIdx.x == 0) b.tmax[tile] = m;
  }
}

__global__ void __launch_bounds__(RI_SCAN_THREADS) k_ri_tilescan(const State st, const ReplicaInbox b) {
  __shared__ int wtot[RI_SCAN_THREADS / 64];
  __shared__ int carry;
  int w0, w1;
  const bool ok = ri_span(st, b, &w0, &w1);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) {
    carry = -1;
    b.hdr[RI_W0] = w0, b.hdr[RI_W1] = w1, b.hdr[RI_OK] = ok ? 1 : 0;
    b.hdr[RI_M] = ok && b.order ? b.rhdr[RM_NRANGES] : 0;
  }
  __syncthreads();
  const int ntiles = (w1 - w0 + RI_TILE - 1) / RI_TILE;
  for (int base = 0; base < ntiles; base += RI_SCAN_THREADS) {
    const int ti = base + t;
    int inc = ti < ntiles ? b.tmax[ti] : -1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d && o > inc) inc = o;
    }
    int excl = __shfl_up(inc, 1);  // the wavefront's earlier lanes
    if (lane == 0) excl = -1;
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; ++w) before = wtot[w] > before ? wtot[w] : before;
    if (ti < ntiles) b.tmax[ti] = excl > before ? excl : before;
    __syncthreads();
    if (t == RI_SCAN_THREADS - 1) carry = inc > before ? inc : before;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_ri_execby(const ReplicaInbox b) {
  __shared__ int wtot[4];
  const int w0 = b.hdr[RI_W0], w1 = b.hdr[RI_W1];
  const int ntiles = (w1 - w0 + RI_TILE - 1) / RI_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int s = w0 + tile * RI_TILE + (int)threadIdx.x;
    int inc = ri_c(b, s, w1);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d && o > inc) inc = o;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int before = b.tmax[tile];
    for (int w = 0; w < wave; ++w) before = wtot[w] > before ? wtot[w] : before;
    if (s < w1) b.claim[s] = inc > before ? inc : before;
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
  int total;
  const int q = b.blk[blockIdx.x] + block_rank(cls != 0, &total);
  __syncthreads();
  (void)block_rank(cls != 0 && exec >= 0, &total);
  if (!ok) return;  // a bad burst writes no output
  if (threadIdx.x == 0 && total != 0) atomicAdd(&b.hdr[RI_RAN], total);
  if (i >= b.n) return;
  b.exec_count[i] = exec, b.reply_slot[i] = reply;
  if (cls != 0) b.key[0][q] = exec >= 0 ? exec : b.S + 1, b.val[0][q] = i;
}

// ---- the reads by (exec_count, index): a stable LSD radix sort over the RI_M reads, tile <-> workgroup ----------------

struct RiSort {
  const int32_t* hdr;
  int32_t* hist;
  const int32_t *key_in, *val_in;
  int32_t *key_out, *val_out;
  int shift;
};

__global__ void __launch_bounds__(256) k_ri_hist(const RiSort a) {
  __shared__ int wc[4][RI_RADIX];
  const int m = a.hdr[RI_M], tiles = (m + RI_SORT_TILE - 1) / RI_SORT_TILE, tile = blockIdx.x;
  if (tile >= tiles) return;
  const int j = tile * RI_SORT_TILE + threadIdx.x;
  const int d = j < m ? (a.key_in[j] >> a.shift) & (RI_RADIX - 1) : -1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < RI_RADIX; ++v) {
    const int c = __popcll(__ballot(d == v));
    if (lane == 0) wc[wave][v] = c;
  }
  __syncthreads();
  if (threadIdx.x < RI_RADIX) {
    const int v = threadIdx.x;
    a.hist[(size_t)v * tiles + tile] = wc[0][v] + wc[1][v] + wc[2][v] + wc[3][v];
  }
}

// exclusive sums over the digit-major counts, one workgroup (k_rm_offsets with a length known on the device)
__global__ void __launch_bounds__(1024) k_ri_hscan(const RiSort a) {
  __shared__ int wtot[16];
  __shared__ int carry;
  const int m = a.hdr[RI_M], tiles = (m + RI_SORT_TILE - 1) / RI_SORT_TILE;
  const long long len = (long long)tiles * RI_RADIX;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) carry = 0;
  __syncthreads();
  for (long long base = 0; base < len; base += 1024) {
    const long long bi = base + t;
    const int v = bi < len ? a.hist[bi] : 0;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; ++w) before += wtot[w];
    if (bi < len) a.hist[bi] = before + inc - v;
    __syncthreads();
    if (t == 1023) carry = before + inc;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_ri_scatter(const RiSort a) {
  __shared__ int wc[4][RI_RADIX];
  const int m = a.hdr[RI_M], tiles = (m + RI_SORT_TILE - 1) / RI_SORT_TILE, tile = blockIdx.x;
  if (tile >= tiles) return;
  const int j = tile * RI_SORT_TILE + threadIdx.x;
  const bool valid = j < m;
  const int key = valid ? a.key_in[j] : 0, val = valid ? a.val_in[j] : 0;
  const int d = (key >> a.shift) & (RI_RADIX - 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 4 * RI_RADIX) (&wc[0][0])[threadIdx.x] = 0;
  __syncthreads();
  // the lanes of this wavefront with the same digit
  unsigned long long peers = __ballot(valid);
#pragma unroll
  for (int bit = 0; bit < RI_RADIX_BITS; ++bit) {
    const bool one = (d >> bit) & 1;
    const unsigned long long mk = __ballot(valid && one);
    peers &= one ? mk : ~mk;
  }
  const int rank = __popcll(peers & ((1ull << lane) - 1ull));
  if (valid && rank == 0) wc[wave][d] = __popcll(peers);
  __syncthreads();
  if (!valid) return;
  int at = a.hist[(size_t)d * tiles + tile] + rank;
  for (int w = 0; w < wave; ++w) at += wc[w][d];
  a.key_out[at] = key, a.val_out[at] = val;
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
