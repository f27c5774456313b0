// fpx_epaxos.hip -- EPaxos on gfx950: K5 the pre-accept tick (fast path test + slow-path
// union), K6 Prepare / Accept on the command log, K7 handlePreAccept in full (ballots, Nacks, re-sent replies).
//
// K5:
// Per replica the conflict scan is a segmented (by key) exclusive prefix-max over the tick's commands
// in that replica's delivery order, on n-wide watermark vectors (util/TopOne.scala): data-parallel as
//   1. k_epx_keys      scatter every command to its position in the replica's delivery order (rank is a
//                      permutation)
//   2. k_rs_hist / k_rs_scan / k_rs_scatter   stable LSD radix sort (digits of up to 11 bits: 1024 keys are one pass)
//                      of all replicas' sequences at once, on the key bits only (stable => (key, delivery
//                      order)); a workgroup sorts its tile of 4096 elements into LDS (equal digits ranked with
//                      one ballot per digit bit and 64 elements) and writes it out as runs per digit
//   3. k_epx_segments_from_totals  [lo, hi) of every (replica, key) segment from the sort's digit totals (one pass:
//                      digit == key); k_epx_segments (binary search) when the key took several passes
//   4. k_epx_key<N>    one persistent workgroup per CU working through the keys whose commands fit its LDS tables: the scans of all
//                      replicas' segments of the key (steps 4a / 5a below in one kernel, the conflict rows never
//                      leave the chip); the other keys go through
//   4a. k_epx_scan<N>  one wavefront per (replica, key): 64 commands per step, wave-level max-scan of the
//                      2N watermark columns on the DPP network (row_shr / row_bcast), carry in registers;
//                      leader and get/set travel in the sort key's spare bits, the answer row is one aligned
//                      16- / 32-byte store
//   5a. k_epx_decide<N> one thread per command: PreAcceptOk = local conflicts U leader's deps; fast path iff
//                      the n-2 answers agree (Util.popularItems), else the union (preAcceptingSlowPath)
//   6. k_epx_commit    every replica's conflict index learns the tick's instances (commit ->
//                      updateConflictIndex): elementwise max with what the scans saw of this tick (every
//                      command is scanned by its leader's replica at least, so the max over replicas is the
//                      whole tick -- no atomics anywhere)
// Integer max / compare only: HBM- and latency-bound, no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/fpx.h"
#include "../../include/fpx_wire.h"
#include "fpx_host.hpp"
#include "fpx_scan.hpp"

using namespace fpx;

namespace {

// cmdLog entry kinds (epaxos/Replica.scala:303-330)
enum { CL_NONE = 0, CL_NO_COMMAND = 1, CL_PRE_ACCEPTED = 2, CL_ACCEPTED = 3, CL_COMMITTED = 4 };

struct EpxState {
  int n, num_keys;
  int32_t* gets;  // [n][num_keys][n]
  int32_t* sets;  // [n][num_keys][n]
  int32_t* status;
  // the command log of every replica (Replica.scala:440 cmdLog) for the instances (leader, number < num_instances):
  // entry kind, ballot, voteBallot (ballots encoded ordering * 8 + replicaIndex, nullBallot = -1), triple id
  int num_instances;
  uint8_t* cl_status;   // [n][n * num_instances]
  int32_t* cl_ballot;
  int32_t* cl_vote;
  int32_t* cl_triple;
  int32_t* cl_deps;     // [n * n * num_instances][n] the triple's dependencies as watermarks (column 0 = -1: the entry
                        // was written by an Accept, which names its triple by id only)
  int32_t* cl_dend;     // [n * n * num_instances] end of the explicit values number + 1 .. end - 1 of the own-leader column
  int32_t* largest;     // [n]  Replica.largestBallot, encoded
  uint32_t* cl_stamp;   // [n * num_instances]  run id: instances of one batch must be distinct
};

struct EpxBatch {
  int m;
  const int32_t* leader;
  const int32_t* number;
  const int32_t* key;
  const uint8_t* is_set;
  const uint8_t* resp_mask;
  const uint8_t* seen_mask;  // replicas that process the PreAccept (null = resp_mask)
  const int32_t* rank;   // [n][m]
  const int32_t* triple; // [m] or null: the CommandTriple's id, recorded in the command log
  uint2* kv;             // [n][m] in the replica's delivery order: x = key | is_set << 27 | leader << 28
                         // (only the key bits are sorted on), y = message index
  uint2* kv_sorted;      // [n][m]
  int32_t* tick;         // [n][num_keys][2][n] the puts (gets, sets) replica r's scan saw for the key this tick
  int32_t* seg;          // [n][num_keys][2]
  int32_t* conf;         // [m][n][NP] local conflicts of replica r for message i; rows padded to NP = 4 (n = 3)
                         // or 8 ints so a row is one aligned 16- / 32-byte store
  uint8_t* fast;
  int32_t* deps;
  int32_t* leader_deps;
  int32_t* own_values_end;  // [m][2]: explicit values of the own-leader column of deps / leader_deps (0 = none)
  int2* meta;               // [m] or null: (number, resp_mask | seen_mask << 8) of message i, ONE gather for k_epx_key
  uint8_t* fused;           // [num_keys] or null: 1 = k_epx_key did the key's scan and decisions on chip
  int32_t* unfused;         // number of keys left to k_epx_scan / k_epx_decide (null: all of them)
  unsigned long long* census;  // [EPX_CD_WORDS] the first form's device words of fpx_epx_tick_census, or null
};

// the device's words of fpx_epx_tick_census (include/fpx.h: FPX_EPX_CENSUS_SORT_BUCKET1 ... in this order).  The first
// EPX_CD_SORTS are the sort routes of k_epx_key2 (fpx_epaxos_kp.hpp), tallied in LDS per workgroup and kept in the second
// form's own control buffer (launch_kp); EPX_CD_LONG_WAY is the first form's, in the context's census buffer
constexpr int EPX_CD_BUCKET1 = 0, EPX_CD_RADIX1 = 2, EPX_CD_SORTS = 5;  // (bucket attempts 1, 2; radix sorts of 1, 2, 3 passes)
constexpr int EPX_CD_LONG_WAY = 5, EPX_CD_WORDS = 8;

constexpr uint32_t EPX_KEY_MASK = (1u << 27) - 1u;
constexpr int EPX_SET_SHIFT = 27, EPX_LEADER_SHIFT = 28;
template <int N> struct ConfRow { static constexpr int NP = N <= 4 ? 4 : 8; };

// wave64 inclusive max-scan / shifts on the DPP network (values are >= 0, so 0 is the identity): 4 row_shr
// steps inside each row of 16, then row_bcast:15 / row_bcast:31 carry the row totals across rows
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp0(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
// The own-leader column of an instance (leader L, number x) is {0 .. cover-1} \ {x} (dependencies.subtractOne(instance),
// Replica.scala:582): an IntPrefixSet with (watermark cover, no values) if cover <= x, (watermark x, no values) if
// cover == x + 1, else (watermark x, values x+1 .. cover-1), reported as values_end = cover.  Unions are max of covers.
__device__ __forceinline__ void own_column(int cover, int x, int* watermark, int* values_end) {
  *watermark = cover <= x ? cover : x;
  *values_end = cover > x + 1 ? cover : 0;
}
__device__ __forceinline__ int wave_incl_max(int v) {
  v = imax(v, dpp0<0x111, 0xF>(v));  // row_shr:1
  v = imax(v, dpp0<0x112, 0xF>(v));  // row_shr:2
  v = imax(v, dpp0<0x114, 0xF>(v));  // row_shr:4
  v = imax(v, dpp0<0x118, 0xF>(v));  // row_shr:8
  // row_bcast:15 -> rows 1, 3, then row_bcast:31 -> rows 2, 3.  Written out: from update_dpp + max the compiler makes a
  // v_mov, a v_mov_dpp and the v_max per step (it does not fold a move under a partial row mask), 6 instructions where 2
  // do -- and this scan is a third of the K5 key kernel's vector instructions.  The s_nops are the two wait states
  // between a VALU write and a DPP read of the same register, which the hazard recogniser does not see through asm.
  asm("s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_i32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"
      : "+v"(v));
  return v;
}
__device__ __forceinline__ int wave_shr1(int v) { return dpp0<0x138, 0xF>(v); }  // lane 0 gets 0

__device__ __forceinline__ void epx_report(int32_t* status, int code, int index) {
  if (atomicCAS(&status[0], 0, code) == 0) status[1] = index;
}

__global__ void __launch_bounds__(256) k_epx_keys(const EpxState st, const EpxBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  if (i == 0 && b.unfused) *b.unfused = 0;
  const int n = st.n;
  const int L = b.leader[i], k = b.key[i];
  const unsigned mask = b.resp_mask[i];
  bool ok = L >= 0 && L < n && b.number[i] >= 0 && k >= 0 && k < st.num_keys;
  ok = ok && !((mask >> (ok ? L : 0)) & 1u) && (mask >> n) == 0 && (int)__popc(mask) == n - 2;
  const unsigned seen = b.seen_mask ? b.seen_mask[i] : mask;
  ok = ok && (mask & ~seen) == 0 && !((seen >> (ok ? L : 0)) & 1u) && (seen >> n) == 0;
  if (b.meta) b.meta[i] = make_int2(b.number[i], (int)(mask | (seen << 8)));
  for (int r = 0; r < n; ++r) {
    const int p = b.rank[(size_t)r * b.m + i];
    ok = ok && p >= 0 && p < b.m;
    const bool part = ok && (r == L || ((seen >> r) & 1u));
    // rank is a permutation: scattering to position p lays the tick out in replica r's delivery order;
    // a stable sort by key alone then yields (key, delivery order).  Non-participants sort last.
    if (ok) {
      const uint32_t flags = ((uint32_t)(b.is_set[i] ? 1 : 0) << EPX_SET_SHIFT) | ((uint32_t)L << EPX_LEADER_SHIFT);
      b.kv[(size_t)r * b.m + p] = make_uint2((part ? (uint32_t)k : (uint32_t)st.num_keys) | flags, (uint32_t)i);
    }
  }
  if (ok && st.num_instances > 0) {
    // this tick-at-once form covers handlePreAccept's `cmdLog.get(instance) == None` branch only: an instance a
    // participating replica already knows is rejected (nothing of the tick is applied)
    ok = b.number[i] < st.num_instances;
    const unsigned part = (b.seen_mask ? b.seen_mask[i] : mask) | (1u << L);
    for (int r = 0; ok && r < n; ++r)
      if (((part >> r) & 1u) && st.cl_status[((size_t)r * n + L) * st.num_instances + b.number[i]] != CL_NONE) ok = false;
  }
  if (!ok) {
    epx_report(st.status, FPX_EINVAL, i);
    return;
  }
}

// ---- stable LSD radix sort, digits of up to 11 bits, all replicas in one launch (blockIdx.y = replica) --------
// 1024 keys (+ the non-participants' bucket) are ONE pass.  A workgroup owns a tile of RS_TILE consecutive elements,
// wavefront w the w-th quarter of it, walked 64 at a time in lane order: ranking equal digits by (tile, wavefront,
// step, lane) is the input order, so the sort is stable.  The tile is first sorted into LDS and leaves as runs of
// consecutive elements per digit (a scatter straight from the ranking loop wrote 8 bytes per lane and instruction
// to 64 different places: two such passes were 66 us for 5 M pairs, profiles/r02_epaxos_kernel_stats.csv).
constexpr int RS_ITEMS = 16;                // 64-element steps per wavefront (tile = 4 x that); 8 / 16 / 32 measured
                                            // 0.317 / 0.302 / 0.322 ms per tick
constexpr int RS_TILE = 256 * RS_ITEMS;     // elements per workgroup tile
constexpr int RS_MAXW = 11;                 // widest digit
constexpr int RS_MAXB = 1 << RS_MAXW;
constexpr int RS_SW = 8;                    // wavefronts of a scatter workgroup: 4 / 8 / 16 measured 0.259 / 0.240 / 0.255 ms per tick
constexpr size_t RS_SCATTER_LDS = (size_t)RS_TILE * 8 + (size_t)RS_SW * (RS_MAXB / 2) * 4 + (size_t)RS_MAXB * 4 + 64;

struct RsArgs {
  int m, tiles, shift;
  int width;       // digit bits of this pass (<= 11): the key bits are split evenly over the passes
  const uint2* src;  // [n][m] (key word, payload)
  uint2* dst;
  uint32_t* hist;  // [n][tiles][B] per-tile digit counts -> exclusive offsets of the tile within the digit
  uint32_t* tot;   // [n][B] digit totals
  // first pass only (else null): rank[n][m] and the status words, to check that every replica's rank really is
  // a permutation -- position p must hold a message i < m of THIS tick with rank[r][i] == p.  A position no
  // message was scattered to still holds an older tick's pair, which fails one of the two tests (if its i had
  // rank p now, i would have written p).
  const int32_t* rank;
  int32_t* status;
};

__global__ void __launch_bounds__(256) k_rs_hist(const RsArgs a) {
  __shared__ uint32_t h[RS_MAXB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = blockIdx.y, tile = blockIdx.x;
  const int B = 1 << a.width;
  for (int j = threadIdx.x; j < B; j += 256) h[j] = 0;
  __syncthreads();
  const uint2* k = a.src + (size_t)r * a.m;
  const int first = tile * RS_TILE + w * (RS_TILE / 4);
  uint32_t x[RS_ITEMS];
  if (a.rank) {
    uint32_t y[RS_ITEMS];
#pragma unroll
    for (int it = 0; it < RS_ITEMS; ++it) {
      const int idx = first + it * 64 + lane;
      const uint2 e = idx < a.m ? k[idx] : make_uint2(0xffffffffu, 0u);
      x[it] = e.x, y[it] = e.y;
    }
    int bad = -1;
#pragma unroll
    for (int it = 0; it < RS_ITEMS; ++it) {
      const int idx = first + it * 64 + lane;
      if (idx < a.m && (y[it] >= (uint32_t)a.m || a.rank[(size_t)r * a.m + y[it]] != idx)) bad = idx;
    }
    if (bad >= 0) epx_report(a.status, FPX_EINVAL, -1);
  } else {
#pragma unroll
    for (int it = 0; it < RS_ITEMS; ++it) {  // all the loads in flight before the first LDS atomic
      const int idx = first + it * 64 + lane;
      x[it] = idx < a.m ? k[idx].x : 0xffffffffu;
    }
  }
#pragma unroll
  for (int it = 0; it < RS_ITEMS; ++it)
    if (first + it * 64 + lane < a.m) atomicAdd(&h[(x[it] >> a.shift) & (B - 1)], 1u);
  __syncthreads();
  uint32_t* out = a.hist + ((size_t)r * a.tiles + tile) * B;
  for (int j = threadIdx.x; j < B; j += 256) out[j] = h[j];
}

// exclusive scan of every digit's per-tile counts, in place: 64 digits x 4 parts of the tiles per workgroup (the 64
// lanes of a wavefront read neighbouring digits of one tile: coalesced); a part sums its tiles, the parts' sums are
// combined through LDS, then each part rewrites its tiles (second read: L2)
__global__ void __launch_bounds__(256) k_rs_scan(const RsArgs a) {
  __shared__ uint32_t part_sum[4][64];
  const int B = 1 << a.width, lane = threadIdx.x & 63, part = threadIdx.x >> 6, r = blockIdx.y;
  const int d = blockIdx.x * 64 + lane;
  const int per = (a.tiles + 3) / 4, t0 = part * per, t1 = min(a.tiles, t0 + per);
  uint32_t* col = a.hist + (size_t)r * a.tiles * B + d;
  uint32_t sum = 0;
  if (d < B) {
    int t = t0;
    for (; t + 8 <= t1; t += 8) {
      uint32_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = col[(size_t)(t + j) * B];
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[j];
    }
    for (; t < t1; ++t) sum += col[(size_t)t * B];
  }
  part_sum[part][lane] = sum;
  __syncthreads();
  if (d >= B) return;
  uint32_t run = 0;
  for (int p2 = 0; p2 < part; ++p2) run += part_sum[p2][lane];
  if (part == 3) a.tot[r * B + d] = run + sum;
  int t = t0;
  for (; t + 8 <= t1; t += 8) {
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = col[(size_t)(t + j) * B];
#pragma unroll
    for (int j = 0; j < 8; ++j) col[(size_t)(t + j) * B] = run, run += v[j];
  }
  for (; t < t1; ++t) {
    const uint32_t v = col[(size_t)t * B];
    col[(size_t)t * B] = run, run += v;
  }
}

// 8 wavefronts per tile, each ranks an eighth of it (8 steps of 64): twice the wavefronts per CU of a 4-wavefront
// version at the same LDS, and half the serial chain per wavefront.  The per-wavefront digit counters / cursors are
// 16 bits wide (a tile has 4096 elements), two digits per LDS word, updated with 32-bit LDS atomics on the half.
constexpr int RS_SITEMS = RS_TILE / (64 * RS_SW);
static_assert(RS_TILE <= 65535 && RS_TILE % (64 * RS_SW) == 0, "16-bit cursors; whole steps");

__global__ void __launch_bounds__(64 * RS_SW) k_rs_scatter(const RsArgs a) {
  extern __shared__ __align__(16) unsigned char rs_smem[];
  uint2* sorted = reinterpret_cast<uint2*>(rs_smem);                       // the tile in digit order
  uint32_t* cnt = reinterpret_cast<uint32_t*>(sorted + RS_TILE);           // [RS_SW][B / 2] packed 16-bit count, then cursor
  int32_t* gpos = reinterpret_cast<int32_t*>(cnt + RS_SW * (RS_MAXB / 2)); // digit -> (global position - position in tile)
  uint32_t* sh = reinterpret_cast<uint32_t*>(gpos + RS_MAXB);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = blockIdx.y, tile = blockIdx.x;
  const int B = 1 << a.width, HB = B > 1 ? B / 2 : 1;  // words per wavefront
  constexpr int CW = RS_MAXB / 2;
  for (int j = threadIdx.x; j < RS_SW * HB; j += 64 * RS_SW) cnt[(j / HB) * CW + (j % HB)] = 0;
  const uint2* src = a.src + (size_t)r * a.m;
  uint2* dst = a.dst + (size_t)r * a.m;
  const int first = tile * RS_TILE + w * (RS_TILE / RS_SW);
  uint2 kvs[RS_SITEMS];
#pragma unroll
  for (int it = 0; it < RS_SITEMS; ++it) {
    const int idx = first + it * 64 + lane;
    kvs[it] = idx < a.m ? src[idx] : make_uint2(0u, 0u);
  }
  __syncthreads();
  uint32_t* mycnt = cnt + w * CW;
#pragma unroll
  for (int it = 0; it < RS_SITEMS; ++it) {
    if (first + it * 64 + lane < a.m) {
      const uint32_t d = (kvs[it].x >> a.shift) & (B - 1);
      atomicAdd(&mycnt[d >> 1], 1u << (16 * (d & 1u)));
    }
  }
  __syncthreads();
  // thread j owns the digit pairs [j * pp, (j + 1) * pp): where each digit starts in the tile, where in the whole
  // sequence; the counters become every wavefront's first position for the digit
  {
    const int npairs = HB, pp = npairs >= 64 * RS_SW ? npairs / (64 * RS_SW) : 1;
    const int p0 = threadIdx.x * pp;
    uint32_t mine = 0, all = 0;
    for (int j = 0; j < pp; ++j) {
      const int p = p0 + j;
      if (p < npairs) {
        for (int w2 = 0; w2 < RS_SW; ++w2) {
          const uint32_t c = cnt[w2 * CW + p];
          mine += (c & 0xffffu) + (c >> 16);
        }
        all += a.tot[r * B + 2 * p] + (2 * p + 1 < B ? a.tot[r * B + 2 * p + 1] : 0u);
      }
    }
    uint32_t tstart = block_excl_scan<ScanSum, 64 * RS_SW>(mine, 0u, sh);
    uint32_t gstart = block_excl_scan<ScanSum, 64 * RS_SW>(all, 0u, sh + RS_SW);  // (other words: no barrier in between)
    for (int j = 0; j < pp; ++j) {
      const int p = p0 + j;
      if (p < npairs) {
        uint32_t c[RS_SW];
        for (int w2 = 0; w2 < RS_SW; ++w2) c[w2] = cnt[w2 * CW + p];
        // the even digit of the pair, then the odd one
        uint32_t lo_start = tstart, lo_tot = 0;
        for (int w2 = 0; w2 < RS_SW; ++w2) lo_tot += c[w2] & 0xffffu;
        uint32_t hi_start = tstart + lo_tot, hi_tot = 0;
        for (int w2 = 0; w2 < RS_SW; ++w2) hi_tot += c[w2] >> 16;
        const int d = 2 * p;
        const uint32_t* hrow = a.hist + ((size_t)r * a.tiles + tile) * B;
        gpos[d] = (int32_t)(gstart + hrow[d]) - (int32_t)lo_start;
        const uint32_t t_lo = a.tot[r * B + d];
        if (d + 1 < B) gpos[d + 1] = (int32_t)(gstart + t_lo + hrow[d + 1]) - (int32_t)hi_start;
        uint32_t run_lo = lo_start, run_hi = hi_start;
        for (int w2 = 0; w2 < RS_SW; ++w2) {
          cnt[w2 * CW + p] = run_lo | (run_hi << 16);
          run_lo += c[w2] & 0xffffu, run_hi += c[w2] >> 16;
        }
        tstart += lo_tot + hi_tot;
        gstart += t_lo + (d + 1 < B ? a.tot[r * B + d + 1] : 0u);
      }
    }
  }
  __syncthreads();
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
  for (int it = 0; it < RS_SITEMS; ++it) {
    const bool valid = first + it * 64 + lane < a.m;
    const uint2 kv = kvs[it];
    const uint32_t dg = (kv.x >> a.shift) & (B - 1);
    unsigned long long peers = __ballot(valid);
    for (int bit = 0; bit < a.width; ++bit) {
      const bool on = (dg >> bit) & 1u;
      const unsigned long long bb = __ballot(on);
      peers &= on ? bb : ~bb;
    }
    const uint32_t before = __popcll(peers & lt);
    const uint32_t sh16 = 16 * (dg & 1u);
    const uint32_t at = (mycnt[dg >> 1] >> sh16) & 0xffffu;
    __builtin_amdgcn_wave_barrier();
    if (valid && before == 0) atomicAdd(&mycnt[dg >> 1], (uint32_t)__popcll(peers) << sh16);  // the word's other half may move too
    __builtin_amdgcn_wave_barrier();
    if (valid) sorted[at + before] = kv;
  }
  __syncthreads();
  const int have = min(RS_TILE, a.m - tile * RS_TILE);
  for (int j = threadIdx.x; j < have; j += 64 * RS_SW) {
    const uint2 kv = sorted[j];
    dst[gpos[(kv.x >> a.shift) & (B - 1)] + j] = kv;
  }
}

__global__ void __launch_bounds__(256) k_epx_segments(const EpxState st, const EpxBatch b) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= st.n * st.num_keys) return;
  const int r = t / st.num_keys, k = t % st.num_keys;
  const uint2* a = b.kv_sorted + (size_t)r * b.m;
  auto lower = [&](uint32_t x) {
    int lo = 0, hi = b.m;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((a[mid].x & EPX_KEY_MASK) < x) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  b.seg[(size_t)t * 2] = lower((uint32_t)k);
  b.seg[(size_t)t * 2 + 1] = lower((uint32_t)(k + 1));
}

// the same from the sort's digit totals when the whole key was ONE digit (digit == key): the segment of key k starts
// where the digits below k end -- an exclusive scan of B totals per replica instead of 2 binary searches per segment
__global__ void __launch_bounds__(256) k_epx_segments_from_totals(const EpxState st, const EpxBatch b, const uint32_t* tot,
                                                                  int B) {
  __shared__ uint32_t sh[4];
  const int r = blockIdx.x, per = B >= 256 ? B / 256 : 1, d0 = threadIdx.x * per;
  uint32_t mine = 0;
  for (int j = 0; j < per; ++j)
    if (d0 + j < B) mine += tot[r * B + d0 + j];
  uint32_t start = block_excl_scan<ScanSum, 256>(mine, 0u, sh);
  for (int j = 0; j < per; ++j) {
    const int k = d0 + j;
    if (k < B) {
      const uint32_t c = tot[r * B + k];
      if (k < st.num_keys) {
        b.seg[((size_t)r * st.num_keys + k) * 2] = (int32_t)start;
        b.seg[((size_t)r * st.num_keys + k) * 2 + 1] = (int32_t)(start + c);
      }
      start += c;
    }
  }
}

// One chunk of 64 consecutive commands of a (replica, key) segment, one per lane: dep[l] = what the command's
// conflict lookup returns in column l (exclusive prefix over the chunk + carry), and the carries cg / cs (the
// replica's TopOne vectors for the key, KeyValueStore.scala:229-230) and ng / ns (this tick's puts alone) move on.
template <int N>
__device__ __forceinline__ void scan_chunk(bool valid, bool t, int L, int id1, int* cg, int* cs, int* ng, int* ns, int* dep) {
#pragma unroll
  for (int l = 0; l < N; ++l) {
    // inclusive prefix maxima of this chunk's puts into column l
    const int ig = wave_incl_max((valid && !t && L == l) ? id1 : 0);
    const int is = wave_incl_max((valid && t && L == l) ? id1 : 0);
    // exclusive prefix (the command's own put comes after its conflict lookup) + carry
    const int eg = imax(wave_shr1(ig), cg[l]);
    const int es = imax(wave_shr1(is), cs[l]);
    // KeyValueStore.scala:259-302: a get conflicts with sets, a set with sets and gets
    dep[l] = t ? imax(es, eg) : es;
    const int tg = __builtin_amdgcn_readlane(ig, 63), ts = __builtin_amdgcn_readlane(is, 63);
    cg[l] = imax(cg[l], tg), cs[l] = imax(cs[l], ts);
    ng[l] = imax(ng[l], tg), ns[l] = imax(ns[l], ts);
  }
}

// one wavefront per (replica, key) segment
template <int N>
__global__ void __launch_bounds__(256) k_epx_scan(const EpxState st, const EpxBatch b) {
  if (st.status[0] != 0) return;
  const int lane = threadIdx.x & 63;
  const int seg = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (seg >= N * st.num_keys) return;
  const int r = seg / st.num_keys, k = seg % st.num_keys;
  if (b.unfused && (*b.unfused == 0 || b.fused[k])) return;  // k_epx_key did this key on chip
  const int lo = b.seg[(size_t)seg * 2], hi = b.seg[(size_t)seg * 2 + 1];
  const uint2* kvs = b.kv_sorted + (size_t)r * b.m;
  constexpr int NP = ConfRow<N>::NP;
  int cg[N], cs[N];  // carry: the replica's TopOne vectors for this key (KeyValueStore.scala:229-230)
  const size_t ib = ((size_t)r * st.num_keys + k) * N;
#pragma unroll
  for (int l = 0; l < N; ++l) cg[l] = st.gets[ib + l], cs[l] = st.sets[ib + l];
  int ng[N], ns[N];  // this tick's puts alone: what the commit teaches the other replicas
#pragma unroll
  for (int l = 0; l < N; ++l) ng[l] = 0, ns[l] = 0;
  // the next chunk's sort pair and instance number are requested before this chunk is scanned: a segment is ~13
  // dependent round trips otherwise (pair -> number gather -> row store)
  uint2 kv_next = (lo + lane < hi) ? kvs[lo + lane] : make_uint2(0u, 0u);
  int num_next = (lo + lane < hi) ? b.number[kv_next.y] : 0;
  for (int base = lo; base < hi; base += 64) {
    const int p = base + lane;
    const bool valid = p < hi;
    const uint2 kv = kv_next;
    const int id1 = num_next + 1;  // TopOne.put: max(.., id + 1), util/TopOne.scala:12-15
    if (base + 64 < hi) {
      const int pn = base + 64 + lane;
      kv_next = pn < hi ? kvs[pn] : make_uint2(0u, 0u);
      num_next = pn < hi ? b.number[kv_next.y] : 0;
    }
    const int i = (int)kv.y;
    const int L = (int)(kv.x >> EPX_LEADER_SHIFT);
    const bool t = (kv.x >> EPX_SET_SHIFT) & 1u;
    int dep[NP];
#pragma unroll
    for (int l = 0; l < NP; ++l) dep[l] = 0;
    scan_chunk<N>(valid, t, L, id1, cg, cs, ng, ns, dep);
    if (valid) {
      int4* row = reinterpret_cast<int4*>(b.conf + ((size_t)i * N + r) * NP);
      row[0] = make_int4(dep[0], dep[1], dep[2], dep[3]);
      if constexpr (NP == 8) row[1] = make_int4(dep[4], dep[5], dep[6], dep[7]);
    }
  }
  if (lane == 0) {
    int32_t* out = b.tick + (size_t)seg * 2 * N;
#pragma unroll
    for (int l = 0; l < N; ++l) out[l] = ng[l], out[N + l] = ns[l];
  }
}

// handlePreAcceptOk for one command (Replica.scala:1291-1419): the leader's own conflicts D become the PreAccept's
// dependencies, every responder answers its conflicts U D (handlePreAccept :1257-1262), the fast path needs the n-2
// answers identical (popularItems), the slow path proposes their union (preAcceptingSlowPath :796-813).
// load_row(r, out[N]) yields replica r's conflicts for the command.  Writes the command log (if kept); returns the
// decision in o_deps / o_ldeps (watermarks, own column re-encoded) and o_end[2].
template <int N, typename Rows>
__device__ __forceinline__ bool epx_decide_core(const EpxState& st, const EpxBatch& b, int i, int L, unsigned mask,
                                                unsigned seen_in, int x, Rows&& load_row, int* o_deps, int* o_ldeps,
                                                int* o_end) {
  int D[N], uni[N], first[N];
  load_row(L, D);
#pragma unroll
  for (int l = 0; l < N; ++l) uni[l] = D[l], first[l] = 0;
  bool have_first = false, all_equal = true;
  for (int r = 0; r < N; ++r) {
    if (!((mask >> r) & 1u)) continue;
    bool same = true;
    int cr[N];
    load_row(r, cr);
#pragma unroll
    for (int l = 0; l < N; ++l) {
      const int cl = cr[l];
      const int resp = cl > D[l] ? cl : D[l];  // handlePreAccept: local conflicts U preAccept.dependencies
      uni[l] = resp > uni[l] ? resp : uni[l];  // preAcceptingSlowPath: union of all answers
      if (!have_first) first[l] = resp; else same = same && (first[l] == resp);
    }
    if (have_first) all_equal = all_equal && same;
    have_first = true;
  }
  // dependencies.subtractOne(instance) (Replica.scala:582, compact/IntPrefixSet.scala:388-398) only touches the
  // column of the instance's own leader: with w = that column's watermark before the subtraction and x the
  // instance number, the set is {0 .. w-1} \ {x}: (watermark w, no values) if x >= w, else (watermark x,
  // values x+1 .. w-1).  Unions (addAll) and the equality test of popularItems commute with that encoding for a
  // fresh instance (w == x + 1 would need the instance itself in the index), so everything above ran on the
  // plain watermarks w and only the own column is re-encoded here.
  if (st.num_instances > 0) {
    // the command log: a fast-path commit is a CommittedEntry at every replica (commit :815-823, Commit to the
    // others); otherwise every replica that processed the PreAccept holds PreAcceptedEntry(Ballot(0, leader),
    // Ballot(0, leader), triple) (:688-696, :1259-1271) for the Accept phase to find
    const unsigned seen = seen_in | (1u << L);
    const int tr = b.triple ? b.triple[i] : -1;
    for (int r = 0; r < N; ++r) {
      const size_t c = ((size_t)r * N + L) * st.num_instances + x;
      if (!all_equal && !((seen >> r) & 1u)) continue;
      // the triple's dependencies: the agreed ones (fast path, committed everywhere), else what THIS replica
      // answered (its conflicts U the PreAccept's, :1257-1271) / what the leader proposed (:688-696)
      int t[N];
      if (all_equal) {
#pragma unroll
        for (int l = 0; l < N; ++l) t[l] = first[l];
      } else if (r == L) {
#pragma unroll
        for (int l = 0; l < N; ++l) t[l] = D[l];
      } else {
        int cr[N];
        load_row(r, cr);
#pragma unroll
        for (int l = 0; l < N; ++l) t[l] = cr[l] > D[l] ? cr[l] : D[l];
      }
      int wm = 0, end = 0;
#pragma unroll
      for (int l = 0; l < N; ++l)
        if (l == L) own_column(t[l], x, &wm, &end);
#pragma unroll
      for (int l = 0; l < N; ++l) st.cl_deps[c * N + l] = l == L ? wm : t[l];
      st.cl_dend[c] = end;
      if (all_equal) {
        st.cl_status[c] = CL_COMMITTED, st.cl_ballot[c] = -1, st.cl_vote[c] = -1, st.cl_triple[c] = tr;
      } else {
        st.cl_status[c] = CL_PRE_ACCEPTED, st.cl_ballot[c] = L, st.cl_vote[c] = L, st.cl_triple[c] = tr;  // 0 * 8 + L
      }
    }
  }
  o_end[0] = 0, o_end[1] = 0;
#pragma unroll
  for (int l = 0; l < N; ++l) {
    const int w = all_equal ? first[l] : uni[l];
    int ow = w, oe = 0, lw = D[l], le = 0;
    if (l == L) {
      own_column(w, x, &ow, &oe), own_column(D[l], x, &lw, &le);
      o_end[0] = oe, o_end[1] = le;
    }
    o_deps[l] = ow;
    o_ldeps[l] = lw;
  }
  return all_equal;
}

// one thread per command; the n-wide dependency rows leave through LDS as contiguous lines (m x n ints written
// by 256 threads with a stride of n ints were 5 strided store instructions per wave)
template <int N>
__global__ void __launch_bounds__(256) k_epx_decide(const EpxState st, const EpxBatch b) {
  __shared__ int out_deps[256 * N], out_ldeps[256 * N];
  __shared__ uint8_t did[256];
  if (st.status[0] != 0) return;
  if (b.unfused && *b.unfused == 0) return;  // k_epx_key decided every key on chip
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool mine = i < b.m && !(b.unfused && b.fused[b.key[i]]);
  did[threadIdx.x] = mine ? 1 : 0;
  if (mine) {
    constexpr int NP = ConfRow<N>::NP;
    const int32_t* c = b.conf + (size_t)i * N * NP;
    auto load_row = [&](int r, int* out) {
      const int4* row = reinterpret_cast<const int4*>(c + r * NP);
      const int4 a = row[0];
      int tmp[8] = {a.x, a.y, a.z, a.w, 0, 0, 0, 0};
      if constexpr (NP == 8) {
        const int4 b2 = row[1];
        tmp[4] = b2.x, tmp[5] = b2.y, tmp[6] = b2.z, tmp[7] = b2.w;
      }
#pragma unroll
      for (int l = 0; l < N; ++l) out[l] = tmp[l];
    };
    int od[N], ol[N], oe[2];
    const unsigned mask = b.resp_mask[i];
    const bool fast = epx_decide_core<N>(st, b, i, b.leader[i], mask, b.seen_mask ? b.seen_mask[i] : mask, b.number[i],
                                         load_row, od, ol, oe);
    if (b.fast) b.fast[i] = fast ? 1 : 0;
    if (b.own_values_end) b.own_values_end[(size_t)i * 2] = oe[0], b.own_values_end[(size_t)i * 2 + 1] = oe[1];
#pragma unroll
    for (int l = 0; l < N; ++l) out_deps[threadIdx.x * N + l] = od[l], out_ldeps[threadIdx.x * N + l] = ol[l];
  }
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * blockDim.x * N;
  for (int k = threadIdx.x; k < 256 * N; k += 256) {
    if (did[k / N]) {
      if (b.deps) b.deps[base + k] = out_deps[k];
      if (b.leader_deps) b.leader_deps[base + k] = out_ldeps[k];
    }
  }
}

#include "fpx_epaxos_kp.hpp"
#include "fpx_depgraph_dev.hpp"
#include "fpx_depgraph_pk.hpp"

// ---- scan + decide of ONE key on chip ------------------------------------------------------------------------
// k_epx_scan hands every (command, replica) conflict row to k_epx_decide through HBM at [command][replica]: n * m
// rows written in (key, delivery order), i.e. at random -- 5 M random row writes are ~70 us on this GPU whatever
// their size (profiles/r02_random_rows.txt).  Here one workgroup owns a key: wavefront r scans replica r's segment
// of the key, the rows stay in LDS ([command of the key][replica][column]), and the same workgroup decides the
// key's commands; only the decisions cross to message-index order.  A command gets its slot in the LDS tables from
// the wavefront of its LEADER's replica (every command is in its leader's segment exactly once); the other
// wavefronts find the slot through an LDS hash table on the message index.  A key with more commands than the
// tables hold (KeyTile<N>::TC) is left to k_epx_scan / k_epx_decide (b.fused[k] = 0), so skewed workloads stay
// correct and merely lose the shortcut on their hot keys.
template <int N> struct KeyTile {
  static constexpr int TC = N <= 3 ? 2048 : N <= 5 ? 1152 : 576;   // commands of one key held on chip
  static constexpr int HC = N <= 3 ? 8192 : N <= 5 ? 4096 : 2048;  // hash slots: a power of two, load <= 0.28 (at 0.56
                                                                   // the probe chains cost 7 us per tick, n = 5)
  static constexpr int W = N <= 3 ? 4 : N <= 5 ? 3 : 2;             // wavefronts per replica segment
  static constexpr int MAXC = (TC + 63) / 64;                       // 64-command chunks of one segment
  static constexpr int CPW = (MAXC + W - 1) / W;                    // chunks per wavefront
  static constexpr int THREADS = 64 * N * W;
  static constexpr int IDX_BITS = 11;                               // TC <= 2048
  static constexpr size_t BYTES =
      (size_t)TC * N * N * 4 + (size_t)HC * 4 + (size_t)TC * 4 * 3 + (size_t)N * TC * 2 + (size_t)N * W * 2 * N * 4 + 64;
};

template <int N>
__global__ void __launch_bounds__(KeyTile<N>::THREADS) k_epx_key(const EpxState st, const EpxBatch b) {
  using T = KeyTile<N>;
  extern __shared__ __align__(16) unsigned char smem[];
  int* rows = reinterpret_cast<int*>(smem);                                   // [TC][N replicas][N columns]
  uint32_t* hk = reinterpret_cast<uint32_t*>(rows + (size_t)T::TC * N * N);   // (message index + 1) << 11 | slot
  int* list_i = reinterpret_cast<int*>(hk + T::HC);                           // slot -> message index
  int* num = list_i + T::TC;                                                  // slot -> instance number
  uint32_t* msk = reinterpret_cast<uint32_t*>(num + T::TC);                   // slot -> resp_mask | seen << 8 | leader << 16
  uint16_t* stage = reinterpret_cast<uint16_t*>(msk + T::TC);                 // [N][TC] slot | is_set << 11 | leader << 12
  int* tot = reinterpret_cast<int*>(stage + (size_t)N * T::TC);               // [N][W][2N] puts of a wavefront's chunks
  int* ctl = tot + N * T::W * 2 * N;                                          // [0] slots handed out, [1] give up
  if (st.status[0] != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = wave / T::W, w = wave - r * T::W;  // replica, part of its segment
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));

  // A workgroup works through the keys blockIdx.x, + gridDim.x, ...  With 149 KB of LDS it is alone on its CU, so
  // nothing else hides its memory round trips: what the NEXT key needs from memory -- segment bounds and the
  // replica's TopOne vectors (A), the sort pairs of this wavefront's part (B), number / masks of the commands it
  // leads (C), each addressed with the one before -- is requested while the current key is worked on.
  struct SegA {
    int lo, len, cpw, first;
    int cg[N], cs[N];
  };
  auto fetch_a = [&](int k, SegA& s) {
    const int seg = r * st.num_keys + k;
    s.lo = b.seg[(size_t)seg * 2];
    s.len = b.seg[(size_t)seg * 2 + 1] - s.lo;
    s.cpw = ((s.len + 63) / 64 + T::W - 1) / T::W;  // chunks per wavefront of THIS segment
    s.first = w * s.cpw * 64;                       // where this wavefront's part starts
    const size_t ib = (size_t)seg * N;
#pragma unroll
    for (int l = 0; l < N; ++l) s.cg[l] = st.gets[ib + l], s.cs[l] = st.sets[ib + l];
  };
  auto fetch_b = [&](const SegA& s, uint2* kv, bool* have) {
    const uint2* kvs = b.kv_sorted + (size_t)r * b.m + s.lo;
#pragma unroll
    for (int c = 0; c < T::CPW; ++c) {
      const int p = s.first + c * 64 + lane;
      have[c] = c < s.cpw && p < s.len && s.len <= T::MAXC * 64;
      kv[c] = have[c] ? kvs[p] : make_uint2(0u, 0u);
    }
  };
  auto fetch_c = [&](const uint2* kv, const bool* have, int* gnum, unsigned* gmask) {
#pragma unroll
    for (int c = 0; c < T::CPW; ++c) {
      gnum[c] = 0, gmask[c] = 0;
      if (have[c] && (int)(kv[c].x >> EPX_LEADER_SHIFT) == r) {
        const int2 mt = b.meta[kv[c].y];  // written by k_epx_keys: three arrays in one 8-byte gather
        gnum[c] = mt.x;
        gmask[c] = (unsigned)mt.y;
      }
    }
  };

  SegA cur, nxt;
  uint2 kvq[T::CPW], kvn[T::CPW];
  bool have[T::CPW], haven[T::CPW];
  int gnum[T::CPW], gnumn[T::CPW];
  unsigned gmask[T::CPW], gmaskn[T::CPW];
  int k = blockIdx.x;
  if (k >= st.num_keys) return;
  fetch_a(k, cur);
  fetch_b(cur, kvq, have);
  fetch_c(kvq, have, gnum, gmask);
  for (; k < st.num_keys; k += gridDim.x) {
    const int kn = k + gridDim.x;
    const bool more = kn < st.num_keys;
    if (more) fetch_a(kn, nxt);
    for (int j = threadIdx.x; j < T::HC; j += T::THREADS) hk[j] = 0;
    for (int j = threadIdx.x; j < N * T::W * 2 * N + 2; j += T::THREADS) tot[j] = 0;  // tot and ctl
    __syncthreads();
    if (cur.len > T::MAXC * 64 && lane == 0) ctl[1] = 1;
    // the wavefronts of the leader's replica hand out the slots of the commands it leads
#pragma unroll
    for (int c = 0; c < T::CPW; ++c) {
      const bool own = have[c] && (int)(kvq[c].x >> EPX_LEADER_SHIFT) == r;
      const unsigned long long bal = __ballot(own);
      int base = 0;
      if (bal) {
        if (lane == 0) base = atomicAdd(&ctl[0], (int)__popcll(bal));
        base = __builtin_amdgcn_readfirstlane(base);
      }
      const int sl = own ? base + (int)__popcll(bal & lt) : -1;
      if (sl >= T::TC) ctl[1] = 1;
      if (sl >= 0 && sl < T::TC) {
        const int i = (int)kvq[c].y;
        list_i[sl] = i;
        num[sl] = gnum[c];
        msk[sl] = gmask[c] | ((unsigned)r << 16);
        const uint32_t word = ((uint32_t)(i + 1) << T::IDX_BITS) | (uint32_t)sl;
        uint32_t h = ((uint32_t)i * 2654435761u >> 12) & (T::HC - 1);
        while (atomicCAS(&hk[h], 0u, word) != 0u) h = (h + 1) & (T::HC - 1);
      }
    }
    __syncthreads();
    const bool give_up = ctl[1] != 0;  // more commands than the tables hold: the key goes the long way
    if (give_up && threadIdx.x == 0) b.fused[k] = 0, atomicAdd(b.unfused, 1);
    uint16_t* mystage = stage + (size_t)r * T::TC + cur.first;
    if (!give_up) {
      // every command finds its slot; the scan below only needs (slot, is_set, leader) per lane.  The puts of this
      // wavefront's part (per column the largest id + 1) are the carry of the parts behind it.
      int* mytot = tot + (r * T::W + w) * 2 * N;
#pragma unroll
      for (int c = 0; c < T::CPW; ++c) {
        if (have[c]) {
          const uint32_t want = kvq[c].y + 1u;
          uint32_t h = (kvq[c].y * 2654435761u >> 12) & (T::HC - 1);
          uint32_t wd = hk[h];
          while ((wd >> T::IDX_BITS) != want) h = (h + 1) & (T::HC - 1), wd = hk[h];
          const uint32_t sl = wd & ((1u << T::IDX_BITS) - 1u);
          const uint32_t flags = kvq[c].x >> EPX_SET_SHIFT;  // bit 0 is_set, bits 1.. leader
          mystage[c * 64 + lane] = (uint16_t)(sl | (flags << T::IDX_BITS));
          atomicMax(&mytot[(flags & 1u) * N + (flags >> 1)], num[sl] + 1);
        }
      }
    }
    if (more) fetch_b(nxt, kvn, haven);  // the current key's pairs are spent
    __syncthreads();
    if (!give_up) {
      int cg[N], cs[N];
#pragma unroll
      for (int l = 0; l < N; ++l) cg[l] = cur.cg[l], cs[l] = cur.cs[l];
      for (int w2 = 0; w2 < w; ++w2) {
        const int* o = tot + (r * T::W + w2) * 2 * N;
#pragma unroll
        for (int l = 0; l < N; ++l) cg[l] = imax(cg[l], o[l]), cs[l] = imax(cs[l], o[N + l]);
      }
      if (w == 0 && lane == 0) {  // what the commit teaches the other replicas: this tick's puts alone
        int32_t* out = b.tick + ((size_t)r * st.num_keys + k) * 2 * N;
        for (int l = 0; l < 2 * N; ++l) {
          int v = 0;
          for (int w2 = 0; w2 < T::W; ++w2) v = imax(v, tot[(r * T::W + w2) * 2 * N + l]);
          out[l] = v;
        }
      }
      int ng[N], ns[N];
#pragma unroll
      for (int l = 0; l < N; ++l) ng[l] = 0, ns[l] = 0;
      for (int base = 0; base < cur.cpw * 64 && cur.first + base < cur.len; base += 64) {
        const bool valid = cur.first + base + lane < cur.len;
        const unsigned code = valid ? mystage[base + lane] : 0u;
        const int sl = (int)(code & ((1u << T::IDX_BITS) - 1u));
        const bool t = (code >> T::IDX_BITS) & 1u;
        const int L = (int)(code >> (T::IDX_BITS + 1));
        const int id1 = valid ? num[sl] + 1 : 0;  // TopOne.put: max(.., id + 1), util/TopOne.scala:12-15
        int dep[N];
        scan_chunk<N>(valid, t, L, id1, cg, cs, ng, ns, dep);
        if (valid) {
#pragma unroll
          for (int l = 0; l < N; ++l) rows[((size_t)sl * N + r) * N + l] = dep[l];
        }
      }
    }
    if (more) fetch_c(kvn, haven, gnumn, gmaskn);
    __syncthreads();
    if (!give_up) {
      const int count = ctl[0];
      for (int sl = threadIdx.x; sl < count; sl += T::THREADS) {
        const int i = list_i[sl];
        const unsigned mw = msk[sl];
        auto load_row = [&](int rr, int* out) {
#pragma unroll
          for (int l = 0; l < N; ++l) out[l] = rows[((size_t)sl * N + rr) * N + l];
        };
        int od[N], ol[N], oe[2];
        const bool fast = epx_decide_core<N>(st, b, i, (int)(mw >> 16), mw & 0xffu, (mw >> 8) & 0xffu, num[sl], load_row,
                                             od, ol, oe);
        if (b.fast) b.fast[i] = fast ? 1 : 0;
        if (b.own_values_end) *reinterpret_cast<int2*>(b.own_values_end + (size_t)i * 2) = make_int2(oe[0], oe[1]);
        // the command's rows are spent: its decision takes their place, to leave below as whole n-int lines (one
        // store instruction per column and thread here would touch 64 different lines each)
#pragma unroll
        for (int l = 0; l < N; ++l) rows[((size_t)sl * N + 0) * N + l] = od[l], rows[((size_t)sl * N + 1) * N + l] = ol[l];
      }
      __syncthreads();
      for (int t = threadIdx.x; t < count * N; t += T::THREADS) {
        const int sl = t / N, l = t - sl * N;
        const size_t o = (size_t)list_i[sl] * N + l;
        if (b.deps) b.deps[o] = rows[((size_t)sl * N + 0) * N + l];
        if (b.leader_deps) b.leader_deps[o] = rows[((size_t)sl * N + 1) * N + l];
      }
      if (threadIdx.x == 0) b.fused[k] = 1;
    }
    __syncthreads();  // the tables are reused by the next key
    cur = nxt;
#pragma unroll
    for (int c = 0; c < T::CPW; ++c) kvq[c] = kvn[c], have[c] = haven[c], gnum[c] = gnumn[c], gmask[c] = gmaskn[c];
  }
}

__global__ void __launch_bounds__(256) k_epx_commit(const EpxState st, const EpxBatch b) {
  if (st.status[0] != 0) return;
  const long long per = (long long)st.num_keys * st.n;            // entries of one replica's gets (or sets)
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  // fpx_epx_tick_census: the keys k_epx_key left to the long way this tick (kernels of one stream: no atomic needed)
  if (t == 0 && b.census && b.unfused) b.census[EPX_CD_LONG_WAY] += (unsigned long long)*b.unfused;
  if (t >= per * st.n) return;
  const int r = (int)(t / per);
  const long long e = t % per;                                    // key * n + leader
  const int k = (int)(e / st.n), l = (int)(e % st.n);
  int tg = 0, ts = 0;
  for (int q = 0; q < st.n; ++q) {
    const int32_t* seen = b.tick + (((size_t)q * st.num_keys + k) * 2) * st.n;
    tg = imax(tg, seen[l]), ts = imax(ts, seen[st.n + l]);
  }
  int32_t* g = &st.gets[(size_t)r * per + e];
  int32_t* s2 = &st.sets[(size_t)r * per + e];
  if (tg > *g) *g = tg;
  if (ts > *s2) *s2 = ts;
}

// the four output arrays -> one packed line per command (fpx_epx_preaccept_packed_dev through the first form): 256
// commands per workgroup, every array read and the lines written with consecutive lanes on consecutive words
__global__ void __launch_bounds__(256) k_epx_pack(const EpxState st, int m, const uint8_t* fast, const int32_t* deps,
                                                  const int32_t* ldeps, const int32_t* own, int32_t* packed, int stride) {
  __shared__ int32_t line[256 * 20];
  if (st.status[0] != 0) return;
  const int n = st.n, i0 = blockIdx.x * 256, cnt = min(256, m - i0);
  for (int t = threadIdx.x; t < cnt * stride; t += 256) line[t] = 0;
  __syncthreads();
  for (int t = threadIdx.x; t < cnt * n; t += 256) {
    const int c = t / n, l = t - c * n;
    line[c * stride + l] = deps[(size_t)i0 * n + t], line[c * stride + n + l] = ldeps[(size_t)i0 * n + t];
  }
  for (int t = threadIdx.x; t < cnt * 2; t += 256) line[(t >> 1) * stride + 2 * n + (t & 1)] = own[(size_t)i0 * 2 + t];
  if ((int)threadIdx.x < cnt) line[threadIdx.x * stride + 2 * n + 2] = fast[i0 + threadIdx.x] ? 1 : 0;
  __syncthreads();
  for (int t = threadIdx.x; t < cnt * stride; t += 256) packed[(size_t)i0 * stride + t] = line[t];
}

// ---- the per-instance Paxos of EPaxos on the command log: Prepare (phase 1) and Accept (phase 2) ---------------
// Messages are delivered in array order to the replicas of target[i]; the instances of a batch are pairwise
// distinct, so every command-log cell has one writer and the only order-dependent quantity is each replica's
// running largestBallot (Replica.scala:458), which only Nacks report: an inclusive prefix max per replica over the
// ballots the replica took in (k_cl_tilemax / k_cl_tilescan / k_cl_nacks).
struct ClBatch {
  int m, accept;           // accept = 0: Prepare
  const int32_t* leader;
  const int32_t* number;
  const int32_t* b_ord;
  const int32_t* b_rep;
  const int32_t* triple;   // Accept
  const int32_t* key;      // Accept: the command's key, -1 = Noop
  const uint8_t* is_set;   // Accept
  const int32_t* key_off;  // Accept, multi-key form (else null): message i's keys are keys[key_off[i] .. key_off[i + 1])
  const int32_t* keys;
  const uint8_t* target;
  uint8_t* ok_bits;
  uint8_t* nack_bits;
  uint8_t* commit_bits;
  int32_t* nack_ballot;
  uint8_t* committed;      // Accept
  int32_t* reply_status;   // Prepare: [m][n]
  int32_t* reply_vote;
  int32_t* reply_triple;
  int32_t* contrib;        // [n][m] scratch: the ballot replica r took in with message i, or -1
  uint8_t* nackflag;       // [n][m] scratch
  int32_t* tilemax;        // [n][tiles] scratch
  uint8_t* skip;           // [m] scratch: Accept whose proposer refused it (logger.fatal / checkLe)
  uint32_t run_id;
};
constexpr int CL_TILE = 1024;

// updateConflictIndex(instance, commandOrNoop) (Replica.scala:602-614) at replica r: conflictIndex.put = a max-merge of
// the TopOne column of the instance's leader (util/TopOne.scala:14-17), so several messages of one batch may land on
// one cell in any order; a Noop leaves the index alone
__device__ __forceinline__ void index_put(const EpxState& st, int r, int key, int is_set, int L, int x) {
  if (key < 0) return;
  int32_t* a = is_set ? st.sets : st.gets;
  atomicMax(&a[((size_t)r * st.num_keys + key) * st.n + L], x + 1);
}
// the same for message i's command: its single key (key_off null) or every key of its list (KeyValueStore.scala:236-254:
// put records the instance under each key of the command; a repeated key is the same maximum twice, no keys = nothing)
__device__ __forceinline__ void index_put_cmd(const EpxState& st, int r, const int32_t* key, const int32_t* key_off,
                                              const int32_t* keys, int i, int is_set, int L, int x) {
  if (!key_off) {
    index_put(st, r, key[i], is_set, L, x);
    return;
  }
  for (int j = key_off[i]; j < key_off[i + 1]; ++j) index_put(st, r, keys[j], is_set, L, x);
}

// an Accept names its triple by the caller's id alone: the stored dependencies are marked unknown
__device__ __forceinline__ void deps_by_id(const EpxState& st, size_t cell) {
  for (int l = 0; l < st.n; ++l) st.cl_deps[cell * st.n + l] = -1;
  st.cl_dend[cell] = 0;
}

__global__ void __launch_bounds__(256) k_cl_validate(const EpxState st, const ClBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n, L = b.leader[i], x = b.number[i], bo = b.b_ord[i], br = b.b_rep[i];
  bool ok = L >= 0 && L < n && x >= 0 && x < st.num_instances && bo >= 0 && bo < (1 << 27) && br >= 0 && br < n &&
            (b.target[i] >> n) == 0;
  if (ok && b.accept) ok = !((b.target[i] >> br) & 1u);  // thriftyOtherReplicas: never the proposer itself (:774)
  if (ok && b.accept && !b.key_off) ok = b.key[i] >= -1 && b.key[i] < st.num_keys;  // (key lists: checked on the host)
  if (ok) ok = atomicExch(&st.cl_stamp[(size_t)L * st.num_instances + x], b.run_id) != b.run_id;
  if (!ok) epx_report(st.status, FPX_EINVAL, i);
}

// Accept: transitionToAcceptPhase at the proposer (Replica.scala:732-792), one thread per message
__global__ void __launch_bounds__(256) k_cl_propose(const EpxState st, const ClBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n, P = b.b_rep[i], ballot = b.b_ord[i] * 8 + P;
  const size_t c = ((size_t)P * n + b.leader[i]) * st.num_instances + b.number[i];
  const int kind = st.cl_status[c];
  // :740-744 a CommittedEntry is logger.fatal; :749-757 logger.checkLe(entry.ballot / voteBallot, ballot)
  const bool refuse = kind == CL_COMMITTED || (kind != CL_NONE && st.cl_ballot[c] > ballot) ||
                      (kind >= CL_PRE_ACCEPTED && st.cl_vote[c] > ballot);
  b.skip[i] = refuse ? 1 : 0;
  if (refuse) {
    if (atomicCAS(&st.status[0], 0, FPX_EFATAL_PROTOCOL) == 0) st.status[1] = i;
    return;
  }
  st.cl_status[c] = CL_ACCEPTED, st.cl_ballot[c] = ballot, st.cl_vote[c] = ballot, st.cl_triple[c] = b.triple[i];  // :759-762
  deps_by_id(st, c);
  index_put_cmd(st, P, b.key, b.key_off, b.keys, i, b.is_set[i], b.leader[i], b.number[i]);  // :763
}

// handlePrepare (:1632-1757) / handleAccept (:1421-1511) at replica r for message i: one thread per (i, r)
__global__ void __launch_bounds__(256) k_cl_handle(const EpxState st, const ClBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int n = st.n;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)b.m * n) return;
  const int r = (int)(t / b.m), i = (int)(t % b.m);  // replica-major: the scratch rows are contiguous per replica
  const int ballot = b.b_ord[i] * 8 + b.b_rep[i];
  int contrib = -1, rs = -1, rv = -1, rt = -1;
  uint8_t nack = 0;
  const bool live = ((b.target[i] >> r) & 1u) && !(b.accept && b.skip[i]);
  if (live) {
    const size_t c = ((size_t)r * n + b.leader[i]) * st.num_instances + b.number[i];
    const int kind = st.cl_status[c];
    if (!b.accept) contrib = ballot;  // :1637 largestBallot = max(.., prepare.ballot) before anything else
    if (kind == CL_COMMITTED) {
      atomicOr(reinterpret_cast<unsigned int*>(b.commit_bits) + (i >> 2), (1u << r) << (8 * (i & 3)));
    } else if (kind != CL_NONE && ballot < st.cl_ballot[c]) {
      nack = 1;  // Nack(instance, largestBallot): the value comes from the scan
      atomicOr(reinterpret_cast<unsigned int*>(b.nack_bits) + (i >> 2), (1u << r) << (8 * (i & 3)));
    } else {
      atomicOr(reinterpret_cast<unsigned int*>(b.ok_bits) + (i >> 2), (1u << r) << (8 * (i & 3)));
      if (!b.accept) {
        if (kind == CL_NONE || kind == CL_NO_COMMAND) {  // :1654-1669, :1686-1701
          rs = 0;
          st.cl_status[c] = CL_NO_COMMAND, st.cl_vote[c] = -1, st.cl_triple[c] = -1;
        } else {  // :1711-1743 the entry keeps its vote, only `ballot` moves
          rs = kind, rv = st.cl_vote[c], rt = st.cl_triple[c];
        }
        st.cl_ballot[c] = ballot;
      } else if (!(kind == CL_ACCEPTED && ballot == st.cl_vote[c])) {  // (:1451-1461: already answered, re-send only)
        contrib = ballot;  // :1487
        st.cl_status[c] = CL_ACCEPTED, st.cl_ballot[c] = ballot, st.cl_vote[c] = ballot, st.cl_triple[c] = b.triple[i];
        deps_by_id(st, c);
        index_put_cmd(st, r, b.key, b.key_off, b.keys, i, b.is_set[i], b.leader[i], b.number[i]);  // :1503
      }
    }
  }
  b.contrib[(size_t)r * b.m + i] = contrib;
  b.nackflag[(size_t)r * b.m + i] = nack;
  if (!b.accept) {
    if (b.reply_status) b.reply_status[(size_t)i * n + r] = rs;
    if (b.reply_vote) b.reply_vote[(size_t)i * n + r] = rv;
    if (b.reply_triple) b.reply_triple[(size_t)i * n + r] = rt;
  }
}

__global__ void __launch_bounds__(256) k_cl_tilemax(const ClBatch b, int tiles) {
  __shared__ int sh[4];
  const int r = blockIdx.y, t = blockIdx.x;
  int v = -1;
  for (int k = threadIdx.x; k < CL_TILE; k += 256) {
    const int i = t * CL_TILE + k;
    if (i < b.m) v = imax(v, b.contrib[(size_t)r * b.m + i]);
  }
  v = block_reduce<ScanMax, 256>(v, sh);
  if (threadIdx.x == 0) b.tilemax[(size_t)r * tiles + t] = v;
}

// one block per replica: tilemax -> what the replica had seen BEFORE each tile; the replica's new largestBallot.  (ScanMax:
// ballots are >= 0 and k_cl_tilemax starts from -1, so nothing scanned is below -1.)
__global__ void __launch_bounds__(256) k_cl_tilescan(const EpxState st, const ClBatch b, int tiles) {
  __shared__ int lds[SCAN_ARRAY_LDS(256)];
  if (st.status[0] == FPX_EINVAL) return;
  const int r = blockIdx.x;
  const int run = scan_array_excl<ScanMax, 256, 1>(b.tilemax + (size_t)r * tiles, tiles, lds, st.largest[r]);
  if (threadIdx.x == 0) st.largest[r] = run;
}

// the largestBallot a Nack of (i, r) carries = max(before the tile, inclusive prefix inside the tile)
__global__ void __launch_bounds__(256) k_cl_nacks(const ClBatch b, int tiles) {
  __shared__ int wmax[4];
  const int r = blockIdx.y, t = blockIdx.x;
  int carry = b.tilemax[(size_t)r * tiles + t];
  for (int k0 = 0; k0 < CL_TILE; k0 += 256) {
    const int i = t * CL_TILE + k0 + threadIdx.x;
    const int v = i < b.m ? b.contrib[(size_t)r * b.m + i] : -1;
    int inc = wave_incl_max(v + 1) - 1;  // the DPP scan's identity is 0: shift ballots (>= -1) up by one
    if ((threadIdx.x & 63) == 63) wmax[threadIdx.x >> 6] = inc;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before = imax(before, wmax[w]);
    const int total = imax(imax(wmax[0], wmax[1]), imax(wmax[2], wmax[3]));
    inc = imax(inc, before);
    if (i < b.m && b.nackflag[(size_t)r * b.m + i] && b.nack_ballot) atomicMax(&b.nack_ballot[i], inc);
    carry = imax(carry, total);
    __syncthreads();
  }
}

// handleAcceptOk (:1513-1565): f + 1 responses, the proposer's own included -> commit (:815-860) at every replica
__global__ void __launch_bounds__(256) k_cl_commit(const EpxState st, const ClBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n, f = (n - 1) / 2;
  uint8_t done = 0;
  if (!b.skip[i]) {
    const unsigned ok = b.ok_bits[i] | (1u << b.b_rep[i]);  // :780-789 the proposer's own AcceptOk
    b.ok_bits[i] = (uint8_t)ok;
    if ((int)__popc(ok) >= f + 1) {
      done = 1;
      for (int r = 0; r < n; ++r) {
        const size_t c = ((size_t)r * n + b.leader[i]) * st.num_instances + b.number[i];
        st.cl_status[c] = CL_COMMITTED, st.cl_ballot[c] = -1, st.cl_vote[c] = -1, st.cl_triple[c] = b.triple[i];
        deps_by_id(st, c);
        index_put_cmd(st, r, b.key, b.key_off, b.keys, i, b.is_set[i], b.leader[i], b.number[i]);  // commit :828, at every replica (Commit)
      }
    }
  }
  if (b.committed) b.committed[i] = done;
}

// Replica.handleCommit (:1567-1575) -> commit (:815-830) at replica r for message i: one thread per (i, r).  A Commit is
// final: no ballot is looked at, whatever entry the replica held is replaced (:826-827), the conflict index learns the
// command (:828).
struct LcBatch {
  int m;
  const int32_t* leader;
  const int32_t* number;
  const int32_t* triple;
  const int32_t* key;
  const uint8_t* is_set;
  const int32_t* key_off;   // multi-key form (else null): message i's keys are keys[key_off[i] .. key_off[i + 1])
  const int32_t* keys;
  const int32_t* deps;      // [m][n] or null: the triple is known by its id alone
  const int32_t* deps_end;  // [m] or null
  const uint8_t* target;
  const uint8_t* writer;    // [m] the replicas whose ENTRY this message writes: target minus the replicas a later message of the
                            // batch for the same instance goes to -- of several Commits for one instance the last one wins
                            // WHOLE (triple, dependencies and all), as when the reference applies them in order; cell by cell
                            // from different threads the entry could end up with one message's triple and another's
                            // dependencies
};
__global__ void __launch_bounds__(256) k_cl_learn_commit(const EpxState st, const LcBatch b) {
  const int n = st.n;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)b.m * n) return;
  const int r = (int)(t / b.m), i = (int)(t % b.m);
  if (!((b.target[i] >> r) & 1u)) return;
  if ((b.writer[i] >> r) & 1u) {
    const size_t c = ((size_t)r * n + b.leader[i]) * st.num_instances + b.number[i];
    st.cl_status[c] = CL_COMMITTED, st.cl_ballot[c] = -1, st.cl_vote[c] = -1, st.cl_triple[c] = b.triple[i];
    if (b.deps) {
      for (int l = 0; l < n; ++l) st.cl_deps[c * n + l] = b.deps[(size_t)i * n + l];
      st.cl_dend[c] = b.deps_end ? b.deps_end[i] : 0;
    } else {
      deps_by_id(st, c);
    }
  }
  index_put_cmd(st, r, b.key, b.key_off, b.keys, i, b.is_set[i], b.leader[i], b.number[i]);  // (a maximum: every message's put, in any order)
}

// ---- K8: Replica.handlePrepareOk (Replica.scala:1759-1884), the recovering replica's decision -- one thread per instance
struct RcBatch {
  int m, as_intended;
  const int32_t* leader;
  const int32_t* number;
  const int32_t* b_ord;
  const int32_t* b_rep;
  const uint8_t* resp_mask;
  const int32_t* rs;  // [m][n] PrepareOk.status as the entry kind
  const int32_t* rv;  // [m][n] PrepareOk.voteBallot, encoded
  const int32_t* rt;  // [m][n] triple id
  int32_t* action;
  int32_t* source;
  int32_t* triple;
};

__global__ void __launch_bounds__(256) k_cl_recover(const EpxState st, const RcBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n, f = (n - 1) / 2;
  const int L = b.leader[i], x = b.number[i], me = b.b_rep[i];
  const unsigned mask = b.resp_mask[i];
  bool ok = L >= 0 && L < n && x >= 0 && x < st.num_instances && me >= 0 && me < n && b.b_ord[i] >= 0 && (mask >> n) == 0;
  const int32_t* rs = b.rs + (size_t)i * n;
  const int32_t* rv = b.rv + (size_t)i * n;
  const int32_t* rt = b.rt + (size_t)i * n;
  for (int r = 0; ok && r < n; ++r)
    if (((mask >> r) & 1u) && rs[r] < 0) ok = false;  // no PrepareOk from r
  if (!ok) {
    epx_report(st.status, FPX_EINVAL, i);
    return;
  }
  if (st.status[0] != 0) return;
  int act = 0, src = -1, tr = -1;
  if ((int)__popc(mask) >= f + 1) {  // :1799 responses.size < slowQuorumSize -> wait
    int maxvb = -2;                  // :1805-1807 only the responses of the highest voteBallot count
    for (int r = 0; r < n; ++r)
      if (((mask >> r) & 1u) && rv[r] > maxvb) maxvb = rv[r];
    if (b.as_intended) {             // :1810-1824 -- never true as the reference evaluates it (status is no Option)
      for (int r = 0; r < n && act == 0; ++r)
        if (((mask >> r) & 1u) && rv[r] == maxvb && rs[r] == CL_ACCEPTED) act = 1, src = r, tr = rt[r];
    }
    if (act == 0) {
      // :1830-1851 f matching PreAccepted triples of the default ballot, not from the recovering replica.  The
      // reference tests the ballot of the Prepare that was answered (p.ballot), which is the recovery ballot
      const int dflt = L;  // Ballot(0, leader) encoded: 0 * 8 + L
      const bool in_default = b.as_intended ? maxvb == dflt : (b.b_ord[i] * 8 + me) == dflt;
      for (int r = 0; r < n && act == 0 && in_default; ++r) {
        if (!((mask >> r) & 1u) || rv[r] != maxvb || rs[r] != CL_PRE_ACCEPTED || r == me) continue;
        const size_t cr = ((size_t)r * n + L) * st.num_instances + x;
        int same = 0;
        for (int q = 0; q < n; ++q) {
          if (!((mask >> q) & 1u) || rv[q] != maxvb || rs[q] != CL_PRE_ACCEPTED || q == me) continue;
          const size_t cq = ((size_t)q * n + L) * st.num_instances + x;
          // (the triples' dependencies are read from the command log, not from the replies: the caller keeps these
          // instances untouched between fpx_epx_prepare and this call -- include/fpx.h)
          bool eq = rt[q] == rt[r] && st.cl_dend[cq] == st.cl_dend[cr];
          for (int l = 0; l < n && eq; ++l) eq = st.cl_deps[cq * n + l] == st.cl_deps[cr * n + l];
          same += eq ? 1 : 0;
        }
        if (same >= f) act = 1, src = r, tr = rt[r];  // Util.popularItems(.., config.f)
      }
    }
    if (act == 0) {  // :1856-1868 start over, avoiding the fast path: with a pre-accepted command, else with a Noop
      act = 3;
      for (int r = 0; r < n && act == 3; ++r)
        if (((mask >> r) & 1u) && rv[r] == maxvb && rs[r] == CL_PRE_ACCEPTED) act = 2, src = r, tr = rt[r];
    }
  }
  if (b.action) b.action[i] = act;
  if (b.source) b.source[i] = src;
  if (b.triple) b.triple[i] = tr;
}

// ---- handlePreAccept in full (Replica.scala:1159-1289): ballots, Nacks, re-sent replies ------------------------
// Like Prepare / Accept above: messages delivered in array order to the replicas of target[i], instances pairwise
// distinct per batch -- so what a replica does with a message (process / Nack / answer again / ignore / answer with
// the Commit) follows from its command-log entry alone (k_hp_gate); the messages a replica processes run through
// K5's conflict scan in array order (sort by key, segmented prefix max) and k_hp_reply forms the PreAcceptOk's.
enum { HP_NONE = 0, HP_PROCESS = 1, HP_NACK = 2, HP_RESEND = 3, HP_IGNORE = 4, HP_COMMIT = 5 };
struct HpBatch {
  int m;
  const int32_t* leader;
  const int32_t* number;
  const int32_t* b_ord;
  const int32_t* b_rep;
  const int32_t* key;       // -1 = Noop; null in the multi-key form
  const int32_t* key_off;   // multi-key form (else null): message i's keys are keys[key_off[i] .. key_off[i + 1]), the pair
  const int32_t* keys;      // sequences are P long (pair j at position j: array order) and uniq[j] = 0 drops a repeated key
  const uint8_t* uniq;
  int P;
  const uint8_t* is_set;
  const int32_t* triple;    // may be null
  const int32_t* deps_in;   // [m][n]
  const int32_t* dend_in;   // [m] or null
  const uint8_t* target;
  uint8_t* ok_bits;
  uint8_t* resend_bits;
  uint8_t* nack_bits;
  uint8_t* commit_bits;
  int32_t* reply_deps;      // [m][n][n]
  int32_t* reply_end;       // [m][n]
  int32_t* reply_triple;    // [m][n]
  uint8_t* act;             // [n][m] scratch
  int32_t* contrib;         // [n][m] scratch (k_cl_tilemax / k_cl_nacks)
  uint8_t* nackflag;        // [n][m] scratch
  uint2* kv;                // [n][m] sort pairs
  const int32_t* conf;      // [m][n][NP] from k_epx_scan
  const int32_t* tick;      // [n][num_keys][2][n] from k_epx_scan
  uint32_t run_id;
};

__global__ void __launch_bounds__(256) k_hp_validate(const EpxState st, const HpBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n, L = b.leader[i], x = b.number[i], bo = b.b_ord[i], br = b.b_rep[i];
  const int k = b.key_off ? 0 : b.key[i];  // (key lists: checked on the host)
  bool ok = L >= 0 && L < n && x >= 0 && x < st.num_instances && bo >= 0 && bo < (1 << 27) && br >= 0 && br < n &&
            (b.target[i] >> n) == 0 && k >= -1 && k < st.num_keys;
  if (ok) {
    for (int l = 0; l < n; ++l) ok = ok && b.deps_in[(size_t)i * n + l] >= 0;
    // a PreAccept never depends on its own instance (:582); explicit values are the run number + 1 .. end - 1
    const int w = b.deps_in[(size_t)i * n + L], end = b.dend_in ? b.dend_in[i] : 0;
    ok = ok && (end == 0 ? w <= x : (w == x && end >= x + 2));
  }
  if (ok) ok = atomicExch(&st.cl_stamp[(size_t)L * st.num_instances + x], b.run_id) != b.run_id;
  if (!ok) epx_report(st.status, FPX_EINVAL, i);
}

// one thread per (replica, message), replica-major
__global__ void __launch_bounds__(256) k_hp_gate(const EpxState st, const HpBatch b) {
  const int n = st.n;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)b.m * n) return;
  const int r = (int)(t / b.m), i = (int)(t % b.m);
  int act = HP_NONE;
  const int L = b.leader[i], ballot = b.b_ord[i] * 8 + b.b_rep[i], k = b.key_off ? 0 : b.key[i];
  // (a malformed message is reported by k_hp_validate; here it only must not index out of bounds)
  if (((b.target[i] >> r) & 1u) && L >= 0 && L < n && b.number[i] >= 0 && b.number[i] < st.num_instances) {
    const size_t c = ((size_t)r * n + L) * st.num_instances + b.number[i];
    const int kind = st.cl_status[c];
    if (kind == CL_COMMITTED) act = HP_COMMIT;                                        // :1227-1238
    else if (kind != CL_NONE && ballot < st.cl_ballot[c]) act = HP_NACK;              // :1180-1184, 1189-1192, 1215-1218
    else if (kind == CL_PRE_ACCEPTED && ballot == st.cl_vote[c]) act = HP_RESEND;     // :1196-1210
    else if (kind == CL_ACCEPTED && ballot == st.cl_vote[c]) act = HP_IGNORE;         // :1222-1224
    else act = HP_PROCESS;
  }
  const size_t o = (size_t)r * b.m + i;
  b.act[o] = (uint8_t)act;
  b.contrib[o] = act == HP_PROCESS ? ballot : -1;   // :1251 largestBallot = max(largestBallot, preAccept.ballot)
  b.nackflag[o] = act == HP_NACK ? 1 : 0;
  // only what the replica processes takes part in its conflict scan; the rest (and Noops, :592-593) sorts last
  const bool scanned = act == HP_PROCESS && k >= 0 && k < st.num_keys;
  const uint32_t flags = ((uint32_t)(b.is_set[i] ? 1 : 0) << EPX_SET_SHIFT) | ((uint32_t)(L & 7) << EPX_LEADER_SHIFT);
  if (b.key_off) {  // one pair per (message, distinct key), in array order; the payload is the pair index
    for (int j = b.key_off[i]; j < b.key_off[i + 1]; ++j)
      b.kv[(size_t)r * b.P + j] = make_uint2((scanned && b.uniq[j] ? (uint32_t)b.keys[j] : (uint32_t)st.num_keys) | flags, (uint32_t)j);
    return;
  }
  b.kv[o] = make_uint2((scanned ? (uint32_t)k : (uint32_t)st.num_keys) | flags, (uint32_t)i);
}

// one thread per (message, replica): the reply and the new command-log entry
template <int N>
__global__ void __launch_bounds__(256) k_hp_reply(const EpxState st, const HpBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)b.m * N) return;
  const int i = (int)(t / N), r = (int)(t % N);
  constexpr int NP = ConfRow<N>::NP;
  const int act = b.act[(size_t)r * b.m + i];
  const int L = b.leader[i], x = b.number[i];
  const size_t c = ((size_t)r * N + L) * st.num_instances + x;
  int out[N], end = 0, tr = -1;
#pragma unroll
  for (int l = 0; l < N; ++l) out[l] = 0;
  uint8_t* bits = nullptr;
  if (act == HP_PROCESS) {
    const int ballot = b.b_ord[i] * 8 + b.b_rep[i];
    int row[N];
#pragma unroll
    for (int l = 0; l < N; ++l) row[l] = 0;
    if (b.key_off || b.key[i] >= 0) {  // computeSequenceNumberAndDependencies :569-600: the conflicts the scan found
      // (key lists: the row k_mk_merge formed from the command's pairs, zeros for a command without keys)
      const int32_t* cr = b.conf + ((size_t)i * N + r) * NP;
#pragma unroll
      for (int l = 0; l < N; ++l) row[l] = cr[l];
    }
    const int in_end = b.dend_in ? b.dend_in[i] : 0;
#pragma unroll
    for (int l = 0; l < N; ++l) {
      const int in = b.deps_in[(size_t)i * N + l];
      if (l == L) {
        // local {0 .. row-1} \ {x}  U  the message's own column (cover in_end, or its plain watermark): :582, :1257-1262
        const int cover = imax(row[l], in_end ? in_end : in);
        own_column(cover, x, &out[l], &end);
      } else {
        out[l] = imax(row[l], in);
      }
    }
    tr = b.triple ? b.triple[i] : -1;
    st.cl_status[c] = CL_PRE_ACCEPTED, st.cl_ballot[c] = ballot, st.cl_vote[c] = ballot, st.cl_triple[c] = tr;  // :1265-1276
#pragma unroll
    for (int l = 0; l < N; ++l) st.cl_deps[c * N + l] = out[l];
    st.cl_dend[c] = end;
    bits = b.ok_bits;
  } else if (act == HP_RESEND || act == HP_COMMIT) {
#pragma unroll
    for (int l = 0; l < N; ++l) out[l] = st.cl_deps[c * N + l];
    end = st.cl_dend[c], tr = st.cl_triple[c];
    bits = act == HP_RESEND ? b.resend_bits : b.commit_bits;
  } else if (act == HP_NACK) {
    bits = b.nack_bits;
  }
  if (bits) atomicOr(reinterpret_cast<unsigned int*>(bits) + (i >> 2), (1u << r) << (8 * (i & 3)));
  if (b.reply_deps) {
#pragma unroll
    for (int l = 0; l < N; ++l) b.reply_deps[((size_t)i * N + r) * N + l] = out[l];
  }
  if (b.reply_end) b.reply_end[(size_t)i * N + r] = end;
  if (b.reply_triple) b.reply_triple[(size_t)i * N + r] = tr;
}

// updateConflictIndex (:1279) at the replicas that processed: replica r's index learns what ITS scan saw
__global__ void __launch_bounds__(256) k_hp_commit(const EpxState st, const HpBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const long long per = (long long)st.num_keys * st.n;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= per * st.n) return;
  const int r = (int)(t / per);
  const long long e = t % per;
  const int k = (int)(e / st.n), l = (int)(e % st.n);
  const int32_t* seen = b.tick + (((size_t)r * st.num_keys + k) * 2) * st.n;
  int32_t* g = &st.gets[(size_t)r * per + e];
  int32_t* s2 = &st.sets[(size_t)r * per + e];
  if (seen[l] > *g) *g = seen[l];
  if (seen[st.n + l] > *s2) *s2 = seen[st.n + l];
}

#include "fpx_epaxos_mk.hpp"
#include "fpx_epx_leader.hpp"
#include "fpx_epx_recovery.hpp"
#include "fpx_epx_inbox.hpp"
#include "fpx_intern.hpp"
#include "fpx_wire_epx_dev.hpp"
#include "fpx_epx_cmds.hpp"
#include "fpx_wire_epx_enc_dev.hpp"

}  // namespace

struct fpx_epx {
  fpx_epx_config cfg;
  EpxState st;
  hipStream_t stream = nullptr, own_stream = nullptr;
  int last_hip = 0;
  DevBuf kv, kv2, seg, conf, tmp, tick, fusedb, metab;
  HostStage stage;                                         // the arrays of a host-pointer call and its held outputs (host_call)
  DevBuf mk_misc, mk_rec, mk_pair, mk_pconf;               // multi-key commands (fpx_epaxos_mk.hpp)
  int32_t* mk_host = nullptr;                              // page-locked: k_mk_total's line
  DevBuf p_fast, p_deps, p_ldeps, p_own;   // the four output arrays when a packed tick goes the first form's way
  DevBuf kp_hist, kp_recs, kp_misc;       // K5 second form (fpx_epaxos_kp.hpp)
  DevBuf dg_msg, dg_direct, dg_clo, dg_pre, dg_tmax, dg_pairs, dg_pairs2, dg_ctl, dg_key;  // device dependency-graph execution
  int32_t dg_seq = 0;
  int dg_rounds_hint = 8;                 // closure rounds the first chunk of the next fpx_epx_execute_dev enqueues (DG_ROUNDS at first)
  uint32_t* kp_flag = nullptr;            // page-locked: [0] sequence number of the tick whose count [1] is valid
  uint32_t* kp_flag_dev = nullptr;
  uint32_t kp_seq = 0;
  bool kp_lds_allowed = false, kp_off = false;
  int64_t census[FPX_EPX_CENSUS_WORDS] = {};       // fpx_epx_tick_census: the host's words (the device's are added when it is read)
  unsigned long long* census_dev = nullptr;        // [EPX_CD_WORDS]
  uint32_t cl_run = 0;
  EpxLeader ls = {nullptr, nullptr, nullptr};  // FPX_EPX_F_LEADER_STATE: Replica.leaderStates (fpx_epx_leader.hpp), else not
                                          // allocated; prep with FPX_EPX_F_RECOVERY (fpx_epx_recovery.hpp)
  DevBuf lr_misc;                         // fpx_epx_leader_replies: the decided flags and the compaction's block counts
  DevBuf ri_misc;                         // fpx_epx_replica_inbox: lay_epx_inbox
  DevBuf wire_misc;                       // fpx_wire_epx_leader_tick_dev: the decoded arrays of the tick
  InternTable keys = {};                  // fpx_epx_keys_enable: the key table (fpx_intern.hpp), else not allocated
  DevBuf keys_misc, rt_misc;              // fpx_epx_keys_intern_dev: lay_intern; the classify and the replica tick: their layouts
  DevBuf enc_misc;                        // fpx_wire_epx_encode_replica_replies_dev and the bytes tick: their layouts
  bool enc_direct = false;                // FPX_EPX_ENC_DIRECT: the reply encoder's direct form for every wavefront
  CmdStore cmds = {};                     // fpx_epx_cmds_enable: the command store (fpx_epx_cmds.hpp), else not allocated
  DevBuf cmds_misc;                       // a put: lay_epx_cmds_put
  bool cmds_bytewise = true;              // the command copy's single-byte form, the default; FPX_EPX_CMDS_WORDS: the 16-byte-word form
  bool lds_allowed = false, sort_lds_allowed = false;
  int num_cus = 256;
};

namespace {

// f(std::integral_constant<int, n>) for the replica counts a context can have (3, 5, 7)
template <typename F>
auto by_n(int n, F&& f) {
  switch (n) {
    case 3: return f(std::integral_constant<int, 3>());
    case 5: return f(std::integral_constant<int, 5>());
    default: return f(std::integral_constant<int, 7>());
  }
}

// the run id of a Prepare / Accept / handlePreAccept batch: the validation kernels stamp every instance with it, so the
// instances of one batch must be distinct
int next_run_id(fpx_epx* e, uint32_t* id) {
  if (++e->cl_run == 0) {  // stamp space exhausted: start over
    HIPCHK(e, hipMemsetAsync(e->st.cl_stamp, 0, (size_t)e->st.n * e->st.num_instances * 4, e->stream));
    e->cl_run = 1;
  }
  *id = e->cl_run;
  return FPX_OK;
}

// a packed tick that goes the first form's way writes the four output arrays into the context's own, packed at the end
int packed_fallback(fpx_epx* e, int m, uint8_t** fast, int32_t** deps, int32_t** leader_deps, int32_t** own_values_end) {
  const int n = e->st.n;
  int rc;
  if ((rc = grow(e, &e->p_fast, (size_t)m))) return rc;
  if ((rc = grow(e, &e->p_deps, (size_t)m * n * 4))) return rc;
  if ((rc = grow(e, &e->p_ldeps, (size_t)m * n * 4))) return rc;
  if ((rc = grow(e, &e->p_own, (size_t)m * 8))) return rc;
  *fast = (uint8_t*)e->p_fast.p, *deps = (int32_t*)e->p_deps.p, *leader_deps = (int32_t*)e->p_ldeps.p;
  *own_values_end = (int32_t*)e->p_own.p;
  return FPX_OK;
}

// ---- host-pointer calls: the shared driver (fpx_host.hpp), ended the way of this context -------------------------------
// fpx_epx_sync synchronises once and returns the device's status; the held outputs go to the caller when the call ends in
// FPX_OK or FPX_EFATAL_PROTOCOL
struct EpxEnd {
  fpx_epx* e;
  int operator()() const { return fpx_epx_sync(e); }
  static bool applied(int rc) { return rc == FPX_OK || rc == FPX_EFATAL_PROTOCOL; }
};
template <typename Launch>
int host_call(fpx_epx* e, std::initializer_list<Staged> arrays, Launch launch) {
  return fpx::host_call(e, arrays, launch, EpxEnd{e});
}

template <int N>
void launch_scan_decide(fpx_epx* e, const EpxBatch& b) {
  const int segs = N * e->st.num_keys;
  if (b.fused) {
    // keys whose commands fit the on-chip tables are scanned and decided by one workgroup each; the two kernels
    // below then only see what is left (usually nothing: they return at once)
    if (!e->lds_allowed) {  // more than the default 64 KiB of LDS needs an opt-in, per device: once per context
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_epx_key<N>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)KeyTile<N>::BYTES);
      e->lds_allowed = true;
    }
    hipLaunchKernelGGL((k_epx_key<N>), dim3(std::min(e->st.num_keys, e->num_cus)), dim3(KeyTile<N>::THREADS), KeyTile<N>::BYTES, e->stream, e->st, b);
  }
  hipLaunchKernelGGL((k_epx_scan<N>), dim3((segs + 3) / 4), dim3(256), 0, e->stream, e->st, b);
  hipLaunchKernelGGL((k_epx_decide<N>), dim3((b.m + 255) / 256), dim3(256), 0, e->stream, e->st, b);
}

template <int N>
void launch_hp(fpx_epx* e, const EpxBatch& sb, const HpBatch& hb, const MkMerge* mm = nullptr, bool scan = true) {
  const int segs = N * e->st.num_keys;
  if (scan) hipLaunchKernelGGL((k_epx_scan<N>), dim3((segs + 3) / 4), dim3(256), 0, e->stream, e->st, sb);
  // key lists: the command's row at a replica = the max of its pairs' rows (k_hp_reply reads the command's row)
  if (mm) hipLaunchKernelGGL((k_mk_merge<N>), dim3((mm->m + 255) / 256), dim3(256), 0, e->stream, e->st, *mm);
  hipLaunchKernelGGL((k_hp_reply<N>), dim3((unsigned)(((long long)hb.m * N + 255) / 256)), dim3(256), 0, e->stream, e->st, hb);
}

void launch_segments(fpx_epx* e, const EpxBatch& b, const uint32_t* key_totals, int key_buckets) {
  if (key_totals)
    hipLaunchKernelGGL(k_epx_segments_from_totals, dim3(e->st.n), dim3(256), 0, e->stream, e->st, b, key_totals, key_buckets);
  else
    hipLaunchKernelGGL(k_epx_segments, dim3((e->st.n * e->st.num_keys + 255) / 256), dim3(256), 0, e->stream, e->st, b);
}

// the bytes of e->tmp a sort of nseq sequences of m pairs on `bits` bits counts its digits in (radix_sort_pairs)
size_t radix_sort_bytes(size_t nseq, int m, unsigned bits) {
  const unsigned passes = (bits + RS_MAXW - 1) / RS_MAXW, width = (bits + passes - 1) / passes;
  return (nseq * ((m + RS_TILE - 1) / RS_TILE) + nseq) * ((size_t)4 << width);
}

// stable LSD radix sort of nseq sequences of m pairs on the low `bits` bits of the key word; returns the buffer that
// holds the result
uint2* radix_sort_pairs(fpx_epx* e, int nseq, int m, unsigned bits, uint2* a_buf, uint2* b_buf, const int32_t* check_rank, int* rc_out,
                        const uint32_t** key_totals, int* key_buckets) {
  const int n = nseq;
  const unsigned passes = (bits + RS_MAXW - 1) / RS_MAXW, width = (bits + passes - 1) / passes;
  const unsigned B = 1u << width;
  RsArgs a;
  a.m = m, a.tiles = (m + RS_TILE - 1) / RS_TILE;
  *rc_out = grow(e, &e->tmp, radix_sort_bytes(n, m, bits));
  if (*rc_out) return nullptr;
  a.hist = (uint32_t*)e->tmp.p, a.tot = a.hist + (size_t)n * a.tiles * B;
  if (!e->sort_lds_allowed) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_rs_scatter), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)RS_SCATTER_LDS);
    e->sort_lds_allowed = true;
  }
  uint2* buf[2] = {a_buf, b_buf};
  int cur = 0;
  for (unsigned shift = 0; shift < bits; shift += width, cur ^= 1) {
    a.shift = (int)shift;
    a.width = (int)width;
    a.rank = shift == 0 ? check_rank : nullptr;
    a.status = e->st.status;
    a.src = buf[cur], a.dst = buf[cur ^ 1];
    const dim3 tg(a.tiles, n);
    hipLaunchKernelGGL(k_rs_hist, tg, dim3(256), 0, e->stream, a);
    hipLaunchKernelGGL(k_rs_scan, dim3((B + 63) / 64, n), dim3(256), 0, e->stream, a);
    hipLaunchKernelGGL(k_rs_scatter, tg, dim3(64 * RS_SW), RS_SCATTER_LDS, e->stream, a);
  }
  // one pass: the digit was the whole key, its totals are the sizes of the key segments
  if (key_totals) *key_totals = passes == 1 ? a.tot : nullptr;
  if (key_buckets) *key_buckets = (int)B;
  return buf[cur];  // where the last pass left the sequence
}

unsigned key_bits(const fpx_epx* e) {
  unsigned bits = 1;
  while ((1u << bits) <= (unsigned)e->st.num_keys) ++bits;
  return bits;
}

// the n replicas' sequences of a tick on the key bits
uint2* sort_by_key(fpx_epx* e, int m, uint2* a_buf, uint2* b_buf, const int32_t* check_rank, int* rc_out,
                   const uint32_t** key_totals, int* key_buckets) {
  return radix_sort_pairs(e, e->st.n, m, key_bits(e), a_buf, b_buf, check_rank, rc_out, key_totals, key_buckets);
}

unsigned cell_bits(const fpx_epx* e) {  // the cells of the context: (to, leader, number)
  unsigned bits = 1;
  while (((uint64_t)1 << bits) < (uint64_t)e->st.n * e->st.n * e->st.num_instances) ++bits;
  return bits;
}

// a burst's (cell, message index) pairs on the cell bits: a cell's messages become one run, in delivery order
const uint2* sort_by_cell(fpx_epx* e, int m, uint2* a_buf, uint2* b_buf, int* rc_out) {
  return radix_sort_pairs(e, 1, m, cell_bits(e), a_buf, b_buf, nullptr, rc_out, nullptr, nullptr);
}

// the buffers of a conflict scan of m messages at the n replicas (K7's): the sort pairs twice, the rows a tick sees, the
// key segments, the conflicts.  Key lists (pairs >= 0): the sort pairs are per (message, key) pair, at least one
int grow_conflict_scan(fpx_epx* e, int m, int pairs = -1) {
  const int n = e->st.n, NP = n <= 4 ? 4 : 8;
  const size_t mn = (size_t)m * n, pn = pairs < 0 ? mn : (size_t)std::max(pairs, 1) * n;
  int rc;
  if ((rc = grow(e, &e->kv, pn * 8))) return rc;
  if ((rc = grow(e, &e->kv2, pn * 8))) return rc;
  if (pairs >= 0 && (rc = grow(e, &e->mk_pconf, pn * NP * 4))) return rc;
  if ((rc = grow(e, &e->tick, (size_t)n * e->st.num_keys * 2 * n * 4))) return rc;
  if ((rc = grow(e, &e->seg, (size_t)n * e->st.num_keys * 8))) return rc;
  return grow(e, &e->conf, mn * NP * 4);
}

// K7's sort and segments over the pairs the caller's kernels left in e->kv, in array order: *sb is what k_epx_scan takes
int sort_conflict_scan(fpx_epx* e, int m, const int32_t* number, EpxBatch* sb) {
  memset(sb, 0, sizeof(*sb));
  sb->m = m, sb->number = number, sb->kv = (uint2*)e->kv.p;
  const uint32_t* key_totals = nullptr;
  int key_buckets = 0, rc;
  sb->kv_sorted = sort_by_key(e, m, sb->kv, (uint2*)e->kv2.p, nullptr, &rc, &key_totals, &key_buckets);
  if (rc) return rc;
  sb->tick = (int32_t*)e->tick.p, sb->seg = (int32_t*)e->seg.p, sb->conf = (int32_t*)e->conf.p;
  launch_segments(e, *sb, key_totals, key_buckets);
  return FPX_OK;
}

// decided_index = the indices of the flagged messages of a burst, in message order, and their number (fpx_epx_leader.hpp);
// a caller that wants the number alone gets it without the placing
void launch_compaction(fpx_epx* e, int m, const LrScratch& s, int32_t* d_decided, int32_t* d_num_decided) {
  if (!d_decided && !d_num_decided) return;
  LrBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m, b.flag = s.flag, b.bsum = s.bsum, b.decided = d_decided, b.blocks = (m + LR_BLOCK - 1) / LR_BLOCK;
  const dim3 blk(256);
  hipLaunchKernelGGL(k_lr_count, dim3(b.blocks), blk, 0, e->stream, e->st, b);
  hipLaunchKernelGGL(k_lr_bscan, dim3(1), blk, 0, e->stream, e->st, b.bsum, b.blocks, (size_t)0, d_num_decided);
  if (d_decided) hipLaunchKernelGGL(k_lr_compact, dim3(b.blocks), blk, 0, e->stream, e->st, b);
}

// K5, second form: returns FPX_OK with *done = true when the tick went through it, *done = false when the first
// form has to take the tick (a key with more commands than the on-chip tables hold; nothing was applied)
template <int N>
int launch_kp(fpx_epx* e, const EpxBatch& b, int32_t* d_packed, bool* done) {
  using T = KpTile<N>;
  *done = false;
  KpArgs a;
  memset(&a, 0, sizeof(a));
  a.m = b.m, a.tiles = (b.m + KP_TILE - 1) / KP_TILE, a.B = e->st.num_keys;
  a.groups = (a.tiles + KP_HG - 1) / KP_HG;
  a.seq = ++e->kp_seq;
  int rc;
  if ((rc = grow(e, &e->kp_hist, (size_t)a.tiles * a.B * 2))) return rc;
  if ((rc = grow(e, &e->kp_recs, (size_t)a.B * T::TC * T::NI * 4))) return rc;
  {
    // fingerprints, control and verdict words, the census of the sort routes, one word per group of tiles (m < 2^21: at
    // most 128 groups), then the claim counters (one 64-byte sector per key): they must read zero before the first tick,
    // later the key kernel leaves them at zero.  (num_keys is the context's: the buffer grows once, the census is never lost)
    const size_t need = 1024 + (size_t)a.B * KP_TOT_STRIDE * 4;
    if (need > e->kp_misc.cap) {
      if ((rc = grow(e, &e->kp_misc, need))) return rc;
      HIPCHK(e, hipMemsetAsync(e->kp_misc.p, 0, e->kp_misc.cap, e->stream));
    }
  }
  char* misc = (char*)e->kp_misc.p;
  a.hist = (uint16_t*)e->kp_hist.p, a.recs = (uint32_t*)e->kp_recs.p;
  a.fp = (unsigned long long*)misc;              // 16 words of 8 bytes
  a.ctl = (uint32_t*)(misc + 128);               // 1 word
  a.bad = (uint32_t*)(misc + 192);               // 2 words
  // misc + 256: EPX_CD_SORTS words of 8 bytes, the census of k_epx_key2's sort routes.  The kernel reaches them from a.tot
  // (tot - KP_CENSUS_BACK), a pointer it holds anyway: a pointer of their own was two more registers at n = 5
  static_assert(1024 - KP_CENSUS_BACK * 4 == 256 && 256 + EPX_CD_SORTS * 8 <= 512, "the census words lie between bad and big");
  a.big = (uint32_t*)(misc + 512);               // [groups <= 128]
  a.tot = (uint32_t*)(misc + 1024);
  a.host_flag = e->kp_flag_dev, a.tc = T::TC;
  a.packed = d_packed, a.stride = fpx_epx_packed_stride(N);
  {
    uintptr_t bits = (uintptr_t)b.leader | (uintptr_t)b.key | (uintptr_t)b.number | (uintptr_t)b.rank | (uintptr_t)b.resp_mask |
                     (uintptr_t)b.is_set | (uintptr_t)b.seen_mask;
    a.vec = (bits & 15u) == 0 && (b.m & 3) == 0;
  }
  if (!a.vec) ++e->census[FPX_EPX_CENSUS_SCALAR_LOADS];
  if (!e->kp_lds_allowed) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_epx_key2<N, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)T::BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_epx_key2<N, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)T::BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_kp_hist), hipFuncAttributeMaxDynamicSharedMemorySize,
                              KP_HG * KP_MAXB * 4);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_kp_scatter<N>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)KpScat<N>::BYTES);
    e->kp_lds_allowed = true;
  }
  // (Round 4 tried the partition of tick t + 1 on a stream of its own beside the key kernel of tick t: the key kernel's
  // 15 wavefronts of 128 registers fill the register files of three of a CU's four SIMDs, no partition workgroup finds
  // room beside it, and the two event hops between the streams cost 15 us per tick -- 0.125 ms against 0.119 in order.)
  hipStream_t ps = e->stream;
  hipLaunchKernelGGL(k_kp_hist, dim3(a.groups), dim3(128 * KP_HG), (size_t)KP_HG * a.B * 4, ps, e->st, b, a);
  const int units = (a.tiles + KpScat<N>::TILES - 1) / KpScat<N>::TILES;
  hipLaunchKernelGGL((k_kp_scatter<N>), dim3(8 * ((units + 7) / 8)), dim3(KpScat<N>::THREADS), KpScat<N>::BYTES, ps, e->st, b, a);
  // k_epx_key2 is enqueued at once -- it returns at its first instruction when a key does not fit -- and the host then
  // learns, while the GPU works on, whether the first form has to take the tick after all (launching the kernel
  // only after the answer left the GPU idle for ~30 us per tick when ticks were enqueued back to back)
  const int grid = std::min(e->st.num_keys, e->num_cus);
  if (e->st.num_instances > 0)
    hipLaunchKernelGGL((k_epx_key2<N, true>), dim3(grid), dim3(T::THREADS), T::BYTES, e->stream, e->st, b, a);
  else
    hipLaunchKernelGGL((k_epx_key2<N, false>), dim3(grid), dim3(T::THREADS), T::BYTES, e->stream, e->st, b, a);
  volatile uint32_t* flag = e->kp_flag;
  bool seen = false;
  for (long spin = 0; spin < 200000000L; ++spin) {
    if (flag[0] == a.seq) { seen = true; break; }
    if ((spin & 0xffff) == 0xffff && hipStreamQuery(ps) != hipErrorNotReady) break;  // finished, or failed
  }
  if (!seen) {
    HIPCHK(e, hipStreamSynchronize(ps));
    if (flag[0] != a.seq) return FPX_EHIP;
  }
  if (flag[1] != 0) {  // a hot key: the first form takes the whole tick
    ++e->census[FPX_EPX_CENSUS_KP_HANDED_OVER];
    return FPX_OK;
  }
  ++e->census[FPX_EPX_CENSUS_KP];
  *done = true;
  return FPX_OK;
}

// bits of the closure hash that groups the cyclic vertices of one sort key into components.  FPX_DG_HASH_BITS (2 .. 22) is a
// test hook: with few bits different closures of one key share a hash, which is exactly the case needs_host_path reports
int dg_hash_bits() {
  const char* s = getenv("FPX_DG_HASH_BITS");
  const int b = s ? atoi(s) : DG_HASH_BITS;
  return b < 2 ? 2 : b > DG_HASH_BITS ? DG_HASH_BITS : b;
}

// What a form of the closure rounds brings to dg_run: its argument struct `a` (dg_run fills the DgCommon part), its row
// buffers, the launches in front of the first round and those of round k, its keys kernel, and its closures as the
// kernels behind the sorts read them.

// the wide form (fpx_depgraph_dev.hpp): 32-byte rows, every n and every column length
template <int N>
struct DgWide {
  static constexpr int NP = DgRow<N>::NP;
  static constexpr const char* name = "wide";
  DgArgs a{};
  // sizes and carves the rows; *behind = the `extra` bytes of dg_tmax behind the form's own
  int rows(fpx_epx* e, size_t extra, int32_t** behind) {
    for (int l = 0; l < N; ++l) a.tiles[l] = (a.count[l] + DG_TILE - 1) / DG_TILE, a.tile_base[l] = a.ntiles, a.ntiles += a.tiles[l];
    for (int l = N; l < 8; ++l) a.tile_base[l] = a.ntiles;
    int rc;
    if ((rc = grow(e, &e->dg_direct, (size_t)a.m * NP * 4))) return rc;
    if ((rc = grow(e, &e->dg_clo, (size_t)a.m * NP * 4))) return rc;
    if ((rc = grow(e, &e->dg_pre, (size_t)a.m * NP * 4))) return rc;
    if ((rc = grow(e, &e->dg_tmax, (size_t)DG_SUB * a.ntiles * NP * 4 + extra))) return rc;
    a.direct = (int32_t*)e->dg_direct.p, a.clo = (int32_t*)e->dg_clo.p, a.pre = (int32_t*)e->dg_pre.p;
    a.tmax = (int32_t*)e->dg_tmax.p, *behind = a.tmax + (size_t)DG_SUB * a.ntiles * NP;
    return FPX_OK;
  }
  void before_rounds(hipStream_t st, int grid) {
    hipLaunchKernelGGL((k_dg_scatter<N>), dim3(grid), dim3(256), 0, st, a);
    // round 1 scans from the direct covers' tile maxima; every later round from what the gather before it folded
    hipLaunchKernelGGL((k_dg_tilemax<N>), dim3(a.ntiles), dim3(256), 0, st, a);
  }
  void round(hipStream_t st, int k) {
    hipLaunchKernelGGL((k_dg_prefix<N>), dim3(a.ntiles), dim3(256), 0, st, a, k);
    hipLaunchKernelGGL((k_dg_relax<N>), dim3(a.ntiles * DG_SUB), dim3(256), 0, st, a, k);
  }
  void keys(hipStream_t st, int grid) { hipLaunchKernelGGL((k_dg_keys<N>), dim3(grid), dim3(256), 0, st, a); }
  DgClosures<N> closures() const { return {a.clo}; }
};

// the packed form (fpx_depgraph_pk.hpp): 16-byte rows, n <= 5 and columns of at most PK_MAX_COUNT instances
template <int N>
struct DgPacked {
  static_assert(N <= 5, "five 21-bit watermarks per 16-byte row");
  static constexpr const char* name = "packed";
  DpArgs a{};
  int cur = 0;  // the half of lp / bt / cy the next round gathers from
  int rows(fpx_epx* e, size_t extra, int32_t** behind) {
    for (int l = 0; l < N; ++l) a.nblk[l] = (a.count[l] + 255) / 256, a.blk_base[l] = a.nblocks, a.nblocks += a.nblk[l];
    for (int l = N; l < 8; ++l) a.blk_base[l] = a.nblocks;
    const size_t nb = (size_t)std::max(a.nblocks, 1);
    int rc;
    if ((rc = grow(e, &e->dg_direct, (size_t)a.m * 16))) return rc;
    if ((rc = grow(e, &e->dg_clo, (size_t)a.m * 16))) return rc;
    if ((rc = grow(e, &e->dg_pre, (size_t)a.m * 32))) return rc;
    if ((rc = grow(e, &e->dg_tmax, nb * 16 * 4 + extra))) return rc;
    a.direct = (ulonglong2*)e->dg_direct.p, a.clo = (ulonglong2*)e->dg_clo.p;
    a.lp[0] = (ulonglong2*)e->dg_pre.p, a.lp[1] = a.lp[0] + a.m;
    a.bt[0] = (ulonglong2*)e->dg_tmax.p, a.bt[1] = a.bt[0] + nb, a.cy[0] = a.bt[1] + nb, a.cy[1] = a.cy[0] + nb;
    *behind = (int32_t*)(a.cy[1] + nb);
    return FPX_OK;
  }
  void before_rounds(hipStream_t st, int grid) {
    hipLaunchKernelGGL((k_dp_scatter<N>), dim3(grid), dim3(256), 0, st, a);
    hipLaunchKernelGGL((k_dp_scan0<N>), dim3(dp_grid(a.nblocks)), dim3(256), 0, st, a);
    hipLaunchKernelGGL((k_dp_carry<N>), dim3(N), dim3(1024), 0, st, a, 0, 1);
  }
  void round(hipStream_t st, int k) {
    // round k gathers from half `cur` and leaves its scan in the other half.  (A skipped round does not flip anything on
    // the device, but after the round that moved nothing both halves hold the same, final values.)
    hipLaunchKernelGGL((k_dp_relax<N>), dim3(dp_grid(a.nblocks)), dim3(256), 0, st, a, cur, k);
    hipLaunchKernelGGL((k_dp_carry<N>), dim3(N), dim3(1024), 0, st, a, cur ^ 1, k);
    cur ^= 1;
  }
  void keys(hipStream_t st, int grid) { hipLaunchKernelGGL((k_dp_keys<N>), dim3(dp_grid(grid)), dim3(256), 0, st, a); }
  DpClosures closures() const { return {a.clo}; }
};

// one tick through one form: the closure rounds in chunks until nothing moves, keys, the two sorts, component starts
template <int N, class Form>
int dg_run(fpx_epx* e, Form& form, int m, const int32_t* d_leader, const int32_t* d_number, const int32_t* d_packed, const uint8_t* d_mask,
           const int32_t* first, const int32_t* count, int32_t* d_order, int32_t* d_comp, int64_t* nexec, int64_t* ncomp,
           int32_t* needs_host) {
  using Clo = decltype(form.closures());
  DgCommon& a = form.a;
  a.m = m, a.n = N, a.stride = fpx_epx_packed_stride(N);
  for (int l = 0, base = 0; l < 8; base += a.count[l], ++l) {  // (the columns behind N are empty: their base is m)
    if (l < N) a.first[l] = first[l], a.count[l] = count[l];
    a.base[l] = base;
  }
  int rc;
  const int out_tiles = (m + DG_TILE - 1) / DG_TILE;
  const int grid = (m + 255) / 256;
  if ((rc = form.rows(e, ((size_t)out_tiles + (size_t)grid) * 4 + 64, &a.tstarts))) return rc;
  a.belig = a.tstarts + out_tiles;
  if ((rc = grow(e, &e->dg_msg, (size_t)m * 4))) return rc;
  if ((rc = grow(e, &e->dg_pairs, (size_t)m * 8))) return rc;
  if ((rc = grow(e, &e->dg_pairs2, (size_t)m * 8))) return rc;
  if ((rc = grow(e, &e->dg_key, (size_t)m * 4))) return rc;
  if ((rc = grow(e, &e->dg_ctl, 256))) return rc;
  if (!e->kp_flag_dev) return FPX_EHIP;
  a.leader = d_leader, a.number = d_number, a.packed = d_packed, a.mask = d_mask;
  a.msg_of = (int32_t*)e->dg_msg.p;
  a.pairs = (uint2*)e->dg_pairs.p, a.pairs2 = (uint2*)e->dg_pairs2.p, a.ctl = (int32_t*)e->dg_ctl.p;
  a.key32 = (uint32_t*)e->dg_key.p;
  a.host = reinterpret_cast<volatile int32_t*>(e->kp_flag_dev + 8);  // the second half of the page-locked line
  a.order = d_order, a.comp = d_comp;
  volatile int32_t* host = reinterpret_cast<volatile int32_t*>(e->kp_flag + 8);
  const int call = (++e->dg_seq) & 0xffff;
  a.count_moved = getenv("FPX_DG_DEBUG") ? 1 : 0;
  a.hash_bits = dg_hash_bits();
  auto wait_for = [&](int chunk) -> int {
    const int32_t want = call * 64 + chunk;
    for (long spin = 0; spin < 400000000L; ++spin) {
      if (host[7] == want) return FPX_OK;
      if ((spin & 0xfffff) == 0xfffff) {  // now and then: did the stream die?  (hipErrorNotReady is what a live one answers;
        const hipError_t q = hipStreamQuery(e->stream);  // it must not stay behind as the thread's last error)
        (void)hipGetLastError();
        if (q != hipErrorNotReady) break;
      }
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return host[7] == want ? FPX_OK : FPX_EHIP;
  };
  HIPCHK(e, hipMemsetAsync(a.msg_of, 0xFF, (size_t)m * 4, e->stream));
  HIPCHK(e, hipMemsetAsync(a.ctl, 0, 256, e->stream));
  form.before_rounds(e->stream, grid);
  const Clo clo = form.closures();
  int enqueued = 0, executables = 0;
  for (int chunk = 0;; ++chunk) {
    // A chunk of closure rounds at once: a round returns at its first instruction when the one before it moved nothing,
    // and everything behind them is enqueued right away -- one host read per chunk, and a full chunk covers 2^8 hops
    if (chunk > 0) HIPCHK(e, hipMemsetAsync(a.ctl + 8, 0, (DG_ROUNDS + 1) * 4, e->stream));
    // How many rounds to enqueue: a round that finds "the one before moved nothing" leaves at its first instruction, but it
    // is still a launch (and its second kernel another): ~8 us per skipped round, four of them per FIFO tick.  The first
    // chunk enqueues one round more than moved something in the context's previous call (ticks of one deployment need the
    // same depth, 4 with FIFO channels, 7 - 8 with reordering ones); a tick that needs more gets full chunks as before.
    const int rounds = chunk == 0 ? std::max(2, std::min(DG_ROUNDS, e->dg_rounds_hint)) : DG_ROUNDS;
    for (int k = 1; k <= rounds; ++k) form.round(e->stream, k);
    enqueued += rounds;
    // (ctl[3], the executables, is WRITTEN by the rekey kernel's first workgroup since round 6 and ctl[4], the components,
    // by the emit kernel's last: nothing accumulates in them any more, so nothing has to be cleared in front of the keys)
    form.keys(e->stream, grid);
    // least significant first: the closures' hashes, then (stable) the closure sums and kinds
    uint2* sorted = radix_sort_pairs(e, 1, m, (unsigned)a.hash_bits, a.pairs, a.pairs2, nullptr, &rc, nullptr, nullptr);
    if (rc) return rc;
    if (sorted != a.pairs) std::swap(a.pairs, a.pairs2);
    hipLaunchKernelGGL(k_dg_rekey, dim3(grid), dim3(256), 0, e->stream, a);
    unsigned key_bits = 2;  // the keys are 3 x sum + kind <= 3 m + 2; an inexecutable vertex is all ones: strictly behind them
    while (((1ull << key_bits) - 1) <= 3ull * (unsigned long long)m + 2) ++key_bits;
    sorted = radix_sort_pairs(e, 1, m, key_bits, a.pairs, a.pairs2, nullptr, &rc, nullptr, nullptr);
    if (rc) return rc;
    if (sorted != a.pairs) std::swap(a.pairs, a.pairs2);
    // (the number of executables stays on the device: both kernels cover all m positions and leave at once beyond it)
    hipLaunchKernelGGL((k_dg_count_starts<Clo>), dim3(out_tiles), dim3(256), 0, e->stream, a, clo);
    hipLaunchKernelGGL((k_dg_emit<Clo>), dim3(out_tiles), dim3(256), 0, e->stream, a, clo);
    a.seq = call * 64 + (chunk & 31) + 1;
    hipLaunchKernelGGL(k_dg_publish, dim3(1), dim3(64), 0, e->stream, a, rounds);
    if ((rc = wait_for((chunk & 31) + 1))) return rc;
    if (host[1] != 0) return FPX_EINVAL;        // an instance outside its column, twice, or missing
    e->dg_rounds_hint = host[5] != 0 ? DG_ROUNDS : host[6] + 1;
    if (a.count_moved) {
      int32_t dbg[64];
      HIPCHK(e, hipMemcpy(dbg, a.ctl, sizeof(dbg), hipMemcpyDeviceToHost));
      fprintf(stderr, "libfpx: depgraph (%s) chunk %d, vertices moved per round:", Form::name, chunk);
      for (int k = 1; k <= DG_ROUNDS; ++k) fprintf(stderr, " %d", dbg[24 + k]);
      fprintf(stderr, " (%d rounds enqueued)\n", rounds);
    }
    executables = host[3];
    if (host[5] == 0) break;                    // the chunk's last round moved nothing: converged
    if (enqueued >= 48) return FPX_EHIP;        // (a round doubles the hops covered: 2^48 hops do not exist)
  }
  if (nexec) *nexec = executables;
  if (ncomp) *ncomp = executables > 0 ? host[4] : 0;
  if (needs_host) *needs_host = host[2];
  return launch_check(e);
}

// device dependency-graph execution of one tick's commits (fpx_depgraph_dev.hpp): checks the columns, chooses the form
template <int N>
int dg_execute(fpx_epx* e, int m, const int32_t* d_leader, const int32_t* d_number, const int32_t* d_packed, const uint8_t* d_mask,
               const int32_t* first, const int32_t* count, int32_t* d_order, int32_t* d_comp, int64_t* nexec, int64_t* ncomp,
               int32_t* needs_host) {
  long long total = 0;
  for (int l = 0; l < N; ++l) {
    if (first[l] < 0 || count[l] < 0) return FPX_EINVAL;
    // ids are int32 and "beyond the column" has to be expressible: the column ends at DG_ID_END at the latest
    if ((long long)first[l] + count[l] > DG_ID_END) return FPX_EINVAL;
    total += count[l];
  }
  if (total != m) return FPX_EINVAL;  // the columns are dense: every instance first[l] .. first[l] + count[l] - 1, once
  if constexpr (N <= 5) {
    bool fits = !getenv("FPX_DG_WIDE");
    for (int l = 0; l < N; ++l) fits = fits && count[l] <= PK_MAX_COUNT;
    if (fits) {
      DgPacked<N> form;
      return dg_run<N>(e, form, m, d_leader, d_number, d_packed, d_mask, first, count, d_order, d_comp, nexec, ncomp, needs_host);
    }
  }
  DgWide<N> form;
  return dg_run<N>(e, form, m, d_leader, d_number, d_packed, d_mask, first, count, d_order, d_comp, nexec, ncomp, needs_host);
}

}  // namespace

extern "C" {

int32_t fpx_epx_create(const fpx_epx_config* cfg, fpx_epx** out) {
  if (!cfg || !out) return FPX_EINVAL;
  *out = nullptr;
  const int n = cfg->num_replicas;
  if (!(n == 3 || n == 5 || n == 7) || cfg->num_keys < 1 || cfg->num_keys > (1 << 24) || cfg->num_instances < 0 ||
      (int64_t)cfg->num_instances * n > (int64_t)1 << 30)
    return FPX_EINVAL;
  // leader state lives beside the command log; its cells are a sort key of fpx_epx_leader_replies (31 bits)
  if ((cfg->flags & FPX_EPX_F_LEADER_STATE) &&
      (cfg->num_instances <= 0 || (int64_t)cfg->num_instances * n * n > (int64_t)1 << 31))
    return FPX_EINVAL;
  // the Preparing phase is one more phase of the leader state
  if ((cfg->flags & FPX_EPX_F_RECOVERY) && !(cfg->flags & FPX_EPX_F_LEADER_STATE)) return FPX_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev)
    return FPX_ENODEVICE;
  fpx_epx* e = new (std::nothrow) fpx_epx();
  if (!e) return FPX_ENOMEM;
  e->cfg = *cfg;
  e->st.n = n;
  e->st.num_keys = cfg->num_keys;
  e->st.gets = e->st.sets = e->st.status = nullptr;
  e->st.num_instances = cfg->num_instances;
  e->st.cl_status = nullptr, e->st.cl_ballot = e->st.cl_vote = e->st.cl_triple = e->st.largest = nullptr, e->st.cl_stamp = nullptr;
  e->st.cl_deps = e->st.cl_dend = nullptr;
  auto fail = [&](int code) {
    fpx_epx_destroy(e);
    return code;
  };
  DeviceScope _dg(cfg->device);
  if (hipSetDevice(cfg->device) != hipSuccess) return fail(FPX_ENODEVICE);
  if (hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking) != hipSuccess) return fail(FPX_EHIP);
  e->stream = e->own_stream;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0)
      e->num_cus = prop.multiProcessorCount;
  }
  const size_t cells = (size_t)n * cfg->num_keys * n;
  if (hipMalloc((void**)&e->st.gets, cells * 4) != hipSuccess) return fail(FPX_ENOMEM);
  if (hipMalloc((void**)&e->st.sets, cells * 4) != hipSuccess) return fail(FPX_ENOMEM);
  if (hipMalloc((void**)&e->st.status, 32) != hipSuccess) return fail(FPX_ENOMEM);
  // TopOne.scala:10: every watermark starts at 0
  if (hipMemsetAsync(e->st.gets, 0, cells * 4, e->stream) != hipSuccess) return fail(FPX_EHIP);
  if (hipMemsetAsync(e->st.sets, 0, cells * 4, e->stream) != hipSuccess) return fail(FPX_EHIP);
  if (hipMemsetAsync(e->st.status, 0, 32, e->stream) != hipSuccess) return fail(FPX_EHIP);
  {
    // Replica.scala:458  largestBallot = Ballot(0, index)  (encoded 0 * 8 + index)
    int32_t init[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    if (hipMalloc((void**)&e->st.largest, 32) != hipSuccess) return fail(FPX_ENOMEM);
    if (hipMemcpy(e->st.largest, init, 32, hipMemcpyHostToDevice) != hipSuccess) return fail(FPX_EHIP);
  }
  if (cfg->num_instances > 0) {
    const size_t ce = (size_t)n * n * cfg->num_instances;
    if (hipMalloc((void**)&e->st.cl_status, ce) != hipSuccess) return fail(FPX_ENOMEM);
    if (hipMalloc((void**)&e->st.cl_ballot, ce * 4) != hipSuccess) return fail(FPX_ENOMEM);
    if (hipMalloc((void**)&e->st.cl_vote, ce * 4) != hipSuccess) return fail(FPX_ENOMEM);
    if (hipMalloc((void**)&e->st.cl_triple, ce * 4) != hipSuccess) return fail(FPX_ENOMEM);
    if (hipMalloc((void**)&e->st.cl_stamp, (size_t)n * cfg->num_instances * 4) != hipSuccess) return fail(FPX_ENOMEM);
    if (hipMalloc((void**)&e->st.cl_deps, ce * n * 4) != hipSuccess) return fail(FPX_ENOMEM);
    if (hipMalloc((void**)&e->st.cl_dend, ce * 4) != hipSuccess) return fail(FPX_ENOMEM);
    if (hipMemsetAsync(e->st.cl_deps, 0, ce * n * 4, e->stream) != hipSuccess) return fail(FPX_EHIP);
    if (hipMemsetAsync(e->st.cl_dend, 0, ce * 4, e->stream) != hipSuccess) return fail(FPX_EHIP);
    if (hipMemsetAsync(e->st.cl_status, 0, ce, e->stream) != hipSuccess) return fail(FPX_EHIP);
    if (hipMemsetAsync(e->st.cl_ballot, 0xFF, ce * 4, e->stream) != hipSuccess) return fail(FPX_EHIP);
    if (hipMemsetAsync(e->st.cl_vote, 0xFF, ce * 4, e->stream) != hipSuccess) return fail(FPX_EHIP);
    if (hipMemsetAsync(e->st.cl_triple, 0xFF, ce * 4, e->stream) != hipSuccess) return fail(FPX_EHIP);
    if (hipMemsetAsync(e->st.cl_stamp, 0, (size_t)n * cfg->num_instances * 4, e->stream) != hipSuccess) return fail(FPX_EHIP);
    if (cfg->flags & FPX_EPX_F_LEADER_STATE) {
      // every head starts as "not led" (phase 0); a response row is read only once its bit of the head is set
      if (hipMalloc((void**)&e->ls.head, ce * sizeof(int4)) != hipSuccess) return fail(FPX_ENOMEM);
      if (hipMalloc((void**)&e->ls.resp, ce * n * (n + 2) * 4) != hipSuccess) return fail(FPX_ENOMEM);
      if (hipMemsetAsync(e->ls.head, 0, ce * sizeof(int4), e->stream) != hipSuccess) return fail(FPX_EHIP);
      // (a PrepareOk's row of prep, like a response row, is read only once its bit of the head is set)
      if ((cfg->flags & FPX_EPX_F_RECOVERY) && hipMalloc((void**)&e->ls.prep, ce * n * sizeof(int2)) != hipSuccess)
        return fail(FPX_ENOMEM);
    }
  }
  // the word k_kp_scatter tells the host through (did a key of the tick outgrow the on-chip tables?)
  if (hipHostMalloc((void**)&e->kp_flag, 64, hipHostMallocDefault) == hipSuccess) {
    memset(e->kp_flag, 0, 64);
    if (hipHostGetDevicePointer((void**)&e->kp_flag_dev, e->kp_flag, 0) != hipSuccess) e->kp_flag_dev = nullptr;
  } else {
    e->kp_flag = nullptr;
    (void)hipGetLastError();
  }
  e->kp_off = getenv("FPX_EPX_V1") != nullptr;
  e->enc_direct = getenv("FPX_EPX_ENC_DIRECT") != nullptr;
  e->cmds_bytewise = getenv("FPX_EPX_CMDS_WORDS") == nullptr;
  if (hipMalloc((void**)&e->census_dev, EPX_CD_WORDS * 8) != hipSuccess) return fail(FPX_ENOMEM);
  if (hipMemsetAsync(e->census_dev, 0, EPX_CD_WORDS * 8, e->stream) != hipSuccess) return fail(FPX_EHIP);
  if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(FPX_EHIP);
  *out = e;
  return FPX_OK;
}

int32_t fpx_epx_destroy(fpx_epx* e) {
  if (!e) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  void* ps[] = {e->st.gets, e->st.sets, e->st.status, e->st.cl_status, e->st.cl_ballot, e->st.cl_vote, e->st.cl_triple,
                e->st.largest, e->st.cl_stamp, e->st.cl_deps, e->st.cl_dend, e->ls.head, e->ls.resp, e->ls.prep, e->census_dev,
                e->keys.slot, e->keys.first, e->keys.key_off, e->keys.arena, e->keys.meta,
                e->cmds.off, e->cmds.len, e->cmds.claim, e->cmds.arena, e->cmds.meta};
  for (void* p : ps)
    if (p) (void)hipFree(p);
  DevBuf* bs[] = {&e->kv, &e->kv2, &e->seg, &e->conf, &e->tmp, &e->tick, &e->fusedb, &e->metab, &e->mk_misc, &e->mk_rec,
                  &e->mk_pair, &e->mk_pconf, &e->lr_misc, &e->ri_misc, &e->wire_misc, &e->keys_misc, &e->rt_misc, &e->enc_misc,
                  &e->cmds_misc};
  for (DevBuf* b : bs)
    if (b->p) (void)hipFree(b->p);
  free_stage(&e->stage);
  if (e->mk_host) (void)hipHostFree(e->mk_host);
  for (DevBuf* b : {&e->kp_hist, &e->kp_recs, &e->kp_misc, &e->p_fast, &e->p_deps, &e->p_ldeps, &e->p_own, &e->dg_msg, &e->dg_direct,
                    &e->dg_clo, &e->dg_pre, &e->dg_tmax, &e->dg_pairs, &e->dg_pairs2, &e->dg_ctl, &e->dg_key})
    if (b->p) (void)hipFree(b->p);
  if (e->kp_flag) (void)hipHostFree(e->kp_flag);
  if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
  delete e;
  return FPX_OK;
}

int32_t fpx_epx_set_stream(fpx_epx* e, void* hip_stream) {
  if (!e) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->stream = hip_stream == FPX_STREAM_OWN ? e->own_stream : (hipStream_t)hip_stream;
  return FPX_OK;
}

int32_t fpx_epx_sync(fpx_epx* e) {
  if (!e) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  int32_t h[EPX_ST_ENC + 1] = {};
  HIPCHK(e, hipMemcpyAsync(h, e->st.status, sizeof(h), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (h[0] != 0 || h[EPX_ST_ENC] != 0) {
    HIPCHK(e, hipMemsetAsync(e->st.status, 0, 32, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
  }
  // (the reply encoder's per-call code, fpx_wire_epx_enc_dev.hpp: reported when nothing else is)
  return h[0] != 0 ? h[0] : h[EPX_ST_ENC];
}

// key lists (the _mk entry points): key_off[0] = 0, non-decreasing, at most FPX_EPX_MK_MAX_PAIRS keys, each in [0, num_keys)
static int check_key_lists(int32_t m, const int32_t* key_off, const int32_t* keys, int num_keys, int64_t* P) {
  if (!key_off || key_off[0] != 0) return FPX_EINVAL;
  for (int32_t i = 0; i < m; ++i)
    if (key_off[i + 1] < key_off[i]) return FPX_EINVAL;
  *P = key_off[m];
  if (*P > FPX_EPX_MK_MAX_PAIRS || (*P > 0 && !keys)) return FPX_EINVAL;
  for (int64_t j = 0; j < *P; ++j)
    if (keys[j] < 0 || keys[j] >= num_keys) return FPX_EINVAL;
  return FPX_OK;
}

static int32_t preaccept_dev_impl(fpx_epx* e, int32_t m, const int32_t* d_leader, const int32_t* d_number,
                                  const int32_t* d_key, const uint8_t* d_is_set, const uint8_t* d_resp_mask,
                                  const uint8_t* d_seen_mask, const int32_t* d_rank, const int32_t* d_triple_id,
                                  uint8_t* d_fast, int32_t* d_deps, int32_t* d_leader_deps, int32_t* d_own_values_end,
                                  int32_t* d_packed) {
  if (!e || m < 0) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) return FPX_OK;
  const int n = e->st.n;
  int rc;
  // the second form (fpx_epaxos_kp.hpp): one partition pass by key, everything else on chip -- when the keys are
  // one LDS counter each and ranks and slots share a 32-bit sort word
  const int kp_tc = by_n(n, [](auto N) { return KpTile<N>::TC; });
  if (!e->kp_off && e->kp_flag_dev && e->st.num_keys <= KP_MAXB && m < (1 << 21) &&
      (long long)m <= (long long)e->st.num_keys * kp_tc &&  // (else some key must overflow the on-chip tables)
      ((e->st.num_instances == 0 && !d_triple_id) || n >= 5)) {  // (n = 3 with a command log: the first form)
    EpxBatch kb;
    memset(&kb, 0, sizeof(kb));
    kb.m = m, kb.leader = d_leader, kb.number = d_number, kb.key = d_key, kb.is_set = d_is_set, kb.resp_mask = d_resp_mask;
    kb.seen_mask = d_seen_mask, kb.rank = d_rank, kb.triple = d_triple_id;
    kb.fast = d_fast, kb.deps = d_deps, kb.leader_deps = d_leader_deps, kb.own_values_end = d_own_values_end;
    bool done = false;
    if ((rc = by_n(n, [&](auto N) { return launch_kp<N>(e, kb, d_packed, &done); }))) return rc;
    if (done) return launch_check(e);
  } else {
    // fpx_epx_tick_census: why the second form was not tried -- the first reason that holds, in the header's order
    const int why = e->kp_off || !e->kp_flag_dev                            ? FPX_EPX_CENSUS_V1_SWITCHED_OFF
                    : e->st.num_keys > KP_MAXB                              ? FPX_EPX_CENSUS_V1_KEYS
                    : (long long)m > (long long)e->st.num_keys * kp_tc      ? FPX_EPX_CENSUS_V1_FULL
                    : !((e->st.num_instances == 0 && !d_triple_id) || n >= 5) ? FPX_EPX_CENSUS_V1_LOG_N3
                                                                            : FPX_EPX_CENSUS_V1_INDEX_BITS;
    ++e->census[why];
  }
  if (d_packed && (rc = packed_fallback(e, m, &d_fast, &d_deps, &d_leader_deps, &d_own_values_end))) return rc;
  if ((rc = grow(e, &e->kv, (size_t)n * m * 8))) return rc;
  if ((rc = grow(e, &e->kv2, (size_t)n * m * 8))) return rc;
  if ((rc = grow(e, &e->tick, (size_t)n * e->st.num_keys * 2 * n * 4))) return rc;
  if ((rc = grow(e, &e->seg, (size_t)n * e->st.num_keys * 8))) return rc;
  if ((rc = grow(e, &e->conf, (size_t)m * n * (n <= 4 ? 4 : 8) * 4))) return rc;
  EpxBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m, b.leader = d_leader, b.number = d_number, b.key = d_key, b.is_set = d_is_set, b.resp_mask = d_resp_mask;
  b.seen_mask = d_seen_mask;
  b.rank = d_rank;
  b.triple = d_triple_id;
  b.kv = (uint2*)e->kv.p, b.kv_sorted = (uint2*)e->kv2.p;
  b.tick = (int32_t*)e->tick.p;
  b.seg = (int32_t*)e->seg.p, b.conf = (int32_t*)e->conf.p;
  b.fast = d_fast, b.deps = d_deps, b.leader_deps = d_leader_deps, b.own_values_end = d_own_values_end;
  b.census = e->census_dev;
  // the per-key on-chip path (k_epx_key): message indices must fit its 21-bit hash words, one workgroup per key
  const bool key_kernel = m < (1 << 21) - 1 && e->st.num_keys <= (1 << 16) && !getenv("FPX_EPX_NO_KEY_TILES");
  if (!key_kernel) ++e->census[FPX_EPX_CENSUS_NO_KEY_KERNEL];
  if (key_kernel) {
    if ((rc = grow(e, &e->fusedb, (size_t)e->st.num_keys + 64))) return rc;
    b.unfused = (int32_t*)e->fusedb.p;
    b.fused = (uint8_t*)e->fusedb.p + 64;
    if ((rc = grow(e, &e->metab, (size_t)m * 8))) return rc;
    b.meta = (int2*)e->metab.p;
  }
  // (counting the first pass's histogram in k_epx_keys with global atomics was tried: 5 M atomics on 327 k counters
  // took 450 us against 22 us for the histogram kernel)
  hipLaunchKernelGGL(k_epx_keys, dim3((m + 255) / 256), dim3(256), 0, e->stream, e->st, b);
  // stable LSD radix sort on the key bits only (the sequence already is in delivery order)
  const uint32_t* key_totals = nullptr;
  int key_buckets = 0;
  b.kv_sorted = sort_by_key(e, m, b.kv, b.kv_sorted, d_rank, &rc, &key_totals, &key_buckets);
  if (rc) return rc;
  launch_segments(e, b, key_totals, key_buckets);
  by_n(n, [&](auto N) { launch_scan_decide<N>(e, b); });
  const long long tot = (long long)e->st.num_keys * n * n;
  hipLaunchKernelGGL(k_epx_commit, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, e->stream, e->st, b);
  if (d_packed)
    hipLaunchKernelGGL(k_epx_pack, dim3((m + 255) / 256), dim3(256), 0, e->stream, e->st, m, d_fast, d_deps, d_leader_deps,
                       d_own_values_end, d_packed, fpx_epx_packed_stride(n));
  return launch_check(e);
}

int32_t fpx_epx_packed_stride(int32_t num_replicas) { return (2 * num_replicas + 3 + 3) / 4 * 4; }

int32_t fpx_epx_execute_dev(fpx_epx* e, int32_t m, const int32_t* d_leader, const int32_t* d_number, const int32_t* d_packed,
                            const uint8_t* d_committed, const int32_t* first, const int32_t* count, int32_t* d_order,
                            int32_t* d_component, int64_t* num_executed, int64_t* num_components, int32_t* needs_host_path) {
  if (!e || m < 0 || !first || !count || (m > 0 && (!d_leader || !d_number || !d_packed || !d_order || !d_component))) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (num_executed) *num_executed = 0;
  if (num_components) *num_components = 0;
  if (needs_host_path) *needs_host_path = 0;
  if (m == 0) return FPX_OK;
  if (m >= (1 << 21)) return FPX_EINVAL;
  return by_n(e->st.n, [&](auto N) {
    return dg_execute<N>(e, m, d_leader, d_number, d_packed, d_committed, first, count, d_order, d_component, num_executed,
                         num_components, needs_host_path);
  });
}

int32_t fpx_epx_execute(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* deps,
                        const int32_t* deps_values_end, const uint8_t* committed, const int32_t* first, const int32_t* count,
                        int32_t* order, int32_t* component, int64_t* num_executed, int64_t* num_components,
                        int32_t* needs_host_path) {
  if (!e || m < 0 || !first || !count || (m > 0 && (!leader || !number || !deps || !order || !component))) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (num_executed) *num_executed = 0;
  if (num_components) *num_components = 0;
  if (needs_host_path) *needs_host_path = 0;
  if (m == 0) return FPX_OK;
  const int n = e->st.n, stride = fpx_epx_packed_stride(n);
  // the packed lines fpx_epx_preaccept_packed_dev would have written: deps | leader_deps (unused here) | own_values_end | fast
  std::vector<int32_t> lines;
  try {
    lines.assign((size_t)m * stride, 0);
  } catch (const std::bad_alloc&) {  // (no exception crosses the C ABI)
    return FPX_ENOMEM;
  }
  for (int i = 0; i < m; ++i) {
    if (leader[i] < 0 || leader[i] >= n) return FPX_EINVAL;
    int32_t* line = lines.data() + (size_t)i * stride;
    for (int l = 0; l < n; ++l) line[l] = deps[(size_t)i * n + l];
    line[2 * n] = deps_values_end ? deps_values_end[i] : 0;
  }
  const int32_t *d_leader, *d_number, *d_packed;
  const uint8_t* d_mask;
  int32_t *d_order, *d_comp;
  auto launch = [&]() -> int {
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (the host arrays and `lines` may be pageable)
    int64_t ne = 0, nc = 0;
    int32_t nh = 0;
    const int rc = fpx_epx_execute_dev(e, m, d_leader, d_number, d_packed, committed ? d_mask : nullptr, first, count, d_order,
                                       d_comp, &ne, &nc, &nh);
    if (rc) return rc;
    if (ne > 0 && !nh) {  // (the executed entries only)
      HIPCHK(e, hipMemcpyAsync(order, d_order, (size_t)ne * 4, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipMemcpyAsync(component, d_comp, (size_t)ne * 4, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    if (num_executed) *num_executed = ne;
    if (num_components) *num_components = nc;
    if (needs_host_path) *needs_host_path = nh;
    return FPX_OK;
  };
  return host_call(e, {in(d_leader, leader, m), in(d_number, number, m), in(d_packed, lines.data(), lines.size()),
                       in(d_mask, committed, m), scratch(d_order, m), scratch(d_comp, m)},
                   launch);
}

int32_t fpx_epx_preaccept_dev(fpx_epx* e, int32_t m, const int32_t* d_leader, const int32_t* d_number,
                              const int32_t* d_key, const uint8_t* d_is_set, const uint8_t* d_resp_mask,
                              const uint8_t* d_seen_mask, const int32_t* d_rank, const int32_t* d_triple_id,
                              uint8_t* d_fast, int32_t* d_deps, int32_t* d_leader_deps, int32_t* d_own_values_end) {
  return preaccept_dev_impl(e, m, d_leader, d_number, d_key, d_is_set, d_resp_mask, d_seen_mask, d_rank, d_triple_id, d_fast,
                            d_deps, d_leader_deps, d_own_values_end, nullptr);
}

int32_t fpx_epx_preaccept_packed_dev(fpx_epx* e, int32_t m, const int32_t* d_leader, const int32_t* d_number,
                                     const int32_t* d_key, const uint8_t* d_is_set, const uint8_t* d_resp_mask,
                                     const uint8_t* d_seen_mask, const int32_t* d_rank, const int32_t* d_triple_id,
                                     int32_t* d_packed) {
  if (!d_packed && m > 0) return FPX_EINVAL;
  return preaccept_dev_impl(e, m, d_leader, d_number, d_key, d_is_set, d_resp_mask, d_seen_mask, d_rank, d_triple_id, nullptr,
                            nullptr, nullptr, nullptr, d_packed);
}

// K5 with key lists: every command one key -> the single-key tick as it is (keys as key); otherwise the pair form
// (fpx_epaxos_mk.hpp).  One host wait: k_mk_prep's totals (pair count, distinct pairs, commands without exactly one key)
// decide the route and size the pair buffers; a bad list is caught there, before anything is applied.
static int32_t preaccept_mk_impl(fpx_epx* e, int32_t m, const int32_t* d_leader, const int32_t* d_number, const int32_t* d_off,
                                 const int32_t* d_keys, const uint8_t* d_is_set, const uint8_t* d_resp_mask,
                                 const uint8_t* d_seen_mask, const int32_t* d_rank, const int32_t* d_triple_id, uint8_t* d_fast,
                                 int32_t* d_deps, int32_t* d_leader_deps, int32_t* d_own_values_end, int32_t* d_packed) {
  if (!e || m < 0) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) return FPX_OK;
  if (!d_off) return FPX_EINVAL;
  const int n = e->st.n;
  const int tiles = (m + MK_TILE - 1) / MK_TILE;
  int rc;
  const int blocks = (m + 255) / 256;
  MkPrologueScratch ps;
  if ((rc = carve(e, &e->mk_misc, &ps, [&](Carver& c) { return lay_mk_prologue(c, m, n, tiles, blocks); }))) return rc;
  if (!e->mk_host && hipHostMalloc((void**)&e->mk_host, 64, hipHostMallocDefault) != hipSuccess) {
    e->mk_host = nullptr;
    return FPX_ENOMEM;
  }
  MkBatch mb;
  memset(&mb, 0, sizeof(mb));
  mb.m = m, mb.tiles = tiles, mb.off = d_off, mb.keys = d_keys, mb.leader = d_leader, mb.number = d_number;
  mb.is_set = d_is_set, mb.resp_mask = d_resp_mask, mb.seen_mask = d_seen_mask, mb.rank = d_rank;
  mb.info = ps.info, mb.ucnt = ps.ucnt, mb.tsum = ps.tsum, mb.part = (int2*)ps.part;
  const dim3 gm(blocks), blk(256);
  hipLaunchKernelGGL(k_mk_prep, gm, blk, 0, e->stream, e->st, mb);
  hipLaunchKernelGGL(k_mk_total, dim3(1), blk, 0, e->stream, e->st, mb, blocks);
  int32_t* h = e->mk_host;  // page-locked
  HIPCHK(e, hipMemcpyAsync(h, mb.info, 16, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (h[3] != 0) return fpx_epx_sync(e);  // (returns the status and clears it)
  const int U = h[0], P = h[2];
  if (P > FPX_EPX_MK_MAX_PAIRS) return FPX_EINVAL;
  if (h[1] == 0)  // key_off[i] = i: today's tick, on chip where it fits
    return preaccept_dev_impl(e, m, d_leader, d_number, d_keys, d_is_set, d_resp_mask, d_seen_mask, d_rank, d_triple_id, d_fast,
                              d_deps, d_leader_deps, d_own_values_end, d_packed);
  if (d_packed && (rc = packed_fallback(e, m, &d_fast, &d_deps, &d_leader_deps, &d_own_values_end))) return rc;
  const int NP = n <= 4 ? 4 : 8, Ux = std::max(U, 1);
  if ((rc = grow(e, &e->mk_rec, (size_t)n * m * 16))) return rc;
  MkPairScratch pairs;
  if ((rc = carve(e, &e->mk_pair, &pairs, [&](Carver& c) { return lay_mk_pairs(c, P); }))) return rc;
  if ((rc = grow(e, &e->mk_pconf, (size_t)std::max(P, 1) * n * NP * 4))) return rc;
  if ((rc = grow(e, &e->kv, (size_t)n * Ux * 8))) return rc;
  if ((rc = grow(e, &e->kv2, (size_t)n * Ux * 8))) return rc;
  if ((rc = grow(e, &e->tick, (size_t)n * e->st.num_keys * 2 * n * 4))) return rc;
  if ((rc = grow(e, &e->seg, (size_t)n * e->st.num_keys * 8))) return rc;
  if ((rc = grow(e, &e->conf, (size_t)m * n * NP * 4))) return rc;
  mb.P = P, mb.U = U, mb.rec = (int4*)e->mk_rec.p, mb.kv = (uint2*)e->kv.p;
  mb.pnum = pairs.pnum, mb.uniq = pairs.uniq;
  hipLaunchKernelGGL(k_mk_pairs, gm, blk, 0, e->stream, mb);
  hipLaunchKernelGGL(k_mk_place, gm, blk, 0, e->stream, e->st, mb);
  hipLaunchKernelGGL(k_mk_tilesum, dim3(tiles, n), blk, 0, e->stream, mb);
  hipLaunchKernelGGL(k_mk_tilescan, dim3(n), blk, 0, e->stream, mb);
  hipLaunchKernelGGL(k_mk_scatter, dim3(tiles, n), blk, 0, e->stream, e->st, mb);
  // the pairs through K5's first form: sort by key (stable: delivery order within a key), segments, scan -> pair rows
  EpxBatch sb;
  memset(&sb, 0, sizeof(sb));
  sb.m = U, sb.number = mb.pnum, sb.kv = mb.kv, sb.kv_sorted = (uint2*)e->kv2.p;
  sb.tick = (int32_t*)e->tick.p, sb.seg = (int32_t*)e->seg.p, sb.conf = (int32_t*)e->mk_pconf.p;
  if (U > 0) {
    const uint32_t* key_totals = nullptr;
    int key_buckets = 0;
    sb.kv_sorted = sort_by_key(e, U, sb.kv, sb.kv_sorted, nullptr, &rc, &key_totals, &key_buckets);
    if (rc) return rc;
    launch_segments(e, sb, key_totals, key_buckets);
  }
  // ... and the commands: merged rows -> k_epx_decide as in the first form
  EpxBatch db;
  memset(&db, 0, sizeof(db));
  db.m = m, db.leader = d_leader, db.number = d_number, db.is_set = d_is_set, db.resp_mask = d_resp_mask;
  db.seen_mask = d_seen_mask, db.rank = d_rank, db.triple = d_triple_id, db.conf = (int32_t*)e->conf.p;
  db.fast = d_fast, db.deps = d_deps, db.leader_deps = d_leader_deps, db.own_values_end = d_own_values_end;
  MkMerge mm;
  memset(&mm, 0, sizeof(mm));
  mm.m = m, mm.off = d_off, mm.uniq = mb.uniq, mm.pconf = sb.conf, mm.conf = db.conf, mm.leader = d_leader;
  mm.resp_mask = d_resp_mask, mm.seen_mask = d_seen_mask;
  const int segs = n * e->st.num_keys;
  by_n(n, [&](auto N) {
    if (U > 0) hipLaunchKernelGGL((k_epx_scan<N>), dim3((segs + 3) / 4), blk, 0, e->stream, e->st, sb);
    hipLaunchKernelGGL((k_mk_merge<N>), gm, blk, 0, e->stream, e->st, mm);
    hipLaunchKernelGGL((k_epx_decide<N>), gm, blk, 0, e->stream, e->st, db);
  });
  const long long tot = (long long)e->st.num_keys * n * n;
  if (U > 0) hipLaunchKernelGGL(k_epx_commit, dim3((unsigned)((tot + 255) / 256)), blk, 0, e->stream, e->st, sb);
  if (d_packed)
    hipLaunchKernelGGL(k_epx_pack, gm, blk, 0, e->stream, e->st, m, d_fast, d_deps, d_leader_deps, d_own_values_end, d_packed,
                       fpx_epx_packed_stride(n));
  return launch_check(e);
}

int32_t fpx_epx_preaccept_mk_dev(fpx_epx* e, int32_t m, const int32_t* d_leader, const int32_t* d_number, const int32_t* d_key_offsets,
                                 const int32_t* d_keys, const uint8_t* d_is_set, const uint8_t* d_resp_mask,
                                 const uint8_t* d_seen_mask, const int32_t* d_rank, const int32_t* d_triple_id, uint8_t* d_fast,
                                 int32_t* d_deps, int32_t* d_leader_deps, int32_t* d_own_values_end) {
  return preaccept_mk_impl(e, m, d_leader, d_number, d_key_offsets, d_keys, d_is_set, d_resp_mask, d_seen_mask, d_rank,
                           d_triple_id, d_fast, d_deps, d_leader_deps, d_own_values_end, nullptr);
}

int32_t fpx_epx_preaccept_mk_packed_dev(fpx_epx* e, int32_t m, const int32_t* d_leader, const int32_t* d_number,
                                        const int32_t* d_key_offsets, const int32_t* d_keys, const uint8_t* d_is_set,
                                        const uint8_t* d_resp_mask, const uint8_t* d_seen_mask, const int32_t* d_rank,
                                        const int32_t* d_triple_id, int32_t* d_packed) {
  if (!d_packed && m > 0) return FPX_EINVAL;
  return preaccept_mk_impl(e, m, d_leader, d_number, d_key_offsets, d_keys, d_is_set, d_resp_mask, d_seen_mask, d_rank,
                           d_triple_id, nullptr, nullptr, nullptr, nullptr, d_packed);
}

// fpx_epx_preaccept and fpx_epx_preaccept_mk: one key per command (key) or key lists (key_off / keys)
static int32_t preaccept_host(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* key,
                              const int32_t* key_off, const int32_t* keys, const uint8_t* is_set, const uint8_t* resp_mask,
                              const uint8_t* seen_mask, const int32_t* rank, const int32_t* triple_id, uint8_t* fast,
                              int32_t* deps, int32_t* leader_deps, int32_t* own_values_end) {
  if (!e || m < 0 || (m > 0 && (!leader || !number || !(key || key_off) || !is_set || !resp_mask || !rank))) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) return FPX_OK;
  const int n = e->st.n;
  int64_t P = 0;
  int rc;
  if (key_off && (rc = check_key_lists(m, key_off, keys, e->st.num_keys, &P))) return rc;
  const int32_t *d_leader, *d_number, *d_key, *d_off, *d_keys, *d_rank, *d_triple;
  const uint8_t *d_set, *d_mask, *d_seen;
  uint8_t* d_fast;
  int32_t *d_deps, *d_ldeps, *d_own;
  auto launch = [&]() -> int {
    const uint8_t* seen = seen_mask ? d_seen : nullptr;
    const int32_t* triple = triple_id ? d_triple : nullptr;
    if (key_off)
      return preaccept_mk_impl(e, m, d_leader, d_number, d_off, d_keys, d_set, d_mask, seen, d_rank, triple, d_fast, d_deps, d_ldeps,
                               d_own, nullptr);
    return preaccept_dev_impl(e, m, d_leader, d_number, d_key, d_set, d_mask, seen, d_rank, triple, d_fast, d_deps, d_ldeps, d_own,
                              nullptr);
  };
  return host_call(e, {in(d_leader, leader, m), in(d_number, number, m), in(d_key, key, key_off ? 0 : m),
                       in(d_off, key_off, key_off ? m + 1 : 0), in(d_keys, keys, P), in(d_set, is_set, m), in(d_mask, resp_mask, m),
                       in(d_seen, seen_mask, m), in(d_rank, rank, (size_t)n * m), in(d_triple, triple_id, m), out(d_fast, fast, m),
                       out(d_deps, deps, (size_t)m * n), out(d_ldeps, leader_deps, (size_t)m * n), out(d_own, own_values_end, (size_t)m * 2)},
                   launch);
}

int32_t fpx_epx_preaccept(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* key,
                          const uint8_t* is_set, const uint8_t* resp_mask, const uint8_t* seen_mask,
                          const int32_t* rank, const int32_t* triple_id, uint8_t* fast, int32_t* deps,
                          int32_t* leader_deps, int32_t* own_values_end) {
  return preaccept_host(e, m, leader, number, key, nullptr, nullptr, is_set, resp_mask, seen_mask, rank, triple_id, fast, deps,
                        leader_deps, own_values_end);
}

int32_t fpx_epx_preaccept_mk(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* key_offsets,
                             const int32_t* keys, const uint8_t* is_set, const uint8_t* resp_mask, const uint8_t* seen_mask,
                             const int32_t* rank, const int32_t* triple_id, uint8_t* fast, int32_t* deps, int32_t* leader_deps,
                             int32_t* own_values_end) {
  return preaccept_host(e, m, leader, number, nullptr, key_offsets, keys, is_set, resp_mask, seen_mask, rank, triple_id, fast, deps,
                        leader_deps, own_values_end);
}

// Prepare / Accept on the command log: stage, validate, handle, scan the largestBallot's, (Accept) tally + commit
static int32_t cl_run(fpx_epx* e, int accept, int32_t m, const int32_t* leader, const int32_t* number,
                      const int32_t* b_ord, const int32_t* b_rep, const int32_t* triple, const int32_t* key,
                      const uint8_t* is_set, const uint8_t* target, uint8_t* ok_bits, uint8_t* nack_bits,
                      uint8_t* commit_bits, int32_t* nack_ballot, uint8_t* committed, int32_t* reply_status,
                      int32_t* reply_vote, int32_t* reply_triple, const int32_t* key_off = nullptr,
                      const int32_t* keys = nullptr) {
  if (!e || m < 0) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (e->st.num_instances <= 0) return FPX_EINVAL;
  if (m == 0) return FPX_OK;
  if (!leader || !number || !b_ord || !b_rep || !target || (accept && (!triple || !(key || key_off) || !is_set))) return FPX_EINVAL;
  const int n = e->st.n;
  int64_t P = 0;
  int rc;
  if (key_off && (rc = check_key_lists(m, key_off, keys, e->st.num_keys, &P))) return rc;
  const int tiles = (m + CL_TILE - 1) / CL_TILE;
  const size_t mn = (size_t)m * n;
  const int32_t *d_leader, *d_number, *d_bo, *d_br, *d_tr, *d_key, *d_off, *d_keys;
  const uint8_t *d_set, *d_tgt;
  uint8_t *d_ok, *d_nack, *d_com, *d_skip, *d_done, *d_flag;
  int32_t *d_nb, *d_rs, *d_rv, *d_rt, *d_contrib, *d_tm;
  auto launch = [&]() -> int {
    ClBatch b;
    memset(&b, 0, sizeof(b));
    b.m = m, b.accept = accept, b.leader = d_leader, b.number = d_number, b.b_ord = d_bo, b.b_rep = d_br, b.triple = d_tr;
    b.key = d_key, b.is_set = d_set;
    if (key_off) b.key_off = d_off, b.keys = d_keys;
    b.target = d_tgt, b.ok_bits = d_ok, b.nack_bits = d_nack, b.commit_bits = d_com, b.nack_ballot = d_nb;
    b.committed = d_done, b.reply_status = d_rs, b.reply_vote = d_rv, b.reply_triple = d_rt;
    b.contrib = d_contrib, b.nackflag = d_flag, b.tilemax = d_tm, b.skip = d_skip;
    int rc2;
    if ((rc2 = next_run_id(e, &b.run_id))) return rc2;
    const dim3 gm((m + 255) / 256), blk(256);
    hipLaunchKernelGGL(k_cl_validate, gm, blk, 0, e->stream, e->st, b);
    if (accept) hipLaunchKernelGGL(k_cl_propose, gm, blk, 0, e->stream, e->st, b);
    hipLaunchKernelGGL(k_cl_handle, dim3((unsigned)(((long long)m * n + 255) / 256)), blk, 0, e->stream, e->st, b);
    hipLaunchKernelGGL(k_cl_tilemax, dim3(tiles, n), blk, 0, e->stream, b, tiles);
    hipLaunchKernelGGL(k_cl_tilescan, dim3(n), blk, 0, e->stream, e->st, b, tiles);
    hipLaunchKernelGGL(k_cl_nacks, dim3(tiles, n), blk, 0, e->stream, b, tiles);
    if (accept) hipLaunchKernelGGL(k_cl_commit, gm, blk, 0, e->stream, e->st, b);
    return FPX_OK;
  };
  // ok, nack, commit, skip and committed start at 0 (one memset), nack_ballot at -1
  return host_call(e, {in(d_leader, leader, m), in(d_number, number, m), in(d_bo, b_ord, m), in(d_br, b_rep, m), in(d_tr, triple, m),
                       in(d_key, key, m), in(d_off, key_off, key_off ? m + 1 : 0), in(d_keys, keys, P), in(d_set, is_set, m),
                       in(d_tgt, target, m), out(d_ok, ok_bits, m, 0), out(d_nack, nack_bits, m, 0), out(d_com, commit_bits, m, 0),
                       scratch(d_skip, m, 0), out(d_done, committed, m, 0), out(d_nb, nack_ballot, m, 0xFF),
                       out(d_rs, reply_status, mn), out(d_rv, reply_vote, mn), out(d_rt, reply_triple, mn), scratch(d_contrib, mn),
                       scratch(d_flag, mn), scratch(d_tm, (size_t)n * tiles)},
                   launch);
}

int32_t fpx_epx_prepare(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* ballot_ordering,
                        const int32_t* ballot_replica, const uint8_t* target_mask, uint8_t* ok_bits, uint8_t* nack_bits,
                        uint8_t* commit_bits, int32_t* nack_ballot, int32_t* reply_status, int32_t* reply_vote_ballot,
                        int32_t* reply_triple) {
  return cl_run(e, 0, m, leader, number, ballot_ordering, ballot_replica, nullptr, nullptr, nullptr, target_mask, ok_bits,
                nack_bits, commit_bits, nack_ballot, nullptr, reply_status, reply_vote_ballot, reply_triple);
}

static int32_t handle_commit_impl(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* triple_id,
                                  const int32_t* key, const int32_t* key_off, const int32_t* keys, const uint8_t* is_set,
                                  const int32_t* deps, const int32_t* deps_values_end, const uint8_t* target_mask) {
  if (!e || m < 0) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (e->st.num_instances <= 0) return FPX_EINVAL;
  if (m == 0) return FPX_OK;
  if (!leader || !number || !triple_id || !(key || key_off) || !is_set || !target_mask) return FPX_EINVAL;
  const int n = e->st.n;
  int64_t P = 0;
  if (key_off && check_key_lists(m, key_off, keys, e->st.num_keys, &P)) return FPX_EINVAL;
  for (int i = 0; i < m; ++i) {  // host arrays: checked here, nothing is applied on a bad one
    if (leader[i] < 0 || leader[i] >= n || number[i] < 0 || number[i] >= e->st.num_instances ||
        (!key_off && (key[i] < -1 || key[i] >= e->st.num_keys)) || (target_mask[i] >> n) != 0)
      return FPX_EINVAL;
    if (deps) {
      for (int l = 0; l < n; ++l)
        if (deps[(size_t)i * n + l] < 0) return FPX_EINVAL;
      const int end = deps_values_end ? deps_values_end[i] : 0;
      if (end != 0 && (end <= number[i] + 1 || deps[(size_t)i * n + leader[i]] > number[i])) return FPX_EINVAL;
    }
  }
  // who writes the entry: walking the batch from its end, a message leaves to the later messages of its instance the
  // replicas they go to
  std::vector<uint8_t> writer;
  std::vector<std::pair<long long, int>> order;
  try {
    writer.resize((size_t)m), order.resize((size_t)m);
  } catch (const std::bad_alloc&) {  // (no exception crosses the C ABI)
    return FPX_ENOMEM;
  }
  {
    for (int i = 0; i < m; ++i) order[i] = {(long long)leader[i] * e->st.num_instances + number[i], i};
    std::sort(order.begin(), order.end());
    for (size_t a = 0; a < order.size();) {
      size_t z = a;
      while (z < order.size() && order[z].first == order[a].first) ++z;
      unsigned later = 0;
      for (size_t q = z; q-- > a;) {  // the instance's messages, last first
        const int i = order[q].second;
        writer[i] = (uint8_t)(target_mask[i] & ~later);
        later |= target_mask[i];
      }
      a = z;
    }
  }
  const int32_t *d_leader, *d_number, *d_tr, *d_key, *d_off, *d_keys, *d_end, *d_deps;
  const uint8_t *d_set, *d_tgt, *d_wr;
  auto launch = [&]() -> int {
    LcBatch b;
    b.m = m, b.leader = d_leader, b.number = d_number, b.triple = d_tr, b.key = d_key, b.is_set = d_set;
    b.key_off = key_off ? d_off : nullptr, b.keys = key_off ? d_keys : nullptr;
    b.deps = deps ? d_deps : nullptr, b.deps_end = (deps && deps_values_end) ? d_end : nullptr, b.target = d_tgt, b.writer = d_wr;
    hipLaunchKernelGGL(k_cl_learn_commit, dim3((unsigned)(((long long)m * n + 255) / 256)), dim3(256), 0, e->stream, e->st, b);
    return FPX_OK;
  };
  return host_call(e, {in(d_leader, leader, m), in(d_number, number, m), in(d_tr, triple_id, m), in(d_key, key, m),
                       in(d_end, deps ? deps_values_end : nullptr, m), in(d_set, is_set, m), in(d_tgt, target_mask, m),
                       in(d_wr, writer.data(), m), in(d_deps, deps, (size_t)m * n), in(d_off, key_off, key_off ? m + 1 : 0),
                       in(d_keys, keys, P)},
                   launch);
}

int32_t fpx_epx_handle_prepare_oks(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number,
                                   const int32_t* ballot_ordering, const int32_t* ballot_replica, const uint8_t* resp_mask,
                                   const int32_t* reply_status, const int32_t* reply_vote_ballot, const int32_t* reply_triple,
                                   int32_t as_intended, int32_t* action, int32_t* source, int32_t* triple) {
  if (!e || m < 0) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (e->st.num_instances <= 0) return FPX_EINVAL;
  if (m == 0) return FPX_OK;
  if (!leader || !number || !ballot_ordering || !ballot_replica || !resp_mask || !reply_status || !reply_vote_ballot || !reply_triple)
    return FPX_EINVAL;
  const int n = e->st.n;
  const size_t mn = (size_t)m * n;
  const int32_t *d_leader, *d_number, *d_bo, *d_br, *d_rs, *d_rv, *d_rt;
  const uint8_t* d_mask;
  int32_t *d_act, *d_src, *d_tr;
  auto launch = [&]() -> int {
    RcBatch b;
    memset(&b, 0, sizeof(b));
    b.m = m, b.as_intended = as_intended ? 1 : 0, b.leader = d_leader, b.number = d_number, b.b_ord = d_bo, b.b_rep = d_br;
    b.resp_mask = d_mask, b.rs = d_rs, b.rv = d_rv, b.rt = d_rt, b.action = d_act, b.source = d_src, b.triple = d_tr;
    hipLaunchKernelGGL(k_cl_recover, dim3((m + 255) / 256), dim3(256), 0, e->stream, e->st, b);
    return FPX_OK;
  };
  return host_call(e, {in(d_leader, leader, m), in(d_number, number, m), in(d_bo, ballot_ordering, m), in(d_br, ballot_replica, m),
                       out(d_act, action, m), out(d_src, source, m), out(d_tr, triple, m), in(d_mask, resp_mask, m),
                       in(d_rs, reply_status, mn), in(d_rv, reply_vote_ballot, mn), in(d_rt, reply_triple, mn)},
                   launch);
}

int32_t fpx_epx_accept(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* ballot_ordering,
                       const int32_t* ballot_replica, const int32_t* triple_id, const int32_t* key, const uint8_t* is_set,
                       const uint8_t* target_mask, uint8_t* ok_bits, uint8_t* nack_bits, uint8_t* commit_bits,
                       int32_t* nack_ballot, uint8_t* committed) {
  return cl_run(e, 1, m, leader, number, ballot_ordering, ballot_replica, triple_id, key, is_set, target_mask, ok_bits,
                nack_bits, commit_bits, nack_ballot, committed, nullptr, nullptr, nullptr);
}

static int32_t handle_preaccept_impl(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number,
                                     const int32_t* ballot_ordering, const int32_t* ballot_replica, const int32_t* key,
                                     const int32_t* key_off, const int32_t* keys,
                                     const uint8_t* is_set, const int32_t* triple_id, const int32_t* deps_in,
                                     const int32_t* deps_in_values_end, const uint8_t* target_mask, uint8_t* ok_bits,
                                     uint8_t* resend_bits, uint8_t* nack_bits, uint8_t* commit_bits, int32_t* nack_ballot,
                                     int32_t* reply_deps, int32_t* reply_values_end, int32_t* reply_triple) {
  if (!e || m < 0) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (e->st.num_instances <= 0) return FPX_EINVAL;
  if (m == 0) return FPX_OK;
  if (!leader || !number || !ballot_ordering || !ballot_replica || !(key || key_off) || !is_set || !deps_in || !target_mask)
    return FPX_EINVAL;
  const int n = e->st.n;
  // key lists: P pairs in array order instead of m messages in the scan (pair j of the CSR at position j)
  int64_t P64 = 0;
  if (key_off && check_key_lists(m, key_off, keys, e->st.num_keys, &P64)) return FPX_EINVAL;
  const int P = key_off ? (int)P64 : m;
  const int tiles = (m + CL_TILE - 1) / CL_TILE;
  const size_t mn = (size_t)m * n;
  const int NP = n <= 4 ? 4 : 8;
  int rc;
  if ((rc = grow(e, &e->kv, (size_t)n * std::max(P, 1) * 8))) return rc;
  if ((rc = grow(e, &e->kv2, (size_t)n * std::max(P, 1) * 8))) return rc;
  if ((rc = grow(e, &e->tick, (size_t)n * e->st.num_keys * 2 * n * 4))) return rc;
  if ((rc = grow(e, &e->seg, (size_t)n * e->st.num_keys * 8))) return rc;
  if ((rc = grow(e, &e->conf, (size_t)m * n * NP * 4))) return rc;
  MkPairScratch pairs = {nullptr, nullptr};
  if (key_off) {
    if ((rc = carve(e, &e->mk_pair, &pairs, [&](Carver& c) { return lay_mk_pairs(c, P); }))) return rc;
    if ((rc = grow(e, &e->mk_pconf, (size_t)std::max(P, 1) * n * NP * 4))) return rc;
  }
  const int32_t *d_leader, *d_number, *d_bo, *d_br, *d_key, *d_tr, *d_dend, *d_din, *d_off, *d_keys;
  const uint8_t *d_set, *d_tgt;
  uint8_t *d_ok, *d_resend, *d_nack, *d_com, *d_act, *d_flag;
  int32_t *d_nb, *d_rd, *d_re, *d_rt, *d_contrib, *d_tm;
  auto launch = [&]() -> int {
    int32_t* d_pconf = nullptr;
    MkBatch mb;
    memset(&mb, 0, sizeof(mb));
    if (key_off) {
      d_pconf = (int32_t*)e->mk_pconf.p;
      mb.m = m, mb.P = P, mb.off = d_off, mb.keys = d_keys, mb.number = d_number;
      mb.pnum = pairs.pnum, mb.uniq = pairs.uniq;
    }
    HpBatch hb;
    memset(&hb, 0, sizeof(hb));
    hb.m = m, hb.leader = d_leader, hb.number = d_number, hb.b_ord = d_bo, hb.b_rep = d_br, hb.key = d_key, hb.is_set = d_set;
    if (key_off) hb.key = nullptr, hb.key_off = d_off, hb.keys = d_keys, hb.uniq = mb.uniq, hb.P = P;
    hb.triple = triple_id ? d_tr : nullptr, hb.deps_in = d_din, hb.dend_in = deps_in_values_end ? d_dend : nullptr;
    hb.target = d_tgt, hb.ok_bits = d_ok, hb.resend_bits = d_resend, hb.nack_bits = d_nack, hb.commit_bits = d_com;
    hb.reply_deps = d_rd, hb.reply_end = d_re, hb.reply_triple = d_rt;
    hb.act = d_act, hb.contrib = d_contrib, hb.nackflag = d_flag, hb.kv = (uint2*)e->kv.p;
    hb.conf = (int32_t*)e->conf.p, hb.tick = (int32_t*)e->tick.p;
    int rc2;
    if ((rc2 = next_run_id(e, &hb.run_id))) return rc2;
    const dim3 gm((m + 255) / 256), gmn((unsigned)(((long long)m * n + 255) / 256)), blk(256);
    hipLaunchKernelGGL(k_hp_validate, gm, blk, 0, e->stream, e->st, hb);
    if (key_off) hipLaunchKernelGGL(k_mk_pairs, gm, blk, 0, e->stream, mb);
    hipLaunchKernelGGL(k_hp_gate, gmn, blk, 0, e->stream, e->st, hb);
    // the conflict scan of what each replica processes, in array order: K5's sort / segments / scan
    EpxBatch sb;
    memset(&sb, 0, sizeof(sb));
    sb.m = P, sb.number = key_off ? mb.pnum : d_number, sb.kv = hb.kv;
    const uint32_t* key_totals = nullptr;
    int key_buckets = 0;
    if (P > 0) {  // (key lists that are all empty: nothing to scan, nothing for the index to learn)
      sb.kv_sorted = sort_by_key(e, P, hb.kv, (uint2*)e->kv2.p, nullptr, &rc2, &key_totals, &key_buckets);
      if (rc2) return rc2;
    }
    sb.tick = (int32_t*)e->tick.p, sb.seg = (int32_t*)e->seg.p, sb.conf = key_off ? d_pconf : (int32_t*)e->conf.p;
    if (P > 0) launch_segments(e, sb, key_totals, key_buckets);
    // the largestBallot every Nack carries: prefix max per replica over the ballots it took in (as for Prepare / Accept)
    ClBatch cb;
    memset(&cb, 0, sizeof(cb));
    cb.m = m, cb.contrib = d_contrib, cb.nackflag = d_flag, cb.tilemax = d_tm, cb.nack_ballot = d_nb;
    hipLaunchKernelGGL(k_cl_tilemax, dim3(tiles, n), blk, 0, e->stream, cb, tiles);
    hipLaunchKernelGGL(k_cl_tilescan, dim3(n), blk, 0, e->stream, e->st, cb, tiles);
    hipLaunchKernelGGL(k_cl_nacks, dim3(tiles, n), blk, 0, e->stream, cb, tiles);
    MkMerge mm;
    memset(&mm, 0, sizeof(mm));
    mm.m = m, mm.off = key_off ? d_off : nullptr, mm.uniq = mb.uniq, mm.pconf = d_pconf, mm.conf = (int32_t*)e->conf.p, mm.act = d_act;
    by_n(n, [&](auto N) { launch_hp<N>(e, sb, hb, key_off ? &mm : nullptr, P > 0); });
    const long long tot = (long long)e->st.num_keys * n * n;
    if (P > 0) hipLaunchKernelGGL(k_hp_commit, dim3((unsigned)((tot + 255) / 256)), blk, 0, e->stream, e->st, hb);
    return FPX_OK;
  };
  // ok, resend, nack and commit start at 0 (one memset), nack_ballot at -1
  return host_call(e, {in(d_leader, leader, m), in(d_number, number, m), in(d_bo, ballot_ordering, m), in(d_br, ballot_replica, m),
                       in(d_key, key, m), in(d_tr, triple_id, m), in(d_dend, deps_in_values_end, m), in(d_din, deps_in, mn),
                       in(d_set, is_set, m), in(d_tgt, target_mask, m), in(d_off, key_off, key_off ? m + 1 : 0),
                       in(d_keys, keys, key_off ? P : 0), out(d_ok, ok_bits, m, 0), out(d_resend, resend_bits, m, 0), out(d_nack, nack_bits, m, 0),
                       out(d_com, commit_bits, m, 0), out(d_nb, nack_ballot, m, 0xFF), out(d_rd, reply_deps, mn * n),
                       out(d_re, reply_values_end, mn), out(d_rt, reply_triple, mn), scratch(d_act, mn), scratch(d_flag, mn),
                       scratch(d_contrib, mn), scratch(d_tm, (size_t)n * tiles)},
                   launch);
}

int32_t fpx_epx_read_cmdlog_deps(fpx_epx* e, int32_t replica, int32_t leader, int32_t number, int32_t* deps,
                                 int32_t* values_end) {
  if (!e || !deps || !values_end || e->st.num_instances <= 0 || replica < 0 || replica >= e->st.n || leader < 0 ||
      leader >= e->st.n || number < 0 || number >= e->st.num_instances)
    return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  const size_t c = ((size_t)replica * e->st.n + leader) * e->st.num_instances + number;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipMemcpy(deps, e->st.cl_deps + c * e->st.n, (size_t)e->st.n * 4, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(values_end, e->st.cl_dend + c, 4, hipMemcpyDeviceToHost));
  return FPX_OK;
}

int32_t fpx_epx_read_cmdlog(fpx_epx* e, int32_t replica, int32_t leader, int32_t number, int32_t out[5]) {
  if (!e || !out || e->st.num_instances <= 0 || replica < 0 || replica >= e->st.n || leader < 0 || leader >= e->st.n ||
      number < 0 || number >= e->st.num_instances)
    return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  const size_t c = ((size_t)replica * e->st.n + leader) * e->st.num_instances + number;
  uint8_t kind = 0;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipMemcpy(&kind, e->st.cl_status + c, 1, hipMemcpyDeviceToHost));
  out[0] = kind;
  HIPCHK(e, hipMemcpy(&out[1], e->st.cl_ballot + c, 4, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(&out[2], e->st.cl_vote + c, 4, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(&out[3], e->st.cl_triple + c, 4, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(&out[4], e->st.largest + replica, 4, hipMemcpyDeviceToHost));
  return FPX_OK;
}

int32_t fpx_epx_info(fpx_epx* e, int32_t* num_replicas, int32_t* num_keys, int32_t* num_instances) {
  if (!e) return FPX_EINVAL;
  if (num_replicas) *num_replicas = e->st.n;
  if (num_keys) *num_keys = e->st.num_keys;
  if (num_instances) *num_instances = e->st.num_instances;
  return FPX_OK;
}

int32_t fpx_epx_limits(fpx_epx* e, int32_t cap, int32_t* out, int32_t* n) {
  if (!e || cap < 0 || (cap > 0 && !out)) return FPX_EINVAL;
  int32_t v[FPX_EPX_LIMIT_WORDS];
  by_n(e->st.n, [&](auto N) {
    v[FPX_EPX_LIMIT_KP_TC] = KpTile<N>::TC, v[FPX_EPX_LIMIT_KEY_TC] = KeyTile<N>::TC, v[FPX_EPX_LIMIT_NBK] = KpTile<N>::NBK;
    v[FPX_EPX_LIMIT_KP_WAVES] = KpTile<N>::W;
    return 0;
  });
  v[FPX_EPX_LIMIT_KP_MAX_OCC] = KP_MAX_OCC, v[FPX_EPX_LIMIT_KP_MAXB] = KP_MAXB;
  for (int j = 0; j < std::min<int>(cap, FPX_EPX_LIMIT_WORDS); ++j) out[j] = v[j];
  if (n) *n = FPX_EPX_LIMIT_WORDS;
  return FPX_OK;
}

int32_t fpx_epx_tick_census(fpx_epx* e, int32_t cap, int64_t* out, int32_t* n) {
  if (!e || cap < 0 || (cap > 0 && !out)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  unsigned long long dev[EPX_CD_WORDS] = {};
  HIPCHK(e, hipMemcpyAsync(dev, e->census_dev, sizeof(dev), hipMemcpyDeviceToHost, e->stream));
  if (e->kp_misc.p)  // the sort routes: counted beside the second form's control words (launch_kp)
    HIPCHK(e, hipMemcpyAsync(dev, (char*)e->kp_misc.p + 256, EPX_CD_SORTS * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  int64_t v[FPX_EPX_CENSUS_WORDS];
  for (int j = 0; j < FPX_EPX_CENSUS_WORDS; ++j) v[j] = e->census[j];
  static_assert(FPX_EPX_CENSUS_WORDS - FPX_EPX_CENSUS_SORT_BUCKET1 == EPX_CD_LONG_WAY + 1, "the device's words, in the header's order");
  for (int j = 0; j <= EPX_CD_LONG_WAY; ++j) v[FPX_EPX_CENSUS_SORT_BUCKET1 + j] = (int64_t)dev[j];
  for (int j = 0; j < std::min<int>(cap, FPX_EPX_CENSUS_WORDS); ++j) out[j] = v[j];
  if (n) *n = FPX_EPX_CENSUS_WORDS;
  return FPX_OK;
}

int32_t fpx_epx_read_index(fpx_epx* e, int32_t replica, int32_t key, int32_t* gets, int32_t* sets) {
  if (!e || replica < 0 || replica >= e->st.n || key < 0 || key >= e->st.num_keys) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  const size_t off = ((size_t)replica * e->st.num_keys + key) * e->st.n;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (gets) HIPCHK(e, hipMemcpy(gets, e->st.gets + off, (size_t)e->st.n * 4, hipMemcpyDeviceToHost));
  if (sets) HIPCHK(e, hipMemcpy(sets, e->st.sets + off, (size_t)e->st.n * 4, hipMemcpyDeviceToHost));
  return FPX_OK;
}

int32_t fpx_epx_accept_mk(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* ballot_ordering,
                          const int32_t* ballot_replica, const int32_t* triple_id, const int32_t* key_offsets, const int32_t* keys,
                          const uint8_t* is_set, const uint8_t* target_mask, uint8_t* ok_bits, uint8_t* nack_bits,
                          uint8_t* commit_bits, int32_t* nack_ballot, uint8_t* committed) {
  if (m > 0 && !key_offsets) return FPX_EINVAL;
  return cl_run(e, 1, m, leader, number, ballot_ordering, ballot_replica, triple_id, nullptr, is_set, target_mask, ok_bits,
                nack_bits, commit_bits, nack_ballot, committed, nullptr, nullptr, nullptr, key_offsets, keys);
}

int32_t fpx_epx_handle_commit(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* triple_id,
                              const int32_t* key, const uint8_t* is_set, const int32_t* deps, const int32_t* deps_values_end,
                              const uint8_t* target_mask) {
  return handle_commit_impl(e, m, leader, number, triple_id, key, nullptr, nullptr, is_set, deps, deps_values_end, target_mask);
}

int32_t fpx_epx_handle_commit_mk(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* triple_id,
                                 const int32_t* key_offsets, const int32_t* keys, const uint8_t* is_set, const int32_t* deps,
                                 const int32_t* deps_values_end, const uint8_t* target_mask) {
  if (m > 0 && !key_offsets) return FPX_EINVAL;
  return handle_commit_impl(e, m, leader, number, triple_id, nullptr, key_offsets, keys, is_set, deps, deps_values_end, target_mask);
}

int32_t fpx_epx_handle_preaccept(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number,
                                 const int32_t* ballot_ordering, const int32_t* ballot_replica, const int32_t* key,
                                 const uint8_t* is_set, const int32_t* triple_id, const int32_t* deps_in,
                                 const int32_t* deps_in_values_end, const uint8_t* target_mask, uint8_t* ok_bits,
                                 uint8_t* resend_bits, uint8_t* nack_bits, uint8_t* commit_bits, int32_t* nack_ballot,
                                 int32_t* reply_deps, int32_t* reply_values_end, int32_t* reply_triple) {
  return handle_preaccept_impl(e, m, leader, number, ballot_ordering, ballot_replica, key, nullptr, nullptr, is_set, triple_id,
                               deps_in, deps_in_values_end, target_mask, ok_bits, resend_bits, nack_bits, commit_bits, nack_ballot,
                               reply_deps, reply_values_end, reply_triple);
}

int32_t fpx_epx_handle_preaccept_mk(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number,
                                    const int32_t* ballot_ordering, const int32_t* ballot_replica, const int32_t* key_offsets,
                                    const int32_t* keys, const uint8_t* is_set, const int32_t* triple_id, const int32_t* deps_in,
                                    const int32_t* deps_in_values_end, const uint8_t* target_mask, uint8_t* ok_bits,
                                    uint8_t* resend_bits, uint8_t* nack_bits, uint8_t* commit_bits, int32_t* nack_ballot,
                                    int32_t* reply_deps, int32_t* reply_values_end, int32_t* reply_triple) {
  if (m > 0 && !key_offsets) return FPX_EINVAL;
  return handle_preaccept_impl(e, m, leader, number, ballot_ordering, ballot_replica, nullptr, key_offsets, keys, is_set, triple_id,
                               deps_in, deps_in_values_end, target_mask, ok_bits, resend_bits, nack_bits, commit_bits, nack_ballot,
                               reply_deps, reply_values_end, reply_triple);
}

// ---- the leader half (FPX_EPX_F_LEADER_STATE): csrc/fpx_epx_leader.hpp ---------------------------------------------------
static bool leader_state_on(const fpx_epx* e) { return e && (e->cfg.flags & FPX_EPX_F_LEADER_STATE) && e->ls.head; }

// key or (key_off, keys): the single-key form or the key lists
static int32_t lead_impl(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* at,
                         const int32_t* ballot_ordering, const int32_t* key, const int32_t* key_off, const int32_t* keys,
                         const uint8_t* is_set, const int32_t* triple_id, const uint8_t* avoid_fast_path, int32_t* deps,
                         int32_t* deps_values_end) {
  if (!e || m < 0 || !leader_state_on(e)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) return FPX_OK;
  if (!leader || !number || !at || !ballot_ordering || !(key || key_off) || !is_set || !triple_id || !avoid_fast_path)
    return FPX_EINVAL;
  const int n = e->st.n;
  const size_t mn = (size_t)m * n;
  // key lists: P pairs in array order instead of m messages in the scan, as fpx_epx_handle_preaccept_mk
  int64_t P64 = 0;
  if (key_off && check_key_lists(m, key_off, keys, e->st.num_keys, &P64)) return FPX_EINVAL;
  const int P = key_off ? (int)P64 : m;
  int rc;
  if ((rc = grow_conflict_scan(e, m, key_off ? P : -1))) return rc;
  MkPairScratch pairs = {nullptr, nullptr};
  if (key_off && (rc = carve(e, &e->mk_pair, &pairs, [&](Carver& c) { return lay_mk_pairs(c, P); }))) return rc;
  LdBatch lb;
  memset(&lb, 0, sizeof(lb));
  lb.m = m, lb.kv = (uint2*)e->kv.p, lb.uniq = pairs.uniq, lb.P = P;
  // K7's "processed" branch at replica at[i] alone, with an empty deps_in: its gate table, its scan, its reply kernel
  HpBatch hb;
  memset(&hb, 0, sizeof(hb));
  hb.m = m, hb.kv = lb.kv;
  auto launch = [&]() -> int {
    int rc2;
    if ((rc2 = next_run_id(e, &lb.run_id))) return rc2;
    if (!key_off) lb.key_off = lb.keys = nullptr;
    else lb.key = nullptr;
    hb.leader = lb.leader, hb.number = lb.number, hb.b_ord = lb.b_ord, hb.b_rep = lb.at, hb.key = lb.key, hb.is_set = lb.is_set;
    hb.key_off = lb.key_off, hb.keys = lb.keys, hb.uniq = lb.uniq, hb.P = P;
    hb.triple = lb.triple, hb.act = lb.act, lb.reply_deps = hb.reply_deps, lb.reply_end = hb.reply_end;
    const dim3 gm((m + 255) / 256), gmn((unsigned)(((long long)m * n + 255) / 256)), blk(256);
    hipLaunchKernelGGL(k_ld_validate, gm, blk, 0, e->stream, e->st, lb);
    if (key_off) {
      MkBatch mb;
      memset(&mb, 0, sizeof(mb));
      mb.m = m, mb.P = P, mb.off = lb.key_off, mb.keys = lb.keys, mb.number = lb.number, mb.pnum = pairs.pnum, mb.uniq = pairs.uniq;
      hipLaunchKernelGGL(k_mk_pairs, gm, blk, 0, e->stream, mb);
    }
    hipLaunchKernelGGL(k_ld_gate, gmn, blk, 0, e->stream, e->st, lb);
    EpxBatch sb;
    memset(&sb, 0, sizeof(sb));
    // (key lists that are all empty: nothing to scan, nothing for the index to learn)
    if (P > 0 && (rc2 = sort_conflict_scan(e, P, key_off ? pairs.pnum : lb.number, &sb))) return rc2;
    if (key_off) sb.conf = (int32_t*)e->mk_pconf.p;
    hb.conf = (int32_t*)e->conf.p, hb.tick = (int32_t*)e->tick.p;
    MkMerge mm;
    memset(&mm, 0, sizeof(mm));
    mm.m = m, mm.off = lb.key_off, mm.uniq = pairs.uniq, mm.pconf = sb.conf, mm.conf = (int32_t*)e->conf.p, mm.act = lb.act;
    by_n(n, [&](auto N) {
      launch_hp<N>(e, sb, hb, key_off ? &mm : nullptr, P > 0);
      hipLaunchKernelGGL((k_ld_install<N>), gm, blk, 0, e->stream, e->st, e->ls, lb);
    });
    const long long tot = (long long)e->st.num_keys * n * n;
    if (P > 0) hipLaunchKernelGGL(k_hp_commit, dim3((unsigned)((tot + 255) / 256)), blk, 0, e->stream, e->st, hb);
    return FPX_OK;
  };
  return host_call(e, {in(lb.leader, leader, m), in(lb.number, number, m), in(lb.at, at, m), in(lb.b_ord, ballot_ordering, m),
                       in(lb.key, key, key ? m : 0), in(lb.triple, triple_id, m), in(lb.is_set, is_set, m),
                       in(lb.avoid, avoid_fast_path, m), in(lb.key_off, key_off, key_off ? m + 1 : 0),
                       in(lb.keys, keys, key_off ? P : 0), scratch(hb.deps_in, mn, 0), scratch(lb.skip, m, 0),
                       held(lb.deps, deps, mn), held(lb.dend, deps_values_end, m), scratch(lb.act, mn),
                       scratch(hb.reply_deps, mn * n), scratch(hb.reply_end, mn)},
                   launch);
}

int32_t fpx_epx_lead(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* at,
                     const int32_t* ballot_ordering, const int32_t* key, const uint8_t* is_set, const int32_t* triple_id,
                     const uint8_t* avoid_fast_path, int32_t* deps, int32_t* deps_values_end) {
  if (m > 0 && !key) return FPX_EINVAL;
  return lead_impl(e, m, leader, number, at, ballot_ordering, key, nullptr, nullptr, is_set, triple_id, avoid_fast_path, deps,
                   deps_values_end);
}

int32_t fpx_epx_lead_mk(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* at,
                        const int32_t* ballot_ordering, const int32_t* key_offsets, const int32_t* keys, const uint8_t* is_set,
                        const int32_t* triple_id, const uint8_t* avoid_fast_path, int32_t* deps, int32_t* deps_values_end) {
  if (m > 0 && !key_offsets) return FPX_EINVAL;
  return lead_impl(e, m, leader, number, at, ballot_ordering, nullptr, key_offsets, keys, is_set, triple_id, avoid_fast_path,
                   deps, deps_values_end);
}

// b: the messages and the outputs (any of which may be null); the scratch fields are filled here
static int32_t leader_replies_launch(fpx_epx* e, LrBatch b) {
  const int m = b.m;
  b.blocks = (m + LR_BLOCK - 1) / LR_BLOCK;
  int rc;
  if ((rc = grow(e, &e->kv, (size_t)m * 8))) return rc;
  if ((rc = grow(e, &e->kv2, (size_t)m * 8))) return rc;
  LrScratch ls;
  if ((rc = carve(e, &e->lr_misc, &ls, [&](Carver& c) { return lay_leader_replies(c, m, b.blocks); }))) return rc;
  b.kv = (uint2*)e->kv.p, b.flag = ls.flag, b.bsum = ls.bsum;
  const dim3 gm((m + 255) / 256), blk(256);
  hipLaunchKernelGGL(k_lr_validate, gm, blk, 0, e->stream, e->st, b);
  b.sorted = sort_by_cell(e, m, b.kv, (uint2*)e->kv2.p, &rc);
  if (rc) return rc;
  by_n(e->st.n, [&](auto N) { hipLaunchKernelGGL((k_lr_walk<N>), gm, blk, 0, e->stream, e->st, e->ls, b); });
  launch_compaction(e, m, ls, b.decided, b.num_decided);
  return FPX_OK;
}

int32_t fpx_epx_leader_replies_dev(fpx_epx* e, int32_t m, const int32_t* d_kind, const int32_t* d_to, const int32_t* d_leader,
                                   const int32_t* d_number, const int32_t* d_ballot_ordering, const int32_t* d_ballot_replica,
                                   const int32_t* d_replica_index, const int32_t* d_sequence_number, const int32_t* d_deps,
                                   const int32_t* d_deps_values_end, int32_t* d_outcome, int32_t* d_out_seq, int32_t* d_out_deps,
                                   int32_t* d_out_values_end, int32_t* d_out_triple, int32_t* d_decided_index,
                                   int32_t* d_num_decided) {
  if (!e || m < 0 || m >= (1 << 30) || !leader_state_on(e)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) {
    if (d_num_decided) HIPCHK(e, hipMemsetAsync(d_num_decided, 0, 4, e->stream));
    return FPX_OK;
  }
  if (!d_kind || !d_to || !d_leader || !d_number || !d_ballot_ordering || !d_ballot_replica || !d_replica_index || !d_deps)
    return FPX_EINVAL;
  LrBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m, b.kind = d_kind, b.to = d_to, b.leader = d_leader, b.number = d_number, b.b_ord = d_ballot_ordering;
  b.b_rep = d_ballot_replica, b.ridx = d_replica_index, b.seq = d_sequence_number, b.deps = d_deps, b.dend = d_deps_values_end;
  b.outcome = d_outcome, b.out_seq = d_out_seq, b.out_deps = d_out_deps, b.out_end = d_out_values_end, b.out_triple = d_out_triple;
  b.decided = d_decided_index, b.num_decided = d_num_decided;
  int rc = leader_replies_launch(e, b);
  return rc ? rc : launch_check(e);
}

int32_t fpx_epx_leader_replies(fpx_epx* e, int32_t m, const int32_t* kind, const int32_t* to, const int32_t* leader,
                               const int32_t* number, const int32_t* ballot_ordering, const int32_t* ballot_replica,
                               const int32_t* replica_index, const int32_t* sequence_number, const int32_t* deps,
                               const int32_t* deps_values_end, int32_t* outcome, int32_t* out_seq, int32_t* out_deps,
                               int32_t* out_values_end, int32_t* out_triple, int32_t* decided_index, int32_t* num_decided) {
  if (!e || m < 0 || m >= (1 << 30) || !leader_state_on(e)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) {
    if (num_decided) *num_decided = 0;
    return FPX_OK;
  }
  if (!kind || !to || !leader || !number || !ballot_ordering || !ballot_replica || !replica_index || !deps) return FPX_EINVAL;
  const size_t mn = (size_t)m * e->st.n;
  LrBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m;
  return host_call(e, {in(b.kind, kind, m), in(b.to, to, m), in(b.leader, leader, m), in(b.number, number, m),
                       in(b.b_ord, ballot_ordering, m), in(b.b_rep, ballot_replica, m), in(b.ridx, replica_index, m),
                       opt_in(b.seq, sequence_number, m), opt_in(b.dend, deps_values_end, m), in(b.deps, deps, mn),
                       held(b.outcome, outcome, m), held(b.out_seq, out_seq, m), held(b.out_end, out_values_end, m),
                       held(b.out_triple, out_triple, m), held_first(b.decided, decided_index, m, b.num_decided),
                       held(b.out_deps, out_deps, mn), held(b.num_decided, num_decided, 1)},
                   [&]() -> int { return leader_replies_launch(e, b); });
}

// ---- a leader's reply burst from wire bytes: csrc/fpx_wire_epx_dev.hpp (include/fpx_wire.h) ---------------------------------
static void launch_wire_decode(fpx_epx* e, const uint8_t* d_buf, int64_t buf_len, const int64_t* d_offsets, int32_t n,
                               const fpxw::EpxFoldOut& o) {
  hipLaunchKernelGGL(k_epx_wire_decode, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->st, d_buf, buf_len, d_offsets, n,
                     e->st.n, o);
}

int32_t fpx_wire_epaxos_decode_replica_inbound_dev(
    fpx_epx* e, const uint8_t* d_buf, int64_t buf_len, const int64_t* d_offsets, int32_t n, int32_t* d_kind,
    int32_t* d_instance_leader, int32_t* d_instance_number, int32_t* d_ballot_ordering, int32_t* d_ballot_replica,
    int32_t* d_replica_index, int32_t* d_sequence_number, int32_t* d_vote_ballot_ordering, int32_t* d_vote_ballot_replica,
    int32_t* d_status, int32_t* d_is_noop, int64_t* d_cmd_off, int32_t* d_cmd_len, int32_t* d_deps_num_replicas,
    int32_t* d_deps_watermark, int32_t* d_deps_values_end, int32_t* d_deps_shape, int32_t* d_bad_index) {
  if (!e || n < 0 || n >= (1 << 30) || buf_len < 0 || !d_bad_index) return FPX_EINVAL;
  if (n > 0 && (!d_buf || !d_offsets || !d_kind)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (n > 0)
    launch_wire_decode(e, d_buf, buf_len, d_offsets, n,
                       fpxw::EpxFoldOut{d_kind, d_instance_leader, d_instance_number, d_ballot_ordering, d_ballot_replica,
                                        d_replica_index, d_sequence_number, d_vote_ballot_ordering, d_vote_ballot_replica,
                                        d_status, d_is_noop, d_cmd_off, d_cmd_len, d_deps_num_replicas, d_deps_watermark,
                                        d_deps_values_end, d_deps_shape});
  hipLaunchKernelGGL(k_epx_wire_tail, dim3(1), dim3(1), 0, e->stream, e->st, d_bad_index);
  return launch_check(e);
}

// the decoded arrays of a tick: device scratch of the call, whichever form it takes
struct WireTick {
  int32_t *kind, *nr, *shape, *lr_kind, *leader, *number, *b_ord, *b_rep, *ridx, *seq, *deps, *dend;
};
static WireTick lay_wire_tick(Carver& c, size_t m, size_t n) {
  WireTick w;
  for (int32_t** a : {&w.kind, &w.nr, &w.shape, &w.lr_kind, &w.leader, &w.number, &w.b_ord, &w.b_rep, &w.ridx, &w.seq, &w.dend})
    *a = c.take<int32_t>(m);
  w.deps = c.take<int32_t>(m * n);
  return w;
}

// decode -> check -> fpx_epx_leader_replies on the decoded arrays; b: `to` and the outputs
static int32_t wire_tick_launch(fpx_epx* e, const uint8_t* d_in, int64_t in_len, const int64_t* d_in_offsets, const WireTick& w,
                                int32_t* d_bad_index, LrBatch b) {
  fpxw::EpxFoldOut o;
  memset(&o, 0, sizeof(o));
  o.kind = w.kind, o.il = w.leader, o.in = w.number, o.bo = w.b_ord, o.br = w.b_rep, o.ri = w.ridx, o.seq = w.seq;
  o.nr = w.nr, o.wm = w.deps, o.dend = w.dend, o.shape = w.shape;
  launch_wire_decode(e, d_in, in_len, d_in_offsets, b.m, o);
  hipLaunchKernelGGL(k_epx_wire_tick_check, dim3((b.m + 255) / 256), dim3(256), 0, e->stream, e->st, b.m, w.kind, w.nr, w.shape,
                     w.lr_kind, w.ridx);
  hipLaunchKernelGGL(k_epx_wire_tail, dim3(1), dim3(1), 0, e->stream, e->st, d_bad_index);
  b.kind = w.lr_kind, b.leader = w.leader, b.number = w.number, b.b_ord = w.b_ord, b.b_rep = w.b_rep, b.ridx = w.ridx;
  b.seq = w.seq, b.deps = w.deps, b.dend = w.dend;
  return leader_replies_launch(e, b);
}

int32_t fpx_wire_epx_leader_tick_dev(fpx_epx* e, const uint8_t* d_in, int64_t in_len, const int64_t* d_in_offsets, int32_t m,
                                     const int32_t* d_to, int32_t* d_outcome, int32_t* d_out_seq, int32_t* d_out_deps,
                                     int32_t* d_out_values_end, int32_t* d_out_triple, int32_t* d_decided_index,
                                     int32_t* d_num_decided, int32_t* d_bad_index) {
  if (!e || m < 0 || m >= (1 << 30) || in_len < 0 || !d_bad_index || !leader_state_on(e)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) {
    if (d_num_decided) HIPCHK(e, hipMemsetAsync(d_num_decided, 0, 4, e->stream));
    HIPCHK(e, hipMemsetAsync(d_bad_index, 0xFF, 4, e->stream));
    return FPX_OK;
  }
  if (!d_in || !d_in_offsets || !d_to) return FPX_EINVAL;
  WireTick w;
  int rc;
  if ((rc = carve(e, &e->wire_misc, &w, [&](Carver& c) { return lay_wire_tick(c, (size_t)m, (size_t)e->st.n); }))) return rc;
  LrBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m, b.to = d_to, b.outcome = d_outcome, b.out_seq = d_out_seq, b.out_deps = d_out_deps, b.out_end = d_out_values_end;
  b.out_triple = d_out_triple, b.decided = d_decided_index, b.num_decided = d_num_decided;
  rc = wire_tick_launch(e, d_in, in_len, d_in_offsets, w, d_bad_index, b);
  return rc ? rc : launch_check(e);
}

int32_t fpx_wire_epx_leader_tick(fpx_epx* e, const uint8_t* in_bytes, int64_t in_len, const int64_t* in_offsets, int32_t m,
                                 const int32_t* to, int32_t* outcome, int32_t* out_seq, int32_t* out_deps,
                                 int32_t* out_values_end, int32_t* out_triple, int32_t* decided_index, int32_t* num_decided,
                                 int32_t* bad_index) {
  if (!e || m < 0 || m >= (1 << 30) || in_len < 0 || !leader_state_on(e)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (bad_index) *bad_index = -1;
  if (m == 0) {
    if (num_decided) *num_decided = 0;
    return FPX_OK;
  }
  if ((in_len > 0 && !in_bytes) || !in_offsets || !to) return FPX_EINVAL;
  const size_t mn = (size_t)m * e->st.n;
  const uint8_t* d_in = nullptr;
  const int64_t* d_off = nullptr;
  int32_t* d_bad = nullptr;
  int32_t bad = -1;
  WireTick w;
  LrBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m;
  const int32_t rc = host_call(
      e, {in(d_in, in_bytes, (size_t)in_len), in(d_off, in_offsets, (size_t)m + 1), in(b.to, to, m), scratch(w.kind, m),
          scratch(w.nr, m), scratch(w.shape, m), scratch(w.lr_kind, m), scratch(w.leader, m), scratch(w.number, m),
          scratch(w.b_ord, m), scratch(w.b_rep, m), scratch(w.ridx, m), scratch(w.seq, m), scratch(w.dend, m),
          scratch(w.deps, mn), held(b.outcome, outcome, m), held(b.out_seq, out_seq, m), held(b.out_end, out_values_end, m),
          held(b.out_triple, out_triple, m), held_first(b.decided, decided_index, m, b.num_decided),
          held(b.out_deps, out_deps, mn), held(b.num_decided, num_decided, 1), out(d_bad, &bad, 1)},
      [&]() -> int { return wire_tick_launch(e, d_in, in_len, d_off, w, d_bad, b); });
  // (the bad index comes down whatever the status; it means something on FPX_EINVAL)
  if (bad_index && rc == FPX_EINVAL) *bad_index = bad;
  return rc;
}

// ---- the replica half, a burst at a time: csrc/fpx_epx_inbox.hpp -------------------------------------------------------------
// b: the messages and the outputs (any of which may be null); the scratch fields are filled here.  MK: b.key_off / b.keys
// / b.P in place of b.key
extern "C++" template <bool MK>
int32_t replica_inbox_launch(fpx_epx* e, RiBatch b) {
  const int m = b.m, n = e->st.n;
  const int P = MK ? b.P : m;  // what one replica's conflict scan runs over
  const int tiles = (m + CL_TILE - 1) / CL_TILE;
  int rc;
  if ((rc = grow_conflict_scan(e, m, MK ? P : -1))) return rc;
  EpxInboxScratch s;
  if constexpr (MK) {
    EpxInboxMkScratch ms;
    if ((rc = carve(e, &e->ri_misc, &ms, [&](Carver& c) { return lay_epx_inbox_mk(c, m, P, n, tiles); }))) return rc;
    s = ms.msg, b.uniq = ms.pair.uniq, b.pnum = ms.pair.pnum;
    b.pconf = (int32_t*)e->mk_pconf.p, b.merged = (int32_t*)e->conf.p;
  } else {
    if ((rc = carve(e, &e->ri_misc, &s, [&](Carver& c) { return lay_epx_inbox(c, m, n, tiles); }))) return rc;
  }
  b.ckv = (uint2*)s.cell[0], b.kv = (uint2*)e->kv.p, b.contrib = s.contrib, b.nackflag = s.nackflag, b.src = s.src, b.last = s.last;
  b.conf = (int32_t*)e->conf.p;
  const dim3 gm((m + 255) / 256), blk(256);
  hipLaunchKernelGGL(k_ri_validate<MK>, gm, blk, 0, e->stream, e->st, b);
  if constexpr (MK) hipLaunchKernelGGL(k_ri_lists, gm, blk, 0, e->stream, e->st, b);
  // both sorts of the call count their digits in e->tmp: it has its final size before the first one is enqueued
  if ((rc = grow(e, &e->tmp, std::max(radix_sort_bytes(1, m, cell_bits(e)), radix_sort_bytes(n, P, key_bits(e)))))) return rc;
  b.sorted = sort_by_cell(e, m, b.ckv, (uint2*)s.cell[1], &rc);
  if (rc) return rc;
  by_n(n, [&](auto N) { hipLaunchKernelGGL((k_ri_walk<N, MK>), gm, blk, 0, e->stream, e->st, b); });
  // the conflict scan of what each replica looks up and puts, in array order: K7's sort / segments / scan
  // (key lists that are all empty: nothing to scan, nothing for the index to learn)
  EpxBatch sb;
  memset(&sb, 0, sizeof(sb));
  if (P > 0 && (rc = sort_conflict_scan(e, P, MK ? b.pnum : b.number, &sb))) return rc;
  if constexpr (MK) sb.conf = (int32_t*)e->mk_pconf.p;
  // the largestBallot every Nack carries: prefix max per replica over the ballots it took in (as for Prepare / Accept)
  ClBatch cb;
  memset(&cb, 0, sizeof(cb));
  cb.m = m, cb.contrib = s.contrib, cb.nackflag = s.nackflag, cb.tilemax = s.tilemax, cb.nack_ballot = b.out_ballot;
  hipLaunchKernelGGL(k_cl_tilemax, dim3(tiles, n), blk, 0, e->stream, cb, tiles);
  hipLaunchKernelGGL(k_cl_tilescan, dim3(n), blk, 0, e->stream, e->st, cb, tiles);
  hipLaunchKernelGGL(k_cl_nacks, dim3(tiles, n), blk, 0, e->stream, cb, tiles);
  HpBatch hb;
  memset(&hb, 0, sizeof(hb));
  hb.tick = sb.tick;
  const long long tot = (long long)e->st.num_keys * n * n;
  by_n(n, [&](auto N) {
    if (P > 0) hipLaunchKernelGGL((k_epx_scan<N>), dim3((N * e->st.num_keys + 3) / 4), blk, 0, e->stream, e->st, sb);
    if constexpr (MK) hipLaunchKernelGGL((k_ri_merge<N>), gm, blk, 0, e->stream, e->st, b);
    // the replies read the dependencies the entries held before the burst; only then are the entries' overwritten
    hipLaunchKernelGGL((k_ri_reply<N, MK>), gm, blk, 0, e->stream, e->st, b);
    hipLaunchKernelGGL((k_ri_store<N, MK>), gm, blk, 0, e->stream, e->st, b);
  });
  if (P > 0) hipLaunchKernelGGL(k_hp_commit, dim3((unsigned)((tot + 255) / 256)), blk, 0, e->stream, e->st, hb);
  return FPX_OK;
}

static int32_t replica_inbox_check(const fpx_epx* e, int32_t m) {
  if (!e || m < 0 || m > FPX_EPX_INBOX_MAX || e->st.num_instances <= 0) return FPX_EINVAL;
  if ((uint64_t)e->st.n * e->st.n * e->st.num_instances >= ((uint64_t)1 << 32)) return FPX_EINVAL;  // a cell is 32 bits of the sort
  return FPX_OK;
}

int32_t fpx_epx_replica_inbox_dev(fpx_epx* e, int32_t m, const int32_t* d_kind, const int32_t* d_to, const int32_t* d_leader,
                                  const int32_t* d_number, const int32_t* d_ballot_ordering, const int32_t* d_ballot_replica,
                                  const int32_t* d_key, const uint8_t* d_is_set, const int32_t* d_triple_id,
                                  const int32_t* d_deps, const int32_t* d_deps_values_end, int32_t* d_outcome,
                                  int32_t* d_out_ballot, int32_t* d_out_status, int32_t* d_out_deps, int32_t* d_out_values_end,
                                  int32_t* d_out_triple) {
  if (replica_inbox_check(e, m)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) return FPX_OK;
  if (!d_kind || !d_to || !d_leader || !d_number || !d_ballot_ordering || !d_ballot_replica || !d_key || !d_is_set || !d_triple_id ||
      !d_deps)
    return FPX_EINVAL;
  RiBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m, b.kind = d_kind, b.to = d_to, b.leader = d_leader, b.number = d_number, b.b_ord = d_ballot_ordering;
  b.b_rep = d_ballot_replica, b.key = d_key, b.is_set = d_is_set, b.triple = d_triple_id, b.deps = d_deps, b.dend = d_deps_values_end;
  b.outcome = d_outcome, b.out_ballot = d_out_ballot, b.out_status = d_out_status, b.out_deps = d_out_deps;
  b.out_end = d_out_values_end, b.out_triple = d_out_triple;
  int rc = replica_inbox_launch<false>(e, b);
  return rc ? rc : launch_check(e);
}

int32_t fpx_epx_replica_inbox(fpx_epx* e, int32_t m, const int32_t* kind, const int32_t* to, const int32_t* leader,
                              const int32_t* number, const int32_t* ballot_ordering, const int32_t* ballot_replica,
                              const int32_t* key, const uint8_t* is_set, const int32_t* triple_id, const int32_t* deps,
                              const int32_t* deps_values_end, int32_t* outcome, int32_t* out_ballot, int32_t* out_status,
                              int32_t* out_deps, int32_t* out_values_end, int32_t* out_triple) {
  if (replica_inbox_check(e, m)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) return FPX_OK;
  if (!kind || !to || !leader || !number || !ballot_ordering || !ballot_replica || !key || !is_set || !triple_id || !deps)
    return FPX_EINVAL;
  const size_t mn = (size_t)m * e->st.n;
  RiBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m;
  // (the held outputs reach the caller on FPX_OK and FPX_EFATAL_PROTOCOL; these kernels raise nothing but FPX_EINVAL, so
  // here that is: on FPX_OK alone)
  return host_call(e, {in(b.kind, kind, m), in(b.to, to, m), in(b.leader, leader, m), in(b.number, number, m),
                       in(b.b_ord, ballot_ordering, m), in(b.b_rep, ballot_replica, m), in(b.key, key, m), in(b.triple, triple_id, m),
                       opt_in(b.dend, deps_values_end, m), in(b.deps, deps, mn), in(b.is_set, is_set, m),
                       held(b.outcome, outcome, m), held(b.out_ballot, out_ballot, m), held(b.out_status, out_status, m),
                       held(b.out_end, out_values_end, m), held(b.out_triple, out_triple, m), held(b.out_deps, out_deps, mn)},
                   [&]() -> int { return replica_inbox_launch<false>(e, b); });
}

int32_t fpx_epx_replica_inbox_mk_dev(fpx_epx* e, int32_t m, const int32_t* d_kind, const int32_t* d_to, const int32_t* d_leader,
                                     const int32_t* d_number, const int32_t* d_ballot_ordering, const int32_t* d_ballot_replica,
                                     const int32_t* d_key_offsets, const int32_t* d_keys, int32_t num_pairs,
                                     const uint8_t* d_is_set, const int32_t* d_triple_id, const int32_t* d_deps,
                                     const int32_t* d_deps_values_end, int32_t* d_outcome, int32_t* d_out_ballot,
                                     int32_t* d_out_status, int32_t* d_out_deps, int32_t* d_out_values_end, int32_t* d_out_triple) {
  if (replica_inbox_check(e, m) || num_pairs < 0 || num_pairs > FPX_EPX_MK_MAX_PAIRS) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) return FPX_OK;
  if (!d_kind || !d_to || !d_leader || !d_number || !d_ballot_ordering || !d_ballot_replica || !d_key_offsets ||
      (num_pairs > 0 && !d_keys) || !d_is_set || !d_triple_id || !d_deps)
    return FPX_EINVAL;
  RiBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m, b.kind = d_kind, b.to = d_to, b.leader = d_leader, b.number = d_number, b.b_ord = d_ballot_ordering;
  b.b_rep = d_ballot_replica, b.key_off = d_key_offsets, b.keys = d_keys, b.P = num_pairs, b.is_set = d_is_set;
  b.triple = d_triple_id, b.deps = d_deps, b.dend = d_deps_values_end;
  b.outcome = d_outcome, b.out_ballot = d_out_ballot, b.out_status = d_out_status, b.out_deps = d_out_deps;
  b.out_end = d_out_values_end, b.out_triple = d_out_triple;
  int rc = replica_inbox_launch<true>(e, b);
  return rc ? rc : launch_check(e);
}

int32_t fpx_epx_replica_inbox_mk(fpx_epx* e, int32_t m, const int32_t* kind, const int32_t* to, const int32_t* leader,
                                 const int32_t* number, const int32_t* ballot_ordering, const int32_t* ballot_replica,
                                 const int32_t* key_offsets, const int32_t* keys, const uint8_t* is_set, const int32_t* triple_id,
                                 const int32_t* deps, const int32_t* deps_values_end, int32_t* outcome, int32_t* out_ballot,
                                 int32_t* out_status, int32_t* out_deps, int32_t* out_values_end, int32_t* out_triple) {
  if (replica_inbox_check(e, m)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) return FPX_OK;
  if (!kind || !to || !leader || !number || !ballot_ordering || !ballot_replica || !key_offsets || !is_set || !triple_id || !deps)
    return FPX_EINVAL;
  int64_t P = 0;  // (the device checks the lists again, as it does for the device form)
  if (check_key_lists(m, key_offsets, keys, e->st.num_keys, &P)) return FPX_EINVAL;
  const size_t mn = (size_t)m * e->st.n;
  RiBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m, b.P = (int)P;
  return host_call(e, {in(b.kind, kind, m), in(b.to, to, m), in(b.leader, leader, m), in(b.number, number, m),
                       in(b.b_ord, ballot_ordering, m), in(b.b_rep, ballot_replica, m), in(b.key_off, key_offsets, (size_t)m + 1),
                       in(b.keys, keys, P), in(b.triple, triple_id, m), opt_in(b.dend, deps_values_end, m), in(b.deps, deps, mn),
                       in(b.is_set, is_set, m), held(b.outcome, outcome, m), held(b.out_ballot, out_ballot, m),
                       held(b.out_status, out_status, m), held(b.out_end, out_values_end, m), held(b.out_triple, out_triple, m),
                       held(b.out_deps, out_deps, mn)},
                   [&]() -> int { return replica_inbox_launch<true>(e, b); });
}

// ---- the key table: csrc/fpx_intern.hpp ----------------------------------------------------------------------------------
static bool keys_on(const fpx_epx* e) { return e && e->keys.slot; }

int32_t fpx_epx_keys_enable(fpx_epx* e, int64_t arena_bytes) {
  if (!e || arena_bytes < 0 || arena_bytes > 0x7fffffff || keys_on(e)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  InternTable t = {};
  t.num_keys = e->st.num_keys, t.slots = fpxi::slots_for(t.num_keys), t.arena_bytes = arena_bytes;
  const size_t slots = (size_t)t.slots;
  hipError_t err = hipMalloc((void**)&t.slot, slots * 8);
  if (err == hipSuccess) err = hipMalloc((void**)&t.first, slots * 4);
  if (err == hipSuccess) err = hipMalloc((void**)&t.key_off, ((size_t)t.num_keys + 1) * 4);
  if (err == hipSuccess) err = hipMalloc((void**)&t.arena, (size_t)std::max<int64_t>(arena_bytes, 1));
  if (err == hipSuccess) err = hipMalloc((void**)&t.meta, 8);
  if (err == hipSuccess) err = hipMemsetAsync(t.slot, 0, slots * 8, e->stream);
  if (err == hipSuccess) err = hipMemsetAsync(t.first, INTERN_IDLE & 0xff, slots * 4, e->stream);
  if (err == hipSuccess) err = hipMemsetAsync(t.key_off, 0, ((size_t)t.num_keys + 1) * 4, e->stream);
  if (err == hipSuccess) err = hipMemsetAsync(t.meta, 0, 8, e->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  if (err != hipSuccess) {
    for (void* p : {(void*)t.slot, (void*)t.first, (void*)t.key_off, (void*)t.arena, (void*)t.meta})
      if (p) (void)hipFree(p);
    e->last_hip = (int)err;
    return err == hipErrorOutOfMemory ? FPX_ENOMEM : FPX_EHIP;
  }
  e->keys = t;
  return FPX_OK;
}

int32_t fpx_epx_keys_count(fpx_epx* e, int32_t* count, int64_t* arena_used) {
  if (!keys_on(e)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  int32_t h[2] = {0, 0};
  HIPCHK(e, hipMemcpyAsync(h, e->keys.meta, sizeof(h), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (count) *count = h[0];
  if (arena_used) *arena_used = h[1];
  return FPX_OK;
}

// an exclusive scan of a[0 .. rows * INTERN_ROW) in two levels of k_lr_bscan: inside every row (a row's sum to tot), then
// over tot (the total to *total).  Element i's scan is a[i] + tot[i / INTERN_ROW]
static void scan_rows_launch(fpx_epx* e, uint32_t* a, size_t rows, int32_t* tot, int32_t* total) {
  hipLaunchKernelGGL(k_lr_bscan, dim3((unsigned)rows), dim3(256), 0, e->stream, e->st, a, (int)INTERN_ROW, (size_t)INTERN_ROW, tot);
  hipLaunchKernelGGL(k_lr_bscan, dim3(1), dim3(256), 0, e->stream, e->st, (uint32_t*)tot, (int)rows, (size_t)0, total);
}

// one batch: b's strings, count and ids; the scratch fields are filled here
static int32_t intern_launch(fpx_epx* e, InternBatch b, const InternScratch& s) {
  b.slot_of = s.slot_of, b.rank = s.rank, b.gt = s.gt, b.ctl = s.ctl;
  for (int j = 0; j < 3; ++j) b.sc[j] = s.sc[j], b.tot[j] = s.tot[j];
  static_assert(IC_WORDS == INTERN_CTL_WORDS && INTERN_ROW == INTERN_SCAN_ROW, "a batch's scratch as lay_intern sizes it");
  HIPCHK(e, hipMemsetAsync(b.ctl, 0, IC_WORDS * 8, e->stream));
  const size_t rows = scan_rows((size_t)b.P);
  const dim3 gp((b.P + 255) / 256), blk(256);
  if (b.P > 0) {
    hipLaunchKernelGGL(k_int_probe, gp, blk, 0, e->stream, e->keys, b);
    hipLaunchKernelGGL(k_int_flags, dim3((unsigned)(rows * INTERN_ROW / 256)), blk, 0, e->stream, e->keys, b);
    for (int j = 0; j < 3; ++j) scan_rows_launch(e, b.sc[j], rows, b.tot[j], b.gt + j);
  }
  hipLaunchKernelGGL(k_int_decide, dim3(1), dim3(1), 0, e->stream, e->keys, b, e->st.status);
  if (b.P > 0) {
    hipLaunchKernelGGL(k_int_rollback, gp, blk, 0, e->stream, e->keys, b);
    hipLaunchKernelGGL(k_int_commit, gp, blk, 0, e->stream, e->keys, b);
    hipLaunchKernelGGL(k_int_ids, gp, blk, 0, e->stream, e->keys, b);
  }
  return FPX_OK;
}

static int32_t keys_intern_check(const fpx_epx* e, int64_t bytes_len, int32_t P) {
  return !keys_on(e) || bytes_len < 0 || P < 0 || P > FPX_EPX_MK_MAX_PAIRS ? FPX_EINVAL : FPX_OK;
}

static int32_t keys_intern_impl(fpx_epx* e, const uint8_t* d_bytes, int64_t bytes_len, const int64_t* d_off, const int32_t* d_len,
                                int32_t P, int32_t* d_ids) {
  InternScratch s;
  int rc;
  if ((rc = carve(e, &e->keys_misc, &s, [&](Carver& c) { return lay_intern(c, (size_t)P); }))) return rc;
  InternBatch b;
  memset(&b, 0, sizeof(b));
  b.bytes = d_bytes, b.bytes_len = bytes_len, b.off = d_off, b.len = d_len, b.P = P, b.ids = d_ids;
  return intern_launch(e, b, s);
}

int32_t fpx_epx_keys_intern_dev(fpx_epx* e, const uint8_t* d_bytes, int64_t bytes_len, const int64_t* d_off, const int32_t* d_len,
                                int32_t P, int32_t* d_ids) {
  if (keys_intern_check(e, bytes_len, P)) return FPX_EINVAL;
  if (P == 0) return FPX_OK;
  if ((bytes_len > 0 && !d_bytes) || !d_off || !d_len || !d_ids) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  const int rc = keys_intern_impl(e, d_bytes, bytes_len, d_off, d_len, P, d_ids);
  return rc ? rc : launch_check(e);
}

int32_t fpx_epx_keys_intern(fpx_epx* e, const uint8_t* bytes, int64_t bytes_len, const int64_t* off, const int32_t* len, int32_t P,
                            int32_t* ids) {
  if (keys_intern_check(e, bytes_len, P)) return FPX_EINVAL;
  if (P == 0) return FPX_OK;
  if ((bytes_len > 0 && !bytes) || !off || !len || !ids) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  const uint8_t* d_bytes = nullptr;
  const int64_t* d_off = nullptr;
  const int32_t* d_len = nullptr;
  int32_t* d_ids = nullptr;
  return host_call(e, {in(d_bytes, bytes, (size_t)bytes_len), in(d_off, off, P), in(d_len, len, P), held(d_ids, ids, P)},
                   [&]() -> int { return keys_intern_impl(e, d_bytes, bytes_len, d_off, d_len, P, d_ids); });
}

int32_t fpx_epx_keys_read(fpx_epx* e, int32_t first_id, int32_t n, int32_t* key_off_out, uint8_t* bytes_out, int64_t cap) {
  if (!keys_on(e) || first_id < 0 || n < 0 || cap < 0 || !key_off_out) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  int32_t count = 0;
  HIPCHK(e, hipMemcpyAsync(&count, e->keys.meta, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if ((int64_t)first_id + n > count) return FPX_EINVAL;
  HIPCHK(e, hipMemcpy(key_off_out, e->keys.key_off + first_id, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost));
  const int32_t base = key_off_out[0];
  for (int32_t j = 0; j <= n; ++j) key_off_out[j] -= base;
  if (key_off_out[n] > cap) return FPX_ECAPACITY;
  if (key_off_out[n] > 0) {
    if (!bytes_out) return FPX_EINVAL;
    HIPCHK(e, hipMemcpy(bytes_out, e->keys.arena + base, (size_t)key_off_out[n], hipMemcpyDeviceToHost));
  }
  return FPX_OK;
}

// ---- the command store: csrc/fpx_epx_cmds.hpp ---------------------------------------------------------------------------
static bool cmds_on(const fpx_epx* e) { return e && e->cmds.off; }

int32_t fpx_epx_cmds_enable(fpx_epx* e, int32_t max_triples, int64_t arena_bytes) {
  if (!e || max_triples < 1 || arena_bytes < 0 || cmds_on(e)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  CmdStore t = {};
  t.max_triples = max_triples, t.arena_bytes = arena_bytes;
  const size_t ids = (size_t)max_triples;
  hipError_t err = hipMalloc((void**)&t.off, ids * 8);
  if (err == hipSuccess) err = hipMalloc((void**)&t.len, ids * 4);
  if (err == hipSuccess) err = hipMalloc((void**)&t.claim, ids * 4);
  if (err == hipSuccess) err = hipMalloc((void**)&t.arena, (size_t)std::max<int64_t>(arena_bytes, 1));
  if (err == hipSuccess) err = hipMalloc((void**)&t.meta, 32);
  if (err == hipSuccess) err = hipMemsetAsync(t.off, 0xFF, ids * 8, e->stream);
  if (err == hipSuccess) err = hipMemsetAsync(t.len, 0, ids * 4, e->stream);
  if (err == hipSuccess) err = hipMemsetAsync(t.claim, CMDS_IDLE & 0xff, ids * 4, e->stream);
  if (err == hipSuccess) err = hipMemsetAsync(t.meta, 0, 32, e->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  if (err != hipSuccess) {
    for (void* p : {(void*)t.off, (void*)t.len, (void*)t.claim, (void*)t.arena, (void*)t.meta})
      if (p) (void)hipFree(p);
    e->last_hip = (int)err;
    return err == hipErrorOutOfMemory ? FPX_ENOMEM : FPX_EHIP;
  }
  e->cmds = t;
  return FPX_OK;
}

// one burst; d_result may be null (the ticks': the store's counts say what a put did)
static int32_t cmds_put_launch(fpx_epx* e, const uint8_t* d_buf, int64_t buf_len, const int64_t* d_cmd_off, const int32_t* d_cmd_len,
                               const int32_t* d_triple, int32_t m, bool check_spans, long long* d_result) {
  static_assert(CMC_WORDS == EPX_CMDS_CTL_WORDS && CMD_MAX_LEN == FPX_EPX_CMD_MAX_LEN, "a put's scratch as lay_epx_cmds_put sizes it");
  EpxCmdsPutScratch s;
  int rc;
  if ((rc = carve(e, &e->cmds_misc, &s, [&](Carver& c) { return lay_epx_cmds_put(c, (size_t)m); }))) return rc;
  const size_t rows = scan_rows((size_t)m);
  CmdPut b;
  memset(&b, 0, sizeof(b));
  b.buf = d_buf, b.buf_len = buf_len, b.cmd_off = d_cmd_off, b.cmd_len = d_cmd_len, b.triple = d_triple, b.m = m;
  b.rows = (int32_t)rows, b.check_spans = check_spans ? 1 : 0, b.bytewise = e->cmds_bytewise ? 1 : 0;
  b.result = d_result ? d_result : s.result;
  b.lscan = s.lscan, b.ltot = s.ltot, b.lgt = s.lgt, b.ctl = s.ctl;
  HIPCHK(e, hipMemsetAsync(b.ctl, 0, CMC_WORDS * 4, e->stream));
  HIPCHK(e, hipMemsetAsync(b.ctl + CMC_BAD, CMDS_IDLE & 0xff, 4, e->stream));
  const dim3 gm((unsigned)((m + CMD_BLOCK - 1) / CMD_BLOCK)), blk(CMD_BLOCK);
  hipLaunchKernelGGL(k_cmd_claim, gm, blk, 0, e->stream, e->st, e->cmds, b);
  hipLaunchKernelGGL(k_cmd_len, dim3((unsigned)(rows * INTERN_ROW / CMD_BLOCK)), blk, 0, e->stream, e->st, e->cmds, b);
  scan_rows_launch(e, b.lscan, rows, b.ltot, b.lgt);
  hipLaunchKernelGGL(k_cmd_decide, dim3(1), dim3(256), 0, e->stream, e->st, e->cmds, b);
  hipLaunchKernelGGL(k_cmd_copy, gm, blk, 0, e->stream, e->cmds, b);
  hipLaunchKernelGGL(k_cmd_release, gm, blk, 0, e->stream, e->cmds, b);
  return FPX_OK;
}

static int32_t cmds_put_check(const fpx_epx* e, int64_t buf_len, int32_t m) {
  return !cmds_on(e) || buf_len < 0 || m < 0 || m > FPX_EPX_INBOX_MAX ? FPX_EINVAL : FPX_OK;
}

int32_t fpx_epx_cmds_put_dev(fpx_epx* e, const uint8_t* d_buf, int64_t buf_len, const int64_t* d_cmd_off, const int32_t* d_cmd_len,
                             const int32_t* d_triple_id, int32_t m, int64_t* d_result) {
  if (cmds_put_check(e, buf_len, m) || !d_result) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) {
    HIPCHK(e, hipMemsetAsync(d_result, 0, 32, e->stream));
    return FPX_OK;
  }
  if ((buf_len > 0 && !d_buf) || !d_cmd_off || !d_cmd_len || !d_triple_id) return FPX_EINVAL;
  const int rc = cmds_put_launch(e, d_buf, buf_len, d_cmd_off, d_cmd_len, d_triple_id, m, true, (long long*)d_result);
  return rc ? rc : launch_check(e);
}

int32_t fpx_epx_cmds_put(fpx_epx* e, const uint8_t* buf, int64_t buf_len, const int64_t* cmd_off, const int32_t* cmd_len,
                         const int32_t* triple_id, int32_t m, int64_t* result) {
  if (cmds_put_check(e, buf_len, m) || !result) return FPX_EINVAL;
  result[0] = result[1] = result[2] = result[3] = 0;
  if (m == 0) return FPX_OK;
  if ((buf_len > 0 && !buf) || !cmd_off || !cmd_len || !triple_id) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  const uint8_t* d_buf = nullptr;
  const int64_t* d_off = nullptr;
  const int32_t *d_len = nullptr, *d_triple = nullptr;
  long long* d_res = nullptr;
  return host_call(e, {in(d_buf, buf, (size_t)buf_len), in(d_off, cmd_off, m), in(d_len, cmd_len, m), in(d_triple, triple_id, m),
                       out(d_res, result, 4)},
                   [&]() -> int { return cmds_put_launch(e, d_buf, buf_len, d_off, d_len, d_triple, m, true, d_res); });
}

int32_t fpx_epx_cmds_read(fpx_epx* e, int32_t triple_id, uint8_t* out, int64_t cap, int32_t* len) {
  if (!cmds_on(e) || triple_id < 0 || triple_id >= e->cmds.max_triples || cap < 0 || !len) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  long long off = -1;
  int32_t n = 0;
  HIPCHK(e, hipMemcpyAsync(&off, e->cmds.off + triple_id, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(&n, e->cmds.len + triple_id, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  *len = off < 0 ? -1 : n;
  if (off < 0 || n == 0) return FPX_OK;
  if (n > cap) return FPX_ECAPACITY;
  if (!out) return FPX_EINVAL;
  HIPCHK(e, hipMemcpy(out, e->cmds.arena + off, (size_t)n, hipMemcpyDeviceToHost));
  return FPX_OK;
}

int32_t fpx_epx_cmds_stats(fpx_epx* e, int64_t* out) {
  if (!cmds_on(e) || !out) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  HIPCHK(e, hipMemcpyAsync(out, e->cmds.meta, 32, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return FPX_OK;
}

// ---- a replica's inbox from wire bytes: csrc/fpx_wire_epx_dev.hpp (include/fpx_wire.h) ---------------------------------------
// the tick's check between the count and the scan (a classify on its own has none)
struct ClsTick {
  const int32_t *kind, *nr, *shape;
  int32_t triple_base;
  const int32_t* triple_in;
  int32_t *ri_kind, *triple;
};

// b: the commands and the outputs; the scratch fields are filled here.  d_keys: the ids of the pairs
static int32_t classify_launch(fpx_epx* e, ClsBatch b, const EpxClassifyScratch& s, int32_t* d_keys, const ClsTick* tk) {
  b.cnt = s.cnt, b.cscan = s.cscan, b.ctot = s.ctot, b.cgt = s.cgt, b.np = s.np, b.pair_off = s.pair_off, b.pair_len = s.pair_len;
  const size_t rows = scan_rows((size_t)b.m);
  const dim3 gm((b.m + 255) / 256), blk(256);
  hipLaunchKernelGGL(k_cls_count, dim3((unsigned)(rows * INTERN_ROW / 256)), blk, 0, e->stream, e->st, b);
  if (tk)
    hipLaunchKernelGGL(k_epx_wire_replica_check, gm, blk, 0, e->stream, e->st, b.m, tk->kind, tk->nr, tk->shape, b.shape,
                       tk->triple_base, tk->triple_in, tk->ri_kind, tk->triple);
  // (the tail first: a bad tick is FPX_EINVAL by the time the scans look at the status)
  hipLaunchKernelGGL(k_epx_wire_tail, dim3(1), dim3(1), 0, e->stream, e->st, b.result);
  scan_rows_launch(e, b.cscan, rows, b.ctot, b.cgt);
  hipLaunchKernelGGL(k_cls_decide, dim3(1), dim3(1), 0, e->stream, e->st, b);
  hipLaunchKernelGGL(k_cls_emit, gm, blk, 0, e->stream, b);
  InternBatch ib;
  memset(&ib, 0, sizeof(ib));
  ib.bytes = b.buf, ib.bytes_len = b.buf_len, ib.off = s.pair_off, ib.len = s.pair_len, ib.P = b.max_pairs, ib.count = s.np;
  ib.ids = d_keys;
  const int rc = intern_launch(e, ib, s.in);
  if (rc) return rc;
  hipLaunchKernelGGL(k_cls_result, dim3(1), dim3(1), 0, e->stream, b, (const long long*)s.in.ctl);
  return FPX_OK;
}

static int32_t classify_check(const fpx_epx* e, int64_t buf_len, int32_t m, int32_t max_pairs) {
  return !keys_on(e) || buf_len < 0 || buf_len > 0x7fffffff || m < 0 || m > FPX_EPX_INBOX_MAX || max_pairs < 0 ||
                 max_pairs > FPX_EPX_MK_MAX_PAIRS
             ? FPX_EINVAL
             : FPX_OK;
}

int32_t fpx_wire_epx_classify_dev(fpx_epx* e, const uint8_t* d_buf, int64_t buf_len, const int64_t* d_cmd_off,
                                  const int32_t* d_cmd_len, int32_t m, int32_t max_pairs, int32_t* d_key_offsets, int32_t* d_keys,
                                  uint8_t* d_is_set, int32_t* d_is_noop, int32_t* d_cmd_shape, int32_t* d_result) {
  if (classify_check(e, buf_len, m, max_pairs) || !d_result) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) {
    HIPCHK(e, hipMemsetAsync(d_result, 0, 16, e->stream));
    HIPCHK(e, hipMemsetAsync(d_result, 0xFF, 4, e->stream));
    if (d_key_offsets) HIPCHK(e, hipMemsetAsync(d_key_offsets, 0, 4, e->stream));
    return FPX_OK;
  }
  if ((buf_len > 0 && !d_buf) || !d_cmd_off || !d_cmd_len || !d_key_offsets || (max_pairs > 0 && !d_keys) || !d_is_set ||
      !d_is_noop || !d_cmd_shape)
    return FPX_EINVAL;
  EpxClassifyScratch s;
  int rc;
  if ((rc = carve(e, &e->rt_misc, &s, [&](Carver& c) { return lay_epx_classify(c, (size_t)m, (size_t)max_pairs); }))) return rc;
  ClsBatch b;
  memset(&b, 0, sizeof(b));
  b.buf = d_buf, b.buf_len = buf_len, b.cmd_off = d_cmd_off, b.cmd_len = d_cmd_len, b.m = m, b.max_pairs = max_pairs;
  b.key_offsets = d_key_offsets, b.is_set = d_is_set, b.is_noop = d_is_noop, b.shape = d_cmd_shape, b.result = d_result;
  rc = classify_launch(e, b, s, d_keys, nullptr);
  return rc ? rc : launch_check(e);
}

// stage 1 (decode, check, classify, intern), ONE host wait for the pair count and the status, stage 2
// (fpx_epx_replica_inbox_mk_dev's launches on the decoded arrays); o: `to` and the outputs
static int32_t replica_tick_impl(fpx_epx* e, const uint8_t* d_in, int64_t in_len, const int64_t* d_in_offsets, int32_t triple_base,
                                 const int32_t* d_triple_id, int32_t max_pairs, RiBatch o, int32_t* d_bad_index,
                                 int32_t* d_num_pairs, EpxReplicaTickScratch* decoded = nullptr, bool* stage2 = nullptr) {
  // (the bytes tick: *decoded = the tick's decoded arrays, *stage2 = whether stage 1 let the burst through)
  const int32_t m = o.m;
  EpxReplicaTickScratch w;
  int rc;
  if (stage2) *stage2 = false;
  if ((rc = carve(e, &e->rt_misc, &w,
                  [&](Carver& c) { return lay_epx_replica_tick(c, (size_t)m, (size_t)e->st.n, (size_t)max_pairs); })))
    return rc;
  fpxw::EpxFoldOut fo;
  memset(&fo, 0, sizeof(fo));
  fo.kind = w.kind, fo.il = w.leader, fo.in = w.number, fo.bo = w.b_ord, fo.br = w.b_rep, fo.cmd_off = w.cmd_off;
  fo.cmd_len = w.cmd_len, fo.nr = w.nr, fo.wm = w.deps, fo.dend = w.dend, fo.shape = w.shape;
  launch_wire_decode(e, d_in, in_len, d_in_offsets, m, fo);
  ClsBatch b;
  memset(&b, 0, sizeof(b));
  b.buf = d_in, b.buf_len = in_len, b.cmd_off = w.cmd_off, b.cmd_len = w.cmd_len, b.m = m, b.max_pairs = max_pairs;
  b.key_offsets = w.key_offsets, b.is_set = w.is_set, b.is_noop = w.is_noop, b.shape = w.cmd_shape, b.result = w.result;
  const ClsTick tk{w.kind, w.nr, w.shape, triple_base, d_triple_id, w.ri_kind, w.triple};
  if ((rc = classify_launch(e, b, w.cls, w.keys, &tk))) return rc;
  if (d_bad_index) HIPCHK(e, hipMemcpyAsync(d_bad_index, w.result, 4, hipMemcpyDeviceToDevice, e->stream));
  if (d_num_pairs) HIPCHK(e, hipMemcpyAsync(d_num_pairs, w.result + 1, 4, hipMemcpyDeviceToDevice, e->stream));
  int32_t h[6] = {0, 0, 0, 0, 0, 0};
  HIPCHK(e, hipMemcpyAsync(h, w.result, 16, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(h + 4, e->st.status, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (h[4] != 0) return FPX_OK;  // refused: the status stays on the context for fpx_epx_sync
  if (h[1] < 0 || h[1] > max_pairs) return FPX_EHIP;
  if (decoded) *decoded = w;
  if (stage2) *stage2 = true;
  o.kind = w.ri_kind, o.leader = w.leader, o.number = w.number, o.b_ord = w.b_ord, o.b_rep = w.b_rep;
  o.key_off = w.key_offsets, o.keys = w.keys, o.P = h[1], o.is_set = w.is_set, o.triple = w.triple, o.deps = w.deps, o.dend = w.dend;
  if ((rc = replica_inbox_launch<true>(e, o))) return rc;
  // the burst's commands into the store, behind stage 2 and standing back behind its status: the spans are the decoder's
  return cmds_on(e) ? cmds_put_launch(e, d_in, in_len, w.cmd_off, w.cmd_len, w.triple, m, false, nullptr) : FPX_OK;
}

static int32_t replica_tick_check(const fpx_epx* e, int64_t in_len, int32_t m, int32_t max_pairs) {
  return replica_inbox_check(e, m) || classify_check(e, in_len, m, max_pairs) ? FPX_EINVAL : FPX_OK;
}

int32_t fpx_wire_epx_replica_tick_dev(fpx_epx* e, const uint8_t* d_in, int64_t in_len, const int64_t* d_in_offsets, int32_t m,
                                      const int32_t* d_to, int32_t triple_base, const int32_t* d_triple_id, int32_t max_pairs,
                                      int32_t* d_outcome, int32_t* d_out_ballot, int32_t* d_out_status, int32_t* d_out_deps,
                                      int32_t* d_out_values_end, int32_t* d_out_triple, int32_t* d_bad_index,
                                      int32_t* d_num_pairs) {
  if (replica_tick_check(e, in_len, m, max_pairs) || !d_bad_index) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) {
    HIPCHK(e, hipMemsetAsync(d_bad_index, 0xFF, 4, e->stream));
    if (d_num_pairs) HIPCHK(e, hipMemsetAsync(d_num_pairs, 0, 4, e->stream));
    return FPX_OK;
  }
  if ((in_len > 0 && !d_in) || !d_in_offsets || !d_to) return FPX_EINVAL;
  RiBatch o;
  memset(&o, 0, sizeof(o));
  o.m = m, o.to = d_to, o.outcome = d_outcome, o.out_ballot = d_out_ballot, o.out_status = d_out_status, o.out_deps = d_out_deps;
  o.out_end = d_out_values_end, o.out_triple = d_out_triple;
  const int rc = replica_tick_impl(e, d_in, in_len, d_in_offsets, triple_base, d_triple_id, max_pairs, o, d_bad_index, d_num_pairs);
  return rc ? rc : launch_check(e);
}

int32_t fpx_wire_epx_replica_tick(fpx_epx* e, const uint8_t* in_bytes, int64_t in_len, const int64_t* in_offsets, int32_t m,
                                  const int32_t* to, int32_t triple_base, const int32_t* triple_id, int32_t max_pairs,
                                  int32_t* outcome, int32_t* out_ballot, int32_t* out_status, int32_t* out_deps,
                                  int32_t* out_values_end, int32_t* out_triple, int32_t* bad_index, int32_t* num_pairs) {
  if (replica_tick_check(e, in_len, m, max_pairs)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (bad_index) *bad_index = -1;
  if (num_pairs) *num_pairs = 0;
  if (m == 0) return FPX_OK;
  if ((in_len > 0 && !in_bytes) || !in_offsets || !to) return FPX_EINVAL;
  const size_t mn = (size_t)m * e->st.n;
  const uint8_t* d_in = nullptr;
  const int64_t* d_off = nullptr;
  const int32_t* d_triple = nullptr;
  int32_t *d_bad = nullptr, *d_np = nullptr;
  int32_t res[2] = {-1, 0};
  RiBatch o;
  memset(&o, 0, sizeof(o));
  o.m = m;
  const int32_t rc = host_call(
      e, {in(d_in, in_bytes, (size_t)in_len), in(d_off, in_offsets, (size_t)m + 1), in(o.to, to, m), opt_in(d_triple, triple_id, m),
          held(o.outcome, outcome, m), held(o.out_ballot, out_ballot, m), held(o.out_status, out_status, m),
          held(o.out_end, out_values_end, m), held(o.out_triple, out_triple, m), held(o.out_deps, out_deps, mn),
          out(d_bad, &res[0], 1), out(d_np, &res[1], 1)},
      [&]() -> int { return replica_tick_impl(e, d_in, in_len, d_off, triple_base, d_triple, max_pairs, o, d_bad, d_np); });
  // (the two words come down whatever the status; the bad index means something on FPX_EINVAL)
  if (bad_index && rc == FPX_EINVAL) *bad_index = res[0];
  if (num_pairs) *num_pairs = res[1];
  return rc;
}

// ---- the replies of a replica tick as wire bytes: csrc/fpx_wire_epx_enc_dev.hpp (include/fpx_wire.h) ---------------------------
// a: the records and the outputs; the scratch fields are filled here
static int32_t reply_encode_launch(fpx_epx* e, EreArgs a, const EpxReplyEncScratch& s) {
  static_assert(ERE_C_WORDS == EPX_REPLY_ENC_CTL_WORDS, "a call's control words as lay_epx_reply_enc sizes them");
  const size_t rows = scan_rows((size_t)a.m);
  a.in.n = e->st.n, a.rows = (int32_t)rows, a.direct = e->enc_direct ? 1 : 0, a.bytewise = e->cmds_bytewise ? 1 : 0;
  a.lscan = s.lscan, a.ltot = s.ltot, a.lgt = s.lgt, a.ctl = s.ctl;
  HIPCHK(e, hipMemsetAsync(a.ctl, 0, ERE_C_WORDS * 4, e->stream));
  HIPCHK(e, hipMemsetAsync(a.ctl + ERE_C_BAD, ERE_NO_BAD & 0xff, 4, e->stream));
  const dim3 blk(ERE_BLOCK);
  if (rows) {
    hipLaunchKernelGGL(k_ere_len, dim3((unsigned)(rows * INTERN_ROW / ERE_BLOCK)), blk, 0, e->stream, a);
    scan_rows_launch(e, a.lscan, rows, a.ltot, a.lgt);
  }
  hipLaunchKernelGGL(k_ere_decide, dim3(1), dim3(256), 0, e->stream, e->st, a);
  if (rows) hipLaunchKernelGGL(k_ere_emit, dim3((unsigned)((a.m + ERE_BLOCK - 1) / ERE_BLOCK)), blk, 0, e->stream, a);
  return FPX_OK;
}

static int32_t reply_encode_check(const fpx_epx* e, int32_t m, const uint8_t* d_out, int64_t cap, const int64_t* d_out_offsets,
                                  const uint8_t* d_reply_kind, const int64_t* d_totals) {
  return !e || m < 0 || m > FPX_EPX_INBOX_MAX || cap < 0 || (cap > 0 && !d_out) || !d_out_offsets || !d_totals ||
                 (m > 0 && !d_reply_kind)
             ? FPX_EINVAL
             : FPX_OK;
}

// the context's command store as the encoder's source (none when the store is not enabled)
static fpxw::EpxCmdSource cmds_source(const fpx_epx* e) {
  fpxw::EpxCmdSource c;
  if (cmds_on(e)) c.off = (const int64_t*)e->cmds.off, c.len = e->cmds.len, c.arena = e->cmds.arena, c.max_triples = e->cmds.max_triples;
  return c;
}

// d_out_triple null: the encoder without a command source
static int32_t reply_encode_dev(fpx_epx* e, int32_t m, const int32_t* d_to, const int32_t* d_leader, const int32_t* d_number,
                                const int32_t* d_ballot_ordering, const int32_t* d_ballot_replica, const int32_t* d_outcome,
                                const int32_t* d_out_ballot, const int32_t* d_out_status, const int32_t* d_out_deps,
                                const int32_t* d_out_values_end, const int32_t* d_out_triple, uint8_t* d_out, int64_t cap,
                                int64_t* d_out_offsets, uint8_t* d_reply_kind, int64_t* d_totals) {
  if (reply_encode_check(e, m, d_out, cap, d_out_offsets, d_reply_kind, d_totals)) return FPX_EINVAL;
  if (m > 0 && (!d_to || !d_leader || !d_number || !d_ballot_ordering || !d_ballot_replica || !d_outcome || !d_out_ballot ||
                !d_out_status || !d_out_deps || !d_out_values_end))
    return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  EpxReplyEncScratch s;
  EreArgs a;
  memset(&a, 0, sizeof(a));
  a.m = m;
  int rc;
  if ((rc = carve(e, &e->enc_misc, &s, [&](Carver& c) { return lay_epx_reply_enc(c, (size_t)m); })))
    return rc;
  a.in = fpxw::EpxReplyIn{e->st.n,   d_to,         d_leader,     d_number,   d_ballot_ordering, d_ballot_replica,
                          d_outcome, d_out_ballot, d_out_status, d_out_deps, d_out_values_end};
  if (d_out_triple) a.in.out_triple = d_out_triple, a.in.cmds = cmds_source(e);
  a.out = d_out, a.cap = cap, a.out_offsets = d_out_offsets, a.reply_kind = d_reply_kind, a.totals = d_totals;
  rc = reply_encode_launch(e, a, s);
  return rc ? rc : launch_check(e);
}

int32_t fpx_wire_epx_encode_replica_replies_dev(fpx_epx* e, int32_t m, const int32_t* d_to, const int32_t* d_leader,
                                                const int32_t* d_number, const int32_t* d_ballot_ordering,
                                                const int32_t* d_ballot_replica, const int32_t* d_outcome,
                                                const int32_t* d_out_ballot, const int32_t* d_out_status,
                                                const int32_t* d_out_deps, const int32_t* d_out_values_end, uint8_t* d_out,
                                                int64_t cap, int64_t* d_out_offsets, uint8_t* d_reply_kind, int64_t* d_totals) {
  return reply_encode_dev(e, m, d_to, d_leader, d_number, d_ballot_ordering, d_ballot_replica, d_outcome, d_out_ballot,
                          d_out_status, d_out_deps, d_out_values_end, nullptr, d_out, cap, d_out_offsets, d_reply_kind, d_totals);
}

int32_t fpx_wire_epx_encode_replica_replies_cmds_dev(fpx_epx* e, int32_t m, const int32_t* d_to, const int32_t* d_leader,
                                                     const int32_t* d_number, const int32_t* d_ballot_ordering,
                                                     const int32_t* d_ballot_replica, const int32_t* d_outcome,
                                                     const int32_t* d_out_ballot, const int32_t* d_out_status,
                                                     const int32_t* d_out_deps, const int32_t* d_out_values_end,
                                                     const int32_t* d_out_triple, uint8_t* d_out, int64_t cap,
                                                     int64_t* d_out_offsets, uint8_t* d_reply_kind, int64_t* d_totals) {
  if (m > 0 && !d_out_triple) return FPX_EINVAL;
  return reply_encode_dev(e, m, d_to, d_leader, d_number, d_ballot_ordering, d_ballot_replica, d_outcome, d_out_ballot,
                          d_out_status, d_out_deps, d_out_values_end, d_out_triple, d_out, cap, d_out_offsets, d_reply_kind,
                          d_totals);
}

// replica_tick_impl, then the encoder on the decoded arrays the tick holds in scratch and on the inbox outputs -- the
// caller's where it asks for them, the tick's own otherwise.  o: `to` and the optional outputs; a: the encoder's outputs
static int32_t replica_tick_bytes_impl(fpx_epx* e, const uint8_t* d_in, int64_t in_len, const int64_t* d_in_offsets,
                                       int32_t triple_base, const int32_t* d_triple_id, int32_t max_pairs, RiBatch o, EreArgs a,
                                       int32_t* d_bad_index, int32_t* d_num_pairs, bool* stage2) {
  const int32_t m = o.m;
  EpxTickBytesScratch t;
  int rc;
  if ((rc = carve(e, &e->enc_misc, &t, [&](Carver& c) { return lay_epx_tick_bytes(c, (size_t)m, (size_t)e->st.n, cmds_on(e)); })))
    return rc;
  if (!o.out_triple) o.out_triple = t.out_triple;  // (null without the store: nobody reads it then)
  if (!o.outcome) o.outcome = t.outcome;
  if (!o.out_ballot) o.out_ballot = t.out_ballot;
  if (!o.out_status) o.out_status = t.out_status;
  if (!o.out_end) o.out_end = t.out_end;
  if (!o.out_deps) o.out_deps = t.out_deps;
  // a refused tick encodes nothing: the totals and the first offset say so unless the encoder runs
  HIPCHK(e, hipMemsetAsync(a.totals, 0, 24, e->stream));
  HIPCHK(e, hipMemsetAsync(a.totals + 3, 0xFF, 8, e->stream));
  HIPCHK(e, hipMemsetAsync(a.out_offsets, 0, 8, e->stream));
  EpxReplicaTickScratch w;
  if ((rc = replica_tick_impl(e, d_in, in_len, d_in_offsets, triple_base, d_triple_id, max_pairs, o, d_bad_index, d_num_pairs, &w,
                              stage2)) ||
      !*stage2)
    return rc;
  a.m = m;
  a.in = fpxw::EpxReplyIn{e->st.n,   o.to,         w.leader,     w.number,   w.b_ord,  w.b_rep,
                          o.outcome, o.out_ballot, o.out_status, o.out_deps, o.out_end};
  // (the burst's own commands are in the store by now: the put ran behind stage 2)
  if (cmds_on(e)) a.in.out_triple = o.out_triple, a.in.cmds = cmds_source(e);
  return reply_encode_launch(e, a, t.enc);
}

int32_t fpx_wire_epx_replica_tick_bytes_dev(fpx_epx* e, const uint8_t* d_in, int64_t in_len, const int64_t* d_in_offsets,
                                            int32_t m, const int32_t* d_to, int32_t triple_base, const int32_t* d_triple_id,
                                            int32_t max_pairs, uint8_t* d_out, int64_t out_cap, int64_t* d_out_offsets,
                                            uint8_t* d_reply_kind, int64_t* d_totals, int32_t* d_outcome, int32_t* d_out_ballot,
                                            int32_t* d_out_status, int32_t* d_out_deps, int32_t* d_out_values_end,
                                            int32_t* d_out_triple, int32_t* d_bad_index, int32_t* d_num_pairs) {
  if (replica_tick_check(e, in_len, m, max_pairs) || !d_bad_index ||
      reply_encode_check(e, m, d_out, out_cap, d_out_offsets, d_reply_kind, d_totals))
    return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) {
    HIPCHK(e, hipMemsetAsync(d_bad_index, 0xFF, 4, e->stream));
    if (d_num_pairs) HIPCHK(e, hipMemsetAsync(d_num_pairs, 0, 4, e->stream));
    HIPCHK(e, hipMemsetAsync(d_totals, 0, 24, e->stream));
    HIPCHK(e, hipMemsetAsync(d_totals + 3, 0xFF, 8, e->stream));
    HIPCHK(e, hipMemsetAsync(d_out_offsets, 0, 8, e->stream));
    return FPX_OK;
  }
  if ((in_len > 0 && !d_in) || !d_in_offsets || !d_to) return FPX_EINVAL;
  RiBatch o;
  memset(&o, 0, sizeof(o));
  o.m = m, o.to = d_to, o.outcome = d_outcome, o.out_ballot = d_out_ballot, o.out_status = d_out_status, o.out_deps = d_out_deps;
  o.out_end = d_out_values_end, o.out_triple = d_out_triple;
  EreArgs a;
  memset(&a, 0, sizeof(a));
  a.out = d_out, a.cap = out_cap, a.out_offsets = d_out_offsets, a.reply_kind = d_reply_kind, a.totals = d_totals;
  bool stage2 = false;
  const int rc = replica_tick_bytes_impl(e, d_in, in_len, d_in_offsets, triple_base, d_triple_id, max_pairs, o, a, d_bad_index,
                                         d_num_pairs, &stage2);
  return rc ? rc : launch_check(e);
}

// the host form's end: the encoder's FPX_ECAPACITY means the tick WAS applied, so the held outputs reach the caller then too
// (stage 1's FPX_ECAPACITY -- too many pairs, the key table's limits -- applied nothing: *stage2 tells the two apart)
struct EpxBytesEnd {
  fpx_epx* e;
  const bool* stage2;
  int operator()() const { return fpx_epx_sync(e); }
  bool applied(int rc) const { return EpxEnd::applied(rc) || (rc == FPX_ECAPACITY && *stage2); }
};

int32_t fpx_wire_epx_replica_tick_bytes(fpx_epx* e, const uint8_t* in_bytes, int64_t in_len, const int64_t* in_offsets, int32_t m,
                                        const int32_t* to, int32_t triple_base, const int32_t* triple_id, int32_t max_pairs,
                                        uint8_t* out_bytes, int64_t out_cap, int64_t* out_offsets, uint8_t* reply_kind,
                                        int64_t* totals, int32_t* outcome, int32_t* out_ballot, int32_t* out_status,
                                        int32_t* out_deps, int32_t* out_values_end, int32_t* out_triple, int32_t* bad_index,
                                        int32_t* num_pairs) {
  if (replica_tick_check(e, in_len, m, max_pairs) || reply_encode_check(e, m, out_bytes, out_cap, out_offsets, reply_kind, totals))
    return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (bad_index) *bad_index = -1;
  if (num_pairs) *num_pairs = 0;
  totals[0] = totals[1] = totals[2] = 0, totals[3] = -1;
  out_offsets[0] = 0;
  if (m == 0) return FPX_OK;
  if ((in_len > 0 && !in_bytes) || !in_offsets || !to) return FPX_EINVAL;
  const size_t mn = (size_t)m * e->st.n;
  const uint8_t* d_in = nullptr;
  const int64_t* d_off = nullptr;
  const int32_t* d_triple = nullptr;
  int32_t *d_bad = nullptr, *d_np = nullptr;
  int32_t res[2] = {-1, 0};
  RiBatch o;
  memset(&o, 0, sizeof(o));
  o.m = m;
  EreArgs a;
  memset(&a, 0, sizeof(a));
  a.cap = out_cap;
  bool stage2 = false;
  // an inbox output the caller leaves out is not staged: the tick keeps it in its own scratch
  auto opt_held = [](int32_t*& d, int32_t* dst, size_t count) { return dst ? held(d, dst, count) : absent(d); };
  // the reply bytes, offsets and kinds are scratch of the call: they come down behind it (below), the bytes the encoder wrote
  // and no more, and only when it wrote them -- a refusal leaves the caller's arrays as they were
  const int32_t rc = fpx::host_call(
      e,
      {in(d_in, in_bytes, (size_t)in_len), in(d_off, in_offsets, (size_t)m + 1), in(o.to, to, m), opt_in(d_triple, triple_id, m),
       opt_held(o.outcome, outcome, m), opt_held(o.out_ballot, out_ballot, m), opt_held(o.out_status, out_status, m),
       opt_held(o.out_end, out_values_end, m), opt_held(o.out_triple, out_triple, m), opt_held(o.out_deps, out_deps, mn),
       scratch(a.out, (size_t)out_cap), scratch(a.out_offsets, (size_t)m + 1), scratch(a.reply_kind, m), out(a.totals, totals, 4),
       out(d_bad, &res[0], 1), out(d_np, &res[1], 1)},
      [&]() -> int {
        return replica_tick_bytes_impl(e, d_in, in_len, d_off, triple_base, d_triple, max_pairs, o, a, d_bad, d_np, &stage2);
      },
      EpxBytesEnd{e, &stage2});
  if (bad_index && rc == FPX_EINVAL) *bad_index = res[0];
  if (num_pairs) *num_pairs = res[1];
  if (rc == FPX_OK || rc == FPX_EFATAL_PROTOCOL) {
    HIPCHK(e, hipMemcpyAsync(out_offsets, a.out_offsets, ((size_t)m + 1) * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(reply_kind, a.reply_kind, (size_t)m, hipMemcpyDeviceToHost, e->stream));
    if (totals[1] > 0) HIPCHK(e, hipMemcpyAsync(out_bytes, a.out, (size_t)totals[1], hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
  } else if (!(rc == FPX_ECAPACITY && stage2)) {
    totals[0] = totals[1] = totals[2] = 0, totals[3] = -1;
  }
  return rc;
}

int32_t fpx_epx_read_leader_state(fpx_epx* e, int32_t replica, int32_t leader, int32_t number, int32_t out[8],
                                  int32_t* responses) {
  if (!leader_state_on(e) || !out || replica < 0 || replica >= e->st.n || leader < 0 || leader >= e->st.n || number < 0 ||
      number >= e->st.num_instances)
    return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  const int n = e->st.n;
  const size_t c = ((size_t)replica * n + leader) * e->st.num_instances + number;
  int32_t h[4], ballot = 0, vote = 0;
  uint8_t kind = 0;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipMemcpy(h, e->ls.head + c, 16, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(&kind, e->st.cl_status + c, 1, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(&ballot, e->st.cl_ballot + c, 4, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(&vote, e->st.cl_vote + c, 4, hipMemcpyDeviceToHost));
  const int phase = h[0] & 3;
  const bool live = phase != 0 && kind != CL_COMMITTED && ballot == h[1] && (phase == LS_PREPARING || vote == h[1]);
  out[0] = live ? phase : 0, out[1] = h[1], out[2] = (h[0] >> 2) & 1, out[3] = h[2], out[4] = h[3], out[5] = (h[0] >> 3) & 1;
  out[6] = ((uint32_t)h[0] >> 8) & 0xff, out[7] = phase;
  if (responses) HIPCHK(e, hipMemcpy(responses, e->ls.resp + c * n * (n + 2), (size_t)n * (n + 2) * 4, hipMemcpyDeviceToHost));
  return FPX_OK;
}

// ---- originating recovery (FPX_EPX_F_RECOVERY): csrc/fpx_epx_recovery.hpp ------------------------------------------------
static bool recovery_on(const fpx_epx* e) { return leader_state_on(e) && (e->cfg.flags & FPX_EPX_F_RECOVERY) && e->ls.prep; }

int32_t fpx_epx_recover(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* at, int32_t* outcome,
                        int32_t* out_ballot_ordering, int32_t* out_status, int32_t* out_vote_ballot, int32_t* out_triple) {
  if (!e || m < 0 || !recovery_on(e)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) return FPX_OK;
  if (!leader || !number || !at) return FPX_EINVAL;
  const int n = e->st.n;
  RvBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m;
  auto launch = [&]() -> int {
    int rc;
    if ((rc = next_run_id(e, &b.run_id))) return rc;
    const dim3 gm((m + 255) / 256), blk(256);
    hipLaunchKernelGGL(k_rv_validate, gm, blk, 0, e->stream, e->st, b);
    // every row of `rank` to its exclusive scan, row r's total to count[r]
    hipLaunchKernelGGL(k_lr_bscan, dim3(n), blk, 0, e->stream, e->st, b.rank, m, (size_t)m, b.count);
    hipLaunchKernelGGL(k_rv_base, dim3(1), dim3(64), 0, e->stream, e->st, b);
    by_n(n, [&](auto N) { hipLaunchKernelGGL((k_rv_install<N>), gm, blk, 0, e->stream, e->st, e->ls, b); });
    return FPX_OK;
  };
  return host_call(e, {in(b.leader, leader, m), in(b.number, number, m), in(b.at, at, m), scratch(b.rank, (size_t)m * n),
                       scratch(b.base, 8), scratch(b.count, 8, 0), held(b.outcome, outcome, m),
                       held(b.out_ord, out_ballot_ordering, m), held(b.out_status, out_status, m),
                       held(b.out_vote, out_vote_ballot, m), held(b.out_triple, out_triple, m)},
                   launch);
}

// b: the messages and the outputs (any of which may be null); the scratch fields are filled here
static int32_t recovery_replies_launch(fpx_epx* e, RrBatch b) {
  const int m = b.m;
  int rc;
  if ((rc = grow(e, &e->kv, (size_t)m * 8))) return rc;
  if ((rc = grow(e, &e->kv2, (size_t)m * 8))) return rc;
  LrScratch ls;  // the compaction of fpx_epx_leader_replies, on this burst's flags
  if ((rc = carve(e, &e->lr_misc, &ls, [&](Carver& c) { return lay_leader_replies(c, m, (m + LR_BLOCK - 1) / LR_BLOCK); })))
    return rc;
  b.kv = (uint2*)e->kv.p, b.flag = ls.flag;
  const dim3 gm((m + 255) / 256), blk(256);
  hipLaunchKernelGGL(k_rr_validate, gm, blk, 0, e->stream, e->st, b);
  b.sorted = sort_by_cell(e, m, b.kv, (uint2*)e->kv2.p, &rc);
  if (rc) return rc;
  by_n(e->st.n, [&](auto N) { hipLaunchKernelGGL((k_rr_walk<N>), gm, blk, 0, e->stream, e->st, e->ls, b); });
  launch_compaction(e, m, ls, b.decided, b.num_decided);
  return FPX_OK;
}

int32_t fpx_epx_recovery_replies_dev(fpx_epx* e, int32_t m, const int32_t* d_to, const int32_t* d_leader, const int32_t* d_number,
                                     const int32_t* d_ballot_ordering, const int32_t* d_ballot_replica,
                                     const int32_t* d_replica_index, const int32_t* d_status, const int32_t* d_vote_ballot_ordering,
                                     const int32_t* d_vote_ballot_replica, const int32_t* d_triple_id,
                                     const int32_t* d_sequence_number, const int32_t* d_deps, const int32_t* d_deps_values_end,
                                     int32_t as_intended, int32_t* d_outcome, int32_t* d_out_source, int32_t* d_out_triple,
                                     int32_t* d_out_ballot, int32_t* d_out_seq, int32_t* d_out_deps, int32_t* d_out_values_end,
                                     int32_t* d_decided_index, int32_t* d_num_decided) {
  if (!e || m < 0 || m >= (1 << 30) || !recovery_on(e)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) {
    if (d_num_decided) HIPCHK(e, hipMemsetAsync(d_num_decided, 0, 4, e->stream));
    return FPX_OK;
  }
  if (!d_to || !d_leader || !d_number || !d_ballot_ordering || !d_ballot_replica || !d_replica_index || !d_status ||
      !d_vote_ballot_ordering || !d_vote_ballot_replica || !d_triple_id || !d_deps)
    return FPX_EINVAL;
  RrBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m, b.as_intended = as_intended ? 1 : 0, b.to = d_to, b.leader = d_leader, b.number = d_number, b.b_ord = d_ballot_ordering;
  b.b_rep = d_ballot_replica, b.ridx = d_replica_index, b.status = d_status, b.v_ord = d_vote_ballot_ordering;
  b.v_rep = d_vote_ballot_replica, b.triple = d_triple_id, b.seq = d_sequence_number, b.deps = d_deps, b.dend = d_deps_values_end;
  b.outcome = d_outcome, b.out_source = d_out_source, b.out_triple = d_out_triple, b.out_ballot = d_out_ballot, b.out_seq = d_out_seq;
  b.out_deps = d_out_deps, b.out_end = d_out_values_end, b.decided = d_decided_index, b.num_decided = d_num_decided;
  int rc = recovery_replies_launch(e, b);
  return rc ? rc : launch_check(e);
}

int32_t fpx_epx_recovery_replies(fpx_epx* e, int32_t m, const int32_t* to, const int32_t* leader, const int32_t* number,
                                 const int32_t* ballot_ordering, const int32_t* ballot_replica, const int32_t* replica_index,
                                 const int32_t* status, const int32_t* vote_ballot_ordering, const int32_t* vote_ballot_replica,
                                 const int32_t* triple_id, const int32_t* sequence_number, const int32_t* deps,
                                 const int32_t* deps_values_end, int32_t as_intended, int32_t* outcome, int32_t* out_source,
                                 int32_t* out_triple, int32_t* out_ballot, int32_t* out_seq, int32_t* out_deps,
                                 int32_t* out_values_end, int32_t* decided_index, int32_t* num_decided) {
  if (!e || m < 0 || m >= (1 << 30) || !recovery_on(e)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) {
    if (num_decided) *num_decided = 0;
    return FPX_OK;
  }
  if (!to || !leader || !number || !ballot_ordering || !ballot_replica || !replica_index || !status || !vote_ballot_ordering ||
      !vote_ballot_replica || !triple_id || !deps)
    return FPX_EINVAL;
  const size_t mn = (size_t)m * e->st.n;
  RrBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m, b.as_intended = as_intended ? 1 : 0;
  return host_call(e, {in(b.to, to, m), in(b.leader, leader, m), in(b.number, number, m), in(b.b_ord, ballot_ordering, m),
                       in(b.b_rep, ballot_replica, m), in(b.ridx, replica_index, m), in(b.status, status, m),
                       in(b.v_ord, vote_ballot_ordering, m), in(b.v_rep, vote_ballot_replica, m), in(b.triple, triple_id, m),
                       opt_in(b.seq, sequence_number, m), opt_in(b.dend, deps_values_end, m), in(b.deps, deps, mn),
                       held(b.outcome, outcome, m), held(b.out_source, out_source, m), held(b.out_triple, out_triple, m),
                       held(b.out_ballot, out_ballot, m), held(b.out_seq, out_seq, m), held(b.out_end, out_values_end, m),
                       held_first(b.decided, decided_index, m, b.num_decided), held(b.out_deps, out_deps, mn),
                       held(b.num_decided, num_decided, 1)},
                   [&]() -> int { return recovery_replies_launch(e, b); });
}

// key or (key_off, keys): the single-key form or the key lists
static int32_t lead_accept_impl(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* at,
                                const int32_t* ballot_ordering, const int32_t* key, const int32_t* key_off, const int32_t* keys,
                                const uint8_t* is_set, const int32_t* triple_id, const int32_t* sequence_number,
                                const int32_t* deps, const int32_t* deps_values_end) {
  if (!e || m < 0 || !recovery_on(e)) return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  if (m == 0) return FPX_OK;
  if (!leader || !number || !at || !ballot_ordering || !(key || key_off) || !is_set || !triple_id || !deps) return FPX_EINVAL;
  const int n = e->st.n;
  int64_t P = 0;
  if (key_off && check_key_lists(m, key_off, keys, e->st.num_keys, &P)) return FPX_EINVAL;
  LaBatch b;
  memset(&b, 0, sizeof(b));
  b.m = m;
  auto launch = [&]() -> int {
    int rc;
    if ((rc = next_run_id(e, &b.run_id))) return rc;
    if (!key_off) b.key_off = b.keys = nullptr;
    else b.key = nullptr;
    const dim3 gm((m + 255) / 256), blk(256);
    hipLaunchKernelGGL(k_la_validate, gm, blk, 0, e->stream, e->st, b);
    by_n(n, [&](auto N) { hipLaunchKernelGGL((k_la_install<N>), gm, blk, 0, e->stream, e->st, e->ls, b); });
    return FPX_OK;
  };
  return host_call(e, {in(b.leader, leader, m), in(b.number, number, m), in(b.at, at, m), in(b.b_ord, ballot_ordering, m),
                       in(b.key, key, key ? m : 0), in(b.triple, triple_id, m), opt_in(b.seq, sequence_number, m),
                       opt_in(b.dend, deps_values_end, m), in(b.deps, deps, (size_t)m * n), in(b.is_set, is_set, m),
                       in(b.key_off, key_off, key_off ? m + 1 : 0), in(b.keys, keys, P)},
                   launch);
}

int32_t fpx_epx_lead_accept(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* at,
                            const int32_t* ballot_ordering, const int32_t* key, const uint8_t* is_set, const int32_t* triple_id,
                            const int32_t* sequence_number, const int32_t* deps, const int32_t* deps_values_end) {
  if (m > 0 && !key) return FPX_EINVAL;
  return lead_accept_impl(e, m, leader, number, at, ballot_ordering, key, nullptr, nullptr, is_set, triple_id, sequence_number,
                          deps, deps_values_end);
}

int32_t fpx_epx_lead_accept_mk(fpx_epx* e, int32_t m, const int32_t* leader, const int32_t* number, const int32_t* at,
                               const int32_t* ballot_ordering, const int32_t* key_offsets, const int32_t* keys,
                               const uint8_t* is_set, const int32_t* triple_id, const int32_t* sequence_number,
                               const int32_t* deps, const int32_t* deps_values_end) {
  if (m > 0 && !key_offsets) return FPX_EINVAL;
  return lead_accept_impl(e, m, leader, number, at, ballot_ordering, nullptr, key_offsets, keys, is_set, triple_id,
                          sequence_number, deps, deps_values_end);
}

int32_t fpx_epx_read_recovery_state(fpx_epx* e, int32_t replica, int32_t leader, int32_t number, int32_t* out) {
  if (!recovery_on(e) || !out || replica < 0 || replica >= e->st.n || leader < 0 || leader >= e->st.n || number < 0 ||
      number >= e->st.num_instances)
    return FPX_EINVAL;
  DeviceScope _dg(e->cfg.device);
  const int n = e->st.n;
  const size_t c = ((size_t)replica * n + leader) * e->st.num_instances + number;
  int32_t h[4], p[16];
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipMemcpy(h, e->ls.head + c, 16, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(p, e->ls.prep + c * n, (size_t)n * 8, hipMemcpyDeviceToHost));
  const bool preparing = (h[0] & 3) == LS_PREPARING;
  for (int q = 0; q < n; ++q) {
    const bool has = preparing && (((uint32_t)h[0] >> (8 + q)) & 1u);
    out[q * 3] = has ? (int32_t)(((uint32_t)h[0] >> (16 + 2 * q)) & 3u) : -1;
    out[q * 3 + 1] = has ? p[2 * q] : -1;
    out[q * 3 + 2] = has ? p[2 * q + 1] : -1;
  }
  return FPX_OK;
}

}  // extern "C"
