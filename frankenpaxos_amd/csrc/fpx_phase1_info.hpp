// fpx_phase1_info.hpp -- Phase1b.info of EVERY selected acceptor in one device pass (fpx_acceptor_phase1b_info_all_dev).
//
// Acceptor.handlePhase1a answers with its votes in the slots >= chosenWatermark, ascending (states.iteratorFrom,
// multipaxos/Acceptor.scala:163-181, mencius/Acceptor.scala:181-199).  fpx_acceptor_phase1b_info does that for ONE acceptor:
// a strided gather of its column over the whole window and a host loop.  A leader change asks every acceptor, so here
// the vote rows are read once, coalesced, and compacted for all of them: a stable, acceptor-major compaction of the
// cells.  Entry e = group * R + replica; the records (slot, vote_round, vote_value) of entry e are
// offsets[e] .. offsets[e + 1], the entries back to back in entry order, an unselected entry's run empty.
//
//   k_p1i_count<G>    per (chunk of tiles, group) the number of records of every acceptor: G lanes per slot, one aligned
//                     int4 of vote rounds per lane (k_phase1b_scan's access), a lane owns its four acceptors and keeps a
//                     64-bit "voted" word per owned acceptor over a TILE of 64 slots of the group; the tile's count is a
//                     popcount
//   k_p1i_colscan     per acceptor column the exclusive scan of the chunk counts, in place, and the column's total
//   k_p1i_offsets     ONE workgroup: the exclusive scan of the entries' totals = the offsets, the totals, the verdict
//   k_p1i_scatter<G>  the count pass's walk again, now with both vote rows: a record's place is the entry's offset + its
//                     chunk's base + the votes of the acceptor seen so far in the chunk; a tile's records are compacted
//                     in LDS and leave as whole runs -- no atomics anywhere, so the result is deterministic
//
// Geometry.  The cells of row s belong to group_of_slot(g, s) only, and the groups take the slots in turns with period
// ngroups (slot = (k * num_groups + acceptor group) * num_leader_groups + leader group): slot s and slot s % ngroups
// have the same group, and the ngroups phases of a period are the ngroups groups.  So the window is cut into spans of
// 64 * ngroups slots, and the TILE (t, p) is the 64 slots t * 64 * ngroups + j * ngroups + p, j = 0 .. 63: the slots of
// group group_of_slot(g, p) in the span, ascending.  Which group a phase is and where a slot lives come from
// group_of_slot / phys_slot (fpx_kernels.hpp); nothing here knows the layouts (leader-group-major rows, interleaved
// R <= 4 rows).
//
// Only vote_round / vote_value are read: the lazy Phase1a records and ballot_sum describe ballots.  The scan is [lo, S),
// not bounded by max_voted, so a deferred fold (k_finalize) of the vote launch before it may stay pending.
#pragma once
#include "fpx_kernels.hpp"
#include "fpx_scan.hpp"

namespace fpx {

constexpr int P1I_TILE = 64;   // slots of one group per tile: one bit each of the 64-bit voted word
constexpr int P1I_CHUNK = 4;   // tiles per unit of work (one wavefront): 256 rows of a group
constexpr int P1I_COLS = 16;   // k_p1i_colscan: columns per workgroup ...
constexpr int P1I_SEGS = 64;   // ... and the segments a column's chunks are cut into (COLS * SEGS = 1024 threads)

struct P1iArgs {
  const uint64_t* masks;  // [ngroups][4], bit base + replica (fpx_acceptor_phase1a's target_mask), or null = all
  int32_t lo;             // max(chosen_watermark, 0)
  int32_t vec;            // rows are read as aligned int4 (k_phase1b_scan)
  int32_t ntiles;         // spans of 64 * ngroups slots
  int32_t nchunks;        // ceil(ntiles / P1I_CHUNK)
  int32_t ES;             // columns: ngroups * RS (column of entry (grp, r) = grp * RS + r)
  int32_t* csum;          // [nchunks][ES] records per (chunk, column); after k_p1i_colscan: of the chunks before
  int32_t* ctot;          // [ES] records per column
  int32_t* go;            // [1] 1 = scatter
  int64_t cap;
  int64_t* offsets;       // [E + 1]
  int32_t* slot;
  int32_t* vote_round;
  int32_t* vote_value;
  int64_t* totals;        // [2] needed, written
};

// the lanes of the wavefront that hold the same four acceptors: lane = q * G + gi, bit q * G of the pattern << gi
template <int G>
__device__ __forceinline__ uint64_t p1i_same_quad() {
  uint64_t m = 0;
#pragma unroll
  for (int q = 0; q < 64 / G; ++q) m |= 1ull << (q * G);
  return m;
}

// which of the lane's four acceptors are selected: bit k = acceptor r0 + k (a partial last quad has fewer)
__device__ __forceinline__ uint32_t p1i_selected(const Geom& g, const uint64_t* masks, int grp, int r0) {
  if (r0 >= g.R) return 0u;
  const int left = g.R - r0;
  const uint32_t in_row = left >= 4 ? 0xFu : ((1u << left) - 1u);
  if (!masks) return in_row;
  const int bit = g.base + r0;  // (replica_base is a multiple of 4: the quad's bits share a word)
  return (uint32_t)((masks[(size_t)grp * 4 + (bit >> 6)] >> (bit & 63)) & 0xFull) & in_row;
}

__device__ __forceinline__ int4v p1i_load(const int32_t* a, size_t row, int r0, int R, int vec) {
  int4v v = {-1, -1, -1, -1};
  if (vec) {
    v = *reinterpret_cast<const int4v*>(a + row);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (r0 + k < R) v[k] = a[row + k];
  }
  return v;
}

// the lane's four cells of both vote rows of row `ps` (vv null: the rounds only); a compact row's are its record
__device__ __forceinline__ void p1i_load_votes(const Geom& g, const State& st, size_t ps, int r0, int vec, int4v* vr, int4v* vv) {
  VoteRec rec;
  if (row_record(st, ps, &rec)) {  // (cells past R: masked by the callers' `sel`)
    *vr = int4v{rec.round, rec.round, rec.round, rec.round};
    if (vv) *vv = int4v{rec.value, rec.value, rec.value, rec.value};
    return;
  }
  const size_t row = ps * g.VS + r0;
  *vr = p1i_load(st.vote_round, row, r0, g.R, vec);
  if (vv) *vv = p1i_load(st.vote_value, row, r0, g.R, vec);
}

template <int G>
__global__ void __launch_bounds__(256) k_p1i_count(const Geom g, const State st, const P1iArgs a) {
  if (st.status[ST_ABORT] != 0) return;
  constexpr int Q = 64 / G;
  const int lane = threadIdx.x & 63;
  const int gi = lane & (G - 1), q = lane / G;
  const int r0 = 4 * gi;
  const int NG = g.ngroups;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const int nunits = a.nchunks * NG;
  for (int u = wave; u < nunits; u += nwaves) {
    const int c = u / NG, p = u - c * NG;
    const int grp = group_of_slot(g, p);
    const uint32_t sel = p1i_selected(g, a.masks, grp, r0);
    int run[4] = {0, 0, 0, 0};
    for (int t = 0; t < P1I_CHUNK; ++t) {
      const int T = c * P1I_CHUNK + t;
      if (T >= a.ntiles) break;
      const int64_t first = (int64_t)T * P1I_TILE * NG + p;  // the tile's slot j is first + j * NG
      if (first + (int64_t)(P1I_TILE - 1) * NG < a.lo || first >= g.S) continue;  // wholly below the watermark / past the window
      uint64_t w[4] = {0ull, 0ull, 0ull, 0ull};
      if (sel) {
#pragma unroll 8
        for (int i = 0; i < P1I_TILE / Q; ++i) {
          const int j = i * Q + q;
          const int64_t s = first + (int64_t)j * NG;
          if (s < a.lo || s >= g.S) continue;
          int4v vr;
          p1i_load_votes(g, st, (size_t)phys_slot(g, (int)s), r0, a.vec, &vr, nullptr);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (vr[k] != -1) w[k] |= 1ull << j;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // the lanes of the quad saw different slots of the tile: together, the tile's word
#pragma unroll
        for (int m = G; m < 64; m <<= 1) w[k] |= shfl_xor64(w[k], m);
        if ((sel >> k) & 1u) run[k] += __popcll(w[k]);
      }
    }
    if (q == 0 && r0 < g.R) {
      const int4v v = {run[0], run[1], run[2], run[3]};
      *reinterpret_cast<int4v*>(a.csum + (size_t)c * a.ES + (size_t)grp * g.RS + r0) = v;
    }
  }
}

// workgroup b: columns [b * COLS, ...); thread (seg, col) sums the chunks of its segment, the segments' sums are scanned
// through LDS, then the thread rewrites its chunks as the count of the chunks before them
__global__ void __launch_bounds__(P1I_COLS * P1I_SEGS) k_p1i_colscan(const State st, const P1iArgs a) {
  if (st.status[ST_ABORT] != 0) return;
  __shared__ int part[P1I_SEGS][P1I_COLS];
  const int cl = threadIdx.x % P1I_COLS, seg = threadIdx.x / P1I_COLS;
  const int col = blockIdx.x * P1I_COLS + cl;
  const int per = (a.nchunks + P1I_SEGS - 1) / P1I_SEGS;
  const int c0 = seg * per, c1 = (c0 + per) < a.nchunks ? (c0 + per) : a.nchunks;
  int sum = 0;
  if (col < a.ES)
    for (int c = c0; c < c1; ++c) sum += a.csum[(size_t)c * a.ES + col];
  part[seg][cl] = sum;
  __syncthreads();
  if (col >= a.ES) return;
  int before = 0, all = 0;
  for (int k = 0; k < P1I_SEGS; ++k) {
    const int v = part[k][cl];
    if (k < seg) before += v;
    all += v;
  }
  for (int c = c0; c < c1; ++c) {
    int32_t* w = a.csum + (size_t)c * a.ES + col;
    const int v = *w;
    *w = before;
    before += v;
  }
  if (seg == 0) a.ctot[col] = all;
}

// ONE workgroup of 1024: thread i takes `per` consecutive entries
__global__ void __launch_bounds__(1024) k_p1i_offsets(const Geom g, const State st, const P1iArgs a) {
  __shared__ int64_t wtot[16];
  const int t = threadIdx.x;
  if (st.status[ST_ABORT] != 0) {
    // the run was refused (a bad tick, a contract violation): nothing is answered
    if (t == 0) a.totals[0] = 0, a.totals[1] = 0, a.offsets[0] = 0, *a.go = 0;
    return;
  }
  const int E = g.ngroups * g.R;
  const int per = (E + 1023) / 1024;
  const int e0 = t * per, e1 = (e0 + per) < E ? (e0 + per) : E;
  int64_t mine = 0;
  for (int e = e0; e < e1; ++e) mine += a.ctot[(e / g.R) * g.RS + e % g.R];
  int64_t total;
  int64_t before = block_excl_scan<ScanSum, 1024>(mine, (int64_t)0, wtot, &total);
  for (int e = e0; e < e1; ++e) {
    a.offsets[e] = before;
    before += a.ctot[(e / g.R) * g.RS + e % g.R];
  }
  if (t != 0) return;
  a.offsets[E] = total;
  a.totals[0] = total, a.totals[1] = total < a.cap ? total : a.cap;
  *a.go = a.cap > 0;  // a sizing call is over here
  if (total > a.cap) report(st, 5 /*FPX_ECAPACITY*/, -1, -1, -1);  // the records below cap are written all the same
}

// The scatter, with whole-line stores: the records of a tile are compacted in LDS, per acceptor, and written out as one
// run of up to 64 records (256 contiguous bytes per array) per store instruction.  ONE wavefront per workgroup; a unit
// is (chunk, group, block of 64 acceptors): GL = min(G, 16) lanes per slot, so a row is still read in whole 128-byte
// lines and the staging is 3 x 64 x 65 words (the row stride 65 spreads the owners of one rank over the banks).  A
// record's rank in its tile is the votes of its acceptor in the steps before plus the popcount of a ballot over the
// quad's lanes with earlier slots of the same step.  Storing each record straight to offset + rank instead (4-byte
// stores into 64 runs per instruction) took 5x as long at R = 256 (profiles/phase1_info.md).
constexpr int P1I_LDS_STRIDE = P1I_TILE + 1;

template <int G>
__global__ void __launch_bounds__(64) k_p1i_scatter(const Geom g, const State st, const P1iArgs a) {
  if (st.status[ST_ABORT] != 0 || *a.go == 0) return;
  constexpr int GL = G < 16 ? G : 16;
  constexpr int CB = G / GL;
  constexpr int Q = 64 / GL;
  constexpr int NA = 4 * GL;  // acceptors of a block
  __shared__ int32_t l_slot[NA * P1I_LDS_STRIDE], l_vr[NA * P1I_LDS_STRIDE], l_vv[NA * P1I_LDS_STRIDE];
  __shared__ int64_t l_at[NA];
  __shared__ int32_t l_n[NA];
  const int lane = threadIdx.x;
  const int gi = lane & (GL - 1), q = lane / GL;
  const int NG = g.ngroups;
  const uint64_t quad = p1i_same_quad<GL>() << gi;
  const uint64_t below = quad & ((1ull << lane) - 1ull);
  const int nunits = a.nchunks * NG * CB;
  for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
    const int cb = u % CB, cp = u / CB;
    const int c = cp / NG, p = cp - c * NG;
    const int r0 = 4 * (cb * GL + gi);
    const int grp = group_of_slot(g, p);
    const uint32_t sel = p1i_selected(g, a.masks, grp, r0);
    int64_t at[4] = {0, 0, 0, 0};
    if (sel) {
      const int4v cbase = *reinterpret_cast<const int4v*>(a.csum + (size_t)c * a.ES + (size_t)grp * g.RS + r0);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((sel >> k) & 1u) at[k] = a.offsets[(size_t)grp * g.R + r0 + k] + cbase[k];
    }
    for (int t = 0; t < P1I_CHUNK; ++t) {
      const int T = c * P1I_CHUNK + t;
      if (T >= a.ntiles) break;
      const int64_t first = (int64_t)T * P1I_TILE * NG + p;
      if (first + (int64_t)(P1I_TILE - 1) * NG < a.lo || first >= g.S) continue;
      int cnt[4] = {0, 0, 0, 0};
#pragma unroll 4
      for (int i = 0; i < P1I_TILE / Q; ++i) {
        const int j = i * Q + q;
        const int64_t s = first + (int64_t)j * NG;
        const bool live = sel && s >= a.lo && s < g.S;
        int4v vr = {-1, -1, -1, -1}, vv = {-1, -1, -1, -1};
        if (live) {
          p1i_load_votes(g, st, (size_t)phys_slot(g, (int)s), r0, a.vec, &vr, &vv);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool v = live && ((sel >> k) & 1u) && vr[k] != -1;
          const uint64_t b = __ballot(v);
          const int at_l = (4 * gi + k) * P1I_LDS_STRIDE + cnt[k] + __popcll(b & below);
          cnt[k] += __popcll(b & quad);
          if (v) l_slot[at_l] = (int32_t)s, l_vr[at_l] = vr[k], l_vv[at_l] = vv[k];
        }
      }
      if (q == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) l_at[4 * gi + k] = at[k], l_n[4 * gi + k] = cnt[k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) at[k] += cnt[k];
      __syncthreads();
      for (int ac = 0; ac < NA; ++ac) {
        const int n = __builtin_amdgcn_readfirstlane(l_n[ac]);
        if (n == 0) continue;
        const int64_t pos = l_at[ac] + lane;
        if (lane < n && pos < a.cap) {
          const int from = ac * P1I_LDS_STRIDE + lane;
          a.slot[pos] = l_slot[from], a.vote_round[pos] = l_vr[from], a.vote_value[pos] = l_vv[from];
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace fpx
