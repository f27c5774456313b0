// fpx_mencius_acceptor_inbox.hpp -- mencius.Acceptor's inbox for a BURST of per-acceptor messages in delivery order:
// handlePhase1a / handlePhase2a / handlePhase2aNoopRange (mencius/Acceptor.scala:142-291), the kinds interleaved and
// addressed to any of the context's acceptors, exactly as if every acceptor had handled its messages one by one -- without
// the host reading anything between the passes.  This is what reference mencius.ProxyLeaders send: one Phase2a per
// acceptor address to quorumSize acceptors of the slot's group, one Phase2aNoopRange per acceptor address to quorumSize
// acceptors of EVERY acceptor group of the leader group (mencius/ProxyLeader.scala:216-303).
//
// The rounds are fpx_acceptor_inbox.hpp's: for acceptor e = (leader group * A + acceptor group) * R + index every message
// of the three kinds meets max(promised[e], rounds of e's earlier messages) and is accepted iff its round is not below
// that (:173, :210, :245).  What is new is the cells.  An accepted range (start, end, round) of e writes (round, Noop) to
// cell (s, e) of every s = start, start + L, ... below end whose row q = s / L has q % A == e's acceptor group
// (:261-277); those cells interleave in delivery order with single Phase2as and with other ranges, and every cell keeps
// what the LAST accepted covering message put there.  A range cannot bid per cell in the claim table (that table is
// sized by the burst, a range covers any number of cells), so the last writer of a cell is settled from two sides:
//
//   points    the claim table settles the last accepted Phase2a i of a cell, as in the MultiPaxos call.  It writes unless
//             an accepted range of the same acceptor with a larger index covers its row.
//   ranges    accepted range j writes every owned cell unless a later accepted range of the same acceptor covers the row
//             or the claim table (probed without inserting) holds a Phase2a with an index above j for the cell.
//
// So every cell is written by exactly one thread, and no output depends on the order the hardware runs threads in.  The
// accepted ranges are compacted into a list in sorted position order (count / exclusive sum / scatter by rank, no atomic
// cursor); the sort is stable, so one acceptor's ranges are ONE run of the list in index order, found by binary search.
//
//   k_mai_keys    thread / message: checks the message and writes the sort key (its entry, or E = skipped)
//   k_sort_count, k_sort_scan, k_sort_scatter   the stable radix sort by entry, as in fpx_acceptor_inbox.hpp
//   k_ai_tilemax<2>, k_ai_tilescan         the running maximum of the rounds
//   k_mai_accept  workgroup / tile: accept or Nack, the replies of all three kinds; an accepted Phase2a bids for its cell;
//                 an accepted range leaves its largest owned slot + 1 (0: it owns none) for the second scan and is flagged;
//                 the tile's number of flags
//   k_mai_offsets one workgroup: the exclusive sum of the tiles' counts, the list's length
//   k_mai_list    workgroup / tile: every flagged position writes its list record by rank: entry, first and last owned row
//                 (first > last: none), round, message index
//   k_ai_tilemax<1>, k_ai_tilescan         the running maximum of the voted slots
//   k_mai_points  workgroup / tile: row_voted of every Phase2a's row; the winning Phase2a of a cell writes it unless a later
//                 range of its acceptor covers the row; the acceptor's new max_voted
//   k_mai_ranges  workgroup / (list record, 256 owned cells): the later ranges of the acceptor staged in LDS, MAI_CHUNK at a
//                 time; a cell nobody later covers and no later Phase2a won is written, and its row marked
//   k_ai_finish   commits promised and max_voted, hands the claim words back, turns a bad message into the status
//
// k_mai_ranges costs (owned cells of a range) x (later accepted ranges of the same acceptor in the burst) interval tests:
// quadratic in the ranges ONE acceptor accepts in ONE burst.  A tick of reference leaders carries a handful per acceptor.
#pragma once
#include "fpx_acceptor_inbox.hpp"

namespace fpx {

constexpr int MAI_CHUNK = 256;  // later ranges staged in LDS per step of k_mai_ranges
enum { MAI_NLIST = 5 };         // word of AcceptorInbox::hdr: the length of the list of accepted ranges

struct MenciusAcceptorInbox {
  AcceptorInbox a;          // grid_cols = 0; slot = a Phase2a's slot, a range's start
  const int32_t* slot_end;  // [n]  a range's end (exclusive); read for no other kind
  int32_t* rflag;           // [n]  by position: 1 = an accepted range
  int32_t* rcnt;            // [ceil(n / AI_TILE)]  flags per tile, then their exclusive sums
  // the accepted ranges in sorted position order: entry (ascending), owned rows q0 .. q1 in steps of A, round, message
  // index (ascending within an entry)
  int32_t *lent, *lq0, *lq1, *lround, *lidx;  // [n]  (MenciusAcceptorInboxScratch::list, in this order)
};

// the first and last row q = s / L of range [start, end) that acceptor group ag owns (q % A == ag); *q0 > *q1: none
__device__ __forceinline__ void mai_owned(const Geom& g, int start, int end, int ag, int* q0, int* q1) {
  const int L = g.num_leader_groups, A = g.num_groups;
  const int rows = (int)(((long long)end - start + L - 1) / L);
  const int f = start / L, l = f + rows - 1;  // rows == 0: l = f - 1 >= -1
  *q0 = f + ((ag - f % A) + A) % A;
  *q1 = l - (((l - ag) % A) + A) % A;
}

__global__ void __launch_bounds__(256) k_mai_keys(const Geom g, const State st, const MenciusAcceptorInbox b, int32_t* key0,
                                                  int32_t* val0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) b.a.hdr[AI_M] = b.a.n;
  if (i >= b.a.n) return;
  int key = b.a.E;
  const int k = b.a.kind[i];
  if (st.status[ST_ABORT] == 0 && k != FPX_WIRE_OTHER) {
    bool bad = k != FPX_WIRE_PHASE2A && k != FPX_WIRE_PHASE2A_NOOP_RANGE && k != FPX_WIRE_PHASE1A;
    int e = -1;
    if (!bad) e = ai_entry(g, b.a, i), bad = e < 0;
    if (!bad) {
      const int r = b.a.round[i];
      bad = r < 0 || r > MAX_ROUND;
    }
    if (!bad && k == FPX_WIRE_PHASE2A) {
      const int s = b.a.slot[i];
      bad = s < 0 || s >= g.S || group_of_slot(g, s) != e / g.R;
    }
    if (!bad && k == FPX_WIRE_PHASE2A_NOOP_RANGE) {
      // (a range of another leader group has its cells in rows this acceptor has no column in)
      const int s = b.a.slot[i], t = b.slot_end[i];
      bad = s < 0 || t < s || t > g.S || s % g.num_leader_groups != (e / g.R) / g.num_groups;
    }
    if (bad) atomicMax(&st.status[ST_MSG_BAD], 0x7fffffff - i);
    else key = e;
  }
  key0[i] = key, val0[i] = i;
}

__global__ void __launch_bounds__(256) k_mai_accept(const Geom g, const State st, const MenciusAcceptorInbox b) {
  __shared__ long long wtot[4];
  __shared__ int wcnt[4];
  const int p = blockIdx.x * AI_TILE + threadIdx.x;
  const long long x = block_excl_scan<ScanMax, 256>(ai_word<2>(b.a, p), b.a.tile[blockIdx.x], wtot);
  int acc = 0, tp = -1, flag = 0;
  if (p < b.a.n && b.a.hdr[AI_OK] != 0) {
    const int key = b.a.key[p], i = b.a.perm[p];
    int rk = 0, rv = -1;
    if (key < b.a.E) {
      const int k = b.a.kind[i], r = b.a.round[i];
      int run = ai_running(x, key, st.promised[key]);
      if (r < run) {  // :173, :210, :245
        rk = FPX_WIRE_NACK, rv = run;
      } else {
        rv = r, run = r;
        if (k == FPX_WIRE_PHASE2A) {
          const int s = b.a.slot[i];
          rk = FPX_WIRE_PHASE2B, acc = s + 1, tp = ai_claim(b.a, (unsigned long long)ai_cell(g, s, key), i);
        } else if (k == FPX_WIRE_PHASE2A_NOOP_RANGE) {
          int q0, q1;
          mai_owned(g, b.a.slot[i], b.slot_end[i], (key / g.R) % g.num_groups, &q0, &q1);
          rk = FPX_WIRE_PHASE2B_NOOP_RANGE, flag = 1;
          if (q0 <= q1) acc = q1 * g.num_leader_groups + (key / g.R) / g.num_groups + 1;
        } else {
          rk = FPX_WIRE_PHASE1B;
        }
      }
      if (p == b.a.n - 1 || b.a.key[p + 1] != key) b.a.fin_round[key] = run;
    }
    if (b.a.reply_kind) b.a.reply_kind[i] = rk;
    if (b.a.reply_value) b.a.reply_value[i] = rv;
  }
  if (p < b.a.n) b.a.accslot[p] = acc, b.a.tpos[p] = tp, b.rflag[p] = flag;
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) b.rcnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// the exclusive sum of the tiles' counts, one workgroup; the total is the list's length
__global__ void __launch_bounds__(AI_SCAN_THREADS) k_mai_offsets(const MenciusAcceptorInbox b) {
  __shared__ int lds[SCAN_ARRAY_LDS(AI_SCAN_THREADS)];
  const int total = scan_array_excl<ScanSum, AI_SCAN_THREADS, 1>(b.rcnt, (b.a.n + AI_TILE - 1) / AI_TILE, lds);
  if (threadIdx.x == 0) b.a.hdr[MAI_NLIST] = total;
}

__global__ void __launch_bounds__(256) k_mai_list(const Geom g, const MenciusAcceptorInbox b) {
  __shared__ int wcnt[4];
  const int p = blockIdx.x * AI_TILE + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int flag = p < b.a.n ? b.rflag[p] : 0;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) wcnt[wave] = __popcll(m);
  __syncthreads();
  if (!flag) return;
  int at = b.rcnt[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) at += wcnt[w];
  const int key = b.a.key[p], i = b.a.perm[p];
  int q0, q1;
  mai_owned(g, b.a.slot[i], b.slot_end[i], (key / g.R) % g.num_groups, &q0, &q1);
  b.lent[at] = key, b.lq0[at] = q0, b.lq1[at] = q1, b.lround[at] = b.a.round[i], b.lidx[at] = i;
}

// the first list position in [lo, hi) whose (entry, index) is above (key, i)
__device__ __forceinline__ int mai_after(const MenciusAcceptorInbox& b, int lo, int hi, int key, int i) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int e = b.lent[mid];
    if (e < key || (e == key && b.lidx[mid] <= i)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the bid a cell's claim word holds, -1 = nobody bid for the cell.  Nothing is inserted: k_mai_accept is complete, and
// between calls every word is AI_EMPTY, so a probe that meets an empty word has passed every place the cell could be
__device__ __forceinline__ int mai_find(const AcceptorInbox& b, unsigned long long cell) {
  const unsigned long long z = cell * 0x9E3779B97F4A7C15ull;
  uint32_t h = (uint32_t)(z >> 32) & b.tmask;
  for (uint32_t probes = 0; probes <= b.tmask; ++probes) {
    const unsigned long long k = b.tkey[h];
    if (k == cell) return b.tval[h];
    if (k == AI_EMPTY) return -1;
    h = (h + 1) & b.tmask;
  }
  return -1;
}

__global__ void __launch_bounds__(256) k_mai_points(const Geom g, const State st, const MenciusAcceptorInbox b) {
  __shared__ long long wtot[4];
  const int p = blockIdx.x * AI_TILE + threadIdx.x;
  const long long x = block_excl_scan<ScanMax, 256>(ai_word<1>(b.a, p), b.a.tile[blockIdx.x], wtot);
  if (p >= b.a.n || b.a.hdr[AI_OK] == 0) return;
  const int key = b.a.key[p];
  if (key >= b.a.E) return;
  const int i = b.a.perm[p], acc = b.a.accslot[p];
  int mv = ai_running(x, key, st.max_voted[key]);
  if (b.a.kind[i] == FPX_WIRE_PHASE2A) {
    const int s = b.a.slot[i];
    // the row is no longer known to be all -1: marked for a Nacked Phase2a too, as the vote kernel marks it
    st.row_voted[phys_slot(g, s)] = 1;
    const int tp = b.a.tpos[p];
    if (acc != 0 && tp >= 0 && b.a.tval[tp] == i) {  // the last accepted Phase2a of (acceptor, slot) in the burst
      const int q = s / g.num_leader_groups, nl = b.a.hdr[MAI_NLIST];
      bool covered = false;  // (q is a row of this acceptor's group and so is every q0: the stride needs no test)
      for (int t = mai_after(b, 0, nl, key, i); t < nl && b.lent[t] == key && !covered; ++t)
        covered = b.lq0[t] <= q && q <= b.lq1[t];
      if (!covered) {
        const size_t c = ai_cell(g, s, key);
        st.vote_round[c] = b.a.round[i], st.vote_value[c] = b.a.value[i];
      }
    }
  }
  if (acc - 1 > mv) mv = acc - 1;
  if (p == b.a.n - 1 || b.a.key[p + 1] != key) b.a.fin_slot[key] = mv;
}

// blockIdx.y strides over the list records, blockIdx.x over blocks of 256 owned cells of one record
__global__ void __launch_bounds__(256) k_mai_ranges(const Geom g, const State st, const MenciusAcceptorInbox b) {
  __shared__ int c0[MAI_CHUNK], c1[MAI_CHUNK];
  if (b.a.hdr[AI_OK] == 0) return;
  const int nl = b.a.hdr[MAI_NLIST], A = g.num_groups, L = g.num_leader_groups, tid = threadIdx.x;
  for (int t = blockIdx.y; t < nl; t += gridDim.y) {
    const int q0 = b.lq0[t], q1 = b.lq1[t];
    if (q0 > q1) continue;
    const int ent = b.lent[t], j = b.lidx[t], round = b.lround[t], lg = (ent / g.R) / A;
    const int hi = mai_after(b, t + 1, nl, ent, INT_MAX);  // the end of the entry's run
    const long long cells = ((long long)q1 - q0) / A + 1;
    for (long long base = (long long)blockIdx.x * 256; base < cells; base += (long long)gridDim.x * 256) {
      const bool live = base + tid < cells;
      const int q = live ? (int)(q0 + (base + tid) * A) : -1;
      bool covered = !live;
      for (int u0 = t + 1; u0 < hi; u0 += MAI_CHUNK) {
        const int cn = hi - u0 < MAI_CHUNK ? hi - u0 : MAI_CHUNK;
        __syncthreads();
        if (tid < cn) c0[tid] = b.lq0[u0 + tid], c1[tid] = b.lq1[u0 + tid];
        __syncthreads();
        if (!covered)
          for (int v = 0; v < cn; ++v)
            if (c0[v] <= q && q <= c1[v]) {
              covered = true;
              break;
            }
      }
      if (covered) continue;
      const int s = q * L + lg, ps = phys_slot(g, s);
      const size_t c = (size_t)ps * g.VS + (size_t)(ent % g.R);
      if (mai_find(b.a, (unsigned long long)c) > j) continue;  // a later accepted Phase2a has the cell
      st.vote_round[c] = round, st.vote_value[c] = -1;          // :271-276 State(voteRound = round, voteValue = Noop)
      st.row_voted[ps] = 1;
    }
  }
}

}  // namespace fpx
