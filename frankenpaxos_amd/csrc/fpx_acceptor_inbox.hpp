// fpx_acceptor_inbox.hpp -- multipaxos.Acceptor's inbox for a BURST of per-acceptor messages in delivery order:
// handlePhase1a / handlePhase2a / handleMaxSlotRequest / handleBatchMaxSlotRequest (multipaxos/Acceptor.scala:148-254),
// the kinds interleaved and addressed to any of the context's acceptors, exactly as if every acceptor had handled its
// messages one by one -- without the host reading anything between the passes.  This is how a reference ProxyLeader
// sends Phase2as (one message per acceptor address, to f + 1 of them, ProxyLeader.scala:190-215): every slot comes f + 1
// times, which the run contract of k_phase2 (slots pairwise distinct, one round per group) does not allow in one launch.
//
// For acceptor e (entry = group * R + acceptor) with its messages in index order, every accepted Phase1a / Phase2a has a
// round at least the acceptor's, and a Nacked one a smaller one, so
//
//   round met by message i   = max(promised[e], rounds of e's earlier Phase1a / Phase2a messages)       (exclusive)
//   accepted(i)              = round[i] >= that                                                         (:155, :192)
//   maxVotedSlot met by i    = max(max_voted[e], slots of e's earlier ACCEPTED Phase2as)                (exclusive)
//   cell (slot, e)           = (round, value) of the LAST accepted Phase2a of (e, slot)
//
// Both running maxima are SEGMENTED scans over the messages brought together per acceptor.  With the messages sorted by
// entry the segments are runs of one key, and a plain (unsegmented) running maximum of the 64-bit words
// (entry << 32 | value + 1) is the segmented one: the keys do not decrease along the sorted order, so the maximum before
// position p carries p's own entry in its high half iff the segment has an earlier message, and then its low half is
// the segment's running maximum.  A burst that all goes to ONE acceptor is one segment over every tile and needs nothing
// special.
//
//   k_ai_keys     thread / message: checks the message (kind, index, slot, round, the slot's group) and writes the sort
//                 key: its entry, or E for a message that is skipped
//   k_sort_count, k_sort_scan, k_sort_scatter   (fpx_burst_sort.hpp) a stable LSD radix sort by that key over the bits of
//                 E: rank by position, never an atomic cursor
//   k_ai_tilemax<0>, k_ai_tilescan   workgroup / tile of AI_TILE positions: the tile's largest round word; then one
//                 workgroup, AI_SCAN_THREADS tiles per step with a carry: the exclusive running maximum over the tiles
//                 (the shape of k_ri_tilemax / k_ri_tilescan of fpx_replica_inbox.hpp, on 64-bit words)
//   k_ai_accept   workgroup / tile: the round every message meets, accept or Nack, the replies of Phase1a / Phase2a; an
//                 accepted Phase2a bids for its cell in the claim table with atomicMax of its index; the last message of
//                 a segment leaves the acceptor's new round in fin_round
//   k_ai_tilemax<1>, k_ai_tilescan   the same scan over the accepted slots
//   k_ai_reads    workgroup / tile: maxVotedSlot as every message meets it, the replies of the reads; the accepted
//                 Phase2a whose index the cell's claim settled on writes the cell; row_voted; fin_slot
//   k_ai_finish   thread / position: commits promised and max_voted, hands the claim words back, and turns a bad message
//                 into the context's status
//
// The claim table is an open-addressed table of 64-bit cell numbers sized by the burst (the next power of two at or above
// 2 n; an [S][R] array of claim words would be 1 GiB at the headline shape).  WHERE a cell's word lands depends on the
// order the threads insert in; what the word ends up holding -- the largest index -- does not, and nothing else is read
// from it.  Integer atomics only (CAS, max): no output depends on the order the hardware runs the threads in.
#pragma once
#include <limits.h>

#include "../../include/fpx_wire.h"
#include "fpx_burst_sort.hpp"
#include "fpx_tally_msgs.hpp"

namespace fpx {

constexpr int AI_TILE = BURST_TILE;    // sorted positions per tile (one per thread)
constexpr int AI_SCAN_THREADS = 1024;  // tiles per step of k_ai_tilescan
constexpr unsigned long long AI_EMPTY = ~0ull;

// words of AcceptorInbox::hdr (AI_M is the sort's length word)
enum { AI_OK = 0, AI_M = 2, AI_HDR_WORDS = BURST_HDR_WORDS };

struct AcceptorInbox {
  int32_t n, E;  // E = ngroups * R: the number of entries, and the sort key of a skipped message
  int32_t grid_cols;
  const int32_t *kind, *group, *acceptor, *slot, *round, *value;  // group may be null (= 0)
  int32_t* hdr;                  // [AI_HDR_WORDS]
  const int32_t* key;            // [n]  the sorted keys
  const int32_t* perm;           // [n]  the message at every sorted position
  long long* tile;               // [ceil(n / AI_TILE)]  the tiles' maxima, then their exclusive running maxima
  int32_t* accslot;              // [n]  by position: slot + 1 of an accepted Phase2a, else 0
  int32_t* tpos;                 // [n]  by position: the claim word of an accepted Phase2a, else -1
  int32_t *fin_round, *fin_slot; // [E]  the new round / maxVotedSlot of every entry with a message in the burst
  unsigned long long* tkey;      // [tmask + 1]  AI_EMPTY between calls
  int32_t* tval;                 // [tmask + 1]  -1 between calls
  uint32_t tmask;
  int32_t *reply_kind, *reply_value;  // may be null
};

__device__ __forceinline__ bool ai_moves_round(int kind) { return kind == FPX_WIRE_PHASE2A || kind == FPX_WIRE_PHASE1A; }
__device__ __forceinline__ bool ai_is_read(int kind) {
  return kind == FPX_WIRE_MAX_SLOT_REQUEST || kind == FPX_WIRE_BATCH_MAX_SLOT_REQUEST;
}

// the entry message i was delivered to, -1 = no acceptor of this context (the convention of msgs_claim_one)
__device__ __forceinline__ int ai_entry(const Geom& g, const AcceptorInbox& b, int i) {
  const int a = b.acceptor[i], gi = b.group ? b.group[i] : 0;
  if (a < 0 || gi < 0) return -1;
  if (b.grid_cols > 0) {  // a grid: row = groupIndex, column = acceptorIndex, of the context's one acceptor group
    if (a >= b.grid_cols) return -1;
    const long long r = (long long)gi * b.grid_cols + a;
    return r < g.R ? (int)r : -1;
  }
  return a < g.R && gi < g.ngroups ? gi * g.R + a : -1;
}

__global__ void __launch_bounds__(256) k_ai_keys(const Geom g, const State st, const AcceptorInbox b, int32_t* key0,
                                                 int32_t* val0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) b.hdr[AI_M] = b.n;
  if (i >= b.n) return;
  int key = b.E;
  const int k = b.kind[i];
  if (st.status[ST_ABORT] == 0 && k != FPX_WIRE_OTHER) {
    bool bad = !ai_moves_round(k) && !ai_is_read(k);
    int e = -1;
    if (!bad) e = ai_entry(g, b, i), bad = e < 0;
    if (!bad && ai_moves_round(k)) {
      const int r = b.round[i];
      bad = r < 0 || r > MAX_ROUND;
    }
    if (!bad && k == FPX_WIRE_PHASE2A) {
      // (the cell of a slot belongs to the slot's acceptor group: a Phase2a delivered to another group's acceptor has none)
      const int s = b.slot[i];
      bad = s < 0 || s >= g.S || group_of_slot(g, s) != e / g.R;
    }
    if (bad) atomicMax(&st.status[ST_MSG_BAD], 0x7fffffff - i);
    else key = e;
  }
  key0[i] = key, val0[i] = i;
}

// what position p contributes to the running maximum: MODE 0 the round of a Phase1a / Phase2a, MODE 1 the slot of an
// accepted Phase2a, each + 1 under the position's key (0 = nothing); MODE 2 is MODE 0 for a Mencius acceptor, whose
// Phase2aNoopRanges move the round too (fpx_mencius_acceptor_inbox.hpp)
template <int MODE>
__device__ __forceinline__ long long ai_word(const AcceptorInbox& b, int p) {
  if (p >= b.n) return -1;
  int v;
  if (MODE == 0 || MODE == 2) {
    const int i = b.perm[p], k = b.kind[i];
    v = ai_moves_round(k) || (MODE == 2 && k == FPX_WIRE_PHASE2A_NOOP_RANGE) ? b.round[i] + 1 : 0;
  } else {
    v = b.accslot[p];
  }
  return ((long long)b.key[p] << 32) | (long long)(uint32_t)v;
}

template <int MODE>
__global__ void __launch_bounds__(256) k_ai_tilemax(const AcceptorInbox b) {
  __shared__ long long w[4];
  const int ntiles = (b.n + AI_TILE - 1) / AI_TILE;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long m = block_reduce<ScanMax, 256>(ai_word<MODE>(b, tile * AI_TILE + (int)threadIdx.x), w);
    if (threadIdx.x == 0) b.tile[tile] = m;
  }
}

// the exclusive running maximum over the tiles, one workgroup; also freezes "the burst is applied" for the kernels behind
__global__ void __launch_bounds__(AI_SCAN_THREADS) k_ai_tilescan(const State st, const AcceptorInbox b) {
  __shared__ long long lds[SCAN_ARRAY_LDS(AI_SCAN_THREADS)];
  if (threadIdx.x == 0) b.hdr[AI_OK] = st.status[ST_ABORT] == 0 && st.status[ST_MSG_BAD] == 0 ? 1 : 0;
  (void)scan_array_excl<ScanMax, AI_SCAN_THREADS, 1>(b.tile, (b.n + AI_TILE - 1) / AI_TILE, lds);
}

// the running maximum of the segment of `key` before this position, started at `start` (x = the largest word before the
// position: block_excl_scan over the tile, from the tile's carry)
__device__ __forceinline__ int ai_running(long long x, int key, int start) {
  if (x < 0 || (int)(x >> 32) != key) return start;
  const int v = (int)(x & 0xffffffffll) - 1;
  return v > start ? v : start;
}

// the claim word of a cell: found or taken by CAS, bid for with atomicMax of the message index.  At most n cells are
// inserted into a table of at least 2 n words, so the probe ends
__device__ __forceinline__ int ai_claim(const AcceptorInbox& b, unsigned long long cell, int i) {
  unsigned long long z = cell * 0x9E3779B97F4A7C15ull;
  uint32_t h = (uint32_t)(z >> 32) & b.tmask;
  for (uint32_t probes = 0; probes <= b.tmask; ++probes) {
    const unsigned long long old = atomicCAS(&b.tkey[h], AI_EMPTY, cell);
    if (old == AI_EMPTY || old == cell) {
      atomicMax(&b.tval[h], i);
      return (int)h;
    }
    h = (h + 1) & b.tmask;
  }
  return -1;
}

__device__ __forceinline__ size_t ai_cell(const Geom& g, int slot, int key) {
  return (size_t)phys_slot(g, slot) * g.VS + (size_t)(key % g.R);
}

__global__ void __launch_bounds__(256) k_ai_accept(const Geom g, const State st, const AcceptorInbox b) {
  __shared__ long long wtot[4];
  const int p = blockIdx.x * AI_TILE + threadIdx.x;
  const long long x = block_excl_scan<ScanMax, 256>(ai_word<0>(b, p), b.tile[blockIdx.x], wtot);
  if (p >= b.n) return;
  const int key = b.key[p];
  int acc = 0, tp = -1;
  if (b.hdr[AI_OK] != 0) {
    const int i = b.perm[p];
    int rk = 0, rv = -1;
    if (key < b.E) {
      const int k = b.kind[i];
      int run = ai_running(x, key, st.promised[key]);
      if (ai_moves_round(k)) {
        const int r = b.round[i];
        if (r < run) {  // :155, :192
          rk = FPX_WIRE_NACK, rv = run;
        } else {
          rk = k == FPX_WIRE_PHASE2A ? FPX_WIRE_PHASE2B : FPX_WIRE_PHASE1B, rv = r, run = r;
          if (k == FPX_WIRE_PHASE2A) {
            const int s = b.slot[i];
            acc = s + 1, tp = ai_claim(b, (unsigned long long)ai_cell(g, s, key), i);
          }
        }
      }
      if (p == b.n - 1 || b.key[p + 1] != key) b.fin_round[key] = run;
    }
    // (a read's reply comes from k_ai_reads)
    if (key >= b.E || ai_moves_round(b.kind[i])) {
      if (b.reply_kind) b.reply_kind[i] = rk;
      if (b.reply_value) b.reply_value[i] = rv;
    }
  }
  b.accslot[p] = acc, b.tpos[p] = tp;
}

__global__ void __launch_bounds__(256) k_ai_reads(const Geom g, const State st, const AcceptorInbox b) {
  __shared__ long long wtot[4];
  const int p = blockIdx.x * AI_TILE + threadIdx.x;
  const long long x = block_excl_scan<ScanMax, 256>(ai_word<1>(b, p), b.tile[blockIdx.x], wtot);
  if (p >= b.n || b.hdr[AI_OK] == 0) return;
  const int key = b.key[p];
  if (key >= b.E) return;
  const int i = b.perm[p], k = b.kind[i], acc = b.accslot[p];
  int mv = ai_running(x, key, st.max_voted[key]);
  if (ai_is_read(k)) {  // :222-254
    if (b.reply_kind) b.reply_kind[i] = FPX_WIRE_MAX_SLOT_REQUEST;
    if (b.reply_value) b.reply_value[i] = mv;
  }
  if (k == FPX_WIRE_PHASE2A) {
    const int s = b.slot[i];
    // the row is no longer known to be all -1: marked for a Nacked Phase2a too, as the vote kernel marks it
    st.row_voted[phys_slot(g, s)] = 1;
    const int tp = b.tpos[p];
    if (acc != 0 && tp >= 0 && b.tval[tp] == i) {  // the last accepted Phase2a of (acceptor, slot) in the burst: :205-208
      const size_t c = ai_cell(g, s, key);
      st.vote_round[c] = b.round[i], st.vote_value[c] = b.value[i];
    }
    if (acc - 1 > mv) mv = acc - 1;  // :209
  }
  if (p == b.n - 1 || b.key[p + 1] != key) b.fin_slot[key] = mv;
}

__global__ void __launch_bounds__(256) k_ai_finish(const State st, const AcceptorInbox b) {
  const int p = blockIdx.x * AI_TILE + threadIdx.x;
  if (p < b.n) {
    const int tp = b.tpos[p];
    if (tp >= 0) b.tkey[tp] = AI_EMPTY, b.tval[tp] = -1;  // (every bidder of the word writes the same)
    const int key = b.key[p];
    if (b.hdr[AI_OK] != 0 && key < b.E && (p == b.n - 1 || b.key[p + 1] != key))
      st.promised[key] = b.fin_round[key], st.max_voted[key] = b.fin_slot[key];
  }
  if (p != 0) return;
  // (no other thread of this grid reads the status words)
  const int32_t bad = st.status[ST_MSG_BAD];
  st.status[ST_MSG_BAD] = 0;
  if (bad != 0) {
    const int i = 0x7fffffff - bad;
    if (i >= 0 && i < b.n) report_abort(st, 1 /*FPX_EINVAL*/, i, b.slot[i], b.round[i]);
  }
}

}  // namespace fpx
