// fpx_mencius_msgs.hpp -- mencius.ProxyLeader.handlePhase2b (mencius/ProxyLeader.scala:305-353) and handlePhase2bNoopRange
// (:355-411) for a tick of PER-ACCEPTOR messages as reference Mencius acceptors send them: Phase2b(acceptor_group_index,
// acceptor_index, slot, round) and Phase2bNoopRange(acceptor_group_index, acceptor_index, slot_start, slot_end, round),
// interleaved in delivery order, duplicates and several rounds of one key included.  The same three passes as
// fpx_tally_msgs.hpp, thread per message, branching on the message's kind -- a mixed burst costs the launches a burst of
// Phase2b's costs there, and nothing is read by the host in between:
//
//   k_mm_claim   a Phase2b: msgs_claim_one (fpx_tally_msgs.hpp) with group_index ignored -- the bit is acceptor_index, the
//                acceptor group follows from the slot.  A Phase2bNoopRange: checks the fields, finds the range's entry in
//                the RangeTable with k_ranges_open's own probe in lookup mode (ranges_open_core, which also swallows a
//                length-1 key held by a single-slot tally, :370-385), and bids for a Pending entry with
//                atomicMin(claim[entry], i): the FIRST message of a range in the burst is its owner.  A Done entry is
//                ignored here already (:370-376) -- nothing of it is read or written again in this call.
//   k_mm_gather  a Phase2b: atomicOr of its bit into the owner's row (msgs_gather_dst).  A range message: atomicOr of its
//                bit straight into rt.bits[entry][group * 4 + word] -- what ranges_tally_one's bits |= in & member does
//                with a folded row (:389-390), so the range half needs no per-message scratch rows.  Neighbouring lanes
//                with one destination word merge before the atomic for both kinds (msgs_or_merged): n votes of ONE range
//                in neighbouring lanes are n / 64 atomics, not n, where a group's acceptors share a word (R <= 64).
//   k_mm_tally   a Phase2b: msgs_tally_one.  The owner of a range entry reads the entry's bits, and when every acceptor
//                group has f + 1 of them (:389-391) sets RT_DONE and reports newly chosen; it hands the claim word back
//                (INT_MAX), also when the call applies nothing.  Every other message reports "nothing chosen".
//   k_msgs_tail  (fpx_tally_msgs.hpp, as it is) the lowest bad / unknown message index of either kind -> the status
//
// The claim word is a NEW [cap] array (fpx_ctx::mm_claim, INT_MAX between calls like `owner` of fpx_tally_msgs.hpp), not
// RangeTable.owner: that word is written by the open pass under the launch's stamp, copied by k_ranges_rehash and
// initialised to 0x7f7f7f7f by clear_range_table -- handing it back as INT_MAX would change what those read, and a claim
// left in it would be a message index from another launch.  One array serves both table buffers (equal capacities; no
// claim outlives a call, and fpx_proxy_forget switches buffers between calls only).
//
// Only integer atomics (min / or / max): the result does not depend on the order the hardware runs the threads in.  No
// message walks a list: one table probe (as long as k_ranges_open's) and O(1) work per message whatever the burst.
//
// Bytes and atomics of the range half, per message: 24 B read (six int32 fields), 4 B of entry written and read twice,
// 9 B of outputs; one probe (16 B key words, mostly the home bucket); one atomicMin on a 4-byte claim word; at most one
// atomicOr on an 8-byte word of the entry's bits (one per run of neighbouring lanes with the same word).
#pragma once
#include "fpx_ranges.hpp"
#include "fpx_tally_msgs.hpp"

namespace fpx {

struct MenciusMsgs {
  MsgBatch m;              // the Phase2b half and the burst's common arrays (grid_cols = 0, group = null)
  const int32_t* group;    // acceptor_group_index of a range message
  const int32_t* slot_end; // null: the burst has no range message
  int32_t range_kind;      // FPX_WIRE_PHASE2B_NOOP_RANGE
  int32_t* claim;          // [rt.cap]
  int32_t quorum;          // f + 1
  uint32_t run_id;         // a stamp no table entry carries: the probe is a pure lookup
};

// entry[i]: >= 0 a Phase2b's tally entry, -1 nothing, <= -2 a range message's Pending table entry p as -2 - p
__global__ void __launch_bounds__(256) k_mm_claim(const Geom g, const State st, const RangeTable rt, const MenciusMsgs b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m.n) return;
  int e = -1;
  if (st.status[ST_ABORT] == 0) {
    const int kind = b.m.kind ? b.m.kind[i] : b.m.phase2b;
    if (kind == b.m.phase2b) {
      e = msgs_claim_one(g, st, b.m, i);
    } else if (kind == b.range_kind) {
      const int a = b.m.acceptor[i], s = b.m.slot[i], rnd = b.m.round[i];
      const int grp = b.group ? b.group[i] : 0;
      const int end = b.slot_end ? b.slot_end[i] : -1;  // (no slot_end array and a range message: refused)
      if (a < 0 || a >= 256 || grp < 0 || grp >= g.num_groups || s < 0 || end < s || end > g.S || rnd < 0 || rnd > MAX_ROUND) {
        atomicMax(&st.status[ST_MSG_BAD], 0x7fffffff - i);
      } else if ((g.member[a >> 6] >> (a & 63)) & 1ull) {  // a bit outside the member set contributes nothing
        RangeBatch rb;
        rb.n = b.m.n, rb.run_id = b.run_id;
        bool inserted, shared;
        const int p = ranges_open_core(g, st, rt, rb, 1, i, s, end, rnd, -1, &inserted, &shared);
        if (p == -1) {
          atomicMax(&st.status[ST_MSG_UNKNOWN], 0x7fffffff - i);  // :361-368; the message is dropped
        } else if (p >= 0 && (uint32_t)(rt.key[(size_t)p * 2 + 1] & 3u) == RT_PENDING) {  // Done: ignored (:370-376)
          atomicMin(&b.claim[p], i);
          e = -2 - p;
        }
      }
    }
  }
  b.m.entry[i] = e;
}

__global__ void __launch_bounds__(256) k_mm_gather(const Geom g, const State st, const RangeTable rt, const MenciusMsgs b) {
  if (st.status[ST_ABORT] != 0 || st.status[ST_MSG_BAD] != 0) return;  // nothing is applied
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = i < b.m.n ? b.m.entry[i] : -1;
  unsigned long long v = 0;
  const long long dst = msgs_gather_dst(b.m, i, e, &v);
  long long rdst = -1;  // the word of rt.bits a range message's bit goes to
  unsigned long long rv = 0;
  if (e <= -2) {
    const int a = b.m.acceptor[i];
    rdst = ((long long)(-2 - e) * g.num_groups + (b.group ? b.group[i] : 0)) * 4 + (a >> 6);
    rv = 1ull << (a & 63);
  }
  // (wavefront-uniform: a wavefront without a message of one kind skips that kind's merge -- a burst of Phase2b's alone
  // does k_msgs_gather's work and no more)
  if (__ballot(dst >= 0) != 0) msgs_or_merged(b.m.row_bits, dst, v);
  if (__ballot(rdst >= 0) != 0) msgs_or_merged(reinterpret_cast<unsigned long long*>(rt.bits), rdst, rv);
}

__global__ void __launch_bounds__(256) k_mm_tally(const Geom g, const State st, const RangeTable rt, const MenciusMsgs b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m.n) return;
  const bool apply = st.status[ST_ABORT] == 0 && st.status[ST_MSG_BAD] == 0;
  const int e = b.m.entry[i];
  uint8_t ch = 0;
  int cr = -1, cv = -1;
  if (e <= -2) {
    const int p = -2 - e;
    if (b.claim[p] == i) {
      if (apply) {
        const uint64_t* bits = rt.bits + (size_t)p * g.num_groups * 4;
        bool all = true;
        for (int ag = 0; ag < g.num_groups; ++ag) {
          int c = 0;
#pragma unroll
          for (int w = 0; w < 4; ++w) c += __popcll(bits[ag * 4 + w]);
          all = all && c >= b.quorum;  // :391
        }
        if (all) {
          uint64_t* k1p = &rt.key[(size_t)p * 2 + 1];
          *k1p = (*k1p & ~3ull) | RT_DONE;  // :410 ; ChosenNoopRange(start, end) :395-407
          ch = 1, cr = b.m.round[i];
        }
      }
      b.claim[p] = INT_MAX;
    }
  } else {
    msgs_tally_one(g, st, b.m, i, e, apply, &ch, &cr, &cv);
  }
  if (b.m.chosen) b.m.chosen[i] = ch;
  if (b.m.chosen_round) b.m.chosen_round[i] = cr;
  if (b.m.chosen_value) b.m.chosen_value[i] = cv;
}

// ---- the newly chosen records of a Mencius tick, compacted in message order (fpx_mencius_phase2b_tick) --------------
// k_msgs_count and k_msgs_scan as they are; the emit writes (kind, slot or slot_start, slot_end or -1, round, value id
// or -1) of the k-th newly chosen message.
struct MenciusEmit {
  MsgCompact c;
  const int32_t* kind;      // null: every message is a Phase2b
  const int32_t* slot_end;
  int32_t phase2b, range_kind;
  int32_t *out_kind, *out_slot_end;
};

__global__ void __launch_bounds__(256) k_mm_emit(const State st, const MenciusEmit m) {
  const MsgCompact& c = m.c;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool f = st.status[ST_ABORT] == 0 && i < c.n && c.chosen[i] != 0;
  __shared__ int wsum[4];
  int total;
  const int at = c.blk[blockIdx.x] + block_rank(f, &total, wsum);
  if (f && at < c.cap) {
    const int kind = m.kind ? m.kind[i] : m.phase2b;
    m.out_kind[at] = kind;
    c.out_slot[at] = c.slot[i];
    m.out_slot_end[at] = kind == m.range_kind ? m.slot_end[i] : -1;
    c.out_round[at] = c.chosen_round[i];
    c.out_value[at] = c.chosen_value[i];
  }
}

}  // namespace fpx
