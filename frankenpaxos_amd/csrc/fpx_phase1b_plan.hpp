// fpx_phase1b_plan.hpp -- the host half of fpx_leader_phase1b_msgs[_dev] (kernels: fpx_phase1b_msgs.hpp): argument checks,
// the slot arithmetic both halves share, the offsets check that sizes the host form's uploads, and the layout of the
// per-call scratch.  Plain C++ with no HIP call in it, so that it compiles on its own (tests/leader_phase1b_host_main.cpp
// runs it under the host sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define P1M_HD __host__ __device__
#else
#define P1M_HD
#endif

namespace fpx {

constexpr int P1M_KEYS_PER_GROUP = 256;  // one word per possible acceptor bit (FPX_MAX_REPLICAS)
constexpr int P1M_UNIT = 256;            // records of ONE run a wavefront walks (4 steps of 64)
constexpr int P1M_CTL_WORDS = 16;

// RoundSystem.ClassicRoundRobin(n).nextClassicRound(leaderIndex, round) (roundsystem/RoundSystem.scala:66-81): the
// smallest r > round with r % n == leader; a negative round gives `leader` itself.  n = 1 gives round + 1 (0 for a
// negative round), so MultiPaxos is the n = 1 case of every formula below.
P1M_HD inline int64_t p1m_next_classic_round(int64_t n, int64_t leader, int64_t round) {
  if (round < 0) return leader;
  const int64_t m = n * (round / n);
  return m + leader > round ? m + leader : m + n + leader;
}

// the output slots: first, first + L, ... <= max_slot
P1M_HD inline int64_t p1m_first_slot(int64_t L, int64_t leader_group, int64_t chosen_watermark) {
  return p1m_next_classic_round(L, leader_group, chosen_watermark - 1);
}
P1M_HD inline int64_t p1m_count(int64_t L, int64_t first, int64_t max_slot) {
  return max_slot >= first ? (max_slot - first) / L + 1 : 0;
}

// the key of (group_index, acceptor_index) in the first / last tables, -1 = out of range.  grid_cols > 0: the bit
// group_index * grid_cols + acceptor_index of the single grid group (fpx_proxy_phase2b_msgs' convention).
P1M_HD inline int32_t p1m_key(int32_t grid_cols, int32_t num_groups, int32_t total, int32_t group_index, int32_t acceptor_index) {
  if (group_index < 0 || acceptor_index < 0) return -1;
  if (grid_cols > 0) {
    if (acceptor_index >= grid_cols) return -1;
    const int64_t bit = (int64_t)group_index * grid_cols + acceptor_index;
    return bit < total ? (int32_t)bit : -1;
  }
  if (group_index >= num_groups || acceptor_index >= total) return -1;
  return group_index * P1M_KEYS_PER_GROUP + acceptor_index;
}

// rows of the grid that grid_cols cuts the members into (the context's grid_rows when grid_cols is its own)
P1M_HD inline int32_t p1m_grid_rows(int32_t grid_cols, int32_t total) { return (total + grid_cols - 1) / grid_cols; }

// what both entry points refuse at once, before anything is enqueued
inline bool p1m_scalars_ok(int32_t num_groups, int32_t num_leader_groups, int32_t round, int32_t max_round,
                           int32_t chosen_watermark, int32_t leader_group, int32_t recover_slot, uint32_t flags,
                           uint32_t known_flags, int32_t n, int32_t grid_cols, int32_t cap) {
  if (n < 0 || n >= (1 << 30) || cap < 0) return false;
  if (round < 0 || round > max_round || chosen_watermark < 0 || recover_slot < -1) return false;
  if (leader_group < 0 || leader_group >= num_leader_groups) return false;
  if (flags & ~known_flags) return false;
  if (grid_cols < 0 || grid_cols > P1M_KEYS_PER_GROUP) return false;
  if (grid_cols > 0 && (num_groups != 1 || num_leader_groups != 1)) return false;  // the SINGLE grid group
  return true;
}

// offsets[0] == 0 and non-decreasing: the number of records, or -1 with *bad = the lowest offending message index
// (message i is at fault when offsets[i + 1] < offsets[i]; message 0 when offsets[0] != 0)
inline int64_t p1m_check_offsets(int32_t n, const int64_t* offsets, int32_t* bad) {
  *bad = -1;
  if (n == 0) return 0;
  if (offsets[0] != 0) {
    *bad = 0;
    return -1;
  }
  for (int32_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) {
      *bad = i;
      return -1;
    }
  return offsets[n];
}

// The per-call scratch, one allocation: byte offsets of its parts (8-byte words first).
//   ctl    [P1M_CTL_WORDS] u64   the control block the launches hand each other
//   held   [ngroups x 4]   u64   the acceptors used
//   unit0  [n + 1]         i64   exclusive sums of the winning messages' work units
//   first  [keys]          i32   lowest index of a counted message per acceptor (INT_MAX-like = none)
//   last   [keys]          i32   highest such index <= k (-1 = none)
//   win    [n]             i32   the winning messages, in index order
struct P1mLayout {
  size_t ctl, held, unit0, first, last, win, bytes;
  size_t zero_bytes;  // ctl + held: cleared per call
  int32_t keys;
};
inline P1mLayout p1m_layout(int32_t n, int32_t num_groups, int32_t ngroups, int32_t grid_cols) {
  P1mLayout l;
  l.keys = (grid_cols > 0 ? 1 : num_groups) * P1M_KEYS_PER_GROUP;
  l.ctl = 0;
  l.held = l.ctl + (size_t)P1M_CTL_WORDS * 8;
  l.unit0 = l.held + (size_t)ngroups * 4 * 8;
  l.zero_bytes = l.unit0;
  l.first = l.unit0 + ((size_t)n + 1) * 8;
  l.last = l.first + (size_t)l.keys * 4;
  l.win = l.last + (size_t)l.keys * 4;
  l.bytes = l.win + (size_t)n * 4;
  return l;
}

}  // namespace fpx
