// The host half of fpx_leader_phase1b_msgs (csrc/fpx_phase1b_plan.hpp: argument checks, slot arithmetic, the offsets
// check that sizes the uploads, the scratch layout) driven on its own, with no HIP in sight: built with
// -fsanitize=address,undefined and run on the CPU by tests/test_leader_phase1b_cpu.py.  Offsets live in exactly-sized
// heap arrays so that a read past n + 1 entries is caught.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../frankenpaxos_amd/csrc/fpx_phase1b_plan.hpp"

using namespace fpx;

static int failures = 0;
#define EXPECT(c)                                               \
  do {                                                          \
    if (!(c)) {                                                 \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);      \
      ++failures;                                               \
    }                                                           \
  } while (0)

static int64_t offsets_of(const std::vector<int64_t>& v, int32_t* bad) {
  int64_t* heap = (int64_t*)std::malloc(v.size() * sizeof(int64_t));  // exactly n + 1 words
  for (size_t i = 0; i < v.size(); ++i) heap[i] = v[i];
  const int64_t total = p1m_check_offsets((int32_t)v.size() - 1, heap, bad);
  std::free(heap);
  return total;
}

int main() {
  // nextClassicRound (roundsystem/RoundSystem.scala:66-81) against a direct search
  for (int n = 1; n <= 5; ++n)
    for (int leader = 0; leader < n; ++leader)
      for (int r = -3; r < 40; ++r) {
        int64_t want = r < 0 ? leader : r + 1;
        while (r >= 0 && want % n != leader) ++want;
        EXPECT(p1m_next_classic_round(n, leader, r) == want);
      }
  EXPECT(p1m_next_classic_round(4, 1, 2147483646LL) == 2147483649LL);  // no 32-bit wrap at the top of the slot range
  EXPECT(p1m_first_slot(1, 0, 7) == 7 && p1m_first_slot(4, 1, 3) == 5 && p1m_first_slot(4, 1, 0) == 1);
  EXPECT(p1m_count(1, 1, 5) == 5 && p1m_count(4, 5, 17) == 4 && p1m_count(1, 7, -1) == 0 && p1m_count(1, 0, 2147483647LL) == 2147483648LL);

  // keys
  EXPECT(p1m_key(0, 2, 3, 1, 2) == 256 + 2 && p1m_key(0, 2, 3, 2, 0) == -1 && p1m_key(0, 2, 3, 0, 3) == -1);
  EXPECT(p1m_key(0, 2, 3, -1, 0) == -1 && p1m_key(0, 2, 3, 0, -1) == -1);
  EXPECT(p1m_key(2, 1, 4, 1, 1) == 3 && p1m_key(2, 1, 4, 0, 2) == -1 && p1m_key(2, 1, 4, 2, 0) == -1);
  EXPECT(p1m_key(256, 1, 256, 2147483647, 255) == -1);  // the bit is computed in 64 bits
  EXPECT(p1m_grid_rows(2, 4) == 2 && p1m_grid_rows(3, 7) == 3);

  // scalars
  const int32_t MR = 0x3ffffffe;
  EXPECT(p1m_scalars_ok(1, 1, 4, MR, 1, 0, -1, 0, 1, 3, 0, 0));
  EXPECT(!p1m_scalars_ok(1, 1, 4, MR, 1, 0, -1, 0, 1, -1, 0, 0) && !p1m_scalars_ok(1, 1, 4, MR, 1, 0, -1, 0, 1, 1 << 30, 0, 0));
  EXPECT(!p1m_scalars_ok(1, 1, MR + 1, MR, 1, 0, -1, 0, 1, 3, 0, 0) && !p1m_scalars_ok(1, 1, 4, MR, -1, 0, -1, 0, 1, 3, 0, 0));
  EXPECT(!p1m_scalars_ok(1, 4, 4, MR, 1, 4, -1, 0, 1, 3, 0, 0) && p1m_scalars_ok(1, 4, 4, MR, 1, 3, 20, 0, 1, 3, 0, 0));
  EXPECT(!p1m_scalars_ok(1, 1, 4, MR, 1, 0, -2, 0, 1, 3, 0, 0) && !p1m_scalars_ok(1, 1, 4, MR, 1, 0, -1, 2, 1, 3, 0, 0));
  EXPECT(!p1m_scalars_ok(2, 1, 4, MR, 1, 0, -1, 0, 1, 3, 2, 0) && !p1m_scalars_ok(1, 1, 4, MR, 1, 0, -1, 0, 1, 3, 257, 0));
  EXPECT(!p1m_scalars_ok(1, 1, 4, MR, 1, 0, -1, 0, 1, 3, 0, -1));

  // offsets
  int32_t bad = 0;
  EXPECT(offsets_of({0}, &bad) == 0 && bad == -1);
  EXPECT(offsets_of({0, 2, 2, 7}, &bad) == 7 && bad == -1);
  EXPECT(offsets_of({1, 2, 3}, &bad) == -1 && bad == 0);
  EXPECT(offsets_of({0, 5, 4, 9}, &bad) == -1 && bad == 1);
  EXPECT(offsets_of({0, 5, 6, 2}, &bad) == -1 && bad == 2);
  EXPECT(offsets_of({0, 3000000000LL, 6000000000LL}, &bad) == 6000000000LL);  // int64 all the way

  // the scratch layout: parts in order, aligned, not overlapping, the cleared prefix = ctl + held
  for (int n : {0, 1, 5, 4097})
    for (int groups : {1, 3})
      for (int grid : {0, 2}) {
        const P1mLayout l = p1m_layout(n, groups, groups * 2, grid);
        EXPECT(l.keys == (grid ? 1 : groups) * 256);
        EXPECT(l.ctl == 0 && l.held == 16 * 8 && l.unit0 == l.held + (size_t)groups * 2 * 32 && l.zero_bytes == l.unit0);
        EXPECT(l.first == l.unit0 + ((size_t)n + 1) * 8 && l.last == l.first + (size_t)l.keys * 4);
        EXPECT(l.win == l.last + (size_t)l.keys * 4 && l.bytes == l.win + (size_t)n * 4);
        EXPECT(l.unit0 % 8 == 0 && l.first % 4 == 0 && l.win % 4 == 0);
      }
  if (failures == 0) std::puts("leader_phase1b host half ok");
  return failures != 0;
}
