// host_call_layout_main.cpp -- TEST INFRASTRUCTURE ONLY: lays out array lists of host-pointer calls with lay_stage
// (frankenpaxos_amd/csrc/fpx_host_call.hpp: host code, no HIP) exactly as host_call (fpx_host.hpp) does for fpx_api.hip
// and fpx_epaxos.hip, and checks what the driver relies on: every offset is STAGE_ALIGN-aligned, the arrays are disjoint
// and in list order, the total is the last end, an absent input takes no space, the held offsets are 8-byte aligned and
// disjoint, a held_first finds its length word, and the fill runs cover exactly the spans of the filled arrays, neighbours
// of one value merged.  Every span, of the device arrays and of the held ones, is then written from end to end into heap
// blocks of exactly the computed totals, so that built with -fsanitize=address,undefined
// (tests/test_host_call_layout_cpu.py) a layout that leaves its buffer is an error of its own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../frankenpaxos_amd/csrc/fpx_host_call.hpp"

using namespace fpx;

namespace {

int failures = 0;
#define EXPECT(cond, ...)                                   \
  do {                                                      \
    if (!(cond)) {                                          \
      std::printf("FAIL %s: ", what.c_str());               \
      std::printf(__VA_ARGS__);                             \
      std::printf("\n");                                    \
      ++failures;                                           \
    }                                                       \
  } while (0)

const size_t SIZES[6] = {0, 1, 255, 256, 257, 262969};
const int FILLS[6] = {NO_FILL, 0, 0, 0xFF, NO_FILL, 0};

void check(const std::string& what, const std::vector<Staged>& a) {
  const size_t n = a.size();
  const StageLayout l = lay_stage(a.data(), n);
  EXPECT(l.at.size() == n && l.held_at.size() == n && l.length_at.size() == n, "the layout has not one entry per array");
  // the device arrays: aligned, in list order, disjoint; an array of no bytes (an absent input) takes no space
  size_t end = 0, held_end = 0;
  for (size_t i = 0; i < n; ++i) {
    EXPECT(l.at[i] % STAGE_ALIGN == 0, "array %zu at %zu is not aligned", i, l.at[i]);
    EXPECT(l.at[i] >= end, "array %zu at %zu starts before the end %zu of the one before", i, l.at[i], end);
    EXPECT(l.at[i] < end + STAGE_ALIGN, "array %zu at %zu leaves a gap behind %zu", i, l.at[i], end);
    if (a[i].bytes == 0) EXPECT(i + 1 == n ? l.total == l.at[i] : l.at[i + 1] == l.at[i], "array %zu of no bytes takes space", i);
    end = l.at[i] + a[i].bytes;
    if (a[i].hold) {
      EXPECT(l.held_at[i] % 8 == 0, "held array %zu at %zu is not 8-byte aligned", i, l.held_at[i]);
      EXPECT(l.held_at[i] >= held_end, "held array %zu at %zu starts before the end %zu of the one before", i, l.held_at[i], held_end);
      held_end = l.held_at[i] + a[i].bytes;
    }
    // a held_first finds the held word that is its length, wherever in the list that lies
    size_t want = StageLayout::NONE;
    for (size_t j = 0; a[i].length && j < n; ++j)
      if (a[j].slot == a[i].length) want = l.held_at[j];
    EXPECT(!a[i].length || want != StageLayout::NONE, "the test's list has no length word for array %zu", i);
    EXPECT(l.length_at[i] == want, "array %zu: length word at %zu, expected %zu", i, l.length_at[i], want);
  }
  EXPECT(l.total == ((end + STAGE_ALIGN - 1) & ~(STAGE_ALIGN - 1)), "total %zu is not the last end %zu", l.total, end);
  EXPECT(l.held_total == ((held_end + 7) & ~(size_t)7), "held total %zu is not the last held end %zu", l.held_total, held_end);
  // the fill runs against a map of the buffer in units of STAGE_ALIGN: exactly the filled arrays' spans, each with its
  // value; no run is empty, no two overlap, and two runs that touch differ in value
  const size_t units = l.total / STAGE_ALIGN;
  std::vector<int> want(units, NO_FILL), got(units, NO_FILL);
  for (size_t i = 0; i < n; ++i)
    for (size_t u = l.at[i] / STAGE_ALIGN; u < (l.at[i] + a[i].span()) / STAGE_ALIGN; ++u) want[u] = a[i].fill;
  for (size_t k = 0; k < l.fills.size(); ++k) {
    const StageLayout::Fill& f = l.fills[k];
    EXPECT(f.bytes != 0 && f.at % STAGE_ALIGN == 0 && f.bytes % STAGE_ALIGN == 0 && f.at + f.bytes <= l.total && f.value != NO_FILL,
           "fill run %zu (%zu + %zu, value %d) is empty, unaligned, outside the buffer or of no value", k, f.at, f.bytes, f.value);
    if (f.at + f.bytes > l.total) continue;
    if (k) EXPECT(l.fills[k - 1].at + l.fills[k - 1].bytes < f.at || (l.fills[k - 1].at + l.fills[k - 1].bytes == f.at && l.fills[k - 1].value != f.value),
                  "fill run %zu overlaps the one before, or was not merged with it", k);
    for (size_t u = f.at / STAGE_ALIGN; u < (f.at + f.bytes) / STAGE_ALIGN; ++u) got[u] = f.value;
  }
  EXPECT(want == got, "the fill runs do not cover exactly the filled arrays");
  // what the driver does with the layout, into blocks of exactly the totals: the slots are pointed at the arrays, the
  // fills are written, then every array and every held array from end to end
  char* dev = static_cast<char*>(std::malloc(l.total));
  char* host = static_cast<char*>(std::malloc(l.held_total));
  if ((!dev && l.total) || (!host && l.held_total)) std::abort();
  for (const StageLayout::Fill& f : l.fills)
    if (f.at + f.bytes <= l.total) std::memset(dev + f.at, f.value, f.bytes);
  for (size_t i = 0; i < n; ++i) {
    if (l.at[i] + a[i].bytes > l.total || (a[i].hold && l.held_at[i] + a[i].bytes > l.held_total)) {
      EXPECT(false, "array %zu leaves its buffer", i);
      continue;
    }
    a[i].place(a[i].slot, dev + l.at[i]);
    char* p;
    std::memcpy(&p, a[i].slot, sizeof(p));  // (the slot is a T* of some T)
    EXPECT(p == dev + l.at[i] || (p == nullptr && a[i].bytes == 0), "array %zu: the slot does not point at the array", i);
    if (a[i].bytes) std::memset(dev + l.at[i], (int)(i % 200) + 1, a[i].bytes);
    if (a[i].hold && a[i].bytes) std::memset(host + l.held_at[i], (int)(i % 200) + 1, a[i].bytes);
  }
  for (size_t i = 0; i < n; ++i)  // (no array was written over by a later one)
    for (size_t k = 0; k < a[i].bytes; k += 97) {
      const char v = (char)((i % 200) + 1);
      if (dev[l.at[i] + k] != v || (a[i].hold && host[l.held_at[i] + k] != v)) {
        EXPECT(false, "array %zu was written over", i);
        break;
      }
    }
  std::free(dev), std::free(host);
  if (a.empty()) EXPECT(l.total == 0 && l.held_total == 0 && l.fills.empty(), "an empty list has a size");
  std::printf("ok %s arrays=%zu total=%zu held=%zu fills=%zu\n", what.c_str(), n, l.total, l.held_total, l.fills.size());
}

}  // namespace

int main() {
  uint8_t* s8[16];
  int32_t* s32[16];
  int32_t dst[4];  // (never written: the layout only looks at whether a destination is there)
  uint8_t src[1], sink[1];
  check("empty", {});
  // every size under every fill of the sequence NO_FILL, 0, 0, 0xFF, NO_FILL, 0
  for (size_t shift = 0; shift < 6; ++shift) {
    std::vector<Staged> a;
    for (size_t i = 0; i < 6; ++i) a.push_back(scratch(s8[i], SIZES[(i + shift) % 6], FILLS[i]));
    check("sizes x fills, sizes shifted by " + std::to_string(shift), a);
  }
  // an absent input first, in the middle, last -- between filled neighbours of one value, which stay one run
  for (size_t pos = 0; pos < 3; ++pos) {
    std::vector<Staged> a;
    for (size_t i = 0; i < 6; ++i) {
      if ((pos == 0 && i == 0) || (pos == 1 && i == 3)) a.push_back(opt_in(s8[8 + pos], nullptr, 257));
      a.push_back(i % 2 ? out(s8[i], dst, SIZES[5 - i], 0) : in(s8[i], src, SIZES[5 - i]));
    }
    if (pos == 1) a.push_back(scratch(s8[6], 257, 0)), a.insert(a.begin() + 3, scratch(s8[7], 1, 0));  // (0-fills around the absent one)
    if (pos == 2) a.push_back(opt_in(s8[10], nullptr, 1));
    check(std::string("absent input ") + (pos == 0 ? "first" : pos == 1 ? "in the middle" : "last"), a);
    if (s8[8 + pos] != nullptr) std::printf("FAIL absent input %zu: its slot is not null\n", pos), ++failures;
  }
  // held arrays among plain ones; a held_first whose length word comes after it in the list; held arrays of every size
  for (size_t shift = 0; shift < 6; ++shift) {
    std::vector<Staged> a;
    a.push_back(in(s8[0], src, SIZES[shift]));
    a.push_back(held(s8[1], sink, SIZES[(shift + 1) % 6]));
    a.push_back(held_first(s32[0], dst, (SIZES[(shift + 2) % 6] + 3) / 4, s32[1]));
    a.push_back(out(s8[2], dst, SIZES[(shift + 3) % 6], 0xFF));
    a.push_back(held(s8[3], static_cast<uint8_t*>(nullptr), SIZES[(shift + 4) % 6]));  // (held, and the caller does not want it)
    a.push_back(scratch(s8[4], SIZES[(shift + 5) % 6], 0));
    a.push_back(held(s32[1], dst, 1));  // the length word of the held_first above
    a.push_back(held(s32[2], dst, 3));
    check("held among plain, sizes shifted by " + std::to_string(shift), a);
  }
  if (failures) return std::printf("%d failures\n", failures), 1;
  std::printf("all layouts ok\n");
  return 0;
}
