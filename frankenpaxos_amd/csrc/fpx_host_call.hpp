// fpx_host_call.hpp -- the arrays of a host-pointer call and where they lie: what an entry point lists for the driver in
// fpx_host.hpp (host_call).  Host code with no HIP in it, so the layout is tested in a program of its own
// (tests/host_call_layout_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

namespace fpx {

// An array of a host call, carved out of the context's staging buffer: uploaded from `src` when that is not NULL,
// downloaded to `dst` when that is not NULL, and starting as `fill` bytes (0 or 0xFF; NO_FILL: whatever the buffer held).
// It is staged either way: an input or output the caller leaves out is device scratch.  (But opt_in / absent.)
constexpr int NO_FILL = -1;
constexpr size_t STAGE_ALIGN = 256;  // (what hipMalloc guarantees)
struct Staged {
  void* slot;                   // the caller's T*, pointed at the array
  void (*place)(void*, char*);
  const void* src;
  void* dst;
  size_t bytes;
  int fill;
  bool hold = false;                // held(): dst gets the array only once the call's status is known
  const void* length = nullptr;     // held_first(): the slot of the held word that counts the elements dst gets
  size_t span() const { return (bytes + STAGE_ALIGN - 1) & ~(STAGE_ALIGN - 1); }
  size_t host_span() const { return hold ? (bytes + 7) & ~(size_t)7 : 0; }
};
template <typename T>
Staged arr(T*& d, const void* src, void* dst, size_t count, int fill) {
  return {&d, [](void* s, char* p) { *static_cast<T**>(s) = reinterpret_cast<T*>(p); }, src, dst, count * sizeof(T), fill};
}
template <typename T>
Staged in(T*& d, const void* src, size_t count) {
  return arr(d, src, nullptr, count, NO_FILL);
}
// an array the caller leaves out altogether: it takes no staging space and the kernels see a null pointer
template <typename T>
Staged absent(T*& d) {
  return {&d, [](void* s, char*) { *static_cast<T**>(s) = nullptr; }, nullptr, nullptr, 0, NO_FILL};
}
// an input the caller may leave out
template <typename T>
Staged opt_in(T*& d, const void* src, size_t count) {
  return src ? in(d, src, count) : absent(d);
}
// an output that is downloaded whatever the call's status
template <typename T>
Staged out(T*& d, void* dst, size_t count, int fill = NO_FILL) {
  return arr(d, nullptr, dst, count, fill);
}
// one array that goes up from `src` and comes down to `dst`
template <typename T>
Staged inout(T*& d, const void* src, void* dst, size_t count) {
  return arr(d, src, dst, count, NO_FILL);
}
// an output that reaches `dst` only when the call's status says it was applied (for fpx_epx: FPX_OK or
// FPX_EFATAL_PROTOCOL; for fpx_ctx: FPX_OK): any other status leaves the caller's array as it was.  It is downloaded into
// the context's own host buffer and copied from there.
template <typename T>
Staged held(T*& d, T* dst, size_t count) {
  Staged a = arr(d, nullptr, dst, count, NO_FILL);
  a.hold = true;
  return a;
}
// a held output of which dst gets the first *n elements only, n being another held word of the call (decided_index)
inline Staged held_first(int32_t*& d, int32_t* dst, size_t count, int32_t*& n) {
  Staged a = held(d, dst, count);
  a.length = &n;
  return a;
}
template <typename T>
Staged scratch(T*& d, size_t count, int fill = NO_FILL) {
  return arr(d, nullptr, nullptr, count, fill);
}

// Where the arrays of a call lie, a function of the list alone: array i at byte at[i] of the staging buffer (in list
// order, every offset a multiple of STAGE_ALIGN, `total` bytes in all); a held array also at byte held_at[i] of the host
// buffer (`held_total` bytes), and length_at[i] is where that buffer has the length word of a held_first (or NONE); and
// the memsets that fill the arrays that start filled: neighbours in the list with one fill value are one run.
struct StageLayout {
  static constexpr size_t NONE = ~(size_t)0;
  struct Fill {
    size_t at, bytes;
    int value;
  };
  std::vector<size_t> at, held_at, length_at;
  std::vector<Fill> fills;
  size_t total = 0, held_total = 0;
};
inline StageLayout lay_stage(const Staged* a, size_t n) {
  StageLayout l;
  l.at.resize(n), l.held_at.resize(n), l.length_at.assign(n, StageLayout::NONE);
  int value = NO_FILL;  // the fill of the run that ends at l.total
  for (size_t i = 0; i < n; ++i) {
    l.at[i] = l.total, l.held_at[i] = l.held_total;
    if (a[i].span()) {  // (an array of no bytes neither starts nor ends a run)
      if (a[i].fill != NO_FILL && a[i].fill == value) l.fills.back().bytes += a[i].span();
      else if (a[i].fill != NO_FILL) l.fills.push_back({l.total, a[i].span(), a[i].fill});
      value = a[i].fill;
    }
    l.total += a[i].span(), l.held_total += a[i].host_span();
  }
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; a[i].length && j < n; ++j)
      if (a[j].hold && a[j].slot == a[i].length) l.length_at[i] = l.held_at[j];
  return l;
}
inline StageLayout lay_stage(std::initializer_list<Staged> arrays) { return lay_stage(arrays.begin(), arrays.size()); }

}  // namespace fpx
