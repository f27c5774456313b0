// epx_inbox_mk_scratch_main.cpp -- TEST INFRASTRUCTURE ONLY: tests/epx_inbox_scratch_main.cpp for the key-list form: lays out
// the scratch of fpx_epx_replica_inbox_mk with frankenpaxos_amd/csrc/fpx_scratch.hpp (host code, no HIP) exactly as carve()
// does -- over a null base for the size, then over a buffer of that size -- and holds lay_epx_inbox_mk to the same rules:
// every array is aligned for its type (the pair arrays for the kernels' uint2), lies inside the size of the sizing pass and
// overlaps no other.  The m-sized pieces and the P-sized pieces are swept independently.  Every array is then written from
// end to end, so that built with -fsanitize=address,undefined (tests/test_epaxos_inbox_mk_cpu.py) a layout that leaves its
// buffer is an error of its own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../frankenpaxos_amd/csrc/fpx_scratch.hpp"

using namespace fpx;

namespace {

struct Span {
  const char* name;
  char* p;
  size_t bytes, align;
};

int failures = 0;

template <typename T>
void add(std::vector<Span>* v, const char* name, T* p, size_t count, size_t align = alignof(T)) {
  v->push_back({name, reinterpret_cast<char*>(p), count * sizeof(T), align});
}

// the arrays with the lengths the kernels of fpx_epx_inbox.hpp index: m messages, P pairs (one element when P = 0), n
// replicas, CL_TILE = 1024 messages per tile of the largestBallot scan
void lay(Carver& c, std::vector<Span>* v, size_t m, size_t P, size_t n) {
  const size_t tiles = (m + 1023) / 1024;
  const EpxInboxMkScratch s = lay_epx_inbox_mk(c, m, P, n, tiles);
  add(v, "cell0", s.msg.cell[0], 2 * m, 8), add(v, "cell1", s.msg.cell[1], 2 * m, 8);
  add(v, "src", s.msg.src, m), add(v, "last", s.msg.last, m);
  add(v, "contrib", s.msg.contrib, n * m), add(v, "tilemax", s.msg.tilemax, n * tiles), add(v, "nackflag", s.msg.nackflag, n * m);
  add(v, "pnum", s.pair.pnum, P ? P : 1), add(v, "uniq", s.pair.uniq, P ? P : 1);
}

void check(size_t m, size_t P, size_t n) {
  Carver size(nullptr);
  std::vector<Span> none;
  lay(size, &none, m, P, n);
  const size_t bytes = size.size();
  for (const Span& s : none)
    if (s.p != nullptr) std::printf("FAIL m=%zu P=%zu n=%zu: %s is not null in the sizing pass\n", m, P, n, s.name), ++failures;
  void* mem = nullptr;  // exactly `bytes`: the sanitizer sees a write one byte past the sizing pass's answer
  if (posix_memalign(&mem, Carver::ALIGN, bytes ? bytes : 1) != 0) std::abort();
  char* buf = static_cast<char*>(mem);
  Carver c(buf);
  std::vector<Span> spans;
  lay(c, &spans, m, P, n);
  if (c.size() != bytes) std::printf("FAIL m=%zu P=%zu n=%zu: the passes disagree, %zu != %zu\n", m, P, n, c.size(), bytes), ++failures;
  for (size_t i = 0; i < spans.size(); ++i) {
    const Span& a = spans[i];
    if (reinterpret_cast<uintptr_t>(a.p) % a.align != 0) std::printf("FAIL m=%zu P=%zu n=%zu: %s is misaligned\n", m, P, n, a.name), ++failures;
    if (a.p < buf || a.p + a.bytes > buf + bytes) {
      std::printf("FAIL m=%zu P=%zu n=%zu: %s leaves the buffer\n", m, P, n, a.name), ++failures;
      continue;
    }
    for (size_t j = 0; j < i; ++j) {
      const Span& b = spans[j];
      if (a.bytes && b.bytes && a.p < b.p + b.bytes && b.p < a.p + a.bytes)
        std::printf("FAIL m=%zu P=%zu n=%zu: %s overlaps %s\n", m, P, n, a.name, b.name), ++failures;
    }
    std::memset(a.p, (int)i + 1, a.bytes);
  }
  for (size_t i = 0; i < spans.size(); ++i)  // (no array was written over by a later one)
    for (size_t k = 0; k < spans[i].bytes; k += 97)
      if (spans[i].p[k] != (char)(i + 1)) {
        std::printf("FAIL m=%zu P=%zu n=%zu: %s was written over\n", m, P, n, spans[i].name), ++failures;
        break;
      }
  std::free(buf);
  std::printf("ok epx_inbox_mk m=%zu P=%zu n=%zu bytes=%zu arrays=%zu\n", m, P, n, bytes, spans.size());
}

}  // namespace

int main() {
  for (size_t m : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)3000})
    for (size_t P : {(size_t)0, (size_t)1, m, 5 * m + 1})
      for (size_t n : {(size_t)3, (size_t)5, (size_t)7}) check(m, P, n);
  if (failures) return std::printf("%d failures\n", failures), 1;
  std::printf("all layouts ok\n");
  return 0;
}
