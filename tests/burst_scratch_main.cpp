// burst_scratch_main.cpp -- TEST INFRASTRUCTURE ONLY: lays out the scratch of the four burst entry points and of the
// EPaxos multi-key tick and leader-replies compaction with frankenpaxos_amd/csrc/fpx_scratch.hpp (host code, no HIP)
// exactly as carve() (fpx_host.hpp) does for fpx_api.hip and fpx_epaxos.hip -- over a null base for
// the size, then over a buffer of that size -- and checks that every array is aligned for its type, lies inside the size
// of the sizing pass, and overlaps no other.  Every array is then written from end to end, so that built with
// -fsanitize=address,undefined (tests/test_burst_scratch_cpu.py) a layout that leaves its buffer is an error of its own.
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
void add(std::vector<Span>* v, const char* name, T* p, size_t count) {
  v->push_back({name, reinterpret_cast<char*>(p), count * sizeof(T), alignof(T)});
}

void add_sort(std::vector<Span>* v, const SortScratch& s, size_t tiles) {
  add(v, "hist", s.hist, SORT_RADIX * tiles);
  add(v, "key0", s.key[0], tiles * BURST_TILE), add(v, "key1", s.key[1], tiles * BURST_TILE);
  add(v, "val0", s.val[0], tiles * BURST_TILE), add(v, "val1", s.val[1], tiles * BURST_TILE);
}
void add_replica_msgs(std::vector<Span>* v, const ReplicaMsgsScratch& s, size_t nblk, size_t ranges, size_t parts) {
  add(v, "hdr", s.hdr, BURST_HDR_WORDS), add(v, "parts", s.parts, 3 * parts), add(v, "blk", s.blk, nblk);
  add(v, "list", s.list, ranges), add(v, "res", s.res, ranges);
}
void add_acceptor(std::vector<Span>* v, const AcceptorInboxScratch& s, size_t n, size_t E) {
  const size_t tiles = burst_tiles(n);
  add(v, "hdr", s.hdr, BURST_HDR_WORDS), add(v, "tile", s.tile, tiles);
  add_sort(v, s.sort, tiles);
  add(v, "accslot", s.accslot, tiles * BURST_TILE), add(v, "tpos", s.tpos, tiles * BURST_TILE);
  add(v, "fin_round", s.fin_round, E), add(v, "fin_slot", s.fin_slot, E);
}

// lay(Carver&, std::vector<Span>*): the layout, and the arrays it handed out with the lengths their kernels use
template <typename Lay>
void check(const char* what, size_t n, Lay lay) {
  Carver size(nullptr);
  std::vector<Span> none;
  lay(size, &none);
  const size_t bytes = size.size();
  for (const Span& s : none)
    if (s.p != nullptr) std::printf("FAIL %s n=%zu: %s is not null in the sizing pass\n", what, n, s.name), ++failures;
  // exactly `bytes`, so that the sanitizer sees a write one byte past the sizing pass's answer; aligned as the device's
  // allocations are
  void* mem = nullptr;
  if (posix_memalign(&mem, Carver::ALIGN, bytes) != 0) std::abort();
  char* buf = static_cast<char*>(mem);
  Carver c(buf);
  std::vector<Span> spans;
  lay(c, &spans);
  if (c.size() != bytes) std::printf("FAIL %s n=%zu: the passes disagree, %zu != %zu\n", what, n, c.size(), bytes), ++failures;
  for (size_t i = 0; i < spans.size(); ++i) {
    const Span& a = spans[i];
    if (reinterpret_cast<uintptr_t>(a.p) % a.align != 0) std::printf("FAIL %s n=%zu: %s is misaligned\n", what, n, a.name), ++failures;
    if (a.p < buf || a.p + a.bytes > buf + bytes) {
      std::printf("FAIL %s n=%zu: %s leaves the buffer\n", what, n, a.name), ++failures;
      continue;
    }
    for (size_t j = 0; j < i; ++j) {
      const Span& b = spans[j];
      if (a.bytes && b.bytes && a.p < b.p + b.bytes && b.p < a.p + a.bytes)
        std::printf("FAIL %s n=%zu: %s overlaps %s\n", what, n, a.name, b.name), ++failures;
    }
    std::memset(a.p, (int)i + 1, a.bytes);
  }
  // (no array was written over by a later one)
  for (size_t i = 0; i < spans.size(); ++i)
    for (size_t k = 0; k < spans[i].bytes; k += 97)
      if (spans[i].p[k] != (char)(i + 1)) {
        std::printf("FAIL %s n=%zu: %s was written over\n", what, n, spans[i].name), ++failures;
        break;
      }
  std::free(buf);
  std::printf("ok %s n=%zu bytes=%zu arrays=%zu\n", what, n, bytes, spans.size());
}

}  // namespace

int main() {
  const size_t parts = 4096, E = 3 * 5, S = 1 << 16;
  for (size_t n : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)3000, (size_t)262969}) {
    const size_t nblk = burst_tiles(n);
    check("replica_msgs", n, [&](Carver& c, std::vector<Span>* v) {
      add_replica_msgs(v, lay_replica_msgs(c, nblk, n, parts), nblk, n, parts);
    });
    for (bool outputs : {false, true}) {
      const size_t nb = nblk ? nblk : 1, slot_tiles = burst_tiles(S);  // (a call with n = 0 and outputs still launches)
      check(outputs ? "replica_inbox+outputs" : "replica_inbox", n, [&](Carver& c, std::vector<Span>* v) {
        const ReplicaInboxScratch s = lay_replica_inbox(c, nb, slot_tiles, parts, outputs);
        add_replica_msgs(v, s.m, nb, 0, parts);
        add(v, "rhdr", s.rhdr, BURST_HDR_WORDS), add(v, "ri hdr", s.hdr, BURST_HDR_WORDS), add(v, "tmax", s.tmax, slot_tiles);
        add_sort(v, s.sort, outputs ? nb : 0);
      });
    }
    check("acceptor_inbox", n, [&](Carver& c, std::vector<Span>* v) { add_acceptor(v, lay_acceptor_inbox(c, n, E), n, E); });
    check("mencius_acceptor_inbox", n, [&](Carver& c, std::vector<Span>* v) {
      const MenciusAcceptorInboxScratch s = lay_mencius_acceptor_inbox(c, n, E);
      const size_t tiles = burst_tiles(n);
      add_acceptor(v, s.a, n, E);
      add(v, "rflag", s.rflag, tiles * BURST_TILE), add(v, "rcnt", s.rcnt, tiles);
      for (int j = 0; j < 5; ++j) add(v, "list", s.list[j], tiles * BURST_TILE);
    });
    // EPaxos, n commands / key-list entries / replies: the lengths are what the kernels index (MK_TILE = LR_BLOCK = 1024
    // positions per scan tile, 256 commands per workgroup of k_mk_prep)
    const size_t tiles1k = (n + 1023) / 1024;
    for (size_t replicas : {(size_t)3, (size_t)5, (size_t)7})
      check(replicas == 3 ? "mk_prologue n=3" : replicas == 5 ? "mk_prologue n=5" : "mk_prologue n=7", n,
            [&](Carver& c, std::vector<Span>* v) {
              const MkPrologueScratch s = lay_mk_prologue(c, n, replicas, tiles1k, nblk);
              add(v, "info", s.info, 16), add(v, "ucnt", s.ucnt, n), add(v, "tsum", s.tsum, replicas * tiles1k);
              add(v, "part", s.part, 2 * nblk);
              if (reinterpret_cast<uintptr_t>(s.part) % 8 != 0) std::printf("FAIL mk_prologue: part is no int2 array\n"), ++failures;
            });
    check("mk_pairs", n, [&](Carver& c, std::vector<Span>* v) {  // (no array per replica in this one)
      const MkPairScratch s = lay_mk_pairs(c, n);
      add(v, "pnum", s.pnum, n ? n : 1), add(v, "uniq", s.uniq, n ? n : 1);
    });
    check("leader_replies", n, [&](Carver& c, std::vector<Span>* v) {
      const LrScratch s = lay_leader_replies(c, n, tiles1k);
      add(v, "flag", s.flag, n), add(v, "bsum", s.bsum, tiles1k);
    });
  }
  if (failures) return std::printf("%d failures\n", failures), 1;
  std::printf("all layouts ok\n");
  return 0;
}
