// epx_reply_emit_main.cpp -- TEST INFRASTRUCTURE ONLY: the emitter of a replica tick's replies (csrc/fpx_wire_epx_emit.hpp) and
// the scratch layouts of its device calls (csrc/fpx_scratch.hpp) in a program of their own, built with
// -fsanitize=address,undefined by tests/test_epaxos_reply_encode_cpu.py.  Every reply is emitted into a heap buffer of exactly
// the bytes its closed-form length promises, so a writer that runs past its length is a heap overflow the sanitizer reports;
// the bytes are compared with a writer that appends field by field and counts every id in a loop.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../frankenpaxos_amd/csrc/fpx_scratch.hpp"
#include "../frankenpaxos_amd/csrc/fpx_wire_epx_emit.hpp"

using namespace fpxw;

namespace {

int failures = 0;

// ---- the writer a second time: vectors, appended field by field ------------------------------------------------------------
typedef std::vector<uint8_t> Bytes;
void put_varint(Bytes& b, uint64_t v) {
  for (; v >= 0x80; v >>= 7) b.push_back((uint8_t)(v | 0x80));
  b.push_back((uint8_t)v);
}
void put_i32(Bytes& b, uint32_t field, int32_t v) { put_varint(b, field << 3), put_varint(b, (uint64_t)(int64_t)v); }
void put_ld(Bytes& b, uint32_t field, const Bytes& body) {
  put_varint(b, field << 3 | 2), put_varint(b, body.size());
  b.insert(b.end(), body.begin(), body.end());
}
Bytes two(int32_t a, int32_t c) {
  Bytes b;
  put_i32(b, 1, a), put_i32(b, 2, c);
  return b;
}
Bytes reference(const EpxReplyIn& a, int32_t i) {
  Bytes inner, out;
  const int32_t outcome = a.outcome[i];
  const Bytes inst = two(a.leader[i], a.number[i]), ballot = two(a.b_ord[i], a.b_rep[i]);
  const int32_t ob = a.out_ballot[i];
  if (outcome == 1 || outcome == 2) {
    Bytes deps;
    put_i32(deps, 1, a.n);
    for (int32_t l = 0; l < a.n; ++l) {
      Bytes set;
      put_i32(set, 1, a.out_deps[(size_t)i * a.n + l]);
      if (l == a.leader[i] && a.out_end[i] > 0)
        for (int64_t v = (int64_t)a.number[i] + 1; v < a.out_end[i]; ++v) put_i32(set, 2, (int32_t)v);
      put_ld(deps, 2, set);
    }
    put_ld(inner, 1, inst), put_ld(inner, 2, ballot), put_i32(inner, 3, a.to[i]), put_i32(inner, 4, 0), put_ld(inner, 5, deps);
    put_ld(out, 3, inner);
  } else if (outcome == 3 || outcome == 4) {
    put_ld(inner, 2, inst), put_ld(inner, 3, ballot), put_i32(inner, 7, a.to[i]);
    put_ld(out, 5, inner);
  } else if (outcome == 7) {
    put_ld(inner, 1, inst), put_ld(inner, 2, two(ob >> 3, ob & 7));
    put_ld(out, 9, inner);
  } else if (outcome == 6) {
    put_ld(inner, 1, ballot), put_ld(inner, 2, inst), put_i32(inner, 3, a.to[i]);
    put_ld(inner, 4, ob < 0 ? two(-1, -1) : two(ob >> 3, ob & 7)), put_i32(inner, 5, 0);
    put_ld(out, 8, inner);
  }
  return out;
}

// ---- records on the varint boundaries, and some that no replica puts out (negative numbers: the encoder validates nothing) ----
uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}
int32_t edge_value(bool wild) {
  static const int64_t E[] = {0, 1, 127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28, 0x7fffffff};
  const int64_t e = E[rnd() % 11];
  int64_t v = e + (int64_t)(rnd() % 5) - 2;
  if (wild && rnd() % 8 == 0) v = -(int64_t)(rnd() % 300) - 1;
  if (v > 0x7fffffff) v = 0x7fffffff;
  if (v < 0 && !wild) v = 0;
  return (int32_t)v;
}

void replies() {
  long count[6] = {0, 0, 0, 0, 0, 0};  // PreAcceptOk, AcceptOk, Nack, PrepareOk, deferred, none
  for (int round = 0; round < 6000; ++round) {
    const int32_t n = 3 + 2 * (int32_t)(rnd() % 3), m = 1 + (int32_t)(rnd() % 8);
    const bool wild = round % 3 == 0;
    // every array on the heap, sized exactly
    std::vector<int32_t> to(m), leader(m), number(m), bo(m), br(m), outcome(m), ob(m), os(m), deps((size_t)m * n), end(m);
    for (int32_t i = 0; i < m; ++i) {
      to[i] = (int32_t)(rnd() % n), leader[i] = (int32_t)(rnd() % n), number[i] = edge_value(wild);
      bo[i] = edge_value(false) & ((1 << 27) - 1), br[i] = (int32_t)(rnd() % n), outcome[i] = (int32_t)(rnd() % 9);
      ob[i] = rnd() % 4 == 0 ? -1 : (int32_t)((uint32_t)(edge_value(false) & ((1 << 27) - 1)) << 3 | rnd() % 7);
      os[i] = rnd() % 2 ? 0 : (int32_t)(rnd() % 4);
      for (int32_t l = 0; l < n; ++l) deps[(size_t)i * n + l] = edge_value(wild);
      if (rnd() % 6 == 0) deps[(size_t)i * n] = -1;
      const int64_t ids = rnd() % 3 == 0 ? 0 : rnd() % 70;
      const int64_t e = (int64_t)number[i] + 1 + ids;
      end[i] = rnd() % 4 == 0 ? 0 : (int32_t)(e > 0x7fffffff ? 0x7fffffff : e);
    }
    const EpxReplyIn a{n, to.data(), leader.data(), number.data(), bo.data(), br.data(), outcome.data(), ob.data(), os.data(),
                       deps.data(), end.data()};
    for (int32_t i = 0; i < m; ++i) {
      const EpxReplyPlan p = epx_reply_plan(a, i);
      if (p.kind != EPX_REPLY_ENCODED) {
        if (p.len != 0) std::printf("FAIL round %d: a record without a reply has a length\n", round), ++failures;
        ++count[p.kind == EPX_REPLY_DEFERRED ? 4 : 5];
        continue;
      }
      ++count[outcome[i] <= 2 ? 0 : outcome[i] <= 4 ? 1 : outcome[i] == 7 ? 2 : 3];
      uint8_t* const buf = new uint8_t[(size_t)p.len];  // exactly the promised bytes
      const int64_t wrote = epx_reply_emit(buf, a, i, p.outcome);
      const Bytes want = reference(a, i);
      if (wrote != p.len || (int64_t)want.size() != p.len || std::memcmp(buf, want.data(), (size_t)p.len) != 0)
        std::printf("FAIL round %d message %d outcome %d: len %lld wrote %lld reference %zu\n", round, i, outcome[i],
                    (long long)p.len, (long long)wrote, want.size()),
            ++failures;
      delete[] buf;
    }
  }
  std::printf("ok replies pre_accept_ok=%ld accept_ok=%ld nack=%ld prepare_ok=%ld deferred=%ld none=%ld\n", count[0], count[1],
              count[2], count[3], count[4], count[5]);
}

// the closed-form run length against a loop, across every boundary and below zero
void id_runs() {
  const int64_t edges[] = {-300, -1, 0, 1, 128, 16384, 1 << 21, 1 << 28, 0x7fffffff};
  for (int64_t e : edges)
    for (int64_t lo = e - 70; lo <= e + 2; ++lo)
      for (int64_t cnt : {0, 1, 2, 63, 64, 65, 70}) {
        const int64_t hi = lo + cnt;
        if (lo < -0x80000000ll || hi > 0x7fffffff) continue;
        int64_t want = 0;
        for (int64_t v = lo; v < hi; ++v) want += i32_len((int32_t)v);
        if (epx_id_run_len(lo, hi) != want)
          std::printf("FAIL ids %lld .. %lld: closed form %lld, counted %lld\n", (long long)lo, (long long)hi,
                      (long long)epx_id_run_len(lo, hi), (long long)want),
              ++failures;
      }
  std::printf("ok id runs\n");
}

// ---- the scratch layouts of the device calls: inside the buffer, aligned, disjoint -----------------------------------------
struct Span {
  const char* name;
  char* p;
  size_t bytes, align;
};
template <typename T>
void add(std::vector<Span>* v, const char* name, T* p, size_t count) {
  v->push_back(Span{name, reinterpret_cast<char*>(p), count * sizeof(T), alignof(T)});
}
void lay(fpx::Carver& c, std::vector<Span>* v, size_t m, size_t n) {
  const size_t rows = (m + 1023) / 1024;
  const fpx::EpxTickBytesScratch s = fpx::lay_epx_tick_bytes(c, m, n);
  add(v, "lscan", s.enc.lscan, rows * 1024), add(v, "ltot", s.enc.ltot, rows), add(v, "lgt", s.enc.lgt, (size_t)1);
  add(v, "ctl", s.enc.ctl, (size_t)fpx::EPX_REPLY_ENC_CTL_WORDS);
  add(v, "outcome", s.outcome, m), add(v, "out_ballot", s.out_ballot, m), add(v, "out_status", s.out_status, m);
  add(v, "out_end", s.out_end, m), add(v, "out_deps", s.out_deps, m * n);
  const fpx::EpxReplyEncScratch e = fpx::lay_epx_reply_enc(c, m);
  add(v, "lscan alone", e.lscan, rows * 1024), add(v, "ltot alone", e.ltot, rows), add(v, "lgt alone", e.lgt, (size_t)1);
  add(v, "ctl alone", e.ctl, (size_t)fpx::EPX_REPLY_ENC_CTL_WORDS);
}
void check(size_t m, size_t n) {
  fpx::Carver size(nullptr);
  std::vector<Span> none;
  lay(size, &none, m, n);
  const size_t bytes = size.size();
  void* mem = nullptr;
  if (posix_memalign(&mem, fpx::Carver::ALIGN, bytes ? bytes : 1) != 0) std::abort();
  char* buf = static_cast<char*>(mem);
  fpx::Carver c(buf);
  std::vector<Span> spans;
  lay(c, &spans, m, n);
  if (c.size() != bytes) std::printf("FAIL m=%zu n=%zu: the passes disagree\n", m, n), ++failures;
  for (size_t i = 0; i < spans.size(); ++i) {
    const Span& a = spans[i];
    if (reinterpret_cast<uintptr_t>(a.p) % a.align != 0) std::printf("FAIL m=%zu n=%zu: %s is misaligned\n", m, n, a.name), ++failures;
    if (a.p < buf || a.p + a.bytes > buf + bytes) {
      std::printf("FAIL m=%zu n=%zu: %s leaves the buffer\n", m, n, a.name), ++failures;
      continue;
    }
    for (size_t j = 0; j < i; ++j)
      if (a.bytes && spans[j].bytes && a.p < spans[j].p + spans[j].bytes && spans[j].p < a.p + a.bytes)
        std::printf("FAIL m=%zu n=%zu: %s overlaps %s\n", m, n, a.name, spans[j].name), ++failures;
    std::memset(a.p, (int)i + 1, a.bytes);  // (a write outside the allocation is the sanitizer's)
  }
  std::free(buf);
  std::printf("ok layout m=%zu n=%zu bytes=%zu arrays=%zu\n", m, n, bytes, spans.size());
}

}  // namespace

int main() {
  replies();
  id_runs();
  for (size_t m : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)1025, (size_t)65536, (size_t)70001})
    for (size_t n : {(size_t)3, (size_t)5, (size_t)7}) check(m, n);
  if (failures) return std::printf("%d failures\n", failures), 1;
  std::printf("all ok\n");
  return 0;
}
