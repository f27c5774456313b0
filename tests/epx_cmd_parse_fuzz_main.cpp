// epx_cmd_parse_fuzz_main.cpp -- TEST INFRASTRUCTURE ONLY, built with -fsanitize=address,undefined by
// tests/test_epaxos_cmd_parse_cpu.py.  Two things:
//  1. a seeded mutation fuzz of the command parser (frankenpaxos_amd/csrc/fpx_epx_cmd_parse.hpp): canonical CommandOrNoop
//     messages are flipped, cut, spliced and grown, every variant is copied into a heap buffer of EXACTLY its size -- a
//     read past the end is the sanitizer's error -- and parsed twice, as both classifies do: the count pass and the pass
//     that reports the keys, which must agree and must stay inside the message;
//  2. the scratch layouts of the new calls (lay_intern, lay_epx_classify, lay_epx_replica_tick of fpx_scratch.hpp) laid
//     out as carve() does and held to the rules of tests/epx_inbox_mk_scratch_main.cpp: aligned, inside the size of the
//     sizing pass, disjoint, written end to end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../frankenpaxos_amd/csrc/fpx_epx_cmd_parse.hpp"
#include "../frankenpaxos_amd/csrc/fpx_scratch.hpp"

using namespace fpx;

namespace {

int failures = 0;

// ---- 1. the fuzz -----------------------------------------------------------------------------------------------------
uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

std::string varint(uint64_t v) {
  std::string s;
  do {
    const uint8_t b = v & 0x7f;
    v >>= 7;
    s.push_back((char)(b | (v ? 0x80 : 0)));
  } while (v);
  return s;
}
std::string ld(int field, const std::string& body) { return varint((uint64_t)field << 3 | 2) + varint(body.size()) + body; }
std::string i32(int field, uint64_t v) { return varint((uint64_t)field << 3) + varint(v); }

std::string canonical() {
  if (rnd() % 10 == 0) return ld(2, "");
  const int keys = (int)(rnd() % 6);
  const bool set = rnd() & 1;
  std::string req;
  for (int j = 0; j < keys; ++j) {
    const std::string key((size_t)(rnd() % 9 == 0 ? rnd() % 600 : rnd() % 8), (char)('a' + rnd() % 26));
    req += set ? ld(1, ld(1, key) + ld(2, "v")) : ld(1, key);
  }
  std::string f[4] = {ld(1, "\x0a\x01\x02\x03"), i32(2, rnd() % 100), i32(3, rnd()), ld(4, ld(set ? 2 : 1, req))};
  for (int j = 3; j > 0; --j) std::swap(f[j], f[rnd() % (j + 1)]);
  return ld(1, f[0] + f[1] + f[2] + f[3]);
}

struct CheckSink {
  const uint8_t *lo, *hi;
  int32_t next = 0;
  size_t bytes = 0;
  void key(int32_t j, const uint8_t* at, int32_t len) {
    if (j < next || len < 0 || len > fpxw::EPX_KEY_MAX_LEN || at < lo || at + len > hi)
      std::printf("FAIL a key outside its message (j=%d len=%d)\n", j, len), ++failures;
    next = j + 1;
    for (int32_t k = 0; k < len; ++k) bytes += at[k];  // every byte of the key is read
  }
};

void fuzz() {
  long runs = 0, canonical_n = 0, shape0 = 0, malformed = 0;
  for (int round = 0; round < 30000; ++round) {
    std::string m = canonical();
    const int how = round < 3000 ? 0 : (int)(rnd() % 5);
    if (how == 1 && !m.empty()) m[rnd() % m.size()] ^= (char)(1u << (rnd() % 8));
    else if (how == 2) m.resize(rnd() % (m.size() + 1));
    else if (how == 3) m += canonical().substr(0, rnd() % 12);
    else if (how == 4) m.insert(rnd() % (m.size() + 1), i32((int)(rnd() % 12), rnd()));
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(m.size() ? m.size() : 1));  // exactly the message (malloc(0) may be null)
    if (!buf) std::abort();
    std::memcpy(buf, m.data(), m.size());
    const fpxw::Reader r{buf, buf + m.size()};
    fpxw::EpxCmd a, b;
    fpxw::EpxNoKeys none;
    CheckSink sink{buf, buf + m.size()};
    const bool ok_a = fpxw::epx_parse_command(r, &a, none), ok_b = fpxw::epx_parse_command(r, &b, sink);
    if (ok_a != ok_b || a.shape != b.shape || a.num_keys != b.num_keys || a.is_set != b.is_set || a.is_noop != b.is_noop)
      std::printf("FAIL the two passes disagree in round %d\n", round), ++failures;
    if (ok_a && a.shape == 1 && sink.next != a.num_keys && a.num_keys > 0)
      std::printf("FAIL round %d: %d keys counted, %d reported\n", round, a.num_keys, sink.next), ++failures;
    if ((!ok_a || a.shape == 0) && (a.num_keys | a.is_set | a.is_noop))
      std::printf("FAIL round %d: a refused frame reports fields\n", round), ++failures;
    if (how == 0 && !(ok_a && a.shape == 1)) std::printf("FAIL round %d: a canonical message is not shape 1\n", round), ++failures;
    ++runs, canonical_n += ok_a && a.shape == 1, shape0 += ok_a && a.shape == 0, malformed += !ok_a;
    std::free(buf);
  }
  std::printf("ok fuzz runs=%ld canonical=%ld shape0=%ld malformed=%ld\n", runs, canonical_n, shape0, malformed);
}

// ---- 2. the layouts ------------------------------------------------------------------------------------------------------
struct Span {
  const char* name;
  char* p;
  size_t bytes, align;
};
template <typename T>
void add(std::vector<Span>* v, const char* name, T* p, size_t count) {
  v->push_back({name, reinterpret_cast<char*>(p), count * sizeof(T), alignof(T)});
}

void add_intern(std::vector<Span>* v, const InternScratch& s, size_t P) {
  const size_t rows = (P + 1023) / 1024;
  add(v, "slot_of", s.slot_of, P), add(v, "rank", s.rank, P);
  for (int j = 0; j < 3; ++j) add(v, "sc", s.sc[j], rows * 1024), add(v, "tot", s.tot[j], rows);
  add(v, "gt", s.gt, (size_t)4), add(v, "ctl", s.ctl, (size_t)INTERN_CTL_WORDS);
}
void add_classify(std::vector<Span>* v, const EpxClassifyScratch& s, size_t m, size_t P) {
  const size_t rows = (m + 1023) / 1024;
  add(v, "cnt", s.cnt, m), add(v, "cscan", s.cscan, rows * 1024), add(v, "ctot", s.ctot, rows), add(v, "cgt", s.cgt, (size_t)1);
  add(v, "np", s.np, (size_t)1), add(v, "pair_off", s.pair_off, P), add(v, "pair_len", s.pair_len, P);
  add_intern(v, s.in, P);
}
// the arrays with the lengths the kernels index: m messages, max_pairs pairs, n replicas
void lay(Carver& c, std::vector<Span>* v, size_t m, size_t P, size_t n) {
  const EpxReplicaTickScratch s = lay_epx_replica_tick(c, m, n, P);
  int32_t* const per_msg[] = {s.kind, s.nr, s.shape, s.ri_kind, s.leader, s.number, s.b_ord, s.b_rep, s.dend, s.cmd_len,
                              s.is_noop, s.cmd_shape, s.triple};
  for (int32_t* a : per_msg) add(v, "per message", a, m);
  add(v, "deps", s.deps, m * n), add(v, "key_offsets", s.key_offsets, m + 1), add(v, "keys", s.keys, P);
  add(v, "result", s.result, (size_t)4), add(v, "cmd_off", s.cmd_off, m), add(v, "is_set", s.is_set, m);
  add_classify(v, s.cls, m, P);
  // the two smaller layouts are checked on their own too: the classify and a batch of the table
  const EpxClassifyScratch cl = lay_epx_classify(c, m, P);
  add_classify(v, cl, m, P);
  add_intern(v, lay_intern(c, P), P);
}

void check(size_t m, size_t P, size_t n) {
  Carver size(nullptr);
  std::vector<Span> none;
  lay(size, &none, m, P, n);
  const size_t bytes = size.size();
  for (const Span& s : none)
    if (s.p != nullptr) std::printf("FAIL m=%zu P=%zu n=%zu: %s is not null in the sizing pass\n", m, P, n, s.name), ++failures;
  void* mem = nullptr;
  if (posix_memalign(&mem, Carver::ALIGN, bytes ? bytes : 1) != 0) std::abort();
  char* buf = static_cast<char*>(mem);
  Carver c(buf);
  std::vector<Span> spans;
  lay(c, &spans, m, P, n);
  if (c.size() != bytes) std::printf("FAIL m=%zu P=%zu n=%zu: the passes disagree\n", m, P, n), ++failures;
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
    std::memset(a.p, (int)(i % 250) + 1, a.bytes);
  }
  for (size_t i = 0; i < spans.size(); ++i)
    for (size_t k = 0; k < spans[i].bytes; k += 97)
      if (spans[i].p[k] != (char)(i % 250 + 1)) {
        std::printf("FAIL m=%zu P=%zu n=%zu: %s was written over\n", m, P, n, spans[i].name), ++failures;
        break;
      }
  std::free(buf);
  std::printf("ok layout m=%zu P=%zu n=%zu bytes=%zu arrays=%zu\n", m, P, n, bytes, spans.size());
}

}  // namespace

int main() {
  fuzz();
  for (size_t m : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)3000})
    for (size_t P : {(size_t)0, (size_t)1, m, 5 * m + 1})
      for (size_t n : {(size_t)3, (size_t)5, (size_t)7}) check(m, P, n);
  if (failures) return std::printf("%d failures\n", failures), 1;
  std::printf("all ok\n");
  return 0;
}
