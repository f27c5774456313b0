// epx_cmd_reply_emit_main.cpp -- TEST INFRASTRUCTURE ONLY: the emitter of a replica tick's replies (csrc/fpx_wire_epx_emit.hpp)
// with a command source, as a program of its own for the sanitizers (tests/test_epaxos_cmd_reply_encode_cpu.py builds it with
// -fsanitize=address,undefined and runs it).  Every reply goes into a heap buffer of EXACTLY its planned length and the arena
// is a heap block of EXACTLY the bytes used, so a byte written or read past either is a report; the lengths the plan
// gives, the place of the command and the frame (wrapper tag, inner length) are checked against the bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../frankenpaxos_amd/csrc/fpx_wire_epx_emit.hpp"

using namespace fpxw;

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}
int32_t pick(std::initializer_list<int32_t> v) { return v.begin()[rnd() % v.size()]; }

int fails = 0;
void fail(const char* what, int n, int i) {
  if (++fails < 20) printf("FAIL %s n=%d record=%d\n", what, n, i);
}

// a varint at p: its value, *used = its bytes
uint64_t read_varint(const uint8_t* p, const uint8_t* end, int* used) {
  uint64_t v = 0;
  int k = 0;
  while (p + k < end) {
    v |= (uint64_t)(p[k] & 0x7f) << (7 * k);
    if (!(p[k++] & 0x80)) break;
  }
  *used = k;
  return v;
}

}  // namespace

int main() {
  const int32_t bounds[] = {0, 1, 127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28, 0x7fffffff};
  const int32_t lens[] = {0, 1, 2, 15, 16, 17, 127, 128, 129, 4097, 1 << 16};
  long commit = 0, prepare_ok_cmd = 0, deferred = 0, shorts = 0;
  for (int round = 0; round < 60; ++round) {
    const int n = round % 3 == 0 ? 3 : round % 3 == 1 ? 5 : 7;
    // a store of max_triples ids, about two thirds with bytes; the arena a heap block of exactly the bytes used
    const int32_t max_triples = 1 + (int32_t)(rnd() % 40);
    std::vector<int64_t> coff((size_t)max_triples, -1);
    std::vector<int32_t> clen((size_t)max_triples, 0);
    std::vector<uint8_t> bytes;
    for (int32_t t = 0; t < max_triples; ++t) {
      if (rnd() % 3 == 0) continue;
      const int32_t len = round % 10 == 0 ? lens[rnd() % 11] : lens[rnd() % 9];
      coff[(size_t)t] = (int64_t)bytes.size(), clen[(size_t)t] = len;
      for (int32_t k = 0; k < len; ++k) bytes.push_back((uint8_t)(rnd() | 1));
    }
    uint8_t* arena = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);
    if (!bytes.empty()) memcpy(arena, bytes.data(), bytes.size());
    const int m = 300;
    std::vector<int32_t> to(m), leader(m), number(m), bo(m), br(m), outcome(m), ob(m), os(m), deps((size_t)m * n), end(m), tr(m);
    for (int i = 0; i < m; ++i) {
      leader[i] = (int32_t)(rnd() % n), to[i] = (int32_t)(rnd() % n);
      number[i] = bounds[rnd() % 11];
      if (number[i] > 0x7fffffff - 70) number[i] = 0x7fffffff - 70;
      bo[i] = pick({0, 127, 128, (1 << 27) - 1}), br[i] = (int32_t)(rnd() % n);
      outcome[i] = pick({8, 8, 6, 6, 6, 1, 3, 7, 0});
      ob[i] = rnd() % 4 == 0 ? -1 : (int32_t)((rnd() % 1000) << 3 | (rnd() % n));
      os[i] = outcome[i] == 6 ? pick({0, 1, 2, 2, 3, 3}) : -1;
      for (int l = 0; l < n; ++l) deps[(size_t)i * n + l] = bounds[rnd() % 11];
      if (rnd() % 8 == 0) deps[(size_t)i * n] = -1;  // dependencies by id
      const int32_t ids = pick({0, 0, 1, 63, 64, 65});
      end[i] = ids ? number[i] + 1 + ids : 0;
      if (ids) deps[(size_t)i * n + leader[i]] = number[i];
      tr[i] = pick({-1, max_triples, max_triples + 3}) ;
      if (rnd() % 5) tr[i] = (int32_t)(rnd() % max_triples);
    }
    EpxReplyIn a{n, to.data(), leader.data(), number.data(), bo.data(), br.data(), outcome.data(), ob.data(), os.data(),
                 deps.data(), end.data()};
    a.out_triple = tr.data();
    a.cmds.off = coff.data(), a.cmds.len = clen.data(), a.cmds.arena = arena, a.cmds.max_triples = max_triples;
    EpxReplyIn none = a;
    none.cmds = EpxCmdSource{};
    for (int i = 0; i < m; ++i) {
      const EpxReplyPlan p = epx_reply_plan(a, i), q = epx_reply_plan(none, i);
      const bool carries = outcome[i] == 8 || (outcome[i] == 6 && (os[i] == 2 || os[i] == 3));
      if (!carries && (p.kind != q.kind || p.len != q.len || p.cmd_len >= 0)) fail("a record without a command changed", n, i);
      if (carries && q.kind != EPX_REPLY_DEFERRED) fail("no source, not deferred", n, i);
      const bool stored = tr[i] >= 0 && tr[i] < max_triples && coff[(size_t)tr[i]] >= 0;
      const bool want = carries && stored && deps[(size_t)i * n] >= 0 && epx_own_ids(number[i], end[i]) <= EPX_REPLY_IDS_MAX;
      if (carries && (p.kind == EPX_REPLY_ENCODED) != want) fail("plan", n, i);
      if (p.kind == EPX_REPLY_DEFERRED) ++deferred;
      if (p.kind != EPX_REPLY_ENCODED) continue;
      uint8_t* buf = (uint8_t*)malloc((size_t)p.len);  // exactly the planned length
      memset(buf, 0xEE, (size_t)p.len);
      if (p.cmd_len < 0) {
        if (epx_reply_emit(buf, a, i, p.outcome) != p.len) fail("short length", n, i);
        ++shorts;
      } else {
        int64_t cmd_at = -1;
        if (epx_reply_emit_around(buf, a, i, p, &cmd_at) != p.len) fail("length", n, i);
        if (p.cmd_len != clen[(size_t)tr[i]] || p.cmd_off != coff[(size_t)tr[i]]) fail("the command's place in the arena", n, i);
        if (cmd_at < 0 || cmd_at + p.cmd_len > p.len) {
          fail("the command's place in the reply", n, i);
        } else {
          for (int64_t k = 0; k < p.cmd_len; ++k)
            if (buf[cmd_at + k] != 0xEE) fail("a byte written inside the command's span", n, i);
          if (p.cmd_len > 0) memcpy(buf + cmd_at, arena + p.cmd_off, (size_t)p.cmd_len);
          // in front of the command: the field's tag and the command's length
          int used = 0;
          const int64_t vl = varint_len((uint64_t)p.cmd_len);
          if (cmd_at < 1 + vl || buf[cmd_at - vl - 1] != (uint8_t)(((outcome[i] == 8 ? 2 : 6) << 3) | 2) ||
              (int64_t)read_varint(buf + cmd_at - vl, buf + cmd_at, &used) != p.cmd_len || used != vl)
            fail("the command field's head", n, i);
          // behind it: sequence_number = 0
          if (cmd_at + p.cmd_len + 2 > p.len || buf[cmd_at + p.cmd_len] != (uint8_t)((outcome[i] == 8 ? 3 : 7) << 3) ||
              buf[cmd_at + p.cmd_len + 1] != 0)
            fail("the field behind the command", n, i);
        }
        (outcome[i] == 8 ? commit : prepare_ok_cmd)++;
      }
      // the frame: the wrapper's tag and the inner length
      int used = 0;
      const uint64_t inner = read_varint(buf + 1, buf + p.len, &used);
      const int wrapper = outcome[i] == 8 ? 6 : outcome[i] == 6 ? 8 : outcome[i] == 7 ? 9 : outcome[i] <= 2 ? 3 : 5;
      if (buf[0] != (uint8_t)((wrapper << 3) | 2) || (int64_t)inner + 1 + used != p.len) fail("frame", n, i);
      free(buf);
    }
    free(arena);
  }
  printf("ok replies commit=%ld prepare_ok_cmd=%ld deferred=%ld short=%ld\n", commit, prepare_ok_cmd, deferred, shorts);
  if (fails) {
    printf("FAIL %d checks\n", fails);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
