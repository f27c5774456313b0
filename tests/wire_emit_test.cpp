// The emitter source of the wire adapter (frankenpaxos_amd/csrc/fpx_wire_emit.hpp) compiled by the system compiler
// alone: tests/test_wire_emit.py loads this as a shared library, lets check_lens hold every layout's *_len against the
// bytes its *_emit writes, and compares the bytes of the emit_* wrappers with the host encoders of libfpx.so.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../frankenpaxos_amd/csrc/fpx_wire_emit.hpp"

using namespace fpxw;

static const int32_t EDGES[] = {0,          1,           127,        128,        16383,      16384,     (1 << 21) - 1,
                                1 << 21,    (1 << 28) - 1, 1 << 28,  0x7fffffff, -1,         -128,      INT32_MIN};
static const int NEDGES = sizeof(EDGES) / sizeof(EDGES[0]);

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// a field value: an edge, an edge +- 1, or random bits of a random width (so every varint length turns up)
static int32_t pick() {
  const uint64_t r = rnd();
  switch (r & 3) {
    case 0: return EDGES[(r >> 8) % NEDGES];
    case 1: return (int32_t)((uint32_t)EDGES[(r >> 8) % NEDGES] + (uint32_t)((r >> 20) % 3) - 1u);
    default: return (int32_t)((uint32_t)(r >> 32) >> ((r >> 8) % 32)) * ((r & 4) ? 1 : -1);
  }
}

extern "C" {

// returns the number of (layout, values) cases where *_len != the bytes *_emit wrote, or where a byte landed outside them
int64_t check_lens(int64_t cases, uint64_t seed) {
  rng_state = seed;
  int64_t wrong = 0;
  std::vector<uint8_t> value(70000, 0xAB), out(70100);
  auto run = [&](int64_t want, auto emit) {
    memset(out.data(), 0xEE, 64);
    const int64_t got = emit(out.data());
    if (got != want || (got < 64 && out[(size_t)got] != 0xEE)) ++wrong;
  };
  for (int64_t c = 0; c < cases; ++c) {
    int32_t v[5];
    for (int j = 0; j < 5; ++j) v[j] = c < (int64_t)NEDGES * NEDGES ? EDGES[(c / (j & 1 ? NEDGES : 1)) % NEDGES] : pick();
    const int k = 1 + (int)(rnd() % 5);
    run(ints_len(k, v), [&](uint8_t* o) { return ints_emit(o, 1 + (uint32_t)(rnd() % 15), k, v); });
    for (int d = 0; d < 2; ++d) {
      run(phase2b_len(d, v[0], v[1], v[2], v[3]), [&](uint8_t* o) { return phase2b_emit(o, d, v[0], v[1], v[2], v[3]); });
      run(nack_len(v[0]), [&](uint8_t* o) { return nack_emit(o, d, v[0]); });
    }
    static const int32_t LENS[] = {0, 1, 2, 127, 128, 300, 16383, 16384, 20000, 65000};
    const int32_t vl = (c % 16) ? (int32_t)(rnd() % 200) : LENS[rnd() % 10];
    run(chosen_len(v[0], vl), [&](uint8_t* o) { return chosen_emit(o, v[0], value.data(), vl); });
    run(phase2a_len(v[0], v[1], vl), [&](uint8_t* o) { return phase2a_emit(o, 1 + (uint32_t)(rnd() % 2), v[0], v[1], value.data(), vl); });
    // the head alone: what is left of the message when the value's bytes are taken away
    const int64_t head = chosen_emit(out.data(), v[0], nullptr, vl);
    if (head != chosen_len(v[0], vl) - vl || head > CHOSEN_HEAD_MAX) ++wrong;
    if (phase2b_len(0, v[0], v[1], v[2], v[3]) > PHASE2B_MAX || nack_len(v[0]) > NACK_MAX) ++wrong;
  }
  return wrong;
}

int64_t emit_chosen(uint8_t* out, int32_t slot, const uint8_t* value, int32_t value_len, int32_t is_noop) {
  pick_value(value, value_len, is_noop);
  return chosen_emit(out, slot, value, value_len);
}
int64_t emit_phase2a(uint8_t* out, uint32_t wrapper, int32_t slot, int32_t round, const uint8_t* value, int32_t value_len,
                     int32_t is_noop) {
  pick_value(value, value_len, is_noop);
  return phase2a_emit(out, wrapper, slot, round, value, value_len);
}
int64_t emit_phase2b(uint8_t* out, int32_t dialect, int32_t g, int32_t a, int32_t slot, int32_t round) {
  return phase2b_emit(out, dialect, g, a, slot, round);
}
int64_t emit_nack(uint8_t* out, int32_t dialect, int32_t round) { return nack_emit(out, dialect, round); }
int64_t emit_ints(uint8_t* out, uint32_t wrapper, int32_t k, const int32_t* v) { return ints_emit(out, wrapper, k, v); }

}  // extern "C"
