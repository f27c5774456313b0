// fpx_wire_emit.hpp -- the protobuf WRITER of the wire adapter (include/fpx_wire.h), shared by the host encoders of
// fpx_wire.cpp (g++) and the device encoders of fpx_wire_enc_dev.hpp (hipcc): one source for both, as
// fpx_wire_parse.hpp is for the reader, so a record encodes to the same bytes whichever side writes it.  Canonical
// proto2 as ScalaPB's toByteArray writes it: fields in number order, required fields always present, int32 as a varint
// with negative values sign-extended to ten bytes.
//
// Every message layout has ONE *_len function (the bytes the message takes) and ONE *_emit function (writes them,
// returns how many): tests/test_wire_emit.py holds the two equal on every varint boundary.
#pragma once
#include <stdint.h>

#include "fpx_wire_parse.hpp"  // FPX_HD

namespace fpxw {

struct Writer {
  uint8_t* p;  // null: only count
  int64_t n = 0;
  FPX_HD void byte(uint8_t b) {
    if (p) p[n] = b;
    ++n;
  }
  FPX_HD void varint(uint64_t v) {
    while (v >= 0x80) {
      byte((uint8_t)(v | 0x80));
      v >>= 7;
    }
    byte((uint8_t)v);
  }
  FPX_HD void tag(uint32_t field, uint32_t wt) { varint(((uint64_t)field << 3) | wt); }
  FPX_HD void i32(uint32_t field, int32_t v) {
    tag(field, 0);
    varint((uint64_t)(int64_t)v);  // negative: sign-extended, 10 bytes (protobuf int32)
  }
  FPX_HD void bytes(const uint8_t* src, int64_t len) {
    if (p)
      for (int64_t k = 0; k < len; ++k) p[n + k] = src[k];
    n += len;
  }
};

FPX_HD inline int64_t varint_len(uint64_t v) {
  int64_t k = 1;
  while (v >= 0x80) v >>= 7, ++k;
  return k;
}
FPX_HD inline int64_t i32_len(int32_t v) { return 1 + varint_len((uint64_t)(int64_t)v); }  // fields 1..15: one tag byte

// `inner` bytes as a length-delimited field (number 1..15) of an ...Inbound message
FPX_HD inline int64_t wrapped_len(int64_t inner) { return 1 + varint_len((uint64_t)inner) + inner; }

// the CommandBatchOrNoop body to embed: the caller's bytes, or {noop = 2: empty Noop} = 12 00.  (Host only: it hands out
// the address of a host constant; the device encoder appends the same two bytes to the head it emits.)
static const uint8_t NOOP_VALUE[2] = {0x12, 0x00};
inline void pick_value(const uint8_t*& value, int32_t& len, int32_t is_noop) {
  if (is_noop) value = NOOP_VALUE, len = 2;
  if (len < 0) len = 0;
}

// wraps `inner_len` bytes produced by `emit` as field `wrapper_field` (length-delimited) of an ...Inbound message:
// the host encoders' return convention (the length, or the negated length needed when cap is too small)
template <typename F>
FPX_HD inline int64_t wrapped(uint8_t* out, int64_t cap, uint32_t wrapper_field, int64_t inner_len, F emit) {
  const int64_t total = wrapped_len(inner_len);
  if (total > cap || !out) return -total;
  Writer w{out};
  w.tag(wrapper_field, 2);
  w.varint((uint64_t)inner_len);
  emit(w);
  return w.n;
}

// ---- the layouts ---------------------------------------------------------------------------------------------
// k int32 fields numbered 1 .. k under wrapper field `wrapper`: Phase1a, Phase2b, Nack, the noop ranges, BatchMaxSlotReply
FPX_HD inline int64_t ints_len(int k, const int32_t* v) {
  int64_t inner = 0;
  for (int j = 0; j < k; ++j) inner += i32_len(v[j]);
  return wrapped_len(inner);
}
FPX_HD inline int64_t ints_emit(uint8_t* out, uint32_t wrapper, int k, const int32_t* v) {
  int64_t inner = 0;
  for (int j = 0; j < k; ++j) inner += i32_len(v[j]);
  Writer w{out};
  w.tag(wrapper, 2);
  w.varint((uint64_t)inner);
  for (int j = 0; j < k; ++j) w.i32((uint32_t)j + 1, v[j]);
  return w.n;
}

// Phase2a { slot = 1; round = 2; command_batch_or_noop = 3 } under `wrapper`; value / value_len after pick_value
FPX_HD inline int64_t phase2a_len(int32_t slot, int32_t round, int32_t value_len) {
  return wrapped_len(i32_len(slot) + i32_len(round) + 1 + varint_len((uint64_t)value_len) + value_len);
}
FPX_HD inline int64_t phase2a_emit(uint8_t* out, uint32_t wrapper, int32_t slot, int32_t round, const uint8_t* value,
                                   int32_t value_len) {
  Writer w{out};
  w.tag(wrapper, 2);
  w.varint((uint64_t)(i32_len(slot) + i32_len(round) + 1 + varint_len((uint64_t)value_len) + value_len));
  w.i32(1, slot);
  w.i32(2, round);
  w.tag(3, 2);
  w.varint((uint64_t)value_len);
  w.bytes(value, value_len);
  return w.n;
}

// ReplicaInbound { Chosen { slot = 1; command_batch_or_noop = 2 } = 1 }, the same in MultiPaxos.proto and Mencius.proto.
// The message is a head of 6 .. CHOSEN_HEAD_MAX bytes in front of the value's bytes: chosen_emit with value == nullptr
// writes the head alone (the device encoder splices the value in from where the decoder found it).
constexpr int CHOSEN_HEAD_MAX = 1 + 5 + 11 + 1 + 5;
FPX_HD inline int64_t chosen_len(int32_t slot, int32_t value_len) {
  return wrapped_len(i32_len(slot) + 1 + varint_len((uint64_t)value_len) + value_len);
}
FPX_HD inline int64_t chosen_emit(uint8_t* out, int32_t slot, const uint8_t* value, int32_t value_len) {
  Writer w{out};
  w.tag(1, 2);
  w.varint((uint64_t)(i32_len(slot) + 1 + varint_len((uint64_t)value_len) + value_len));
  w.i32(1, slot);
  w.tag(2, 2);
  w.varint((uint64_t)value_len);
  if (value) w.bytes(value, value_len);
  return w.n;
}

// dialect: which .proto's layout (FPX_WIRE_MULTIPAXOS = 0 / FPX_WIRE_MENCIUS = 1 of include/fpx_wire.h)
// ProxyLeaderInbound { Phase2b }: MultiPaxos (group_index, acceptor_index, slot, round) under field 2,
// Mencius (acceptor_index, slot, round) under field 4
constexpr int PHASE2B_MAX = 2 + 4 * 11;
FPX_HD inline int64_t phase2b_len(int dialect, int32_t g, int32_t a, int32_t slot, int32_t round) {
  return wrapped_len((dialect ? 0 : i32_len(g)) + i32_len(a) + i32_len(slot) + i32_len(round));
}
FPX_HD inline int64_t phase2b_emit(uint8_t* out, int dialect, int32_t g, int32_t a, int32_t slot, int32_t round) {
  const int32_t v[4] = {g, a, slot, round};
  return dialect ? ints_emit(out, 4, 3, v + 1) : ints_emit(out, 2, 4, v);
}

// LeaderInbound { Nack { round = 1 } }: field 6 (MultiPaxos) / 7 (Mencius)
constexpr int NACK_MAX = 2 + 11;
FPX_HD inline int64_t nack_len(int32_t round) { return wrapped_len(i32_len(round)); }
FPX_HD inline int64_t nack_emit(uint8_t* out, int dialect, int32_t round) { return ints_emit(out, dialect ? 7 : 6, 1, &round); }

}  // namespace fpxw
