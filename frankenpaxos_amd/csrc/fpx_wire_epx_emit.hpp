// fpx_wire_epx_emit.hpp -- the protobuf WRITER of the replies an EPaxos replica sends (include/fpx_wire.h,
// fpx_wire_epx_encode_replica_replies[_dev]), shared by the host batch encoder of fpx_wire.cpp (g++) and the device encoder
// of fpx_wire_epx_enc_dev.hpp (hipcc): one source for both, as fpx_wire_emit.hpp is for MultiPaxos and Mencius.  The four
// replies that carry no command bytes, under ReplicaInbound's oneof (EPaxos.proto, field numbers in include/fpx_wire.h):
//   PreAcceptOk { instance = 1; ballot = 2; replica_index = 3; sequence_number = 4; dependencies = 5 }      wrapper field 3
//   AcceptOk    { instance = 2; ballot = 3; replica_index = 7 }                                             wrapper field 5
//   PrepareOk   { ballot = 1; instance = 2; replica_index = 3; vote_ballot = 4; status = 5 }  (NotSeen)     wrapper field 8
//   Nack        { instance = 1; largest_ballot = 2 }                                                        wrapper field 9
// and the two that carry the stored triple's CommandOrNoop, when the caller gives a command source (EpxCmdSource: the
// command store of csrc/fpx_epx_cmds.hpp, or plain host arrays):
//   Commit      { instance = 1; command_or_noop = 2; sequence_number = 3 (0); dependencies = 4 }              wrapper field 6
//   PrepareOk   { ballot = 1; instance = 2; replica_index = 3; vote_ballot = 4; status = 5 (PreAccepted 1 / Accepted 2);
//                 command_or_noop = 6; sequence_number = 7 (0); dependencies = 8 }                            wrapper field 8
// The bytes are, field for field, what fpx_wire_epaxos_encode_replica_inbound writes for the same message: that function
// stays the yardstick (tests/test_epaxos_reply_encode_cpu.py, tests/test_epaxos_cmd_reply_encode_cpu.py).  ONE *_len and ONE
// *_emit per layout, the Writer of fpx_wire_emit.hpp, no allocation.  A reply with a command is emitted AROUND it: the
// emitter writes the fields in front of and behind the command and says where the command's bytes go; who copies them is
// the caller's business (memcpy on the host, the whole wavefront on the device).
//
// Which record of a replica tick becomes which reply is decided here too (epx_reply_plan), so the two sides cannot
// disagree about it either.
#pragma once
#include <stdint.h>

#include "fpx_wire_emit.hpp"

namespace fpxw {

// Instance { replica_index = 1; instance_number = 2 } / Ballot { ordering = 1; replica_index = 2 } as field `field`
FPX_HD inline int64_t epx_pair_len(int32_t a, int32_t b) {
  const int64_t body = i32_len(a) + i32_len(b);  // at most 22: its length is one byte
  return 2 + body;
}
FPX_HD inline void epx_pair_emit(Writer& w, uint32_t field, int32_t a, int32_t b) {
  w.tag(field, 2);
  w.varint((uint64_t)(i32_len(a) + i32_len(b)));
  w.i32(1, a);
  w.i32(2, b);
}

// The bytes of `repeated int32 value = 2` for the ids lo .. hi - 1 (proto2, not packed: one tag byte and a varint each), in
// closed form.  A non-negative int32 v takes 1 + #{k in 1..4 : v >= 2^(7k)} varint bytes, so the ids below x >= 0 take
// S(x) = 2 x + sum_k max(0, x - 2^(7k)) bytes and a run takes S(hi) - S(lo); an id below zero is a ten-byte varint.
FPX_HD inline int64_t epx_ids_below(int64_t x) {
  if (x <= 0) return 0;
  int64_t s = 2 * x;
  s += x > (1 << 7) ? x - (1 << 7) : 0;
  s += x > (1 << 14) ? x - (1 << 14) : 0;
  s += x > (1 << 21) ? x - (1 << 21) : 0;
  s += x > (1 << 28) ? x - (1 << 28) : 0;
  return s;
}
FPX_HD inline int64_t epx_id_run_len(int64_t lo, int64_t hi) {
  if (hi <= lo) return 0;
  const int64_t neg_end = hi < 0 ? hi : 0;
  return (lo < neg_end ? (neg_end - lo) * 11 : 0) + epx_ids_below(hi) - epx_ids_below(lo);
}

// the explicit ids of the own-leader column: number + 1 .. values_end - 1 when values_end > 0 (EPaxosNative.scala,
// prefixSet), else none
FPX_HD inline int64_t epx_own_ids(int32_t number, int32_t values_end) {
  const int64_t cnt = (int64_t)values_end - ((int64_t)number + 1);
  return values_end > 0 && cnt > 0 ? cnt : 0;
}

// InstancePrefixSetProto { numReplicas = 1; n x IntPrefixSetProto { watermark = 1; value = 2 ... } = 2 }: the body's length;
// *own_set (may be null) = the length of the own-leader column's IntPrefixSetProto
FPX_HD inline int64_t epx_deps_len(int32_t n, const int32_t* w, int32_t own, int32_t number, int32_t values_end,
                                   int64_t* own_set) {
  int64_t body = i32_len(n);
  for (int32_t l = 0; l < n; ++l) {
    int64_t set = i32_len(w[l]);
    if (l == own) {
      const int64_t ids = epx_own_ids(number, values_end);
      set += epx_id_run_len((int64_t)number + 1, (int64_t)number + 1 + ids);
      if (own_set) *own_set = set;
    }
    body += 1 + varint_len((uint64_t)set) + set;
  }
  return body;
}

// the same as field `field`: deps and own_set are what epx_deps_len gave
FPX_HD inline void epx_deps_emit(Writer& w, uint32_t field, int32_t n, const int32_t* wm, int32_t own, int32_t number,
                                 int32_t values_end, int64_t deps, int64_t own_set) {
  w.tag(field, 2);
  w.varint((uint64_t)deps);
  w.i32(1, n);
  const int64_t ids = epx_own_ids(number, values_end);
  for (int32_t l = 0; l < n; ++l) {
    w.tag(2, 2);
    w.varint((uint64_t)(l == own ? own_set : i32_len(wm[l])));
    w.i32(1, wm[l]);
    if (l == own)
      for (int64_t k = 0; k < ids; ++k) w.i32(2, (int32_t)((int64_t)number + 1 + k));
  }
}

// ---- PreAcceptOk(instance, ballot, replica_index, 0, dependencies) ---------------------------------------------------------
struct EpxPreAcceptOk {
  int32_t n, leader, number, b_ord, b_rep, replica_index;
  const int32_t* w;  // n watermarks
  int32_t values_end;
};
FPX_HD inline int64_t epx_pre_accept_ok_inner(const EpxPreAcceptOk& m, int64_t* deps, int64_t* own_set) {
  *deps = epx_deps_len(m.n, m.w, m.leader, m.number, m.values_end, own_set);
  return epx_pair_len(m.leader, m.number) + epx_pair_len(m.b_ord, m.b_rep) + i32_len(m.replica_index) + i32_len(0) + 1 +
         varint_len((uint64_t)*deps) + *deps;
}
FPX_HD inline int64_t epx_pre_accept_ok_len(const EpxPreAcceptOk& m) {
  int64_t deps, own_set;
  return wrapped_len(epx_pre_accept_ok_inner(m, &deps, &own_set));
}
FPX_HD inline int64_t epx_pre_accept_ok_emit(uint8_t* out, const EpxPreAcceptOk& m) {
  int64_t deps, own_set = 0;
  const int64_t inner = epx_pre_accept_ok_inner(m, &deps, &own_set);
  Writer w{out};
  w.tag(3, 2);
  w.varint((uint64_t)inner);
  epx_pair_emit(w, 1, m.leader, m.number);
  epx_pair_emit(w, 2, m.b_ord, m.b_rep);
  w.i32(3, m.replica_index);
  w.i32(4, 0);
  epx_deps_emit(w, 5, m.n, m.w, m.leader, m.number, m.values_end, deps, own_set);
  return w.n;
}

// ---- AcceptOk(instance, ballot, replica_index) ------------------------------------------------------------------------------
FPX_HD inline int64_t epx_accept_ok_len(int32_t leader, int32_t number, int32_t b_ord, int32_t b_rep, int32_t replica_index) {
  return wrapped_len(epx_pair_len(leader, number) + epx_pair_len(b_ord, b_rep) + i32_len(replica_index));
}
FPX_HD inline int64_t epx_accept_ok_emit(uint8_t* out, int32_t leader, int32_t number, int32_t b_ord, int32_t b_rep,
                                         int32_t replica_index) {
  Writer w{out};
  w.tag(5, 2);
  w.varint((uint64_t)(epx_pair_len(leader, number) + epx_pair_len(b_ord, b_rep) + i32_len(replica_index)));
  epx_pair_emit(w, 2, leader, number);
  epx_pair_emit(w, 3, b_ord, b_rep);
  w.i32(7, replica_index);
  return w.n;
}

// ---- Nack(instance, largest_ballot) -----------------------------------------------------------------------------------------
FPX_HD inline int64_t epx_nack_len(int32_t leader, int32_t number, int32_t l_ord, int32_t l_rep) {
  return wrapped_len(epx_pair_len(leader, number) + epx_pair_len(l_ord, l_rep));
}
FPX_HD inline int64_t epx_nack_emit(uint8_t* out, int32_t leader, int32_t number, int32_t l_ord, int32_t l_rep) {
  Writer w{out};
  w.tag(9, 2);
  w.varint((uint64_t)(epx_pair_len(leader, number) + epx_pair_len(l_ord, l_rep)));
  epx_pair_emit(w, 1, leader, number);
  epx_pair_emit(w, 2, l_ord, l_rep);
  return w.n;
}

// ---- PrepareOk of status NotSeen: none of the three optional fields ---------------------------------------------------------
FPX_HD inline int64_t epx_prepare_ok_len(int32_t b_ord, int32_t b_rep, int32_t leader, int32_t number, int32_t replica_index,
                                         int32_t v_ord, int32_t v_rep) {
  return wrapped_len(epx_pair_len(b_ord, b_rep) + epx_pair_len(leader, number) + i32_len(replica_index) +
                     epx_pair_len(v_ord, v_rep) + i32_len(0));
}
FPX_HD inline int64_t epx_prepare_ok_emit(uint8_t* out, int32_t b_ord, int32_t b_rep, int32_t leader, int32_t number,
                                          int32_t replica_index, int32_t v_ord, int32_t v_rep) {
  Writer w{out};
  w.tag(8, 2);
  w.varint((uint64_t)(epx_pair_len(b_ord, b_rep) + epx_pair_len(leader, number) + i32_len(replica_index) +
                      epx_pair_len(v_ord, v_rep) + i32_len(0)));
  epx_pair_emit(w, 1, b_ord, b_rep);
  epx_pair_emit(w, 2, leader, number);
  w.i32(3, replica_index);
  epx_pair_emit(w, 4, v_ord, v_rep);
  w.i32(5, 0);
  return w.n;
}

// ---- the two replies around a stored CommandOrNoop of cmd_len bytes ------------------------------------------------------
// *_emit writes everything but the command and returns the whole length; *cmd_at = where the command's bytes go
struct EpxCmdReply {
  int32_t n, leader, number;
  const int32_t* w;  // n watermarks
  int32_t values_end;
  int32_t cmd_len;
  // PrepareOk alone: the message's ballot, the replica that answers, its vote ballot, the wire status
  int32_t b_ord, b_rep, replica_index, v_ord, v_rep, status;
};
FPX_HD inline int64_t epx_cmd_field_len(int32_t cmd_len) { return 1 + varint_len((uint64_t)cmd_len) + cmd_len; }
FPX_HD inline int64_t epx_commit_inner(const EpxCmdReply& m, int64_t* deps, int64_t* own_set) {
  *deps = epx_deps_len(m.n, m.w, m.leader, m.number, m.values_end, own_set);
  return epx_pair_len(m.leader, m.number) + epx_cmd_field_len(m.cmd_len) + i32_len(0) + 1 + varint_len((uint64_t)*deps) + *deps;
}
FPX_HD inline int64_t epx_commit_len(const EpxCmdReply& m) {
  int64_t deps, own_set;
  return wrapped_len(epx_commit_inner(m, &deps, &own_set));
}
FPX_HD inline int64_t epx_commit_emit(uint8_t* out, const EpxCmdReply& m, int64_t* cmd_at) {
  int64_t deps, own_set = 0;
  const int64_t inner = epx_commit_inner(m, &deps, &own_set);
  Writer w{out};
  w.tag(6, 2);
  w.varint((uint64_t)inner);
  epx_pair_emit(w, 1, m.leader, m.number);
  w.tag(2, 2);
  w.varint((uint64_t)m.cmd_len);
  *cmd_at = w.n, w.n += m.cmd_len;
  w.i32(3, 0);
  epx_deps_emit(w, 4, m.n, m.w, m.leader, m.number, m.values_end, deps, own_set);
  return w.n;
}
FPX_HD inline int64_t epx_prepare_ok_cmd_inner(const EpxCmdReply& m, int64_t* deps, int64_t* own_set) {
  *deps = epx_deps_len(m.n, m.w, m.leader, m.number, m.values_end, own_set);
  return epx_pair_len(m.b_ord, m.b_rep) + epx_pair_len(m.leader, m.number) + i32_len(m.replica_index) +
         epx_pair_len(m.v_ord, m.v_rep) + i32_len(m.status) + epx_cmd_field_len(m.cmd_len) + i32_len(0) + 1 +
         varint_len((uint64_t)*deps) + *deps;
}
FPX_HD inline int64_t epx_prepare_ok_cmd_len(const EpxCmdReply& m) {
  int64_t deps, own_set;
  return wrapped_len(epx_prepare_ok_cmd_inner(m, &deps, &own_set));
}
FPX_HD inline int64_t epx_prepare_ok_cmd_emit(uint8_t* out, const EpxCmdReply& m, int64_t* cmd_at) {
  int64_t deps, own_set = 0;
  const int64_t inner = epx_prepare_ok_cmd_inner(m, &deps, &own_set);
  Writer w{out};
  w.tag(8, 2);
  w.varint((uint64_t)inner);
  epx_pair_emit(w, 1, m.b_ord, m.b_rep);
  epx_pair_emit(w, 2, m.leader, m.number);
  w.i32(3, m.replica_index);
  epx_pair_emit(w, 4, m.v_ord, m.v_rep);
  w.i32(5, m.status);
  w.tag(6, 2);
  w.varint((uint64_t)m.cmd_len);
  *cmd_at = w.n, w.n += m.cmd_len;
  w.i32(7, 0);
  epx_deps_emit(w, 8, m.n, m.w, m.leader, m.number, m.values_end, deps, own_set);
  return w.n;
}

// ---- a replica tick's records -> replies --------------------------------------------------------------------------------------
// The decoded messages (to, leader, number, the message's ballot) and what fpx_epx_replica_inbox[_mk] answered (include/fpx.h,
// FPX_EPX_RI_*).  reply kinds: 0 none, 1 encoded here, 2 deferred to the caller (it holds the command bytes, or the
// dependencies of a triple stored by id; or the own column has more than EPX_REPLY_IDS_MAX explicit ids, the folded decoder's
// cap, which bounds one thread's work); EPX_REPLY_UNKNOWN: an outcome outside 0 .. 8.
// With a command source (cmds.off not null) and out_triple, a COMMIT_BACK and a PREPARE_OK of out_status 2 / 3 are encoded
// too when the triple's bytes are in the source, the dependencies are in out_deps (out_deps[i * n] >= 0) and the own column
// has at most EPX_REPLY_IDS_MAX explicit ids; without a source the plan is what it was.
constexpr int EPX_REPLY_NONE = 0, EPX_REPLY_ENCODED = 1, EPX_REPLY_DEFERRED = 2, EPX_REPLY_UNKNOWN = -1;
constexpr int EPX_REPLY_IDS_MAX = 64;  // FPX_WIRE_EPX_FOLD_MAX
// where the triples' serialised CommandOrNoops lie: triple t's bytes are arena[off[t] .. off[t] + len[t]), off[t] < 0 = none
struct EpxCmdSource {
  const int64_t* off = nullptr;  // [max_triples]; null: no source
  const int32_t* len = nullptr;  // [max_triples]
  const uint8_t* arena = nullptr;
  int32_t max_triples = 0;
};
struct EpxReplyIn {
  int32_t n;
  const int32_t *to, *leader, *number, *b_ord, *b_rep;
  const int32_t *outcome, *out_ballot, *out_status, *out_deps, *out_end;
  const int32_t* out_triple = nullptr;  // read only with a source
  EpxCmdSource cmds = {};
};
struct EpxReplyPlan {
  int32_t kind;     // EPX_REPLY_*
  int32_t outcome;
  int64_t len;      // bytes: 0 unless kind is EPX_REPLY_ENCODED
  int32_t cmd_len = -1;  // >= 0: the reply carries that many bytes of a stored command, arena[cmd_off ..)
  int64_t cmd_off = -1;
};
FPX_HD inline EpxPreAcceptOk epx_reply_pre_accept_ok(const EpxReplyIn& a, int32_t i) {
  return EpxPreAcceptOk{a.n,       a.leader[i], a.number[i], a.b_ord[i], a.b_rep[i], a.to[i], a.out_deps + (size_t)i * (size_t)a.n,
                        a.out_end[i]};
}
FPX_HD inline void epx_reply_ballot(int32_t encoded, int32_t* ord, int32_t* rep) {
  if (encoded < 0) *ord = *rep = -1;  // the reference's nullBallot
  else *ord = encoded >> 3, *rep = encoded & 7;
}
// the stored command of record i's triple, when the reply can carry it (above)
FPX_HD inline bool epx_reply_cmd(const EpxReplyIn& a, int32_t i, EpxReplyPlan* p) {
  if (!a.cmds.off || !a.out_triple) return false;
  const int32_t t = a.out_triple[i];
  if (t < 0 || t >= a.cmds.max_triples || a.cmds.off[t] < 0) return false;
  if (a.out_deps[(size_t)i * (size_t)a.n] < 0 || epx_own_ids(a.number[i], a.out_end[i]) > EPX_REPLY_IDS_MAX) return false;
  p->cmd_off = a.cmds.off[t], p->cmd_len = a.cmds.len[t];
  return true;
}
FPX_HD inline EpxCmdReply epx_reply_cmd_reply(const EpxReplyIn& a, int32_t i, int32_t cmd_len) {
  EpxCmdReply m{a.n, a.leader[i], a.number[i], a.out_deps + (size_t)i * (size_t)a.n, a.out_end[i], cmd_len, 0, 0, 0, 0, 0, 0};
  if (a.outcome[i] == 6) {
    m.b_ord = a.b_ord[i], m.b_rep = a.b_rep[i], m.replica_index = a.to[i], m.status = a.out_status[i] - 1;
    epx_reply_ballot(a.out_ballot[i], &m.v_ord, &m.v_rep);
  }
  return m;
}
FPX_HD inline EpxReplyPlan epx_reply_plan(const EpxReplyIn& a, int32_t i) {
  EpxReplyPlan p{EPX_REPLY_NONE, a.outcome[i], 0};
  int32_t ord, rep;
  switch (p.outcome) {
    case 0: case 5: break;
    case 1: case 2:
      if (a.out_deps[(size_t)i * (size_t)a.n] < 0 || epx_own_ids(a.number[i], a.out_end[i]) > EPX_REPLY_IDS_MAX) {
        p.kind = EPX_REPLY_DEFERRED;
      } else {
        p.kind = EPX_REPLY_ENCODED;
        p.len = epx_pre_accept_ok_len(epx_reply_pre_accept_ok(a, i));
      }
      break;
    case 3: case 4:
      p.kind = EPX_REPLY_ENCODED;
      p.len = epx_accept_ok_len(a.leader[i], a.number[i], a.b_ord[i], a.b_rep[i], a.to[i]);
      break;
    case 6:
      if ((a.out_status[i] == 2 || a.out_status[i] == 3) && epx_reply_cmd(a, i, &p)) {
        p.kind = EPX_REPLY_ENCODED;
        p.len = epx_prepare_ok_cmd_len(epx_reply_cmd_reply(a, i, p.cmd_len));
      } else if (a.out_status[i] != 0) {
        p.kind = EPX_REPLY_DEFERRED;
      } else {
        epx_reply_ballot(a.out_ballot[i], &ord, &rep);
        p.kind = EPX_REPLY_ENCODED;
        p.len = epx_prepare_ok_len(a.b_ord[i], a.b_rep[i], a.leader[i], a.number[i], a.to[i], ord, rep);
      }
      break;
    case 7:
      p.kind = EPX_REPLY_ENCODED;
      p.len = epx_nack_len(a.leader[i], a.number[i], a.out_ballot[i] >> 3, a.out_ballot[i] & 7);
      break;
    case 8:
      if (epx_reply_cmd(a, i, &p)) {
        p.kind = EPX_REPLY_ENCODED;
        p.len = epx_commit_len(epx_reply_cmd_reply(a, i, p.cmd_len));
      } else {
        p.kind = EPX_REPLY_DEFERRED;
      }
      break;
    default: p.kind = EPX_REPLY_UNKNOWN; break;
  }
  return p;
}
// writes the reply of a record whose plan is EPX_REPLY_ENCODED and has no command; returns its length (= the plan's)
FPX_HD inline int64_t epx_reply_emit(uint8_t* out, const EpxReplyIn& a, int32_t i, int32_t outcome) {
  int32_t ord, rep;
  switch (outcome) {
    case 1: case 2: return epx_pre_accept_ok_emit(out, epx_reply_pre_accept_ok(a, i));
    case 3: case 4: return epx_accept_ok_emit(out, a.leader[i], a.number[i], a.b_ord[i], a.b_rep[i], a.to[i]);
    case 6:
      epx_reply_ballot(a.out_ballot[i], &ord, &rep);
      return epx_prepare_ok_emit(out, a.b_ord[i], a.b_rep[i], a.leader[i], a.number[i], a.to[i], ord, rep);
    case 7: return epx_nack_emit(out, a.leader[i], a.number[i], a.out_ballot[i] >> 3, a.out_ballot[i] & 7);
  }
  return 0;
}
// the same for a plan with a command (cmd_len >= 0): everything but the command's bytes, which go to out + *cmd_at
FPX_HD inline int64_t epx_reply_emit_around(uint8_t* out, const EpxReplyIn& a, int32_t i, const EpxReplyPlan& p, int64_t* cmd_at) {
  const EpxCmdReply m = epx_reply_cmd_reply(a, i, p.cmd_len);
  return p.outcome == 6 ? epx_prepare_ok_cmd_emit(out, m, cmd_at) : epx_commit_emit(out, m, cmd_at);
}

}  // namespace fpxw
