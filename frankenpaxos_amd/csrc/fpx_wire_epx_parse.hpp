// fpx_wire_epx_parse.hpp -- the reader of epaxos/EPaxos.proto's ReplicaInbound (include/fpx_wire.h, the EPaxos section),
// shared by the host decoders of fpx_wire.cpp (g++) and the device decoder k_epx_wire_decode of fpx_wire_epx_dev.hpp
// (hipcc): one source for both sides, as fpx_wire_parse.hpp is for MultiPaxos.  No allocation and no containers here: what
// a message's dependencies become is the business of a SINK the parser writes through,
//   void reset()                        a member of the oneof starts: nothing of an earlier member stays behind
//   void deps_begin(const Reader& body) a `dependencies` field starts (a repeated one starts over); body = its bytes
//   void value(int leader, int32_t id)  an explicit id of column `leader`, in byte order
//   bool set(int leader, int32_t wm)    column `leader` is complete, with its watermark; false = refuse the message
// and there are three: the host decoder's vectors (fpx_wire.cpp), EpxFoldSink (fixed size: it keeps the reader of the
// last dependencies field and counts) and EpxFoldWalk, which goes over that field again once the whole member is parsed
// -- field order on the wire is free, so `dependencies` may precede the `instance` it is folded against.
#pragma once
#include "fpx_wire_parse.hpp"

#ifndef FPX_WIRE_EPX_FOLD_MAX
#define FPX_WIRE_EPX_FOLD_MAX 64
#endif

namespace fpxw {

// Instance { replica_index = 1; instance_number = 2 } / Ballot { ordering = 1; replica_index = 2 }
FPX_HD inline bool parse_pair(Reader r, int32_t* a, int32_t* b) {
  Fields f;
  if (!parse_flat(r, 0, &f) || (f.seen & 0x6) != 0x6) return false;
  *a = f.i[1], *b = f.i[2];
  return true;
}

struct EpxScalars {  // one decoded message, without its dependency sets
  int32_t kind = 0 /*FPX_WIRE_OTHER*/, il = -1, in = -1, bo = -1, br = -1, ri = -1, seq = -1, vbo = -1, vbr = -1, status = -1;
  Value cmd;
  bool has_cmd = false, has_deps = false, has_seq = false;
  int32_t num_replicas = -1;
};

// IntPrefixSetProto { watermark = 1; repeated int32 value = 2 (unpacked by ScalaPB; packed accepted too) }
template <typename Sink>
FPX_HD inline bool parse_int_prefix_set(Reader r, int leader, Sink& s) {
  bool seen_wm = false;
  int32_t wm = 0;
  while (r.more()) {
    const uint64_t tag = r.varint();
    const uint32_t field = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
    if (field == 1 && wt == 0) {
      wm = as_i32(r.varint());
      seen_wm = true;
    } else if (field == 2 && wt == 0) {
      s.value(leader, as_i32(r.varint()));
    } else if (field == 2 && wt == 2) {
      Reader p = r.sub();
      while (p.more()) s.value(leader, as_i32(p.varint()));
      if (!p.ok) return false;
    } else {
      r.skip(wt);
    }
  }
  if (!r.ok || !seen_wm) return false;
  return s.set(leader, wm);
}

// InstancePrefixSetProto { numReplicas = 1; repeated IntPrefixSetProto int_prefix_set = 2 }
template <typename Sink>
FPX_HD inline bool parse_deps(Reader r, EpxScalars* o, Sink& s) {
  bool seen_n = false;
  s.deps_begin(r);
  int leader = 0;
  while (r.more()) {
    const uint64_t tag = r.varint();
    const uint32_t field = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
    if (field == 1 && wt == 0) {
      o->num_replicas = as_i32(r.varint());
      seen_n = true;
    } else if (field == 2 && wt == 2) {
      Reader sub = r.sub();
      if (!r.ok || !parse_int_prefix_set(sub, leader++, s)) return false;
    } else {
      r.skip(wt);
    }
  }
  // InstancePrefixSet.fromProto (epaxos/InstancePrefixSet.scala:48-53) takes numReplicas and the sets as they come;
  // every producer writes exactly numReplicas of them -- anything else is refused here
  if (!r.ok || !seen_n || o->num_replicas < 0 || leader != o->num_replicas) return false;
  o->has_deps = true;
  return true;
}

// the body of one ReplicaInbound member.  layout: which field numbers carry what, per kind (0: the kind has none)
struct EpxLayout {
  int instance, ballot, command, seq, deps, replica, vote_ballot, status;
  unsigned required;  // bits of the field numbers that must be present
};
// kind: FPX_WIRE_EPX_* = the member's field number + 14; false: no such member
FPX_HD inline bool epx_layout(int32_t kind, EpxLayout* L) {
  switch (kind) {
    case 16: case 18: *L = EpxLayout{1, 2, 3, 4, 5, 0, 0, 0, 0x3e}; return true;  // PreAccept, Accept
    case 17: *L = EpxLayout{1, 2, 0, 4, 5, 3, 0, 0, 0x3e}; return true;           // PreAcceptOk
    case 19: *L = EpxLayout{2, 3, 0, 0, 0, 7, 0, 0, 0x8c}; return true;           // AcceptOk
    case 20: *L = EpxLayout{1, 0, 2, 3, 4, 0, 0, 0, 0x1e}; return true;           // Commit
    case 21: case 23: *L = EpxLayout{1, 2, 0, 0, 0, 0, 0, 0, 0x6}; return true;   // Prepare, Nack
    case 22: *L = EpxLayout{2, 1, 6, 7, 8, 3, 4, 5, 0x3e}; return true;           // PrepareOk
  }
  return false;
}

template <typename Sink>
FPX_HD inline bool parse_epx_member(Reader r, int32_t kind, EpxScalars* o, Sink& s) {
  EpxLayout L;
  if (!epx_layout(kind, &L)) return false;
  unsigned seen = 0;
  o->kind = kind;
  while (r.more()) {
    const uint64_t tag = r.varint();
    const int field = (int)(tag >> 3);
    const uint32_t wt = (uint32_t)(tag & 7);
    bool known = true;
    if (field == 0) return false;  // no such field (a layout entry of 0 means "this kind has none": never a match)
    if (field == L.instance && wt == 2) {
      if (!parse_pair(r.sub(), &o->il, &o->in)) return false;
    } else if (field == L.ballot && wt == 2) {
      if (!parse_pair(r.sub(), &o->bo, &o->br)) return false;
    } else if (field == L.vote_ballot && wt == 2) {
      if (!parse_pair(r.sub(), &o->vbo, &o->vbr)) return false;
    } else if (field == L.command && wt == 2) {
      Reader sub = r.sub();
      if (!r.ok || !parse_value(sub, &o->cmd)) return false;
      o->has_cmd = true;
    } else if (field == L.deps && wt == 2) {
      Reader sub = r.sub();
      if (!r.ok || !parse_deps(sub, o, s)) return false;
    } else if (field == L.seq && wt == 0) {
      o->seq = as_i32(r.varint());
      o->has_seq = true;
    } else if (field == L.replica && wt == 0) {
      o->ri = as_i32(r.varint());
    } else if (field == L.status && wt == 0) {
      o->status = as_i32(r.varint());
    } else {
      known = false;
      r.skip(wt);
    }
    if (known && field < 32) seen |= 1u << field;
    if (!r.ok) return false;
  }
  return r.ok && (seen & L.required) == L.required;
}

// ReplicaInbound { oneof request { ClientRequest = 1 (left to the JVM actor: kind stays OTHER); members 2 - 9 } }
template <typename Sink>
FPX_HD inline bool parse_epx_replica_inbound(Reader r, EpxScalars* o, Sink& s) {
  *o = EpxScalars();
  s.reset();
  while (r.more()) {  // the last member of the oneof that is present wins
    const uint64_t tag = r.varint();
    const uint32_t field = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
    if (field >= 2 && field <= 9 && wt == 2) {
      Reader sub = r.sub();
      *o = EpxScalars();
      s.reset();
      if (!r.ok || !parse_epx_member(sub, (int32_t)field + 14, o, s)) return false;
    } else {
      r.skip(wt);
    }
  }
  return r.ok;
}

// ---- the folded form: fixed-size state, what the device runs -----------------------------------------------------------
// first pass: where the dependencies of the member that wins lie, how many sets and explicit-id entries they hold
struct EpxFoldSink {
  int32_t max_sets;
  Reader deps{nullptr, nullptr};
  int32_t sets = 0, entries = 0;
  FPX_HD void reset() { deps = Reader{nullptr, nullptr}, sets = 0, entries = 0; }
  FPX_HD void deps_begin(const Reader& body) { deps = body, sets = 0, entries = 0; }
  FPX_HD void value(int, int32_t) {
    if (entries <= FPX_WIRE_EPX_FOLD_MAX) ++entries;  // (more than the cap is all the fold asks)
  }
  FPX_HD bool set(int, int32_t) { return ++sets <= max_sets; }  // more sets than the caller's rows hold: malformed
};

// second pass over bytes the first one accepted, the instance known: the watermark row, and the own-leader column's ids
// as a 64-bit set relative to instance_number + 1
struct EpxFoldWalk {
  int32_t il, in, max_sets;
  int32_t* row;  // may be null
  int32_t own_wm = 0, own_max = 0;
  uint64_t mask = 0;
  bool own_any = false, foreign = false, off = false;  // off: an id outside instance_number + 1 .. + 64
  FPX_HD void reset() {}
  FPX_HD void deps_begin(const Reader&) {}
  FPX_HD void value(int leader, int32_t id) {
    if (leader != il) {
      foreign = true;
      return;
    }
    if (!own_any || id > own_max) own_max = id;
    own_any = true;
    const int64_t d = (int64_t)id - in - 1;
    if (d < 0 || d >= 64) off = true;
    else mask |= 1ull << d;
  }
  FPX_HD bool set(int leader, int32_t wm) {
    if (row && leader < max_sets) row[leader] = wm;
    if (leader == il) own_wm = wm;
    return true;
  }
};

struct EpxFoldOut {  // every array but kind may be null
  int32_t *kind, *il, *in, *bo, *br, *ri, *seq, *vbo, *vbr, *status, *is_noop;
  int64_t* cmd_off;
  int32_t *cmd_len, *nr, *wm, *dend, *shape;
};

// message i = the bytes of r, into row i of the arrays; false: malformed (the arrays then hold the values of an empty
// message).  num_replicas: the row length of o.wm and the most sets a message may have.
FPX_HD inline bool epx_decode_folded(const uint8_t* base, Reader r, int32_t i, int32_t num_replicas, const EpxFoldOut& o) {
  EpxScalars m;
  EpxFoldSink s;
  s.max_sets = num_replicas;
  const bool ok = parse_epx_replica_inbound(r, &m, s);
  if (!ok) m = EpxScalars();
  o.kind[i] = m.kind;
  if (o.il) o.il[i] = m.il;
  if (o.in) o.in[i] = m.in;
  if (o.bo) o.bo[i] = m.bo;
  if (o.br) o.br[i] = m.br;
  if (o.ri) o.ri[i] = m.ri;
  if (o.seq) o.seq[i] = m.has_seq ? m.seq : -1;
  if (o.vbo) o.vbo[i] = m.vbo;
  if (o.vbr) o.vbr[i] = m.vbr;
  if (o.status) o.status[i] = m.status;
  if (o.is_noop) o.is_noop[i] = m.has_cmd ? m.cmd.is_noop : -1;
  if (o.cmd_off) o.cmd_off[i] = m.has_cmd ? m.cmd.at - base : -1;
  if (o.cmd_len) o.cmd_len[i] = m.has_cmd ? m.cmd.len : -1;
  if (o.nr) o.nr[i] = m.has_deps ? m.num_replicas : -1;
  int32_t* row = o.wm ? o.wm + (size_t)i * num_replicas : nullptr;
  int32_t end = 0, shape = -1, sets = 0;
  if (m.has_deps) {
    EpxFoldWalk w;
    w.il = m.il, w.in = m.in, w.max_sets = num_replicas, w.row = row;
    EpxScalars again;
    (void)parse_deps(s.deps, &again, w);
    sets = s.sets;
    end = w.own_any ? (int32_t)((uint32_t)w.own_max + 1u) : 0;
    bool form = !w.foreign && s.entries <= FPX_WIRE_EPX_FOLD_MAX && m.il >= 0 && m.il < sets;
    if (form && w.own_any) {
      const int64_t k = (int64_t)w.own_max - m.in;  // 1 .. 64 unless w.off
      form = !w.off && w.own_wm <= m.in && w.mask == (k >= 64 ? ~0ull : (1ull << k) - 1ull);
    }
    shape = form ? 1 : 0;
  }
  if (row)
    for (int l = sets; l < num_replicas; ++l) row[l] = 0;
  if (o.dend) o.dend[i] = end;
  if (o.shape) o.shape[i] = shape;
  return ok;
}

}  // namespace fpxw
