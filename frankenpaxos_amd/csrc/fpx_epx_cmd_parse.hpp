// fpx_epx_cmd_parse.hpp -- the key list of an EPaxos command, read from the serialised CommandOrNoop that the ReplicaInbound
// decoders locate (cmd_off / cmd_len; fpx_wire_epx_parse.hpp).  One source for the host classify of fpx_wire.cpp (g++) and
// the device classify of fpx_wire_epx_dev.hpp (hipcc), as the other parser headers are; no allocation, no containers: the
// keys go to a SINK,
//   void key(int32_t j, const uint8_t* at, int32_t len)   the j-th key of the command, in wire order
// It stands in for what EPaxosNative.scala's classify does with KeyValueStoreInput.parseFrom.
//
//   CommandOrNoop { oneof value { Command command = 1; Noop noop = 2 } }                      epaxos/EPaxos.proto:61-89
//   Command { client_address = 1 (bytes); client_pseudonym = 2; client_id = 3; command = 4 (bytes) }  all four required
//   KeyValueStoreInput { oneof request { GetRequest get_request = 1; SetRequest set_request = 2 } }
//   GetRequest { repeated string key = 1 }                                         statemachine/KeyValueStore.proto:12-45
//   SetRequest { repeated SetKeyValuePair key_value = 1 }     SetKeyValuePair { key = 1; value = 2 }  both required
//
// shape 1 (canonical; the only shape whose keys are reported): exactly one `value` member and nothing else in
//   CommandOrNoop; a Noop's body empty; a Command with its four fields, `command` exactly once, nothing else; exactly one
//   request member and nothing else in KeyValueStoreInput; nothing but keys in a GetRequest, nothing but pairs in a
//   SetRequest, every pair exactly one key, at least one value and nothing else; no key longer than EPX_KEY_MAX_LEN.
//   A GetRequest or SetRequest without keys is shape 1 with an empty list.
// shape 0: any other well-formed protobuf -- a member or `command` twice (ScalaPB merges or takes the last), an unknown
//   field or a known number with another wire type at any level, a required field missing, no member at all
//   (Request.Empty, an empty CommandOrNoop), a key that is too long.  That frame is the JVM's; is_noop, is_set and
//   num_keys are 0 and the sink gets nothing.
// malformed (false): a varint or a length that runs past its parent, wire types 3, 4, 6, 7.  Every occurrence of a known
//   length-delimited field is walked down to the keys, so a frame is malformed or not whatever its shape.
#pragma once
#include "fpx_wire_parse.hpp"

namespace fpxw {

constexpr int32_t EPX_KEY_MAX_LEN = 4096;  // FPX_EPX_KEY_MAX_LEN

struct EpxCmd {
  int32_t is_noop = 0, is_set = 0, num_keys = 0, shape = 0;
};

struct EpxNoKeys {
  FPX_HD void key(int32_t, const uint8_t*, int32_t) {}
};

// what a walk collects: `keys` counts every key met, `odd` anything that is not canonical
struct EpxCmdWalk {
  int32_t keys = 0;
  bool odd = false;
};

template <typename Sink>
FPX_HD inline void epx_cmd_key(Reader k, EpxCmdWalk* w, Sink& s) {
  const int64_t len = k.end - k.p;
  if (len > EPX_KEY_MAX_LEN) w->odd = true;
  else s.key(w->keys, k.p, (int32_t)len);
  ++w->keys;
}

// GetRequest { repeated string key = 1 }
template <typename Sink>
FPX_HD inline bool epx_parse_get(Reader r, EpxCmdWalk* w, Sink& s) {
  while (r.more()) {
    const uint64_t tag = r.varint();
    const uint32_t field = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
    if (field == 1 && wt == 2) {
      Reader k = r.sub();
      if (!r.ok) return false;
      epx_cmd_key(k, w, s);
    } else {
      w->odd = true;
      r.skip(wt);
    }
  }
  return r.ok;
}

// SetRequest { repeated SetKeyValuePair key_value = 1 }
template <typename Sink>
FPX_HD inline bool epx_parse_set(Reader r, EpxCmdWalk* w, Sink& s) {
  while (r.more()) {
    const uint64_t tag = r.varint();
    const uint32_t field = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
    if (field == 1 && wt == 2) {
      Reader p = r.sub();
      if (!r.ok) return false;
      int nkey = 0, nvalue = 0;
      while (p.more()) {
        const uint64_t t = p.varint();
        const uint32_t f = (uint32_t)(t >> 3), pw = (uint32_t)(t & 7);
        if (f == 1 && pw == 2) {
          Reader k = p.sub();
          if (!p.ok) return false;
          if (nkey++ == 0) epx_cmd_key(k, w, s);
        } else if (f == 2 && pw == 2) {
          (void)p.sub();
          ++nvalue;
        } else {
          w->odd = true;
          p.skip(pw);
        }
      }
      if (!p.ok) return false;
      if (nkey != 1 || nvalue < 1) w->odd = true;
    } else {
      w->odd = true;
      r.skip(wt);
    }
  }
  return r.ok;
}

// KeyValueStoreInput: *members counts the request members, *is_set is that of the last one
template <typename Sink>
FPX_HD inline bool epx_parse_kv_input(Reader r, EpxCmdWalk* w, int* members, int32_t* is_set, Sink& s) {
  while (r.more()) {
    const uint64_t tag = r.varint();
    const uint32_t field = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
    if ((field == 1 || field == 2) && wt == 2) {
      Reader sub = r.sub();
      if (!r.ok) return false;
      if (!(field == 1 ? epx_parse_get(sub, w, s) : epx_parse_set(sub, w, s))) return false;
      ++*members;
      *is_set = field == 2;
    } else {
      w->odd = true;
      r.skip(wt);
    }
  }
  return r.ok;
}

// the serialised CommandOrNoop in r -> *o and the keys to s; false: malformed (*o is then all zeros).  A sink sees keys
// of a frame that turns out to be shape 0 as well: a caller that wants the keys of canonical frames only runs the walk
// twice, first with EpxNoKeys for the shape and the count (as both classifies do).
template <typename Sink>
FPX_HD inline bool epx_parse_command(Reader r, EpxCmd* o, Sink& s) {
  *o = EpxCmd();
  EpxCmdWalk w;
  int commands = 0, noops = 0, requests = 0;
  int32_t is_set = 0;
  while (r.more()) {
    const uint64_t tag = r.varint();
    const uint32_t field = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
    if (field == 1 && wt == 2) {  // Command
      Reader c = r.sub();
      if (!r.ok) return false;
      ++commands;
      unsigned seen = 0;
      int bodies = 0;
      while (c.more()) {
        const uint64_t t = c.varint();
        const uint32_t f = (uint32_t)(t >> 3), cw = (uint32_t)(t & 7);
        if (f == 4 && cw == 2) {
          Reader body = c.sub();
          if (!c.ok) return false;
          if (!epx_parse_kv_input(body, &w, &requests, &is_set, s)) return false;
          ++bodies;
        } else if (f == 1 && cw == 2) {
          (void)c.sub();
        } else if ((f == 2 || f == 3) && cw == 0) {
          (void)c.varint();
        } else {
          w.odd = true;
          c.skip(cw);
          continue;
        }
        seen |= 1u << f;
      }
      if (!c.ok) return false;
      if (seen != 0x1e || bodies != 1) w.odd = true;
    } else if (field == 2 && wt == 2) {  // Noop {}
      Reader nb = r.sub();
      if (!r.ok) return false;
      ++noops;
      if (nb.p != nb.end) w.odd = true;
    } else {
      w.odd = true;
      r.skip(wt);
    }
  }
  if (!r.ok) return false;
  const bool noop = commands == 0 && noops == 1, command = commands == 1 && noops == 0 && requests == 1;
  if (w.odd || !(noop || command)) return true;  // shape 0
  o->shape = 1, o->is_noop = noop, o->is_set = command ? is_set : 0, o->num_keys = w.keys;
  return true;
}

}  // namespace fpxw
