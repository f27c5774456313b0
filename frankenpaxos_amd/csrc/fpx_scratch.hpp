// fpx_scratch.hpp -- how the burst entry points of fpx_api.hip and the EPaxos entry points of fpx_epaxos.hip cut their
// per-call scratch buffers into arrays.  Host code, no HIP: tests/burst_scratch_main.cpp runs the layouts under the
// sanitizers.
//
// A layout is ONE function over a Carver.  It runs twice per call: over a null base to learn the size the buffer must
// have, then over the buffer.  The size and the pointers come from the same take() calls and cannot disagree.
#pragma once
#include <cstddef>
#include <cstdint>

namespace fpx {

constexpr int BURST_HDR_WORDS = 8;  // every burst call's header of device-side scalars
constexpr int BURST_TILE = 256;     // messages (slots, sorted positions) per tile: one per thread of a workgroup
constexpr int SORT_RADIX_BITS = 4;  // fpx_burst_sort.hpp
constexpr int SORT_RADIX = 1 << SORT_RADIX_BITS;

// bump allocation: every array starts on a multiple of ALIGN bytes, the alignment of the device allocation itself
struct Carver {
  static constexpr size_t ALIGN = 256;
  char* base;
  size_t at = 0;
  explicit Carver(void* b) : base(static_cast<char*>(b)) {}
  template <typename T>
  T* take(size_t count) {
    static_assert(ALIGN % alignof(T) == 0, "ALIGN covers every element type");
    at = (at + ALIGN - 1) / ALIGN * ALIGN;
    T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
    at += count * sizeof(T);
    return p;
  }
  size_t size() const { return at; }
};

inline size_t burst_tiles(size_t n) { return (n + BURST_TILE - 1) / BURST_TILE; }

// fpx_burst_sort.hpp: the digit counts of `tiles` tiles, and the two key and value buffers of tiles * BURST_TILE pairs
struct SortScratch {
  int32_t* hist;
  int32_t *key[2], *val[2];
};
inline SortScratch lay_sort(Carver& c, size_t tiles) {
  SortScratch s;
  s.hist = c.take<int32_t>(SORT_RADIX * tiles);
  for (int j = 0; j < 2; ++j) s.key[j] = c.take<int32_t>(tiles * BURST_TILE);
  for (int j = 0; j < 2; ++j) s.val[j] = c.take<int32_t>(tiles * BURST_TILE);
  return s;
}

// fpx_replica_msgs.hpp (ReplicaMsgs): nblk workgroups of messages, `ranges` list places (n, or 0 for a burst without)
struct ReplicaMsgsScratch {
  int32_t *hdr, *parts, *blk, *list, *res;
};
inline ReplicaMsgsScratch lay_replica_msgs(Carver& c, size_t nblk, size_t ranges, size_t max_parts) {
  ReplicaMsgsScratch s;
  s.hdr = c.take<int32_t>(BURST_HDR_WORDS);
  s.parts = c.take<int32_t>(3 * max_parts);
  s.blk = c.take<int32_t>(nblk);
  s.list = c.take<int32_t>(ranges);
  s.res = c.take<int32_t>(ranges);
  return s;
}

// fpx_replica_inbox.hpp (ReplicaInbox): the Chosens' ReplicaMsgs, and for a call with outputs the reads' sort
struct ReplicaInboxScratch {
  ReplicaMsgsScratch m;
  int32_t *rhdr, *hdr, *tmax;
  SortScratch sort;
};
inline ReplicaInboxScratch lay_replica_inbox(Carver& c, size_t nblk, size_t slot_tiles, size_t max_parts, bool outputs) {
  ReplicaInboxScratch s;
  s.m = lay_replica_msgs(c, nblk, 0, max_parts);
  s.rhdr = c.take<int32_t>(BURST_HDR_WORDS);
  s.hdr = c.take<int32_t>(BURST_HDR_WORDS);
  s.tmax = c.take<int32_t>(slot_tiles);
  s.sort = lay_sort(c, outputs ? nblk : 0);
  return s;
}

// fpx_acceptor_inbox.hpp (AcceptorInbox): n messages to E entries
struct AcceptorInboxScratch {
  int32_t* hdr;
  long long* tile;
  SortScratch sort;
  int32_t *accslot, *tpos, *fin_round, *fin_slot;
};
inline AcceptorInboxScratch lay_acceptor_inbox(Carver& c, size_t n, size_t E) {
  const size_t tiles = burst_tiles(n);
  AcceptorInboxScratch s;
  s.hdr = c.take<int32_t>(BURST_HDR_WORDS);
  s.tile = c.take<long long>(tiles);
  s.sort = lay_sort(c, tiles);
  s.accslot = c.take<int32_t>(tiles * BURST_TILE);
  s.tpos = c.take<int32_t>(tiles * BURST_TILE);
  s.fin_round = c.take<int32_t>(E);
  s.fin_slot = c.take<int32_t>(E);
  return s;
}

// fpx_mencius_acceptor_inbox.hpp (MenciusAcceptorInbox): the above, the range flags, their tile counts and the list
struct MenciusAcceptorInboxScratch {
  AcceptorInboxScratch a;
  int32_t *rflag, *rcnt;
  int32_t* list[5];  // lent, lq0, lq1, lround, lidx
};
inline MenciusAcceptorInboxScratch lay_mencius_acceptor_inbox(Carver& c, size_t n, size_t E) {
  const size_t tiles = burst_tiles(n);
  MenciusAcceptorInboxScratch s;
  s.a = lay_acceptor_inbox(c, n, E);
  s.rflag = c.take<int32_t>(tiles * BURST_TILE);
  s.rcnt = c.take<int32_t>(tiles);
  for (int j = 0; j < 5; ++j) s.list[j] = c.take<int32_t>(tiles * BURST_TILE);
  return s;
}

// fpx_epaxos_mk.hpp, the prologue of a multi-key tick of m commands at n replicas (k_mk_prep, k_mk_total, k_mk_tilesum,
// k_mk_tilescan): `tiles` scan tiles per replica, `blocks` workgroups of k_mk_prep
struct MkPrologueScratch {
  int32_t *info, *ucnt;
  uint32_t* tsum;
  int32_t* part;  // [blocks][2]: the kernels' int2
};
inline MkPrologueScratch lay_mk_prologue(Carver& c, size_t m, size_t n, size_t tiles, size_t blocks) {
  MkPrologueScratch s;
  s.info = c.take<int32_t>(16);
  s.ucnt = c.take<int32_t>(m);
  s.tsum = c.take<uint32_t>(n * tiles);
  s.part = c.take<int32_t>(2 * blocks);
  return s;
}

// fpx_epaxos_mk.hpp, per key of the commands' key lists (k_mk_pairs): P of them, one array element for P = 0
struct MkPairScratch {
  int32_t* pnum;
  uint8_t* uniq;
};
inline MkPairScratch lay_mk_pairs(Carver& c, size_t P) {
  const size_t len = P ? P : 1;
  MkPairScratch s;
  s.pnum = c.take<int32_t>(len);
  s.uniq = c.take<uint8_t>(len);
  return s;
}

// fpx_epx_leader.hpp, the compaction of a burst of m replies (k_lr_walk's flags; k_lr_count, k_lr_bscan, k_lr_compact)
struct LrScratch {
  uint8_t* flag;
  uint32_t* bsum;
};
inline LrScratch lay_leader_replies(Carver& c, size_t m, size_t blocks) {
  LrScratch s;
  s.flag = c.take<uint8_t>(m);
  s.bsum = c.take<uint32_t>(blocks);
  return s;
}

// fpx_epx_inbox.hpp, a burst of m peer messages at n replicas: the (cell, message index) pairs of the cell sort and its
// other buffer (2 words a pair), per message where a reply's dependencies come from, per sorted position the run's last
// writer of the dependencies, and the n x m tables of the largestBallot scan (k_cl_tilemax / k_cl_tilescan / k_cl_nacks)
// with their `tiles` tile maxima per replica.  (Under the sanitizers: tests/epx_inbox_scratch_main.cpp.)
struct EpxInboxScratch {
  uint32_t* cell[2];
  int32_t *src, *last, *contrib, *tilemax;
  uint8_t* nackflag;
};
inline EpxInboxScratch lay_epx_inbox(Carver& c, size_t m, size_t n, size_t tiles) {
  EpxInboxScratch s;
  for (int j = 0; j < 2; ++j) s.cell[j] = c.take<uint32_t>(2 * m);
  s.src = c.take<int32_t>(m);
  s.last = c.take<int32_t>(m);
  s.contrib = c.take<int32_t>(n * m);
  s.tilemax = c.take<int32_t>(n * tiles);
  s.nackflag = c.take<uint8_t>(n * m);
  return s;
}

// the key-list form (fpx_epx_replica_inbox_mk): the above, sized by the m messages, and the pieces sized by the P (message,
// key) pairs.  (Under the sanitizers: tests/epx_inbox_mk_scratch_main.cpp.)
struct EpxInboxMkScratch {
  EpxInboxScratch msg;
  MkPairScratch pair;
};
inline EpxInboxMkScratch lay_epx_inbox_mk(Carver& c, size_t m, size_t P, size_t n, size_t tiles) {
  EpxInboxMkScratch s;
  s.msg = lay_epx_inbox(c, m, n, tiles);
  s.pair = lay_mk_pairs(c, P);
  return s;
}

// fpx_intern.hpp, one batch of P strings: per pair its slot and its first-occurrence flag; the three arrays the batch scans
// (flag, low and high half of the flagged length), padded to whole rows of INTERN_SCAN_ROW pairs, with the rows' sums and
// the three totals; and the batch's 8 control words.  (Under the sanitizers: tests/epx_cmd_parse_fuzz_main.cpp, as the
// two layouts below.)
constexpr int INTERN_CTL_WORDS = 8;
constexpr size_t INTERN_SCAN_ROW = 1024;
inline size_t scan_rows(size_t n) { return (n + INTERN_SCAN_ROW - 1) / INTERN_SCAN_ROW; }
struct InternScratch {
  int32_t *slot_of, *rank;
  uint32_t* sc[3];
  int32_t* tot[3];
  int32_t* gt;
  long long* ctl;
};
inline InternScratch lay_intern(Carver& c, size_t P) {
  const size_t rows = scan_rows(P);
  InternScratch s;
  s.slot_of = c.take<int32_t>(P);
  s.rank = c.take<int32_t>(P);
  for (int j = 0; j < 3; ++j) s.sc[j] = c.take<uint32_t>(rows * INTERN_SCAN_ROW);
  for (int j = 0; j < 3; ++j) s.tot[j] = c.take<int32_t>(rows);
  s.gt = c.take<int32_t>(4);
  s.ctl = c.take<long long>(INTERN_CTL_WORDS);
  return s;
}

// fpx_wire_epx_dev.hpp, the classify of m commands into at most max_pairs (message, key) pairs: the key count per message,
// its scan in rows as above with the rows' sums and the total, the word that tells the intern batch how many pairs there
// are, where each pair's key lies, and that batch
struct EpxClassifyScratch {
  int32_t *cnt, *np, *ctot, *cgt;
  uint32_t* cscan;
  int64_t* pair_off;
  int32_t* pair_len;
  InternScratch in;
};
inline EpxClassifyScratch lay_epx_classify(Carver& c, size_t m, size_t max_pairs) {
  EpxClassifyScratch s;
  s.cnt = c.take<int32_t>(m);
  s.cscan = c.take<uint32_t>(scan_rows(m) * INTERN_SCAN_ROW);
  s.ctot = c.take<int32_t>(scan_rows(m));
  s.cgt = c.take<int32_t>(1);
  s.np = c.take<int32_t>(1);
  s.pair_off = c.take<int64_t>(max_pairs);
  s.pair_len = c.take<int32_t>(max_pairs);
  s.in = lay_intern(c, max_pairs);
  return s;
}

// fpx_wire_epx_replica_tick: the decoded arrays of m messages at n replicas, the classify's outputs (what
// fpx_epx_replica_inbox_mk takes) and its scratch
struct EpxReplicaTickScratch {
  int32_t *kind, *nr, *shape, *ri_kind, *leader, *number, *b_ord, *b_rep, *dend, *cmd_len, *is_noop, *cmd_shape, *triple;
  int32_t *deps, *key_offsets, *keys, *result;
  int64_t* cmd_off;
  uint8_t* is_set;
  EpxClassifyScratch cls;
};
inline EpxReplicaTickScratch lay_epx_replica_tick(Carver& c, size_t m, size_t n, size_t max_pairs) {
  EpxReplicaTickScratch s;
  for (int32_t** a : {&s.kind, &s.nr, &s.shape, &s.ri_kind, &s.leader, &s.number, &s.b_ord, &s.b_rep, &s.dend, &s.cmd_len,
                      &s.is_noop, &s.cmd_shape, &s.triple})
    *a = c.take<int32_t>(m);
  s.deps = c.take<int32_t>(m * n);
  s.key_offsets = c.take<int32_t>(m + 1);
  s.keys = c.take<int32_t>(max_pairs);
  s.result = c.take<int32_t>(4);
  s.cmd_off = c.take<int64_t>(m);
  s.is_set = c.take<uint8_t>(m);
  s.cls = lay_epx_classify(c, m, max_pairs);
  return s;
}

// fpx_wire_epx_enc_dev.hpp, the replies of m records: the replies' lengths and their scan in rows as above, with the rows'
// sums and the total, and the call's control words.  (Under the sanitizers: tests/epx_reply_emit_main.cpp, as the layout
// below.)
constexpr int EPX_REPLY_ENC_CTL_WORDS = 4;
struct EpxReplyEncScratch {
  uint32_t* lscan;
  int32_t *ltot, *lgt, *ctl;
};
inline EpxReplyEncScratch lay_epx_reply_enc(Carver& c, size_t m) {
  EpxReplyEncScratch s;
  s.lscan = c.take<uint32_t>(scan_rows(m) * INTERN_SCAN_ROW);
  s.ltot = c.take<int32_t>(scan_rows(m));
  s.lgt = c.take<int32_t>(1);
  s.ctl = c.take<int32_t>(EPX_REPLY_ENC_CTL_WORDS);
  return s;
}

// fpx_wire_epx_replica_tick_bytes_dev: the encoder's scratch, and the inbox outputs the encoder reads, which the tick keeps
// here when the caller does not ask for them
// (out_triple: on a context with the command store, which looks the replies' commands up by it)
struct EpxTickBytesScratch {
  EpxReplyEncScratch enc;
  int32_t *outcome, *out_ballot, *out_status, *out_end, *out_deps, *out_triple;
};
inline EpxTickBytesScratch lay_epx_tick_bytes(Carver& c, size_t m, size_t n, bool triple = false) {
  EpxTickBytesScratch s;
  s.enc = lay_epx_reply_enc(c, m);
  for (int32_t** a : {&s.outcome, &s.out_ballot, &s.out_status, &s.out_end}) *a = c.take<int32_t>(m);
  s.out_deps = c.take<int32_t>(m * n);
  s.out_triple = triple ? c.take<int32_t>(m) : nullptr;
  return s;
}

// fpx_epx_cmds.hpp, a put of m records: the writers' lengths and their scan in rows as above, with the rows' sums and the
// total, the call's control words and its result when the caller wants none
constexpr int EPX_CMDS_CTL_WORDS = 8;
struct EpxCmdsPutScratch {
  uint32_t* lscan;
  int32_t *ltot, *lgt, *ctl;
  long long* result;
};
inline EpxCmdsPutScratch lay_epx_cmds_put(Carver& c, size_t m) {
  EpxCmdsPutScratch s;
  s.lscan = c.take<uint32_t>(scan_rows(m) * INTERN_SCAN_ROW);
  s.ltot = c.take<int32_t>(scan_rows(m));
  s.lgt = c.take<int32_t>(1);
  s.ctl = c.take<int32_t>(EPX_CMDS_CTL_WORDS);
  s.result = c.take<long long>(4);
  return s;
}

}  // namespace fpx
