// fpx_epx_inbox.hpp -- the replica half of EPaxos on the device, a burst at a time: fpx_epx_replica_inbox takes what peer
// replicas send a hosted replica -- PreAccept (Replica.handlePreAccept, epaxos/Replica.scala:1159-1289), Accept
// (handleAccept :1421-1511), Commit (handleCommit :1567-1575 -> commit :815-830) and Prepare (handlePrepare :1632-1757) --
// in delivery order, the kinds interleaved, instances and keys repeated freely, and answers every message as if they had
// been handled one at a time.  Included by fpx_epaxos.hip inside its anonymous namespace, after the kernels it reuses.
//
// Two recurrences run through a burst and they decouple.  What a replica DOES with a message (process, Nack, answer again,
// ignore, answer with the Commit) depends on the entry of the message's instance alone -- kind, ballot, vote ballot --
// never on the conflict index.  What a processed PreAccept's dependencies ARE depends on the index alone: on the puts the
// replica made for the key before it, which are known once the first recurrence has said which messages put.
//
//   k_ri_validate   every message checked before anything is applied; (cell, message index) pairs for the sort, and the
//                   n x m tables of the two scans filled with "takes no part"
//   k_rs_*          the stable radix sort on the cell bits: the messages of one (to, leader, number) become one run, in
//                   delivery order
//   k_ri_walk<N>    one thread per run head walks the run with the entry's kind / ballot / vote ballot / triple in
//                   registers.  Per message: the outcome and the reply's scalar fields, the largestBallot contribution,
//                   the conflict scan's sort word, and `src`: the message of the burst whose dependencies the entry holds
//                   at that moment (RI_OLD: the entry's from before the burst), for the replies that answer from the entry.
//                   At the end of the run the entry's scalar fields and the last writer of its dependencies
//   K7's scan       sort_by_key / launch_segments / k_epx_scan<N> over the n x m layout: a processed PreAccept looks up
//                   and puts, an Accept taken in and a Commit put (their conflict rows are not read); k_hp_commit folds the
//                   call's puts into the index
//   k_cl_tilemax / k_cl_tilescan / k_cl_nacks   largestBallot as a running maximum per replica; a Nack carries its value
//   k_ri_reply<N>   out_deps / out_values_end: the stored dependencies of message src (ri_stored: conflict row U deps_in
//                   for a PreAccept, the message's own for an Accept or a Commit), or the pre-burst cl_deps
//   k_ri_store<N>   cl_deps / cl_dend of every touched cell from its last writer -- a launch of its own, AFTER k_ri_reply:
//                   every reply that needs the pre-burst dependencies has read them before any is overwritten
// Integer compares, max and atomics only; plain vector stores.
#pragma once

enum { RI_PRE_ACCEPT = FPX_EPX_IN_PRE_ACCEPT, RI_ACCEPT = FPX_EPX_IN_ACCEPT, RI_COMMIT = FPX_EPX_IN_COMMIT, RI_PREPARE = FPX_EPX_IN_PREPARE };
constexpr int RI_OLD = -1;      // src: the dependencies the entry held before the burst
constexpr int RI_NO_DEPS = -2;  // src: the reply carries no dependencies

struct RiBatch {
  int m;
  const int32_t* kind;
  const int32_t* to;
  const int32_t* leader;
  const int32_t* number;
  const int32_t* b_ord;
  const int32_t* b_rep;
  const int32_t* key;
  const uint8_t* is_set;
  const int32_t* triple;
  const int32_t* deps;  // [m][n]
  const int32_t* dend;  // may be null: 0
  int32_t* outcome;
  int32_t* out_ballot;
  int32_t* out_status;
  int32_t* out_deps;
  int32_t* out_end;
  int32_t* out_triple;
  uint2* ckv;           // (cell, message index)
  const uint2* sorted;
  uint2* kv;            // [n][m] K7's sort pairs
  int32_t* contrib;     // [n][m] k_cl_tilemax / k_cl_nacks
  uint8_t* nackflag;    // [n][m]
  int32_t* src;         // [m]
  int32_t* last;        // [m] by the sorted position of the run head
  const int32_t* conf;  // [m][n][NP] from k_epx_scan
};

__global__ void __launch_bounds__(256) k_ri_validate(const EpxState st, const RiBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n, kind = b.kind[i], to = b.to[i], L = b.leader[i], x = b.number[i];
  bool ok = kind >= RI_PRE_ACCEPT && kind <= RI_PREPARE && to >= 0 && to < n && L >= 0 && L < n && x >= 0 && x < st.num_instances;
  if (ok && kind != RI_COMMIT) {  // a Commit carries no ballot (:1567-1575)
    const int bo = b.b_ord[i], br = b.b_rep[i];
    ok = bo >= 0 && bo < (1 << 27) && br >= 0 && br < n;
  }
  if (ok && kind != RI_PREPARE) ok = b.key[i] >= -1 && b.key[i] < st.num_keys;  // a Prepare carries no command
  const int end = b.dend ? b.dend[i] : 0;
  if (ok && kind == RI_PRE_ACCEPT) {  // k_hp_validate's rules
    for (int l = 0; l < n; ++l) ok = ok && b.deps[(size_t)i * n + l] >= 0;
    const int w = b.deps[(size_t)i * n + L];
    ok = ok && (end == 0 ? w <= x : (w == x && end >= x + 2));
  }
  if (ok && (kind == RI_ACCEPT || kind == RI_COMMIT) && b.deps[(size_t)i * n] != -1) {  // fpx_epx_handle_commit's
    for (int l = 0; l < n; ++l) ok = ok && b.deps[(size_t)i * n + l] >= 0;
    ok = ok && !(end != 0 && (end <= x + 1 || b.deps[(size_t)i * n + L] > x));
  }
  if (!ok) epx_report(st.status, FPX_EINVAL, i);
  b.ckv[i] = make_uint2(ok ? (uint32_t)(((size_t)to * n + L) * st.num_instances + x) : 0u, (uint32_t)i);
  // no (replica, message) pair takes part in the conflict scan or in the largestBallot scan until the walk says so
  for (int r = 0; r < n; ++r) {
    const size_t o = (size_t)r * b.m + i;
    b.kv[o] = make_uint2((uint32_t)st.num_keys, (uint32_t)i);
    b.contrib[o] = -1;
    b.nackflag[o] = 0;
  }
}

template <int N>
__global__ void __launch_bounds__(256) k_ri_walk(const EpxState st, const RiBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int j0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (j0 >= b.m) return;
  const uint2 e0 = b.sorted[j0];
  if (j0 > 0 && b.sorted[j0 - 1].x == e0.x) return;  // not a run head
  const size_t c = e0.x;
  const int to = (int)(c / ((size_t)N * st.num_instances)), L = (int)((c / st.num_instances) % N);
  int kind = st.cl_status[c], ballot = st.cl_ballot[c], vote = st.cl_vote[c], triple = st.cl_triple[c];
  int src = RI_OLD;
  bool dirty = false;

  for (int j = j0; j < b.m; ++j) {
    const uint2 e = j == j0 ? e0 : b.sorted[j];
    if (e.x != e0.x) break;
    const int i = (int)e.y, mk = b.kind[i];
    const int mb = mk == RI_COMMIT ? -1 : b.b_ord[i] * 8 + b.b_rep[i];
    int outcome = FPX_EPX_RI_IGNORED, contrib = -1, ob = -1, os = -1, ot = -1, rsrc = RI_NO_DEPS;
    bool put = false;
    const bool committed = kind == CL_COMMITTED;
    const bool stale = !committed && kind != CL_NONE && mb < ballot;
    if (mk == RI_COMMIT) {
      // commit (:815-830): whatever entry there was is replaced whole (:826-827), no ballot is looked at
      kind = CL_COMMITTED, ballot = -1, vote = -1, triple = b.triple[i], src = i, dirty = true;
      put = true;  // updateConflictIndex :828
      outcome = FPX_EPX_RI_LEARNT;
    } else if (mk == RI_PREPARE) {
      contrib = mb;  // :1637 largestBallot = max(.., prepare.ballot) before anything else
      if (committed) {  // :1744-1755 the Commit goes back
        outcome = FPX_EPX_RI_COMMIT_BACK, rsrc = src, ot = triple;
      } else if (stale) {
        outcome = FPX_EPX_RI_NACK;
      } else if (kind == CL_NONE || kind == CL_NO_COMMAND) {  // :1654-1669, :1686-1701
        kind = CL_NO_COMMAND, ballot = mb, vote = -1, triple = -1, dirty = true;
        outcome = FPX_EPX_RI_PREPARE_OK, os = 0;
      } else {  // :1711-1743 the entry keeps its vote, only `ballot` moves
        outcome = FPX_EPX_RI_PREPARE_OK, os = kind, ob = vote, ot = triple, rsrc = src;
        ballot = mb, dirty = true;
      }
    } else if (committed) {  // :1227-1238, :1463-1474
      outcome = FPX_EPX_RI_COMMIT_BACK, rsrc = src, ot = triple;
    } else if (stale) {  // :1180-1184, 1189-1192, 1215-1218; :1432-1449
      outcome = FPX_EPX_RI_NACK;
    } else if (mk == RI_PRE_ACCEPT) {
      if (kind == CL_PRE_ACCEPTED && mb == vote) {  // :1196-1210 the PreAcceptOk again, from the stored triple
        outcome = FPX_EPX_RI_PRE_ACCEPT_OK_AGAIN, rsrc = src, ot = triple;
      } else if (kind == CL_ACCEPTED && mb == vote) {  // :1222-1224
        outcome = FPX_EPX_RI_IGNORED;
      } else {  // :1251-1289
        contrib = mb;
        kind = CL_PRE_ACCEPTED, ballot = mb, vote = mb, triple = b.triple[i], src = i, dirty = true;
        put = true;  // :1279 (and the lookup before it, :1255)
        outcome = FPX_EPX_RI_PRE_ACCEPT_OK, rsrc = i, ot = triple;
      }
    } else {  // Accept
      if (kind == CL_ACCEPTED && mb == vote) {  // :1451-1461 the AcceptOk again, nothing changes
        outcome = FPX_EPX_RI_ACCEPT_OK_AGAIN;
      } else {  // :1476-1511
        contrib = mb;  // :1487
        kind = CL_ACCEPTED, ballot = mb, vote = mb, triple = b.triple[i], src = i, dirty = true;
        put = true;  // :1503
        outcome = FPX_EPX_RI_ACCEPT_OK;
      }
    }
    const size_t o = (size_t)to * b.m + i;
    if (contrib >= 0) b.contrib[o] = contrib;
    if (outcome == FPX_EPX_RI_NACK) b.nackflag[o] = 1;
    if (put && b.key[i] >= 0) {  // (a Noop has no conflicts and leaves the index alone, :592-593, 602-614)
      const uint32_t flags = ((uint32_t)(b.is_set[i] ? 1 : 0) << EPX_SET_SHIFT) | ((uint32_t)L << EPX_LEADER_SHIFT);
      b.kv[o] = make_uint2((uint32_t)b.key[i] | flags, (uint32_t)i);
    }
    b.src[i] = rsrc;
    if (b.outcome) b.outcome[i] = outcome;
    if (b.out_ballot) b.out_ballot[i] = ob;  // (a Nack's largestBallot: k_cl_nacks)
    if (b.out_status) b.out_status[i] = os;
    if (b.out_triple) b.out_triple[i] = ot;
  }
  if (dirty) st.cl_status[c] = (uint8_t)kind, st.cl_ballot[c] = ballot, st.cl_vote[c] = vote, st.cl_triple[c] = triple;
  b.last[j0] = src;
}

// the dependencies the entry holds once message s has written it: (watermarks, values_end) as the per-kind kernels store them
template <int N>
__device__ __forceinline__ void ri_stored(const RiBatch& b, int s, int* w, int* end) {
  constexpr int NP = ConfRow<N>::NP;
  const int L = b.leader[s], x = b.number[s];
  const int in_end = b.dend ? b.dend[s] : 0;
  if (b.kind[s] != RI_PRE_ACCEPT) {  // an Accept's or a Commit's own, or "known by its id alone" (deps_by_id)
    const bool by_id = b.deps[(size_t)s * N] == -1;
#pragma unroll
    for (int l = 0; l < N; ++l) w[l] = by_id ? -1 : b.deps[(size_t)s * N + l];
    *end = by_id ? 0 : in_end;
    return;
  }
  int row[N], e = 0;
#pragma unroll
  for (int l = 0; l < N; ++l) row[l] = 0;
  if (b.key[s] >= 0) {  // computeSequenceNumberAndDependencies :569-600: the conflicts the scan found at replica to[s]
    const int32_t* cr = b.conf + ((size_t)s * N + b.to[s]) * NP;
#pragma unroll
    for (int l = 0; l < N; ++l) row[l] = cr[l];
  }
#pragma unroll
  for (int l = 0; l < N; ++l) {
    const int in = b.deps[(size_t)s * N + l];
    // as k_hp_reply: local {0 .. row-1} \ {x}  U  the message's own column (:582, :1257-1262)
    if (l == L) own_column(imax(row[l], in_end ? in_end : in), x, &w[l], &e);
    else w[l] = imax(row[l], in);
  }
  *end = e;
}

template <int N>
__global__ void __launch_bounds__(256) k_ri_reply(const EpxState st, const RiBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int s = b.src[i];
  int w[N], end = 0;
#pragma unroll
  for (int l = 0; l < N; ++l) w[l] = 0;
  if (s >= 0) {
    ri_stored<N>(b, s, w, &end);
  } else if (s == RI_OLD) {
    const size_t c = ((size_t)b.to[i] * N + b.leader[i]) * st.num_instances + b.number[i];
#pragma unroll
    for (int l = 0; l < N; ++l) w[l] = st.cl_deps[c * N + l];
    end = st.cl_dend[c];
  }
  if (b.out_deps) {
#pragma unroll
    for (int l = 0; l < N; ++l) b.out_deps[(size_t)i * N + l] = w[l];
  }
  if (b.out_end) b.out_end[i] = end;
}

template <int N>
__global__ void __launch_bounds__(256) k_ri_store(const EpxState st, const RiBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= b.m) return;
  const uint2 e = b.sorted[j];
  if (j > 0 && b.sorted[j - 1].x == e.x) return;  // not a run head
  const int s = b.last[j];
  if (s < 0) return;  // no message of the run wrote the dependencies
  int w[N], end = 0;
  ri_stored<N>(b, s, w, &end);
  const size_t c = e.x;
#pragma unroll
  for (int l = 0; l < N; ++l) st.cl_deps[c * N + l] = w[l];
  st.cl_dend[c] = end;
}
