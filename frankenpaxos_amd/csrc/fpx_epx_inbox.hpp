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
//
// Key lists (fpx_epx_replica_inbox_mk, the MK = true instantiations; fpx_epaxos_mk.hpp has the conflict model): the entry
// walk never looks at keys, so only the conflict scan changes -- from m messages per replica to P = key_off[m] (message,
// key) pairs per replica, in array order, as K7's pair form.
//   k_ri_lists      the lists checked ON THE DEVICE (the device form has no host wait): key_off[0] = 0, non-decreasing,
//                   key_off[m] = the caller's num_pairs, keys in range; uniq / pnum of every pair (mk_command_pairs) and the
//                   n x P sort pairs filled with "takes no part".  A thread touches pairs only inside [0, num_pairs)
//   k_ri_walk       a put writes one sort word per distinct key of the message, at its pair positions
//   K7's scan       over P pairs, number = pnum, rows pconf[P][n][NP]
//   k_ri_merge<N>   for every processed PreAccept the max over its distinct keys' pair rows at replica to[i] -> conf, which
//                   k_ri_reply / k_ri_store read as before
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
  const int32_t* key;      // null in the key-list form
  const int32_t* key_off;  // key-list form (else null): message i's keys are keys[key_off[i] .. key_off[i + 1]), P pairs in all
  const int32_t* keys;
  int P;
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
  uint2* kv;            // [n][m] K7's sort pairs; key lists: [n][P], pair j at position j
  int32_t* contrib;     // [n][m] k_cl_tilemax / k_cl_nacks
  uint8_t* nackflag;    // [n][m]
  int32_t* src;         // [m]
  int32_t* last;        // [m] by the sorted position of the run head
  const int32_t* conf;  // [m][n][NP] from k_epx_scan; key lists: from k_ri_merge
  uint8_t* uniq;        // key lists: [P] the pair's key occurs for the first time in its command
  int32_t* pnum;        // [P] the instance number of the pair's message
  const int32_t* pconf; // [P][n][NP] from k_epx_scan
  int32_t* merged;      // = conf, for k_ri_merge to write
};

template <bool MK>
__global__ void __launch_bounds__(256) k_ri_validate(const EpxState st, const RiBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n, kind = b.kind[i], to = b.to[i], L = b.leader[i], x = b.number[i];
  bool ok = kind >= RI_PRE_ACCEPT && kind <= RI_PREPARE && to >= 0 && to < n && L >= 0 && L < n && x >= 0 && x < st.num_instances;
  if (ok && kind != RI_COMMIT) {  // a Commit carries no ballot (:1567-1575)
    const int bo = b.b_ord[i], br = b.b_rep[i];
    ok = bo >= 0 && bo < (1 << 27) && br >= 0 && br < n;
  }
  if constexpr (!MK) {  // (key lists: k_ri_lists)
    if (ok && kind != RI_PREPARE) ok = b.key[i] >= -1 && b.key[i] < st.num_keys;  // a Prepare carries no command
  }
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
    if constexpr (!MK) b.kv[o] = make_uint2((uint32_t)st.num_keys, (uint32_t)i);
    b.contrib[o] = -1;
    b.nackflag[o] = 0;
  }
}

// Key lists: the CSR checked before anything is applied, then what k_mk_pairs gives.  The offsets are the caller's device
// memory, so a thread believes only its own two: with 0 <= lo <= hi <= P it stays inside keys[P], uniq[P], pnum[P] and
// kv[n][P] whatever the rest of the array says.  (A Prepare's list is checked with the rest of the CSR -- the offsets are
// one array -- but never looked up.)
__global__ void __launch_bounds__(256) k_ri_lists(const EpxState st, const RiBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int P = b.P, lo = b.key_off[i], hi = b.key_off[i + 1];
  bool ok = lo >= 0 && lo <= hi && hi <= P && (i > 0 || lo == 0) && (i < b.m - 1 || hi == P);
  for (int j = lo; ok && j < hi; ++j) ok = b.keys[j] >= 0 && b.keys[j] < st.num_keys;
  if (!ok) {
    epx_report(st.status, FPX_EINVAL, i);
    return;
  }
  mk_command_pairs(b.keys, lo, hi, b.number[i], b.uniq, b.pnum);
  for (int r = 0; r < st.n; ++r)
    for (int j = lo; j < hi; ++j) b.kv[(size_t)r * P + j] = make_uint2((uint32_t)st.num_keys, (uint32_t)j);
}

// message i's pairs [lo, hi), empty unless they lie inside [0, P).  k_ri_lists reports a bad list as FPX_EINVAL and the
// kernels below stand back from that status -- but the status word may already hold an earlier call's other error, which
// they do not stand back from: so they, too, believe no offset they have not bounded themselves
__device__ __forceinline__ void ri_pairs(const RiBatch& b, int i, int* lo, int* hi) {
  const int l = b.key_off[i], h = b.key_off[i + 1];
  const bool ok = l >= 0 && l <= h && h <= b.P;
  *lo = ok ? l : 0, *hi = ok ? h : 0;
}

template <int N, bool MK>
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
    if constexpr (MK) {
      if (put) {  // under every distinct key of the list (KeyValueStore.scala:236-254); no keys = nothing, as a Noop
        const uint32_t flags = ((uint32_t)(b.is_set[i] ? 1 : 0) << EPX_SET_SHIFT) | ((uint32_t)L << EPX_LEADER_SHIFT);
        int lo, hi;
        ri_pairs(b, i, &lo, &hi);
        for (int q = lo; q < hi; ++q)
          if (b.uniq[q]) b.kv[(size_t)to * b.P + q] = make_uint2((uint32_t)b.keys[q] | flags, (uint32_t)q);
      }
    } else if (put && b.key[i] >= 0) {  // (a Noop has no conflicts and leaves the index alone, :592-593, 602-614)
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

// Key lists: the conflict row of every PROCESSED PreAccept (src[i] == i with kind PreAccept is exactly that set) at the
// replica it went to = the element-wise max over its distinct keys of the pair rows; a command without keys: zeros
template <int N>
__global__ void __launch_bounds__(256) k_ri_merge(const EpxState st, const RiBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m || b.kind[i] != RI_PRE_ACCEPT || b.src[i] != i) return;
  constexpr int NP = ConfRow<N>::NP;
  const int r = b.to[i];
  if (r < 0 || r >= N) return;  // (reported by k_ri_validate; see ri_pairs)
  int4 a0 = make_int4(0, 0, 0, 0), a1 = make_int4(0, 0, 0, 0);  // (rows are 16 / 32 bytes, aligned: whole-row loads, as k_mk_merge)
  int lo, hi;
  ri_pairs(b, i, &lo, &hi);
  for (int j = lo; j < hi; ++j) {
    if (!b.uniq[j]) continue;
    const int4* row = reinterpret_cast<const int4*>(b.pconf + ((size_t)j * N + r) * NP);
    const int4 x = row[0];
    a0 = make_int4(imax(a0.x, x.x), imax(a0.y, x.y), imax(a0.z, x.z), imax(a0.w, x.w));
    if constexpr (NP == 8) {
      const int4 y = row[1];
      a1 = make_int4(imax(a1.x, y.x), imax(a1.y, y.y), imax(a1.z, y.z), imax(a1.w, y.w));
    }
  }
  int4* dst = reinterpret_cast<int4*>(b.merged + ((size_t)i * N + r) * NP);
  dst[0] = a0;
  if constexpr (NP == 8) dst[1] = a1;
}

// the dependencies the entry holds once message s has written it: (watermarks, values_end) as the per-kind kernels store them
template <int N, bool MK>
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
  bool has_keys;  // a command with keys (not a Noop, not an empty list)
  if constexpr (MK) has_keys = b.key_off[s + 1] > b.key_off[s];
  else has_keys = b.key[s] >= 0;
  if (has_keys) {  // computeSequenceNumberAndDependencies :569-600: the conflicts the scan found at replica to[s]
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

template <int N, bool MK>
__global__ void __launch_bounds__(256) k_ri_reply(const EpxState st, const RiBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int s = b.src[i];
  int w[N], end = 0;
#pragma unroll
  for (int l = 0; l < N; ++l) w[l] = 0;
  if (s >= 0) {
    ri_stored<N, MK>(b, s, w, &end);
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

template <int N, bool MK>
__global__ void __launch_bounds__(256) k_ri_store(const EpxState st, const RiBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= b.m) return;
  const uint2 e = b.sorted[j];
  if (j > 0 && b.sorted[j - 1].x == e.x) return;  // not a run head
  const int s = b.last[j];
  if (s < 0) return;  // no message of the run wrote the dependencies
  int w[N], end = 0;
  ri_stored<N, MK>(b, s, w, &end);
  const size_t c = e.x;
#pragma unroll
  for (int l = 0; l < N; ++l) st.cl_deps[c * N + l] = w[l];
  st.cl_dend[c] = end;
}
