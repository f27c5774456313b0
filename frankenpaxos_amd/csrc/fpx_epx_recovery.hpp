// fpx_epx_recovery.hpp -- originating an instance's recovery on the device (FPX_EPX_F_RECOVERY, beside
// FPX_EPX_F_LEADER_STATE): the Preparing phase of Replica.leaderStates.  fpx_epx_recover is transitionToPreparePhase
// (epaxos/Replica.scala:969-996) at one hosted replica with that replica's own Prepare (handlePrepare :1632-1757) delivered
// at once, fpx_epx_recovery_replies is handlePrepareOk (:1759-1869) over a burst, fpx_epx_lead_accept is
// transitionToAcceptPhase (:732-793) with a triple the caller names.  Included by fpx_epaxos.hip inside its anonymous
// namespace, after fpx_epx_leader.hpp, whose state, sort and compaction it shares.
//
// A Preparing state of cell c = (replica r, leader L, number x):
//   head[c]   x = LS_PREPARING | responses << 8 (bit q) | statuses << 16 (2 bits per responder q: 0 NotSeen, 2 PreAccepted,
//             3 Accepted), y = the recovery's ballot, z = w = -1
//   prep[c]   n int2, row q = (voteBallot encoded, triple id) of replica q's PrepareOk  -- 8 n bytes per cell
//   resp[c]   row q = the PrepareOk's sequence number, n watermarks, values_end in own_column's canonical form (zeros for
//             a PrepareOk of status 0)
// It is live exactly while the entry at r is not committed and its `ballot` is the state's (a Prepare moves `ballot` only,
// so the vote ballot is not compared).
//
// A burst of PrepareOks:
//   k_rr_validate   every message checked before anything is applied; (cell, message index) pairs for the sort
//   k_rs_*          the stable radix sort on the cell bits: a cell's messages become one run, in delivery order
//   k_rr_walk<N>    one thread per run head walks the run against the cell.  The responses stay in memory: a message
//                   writes its row, the decision at f + 1 responses streams the rows it compares
//   k_lr_count / k_lr_bscan / k_lr_compact   decided_index, in message order
// Integer compares, max and atomics only; plain vector stores.
#pragma once

// ---- fpx_epx_recover ---------------------------------------------------------------------------------------------------
struct RvBatch {
  int m;
  const int32_t* leader;
  const int32_t* number;
  const int32_t* at;
  uint32_t* rank;   // [n][m]: 1 where at[i] is the replica, then its exclusive scan
  int32_t* base;    // [n] the ordering of largestBallot(r) before the call
  int32_t* count;   // [n] the recoveries of the call at replica r
  int32_t* outcome;
  int32_t* out_ord;
  int32_t* out_status;
  int32_t* out_vote;
  int32_t* out_triple;
  uint32_t run_id;
};

__global__ void __launch_bounds__(256) k_rv_validate(const EpxState st, const RvBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n, L = b.leader[i], x = b.number[i], at = b.at[i];
  bool ok = L >= 0 && L < n && x >= 0 && x < st.num_instances && at >= 0 && at < n;
  if (ok) ok = atomicExch(&st.cl_stamp[(size_t)L * st.num_instances + x], b.run_id) != b.run_id;
  if (!ok) epx_report(st.status, FPX_EINVAL, i);
  for (int r = 0; r < n; ++r) b.rank[(size_t)r * b.m + i] = (ok && r == at) ? 1u : 0u;
}

// The k-th recovery of the call at replica r takes ordering(largestBallot(r)) + 1 + k: k is the exclusive scan of row r of
// `rank`, which k_lr_bscan -- the array scan of the compaction -- takes in place, the n rows in one launch of n workgroups,
// leaving row r's total in count[r].  This kernel reads every replica's ordering before any message raises it.
__global__ void __launch_bounds__(64) k_rv_base(const EpxState st, const RvBatch b) {
  const int r = threadIdx.x;
  if (r >= st.n) return;
  const int base = st.largest[r] >> 3;
  b.base[r] = base;
  if ((long long)base + (long long)b.count[r] >= (1ll << 27)) epx_report(st.status, FPX_EINVAL, 0);
}

template <int N>
__global__ void __launch_bounds__(256) k_rv_install(const EpxState st, const EpxLeader ls, const RvBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int r = b.at[i], L = b.leader[i], x = b.number[i];
  const int rank = (int)b.rank[(size_t)r * b.m + i];
  const int ord = b.base[r] + 1 + rank;
  const int ballot = ord * 8 + r;
  // :972-975 largestBallot ends as the replica's last recovery's ballot -- one plain store per replica, not an atomic per
  // message on n words; every message's base was read by k_rv_base, a launch earlier
  if (rank == b.count[r] - 1) st.largest[r] = ballot;
  const size_t c = ((size_t)r * N + L) * st.num_instances + x;
  const int kind = st.cl_status[c];
  int outcome = FPX_EPX_RV_PREPARING, os = -1, ov = -1, ot = -1;
  if (kind == CL_COMMITTED) {
    // the Prepare is answered with the Commit, and commit (:831) clears the state again: nothing is installed
    outcome = FPX_EPX_RV_COMMITTED;
  } else if (kind != CL_NONE && st.cl_ballot[c] >= ballot) {
    outcome = FPX_EPX_RV_FATAL;  // largestBallot bounds every entry's ballot at its replica
    if (atomicCAS(&st.status[0], 0, FPX_EFATAL_PROTOCOL) == 0) st.status[1] = i;
  } else {
    int32_t* row = ls.resp + (c * N + r) * (N + 2);
    row[0] = 0;  // sequence numbers are 0 with top-k dependencies (:575-578, 599)
    if (kind == CL_NONE || kind == CL_NO_COMMAND) {  // :1654-1669, :1686-1701
      st.cl_status[c] = CL_NO_COMMAND, st.cl_ballot[c] = ballot, st.cl_vote[c] = -1, st.cl_triple[c] = -1;
      os = 0;
#pragma unroll
      for (int l = 0; l < N + 1; ++l) row[1 + l] = 0;
    } else {  // :1711-1743 the entry keeps its vote, only `ballot` moves
      st.cl_ballot[c] = ballot;
      os = kind, ov = st.cl_vote[c], ot = st.cl_triple[c];
      int end = st.cl_dend[c];
      const bool by_id = st.cl_deps[c * N] == -1;
#pragma unroll
      for (int l = 0; l < N; ++l) {
        int w = st.cl_deps[c * N + l];
        if (l == L && !by_id) own_column(end ? end : w, x, &w, &end);
        row[1 + l] = w;
      }
      row[1 + N] = by_id ? 0 : end;
    }
    ls.prep[c * N + r] = make_int2(ov, ot);
    ls.head[c] = make_int4(LS_PREPARING | (int)((1u << r) << 8) | (os << (16 + 2 * r)), ballot, -1, -1);
  }
  if (b.outcome) b.outcome[i] = outcome;
  if (b.out_ord) b.out_ord[i] = ord;
  if (b.out_status) b.out_status[i] = os;
  if (b.out_vote) b.out_vote[i] = ov;
  if (b.out_triple) b.out_triple[i] = ot;
}

// ---- fpx_epx_recovery_replies ------------------------------------------------------------------------------------------
struct RrBatch {
  int m, as_intended;
  const int32_t* to;
  const int32_t* leader;
  const int32_t* number;
  const int32_t* b_ord;
  const int32_t* b_rep;
  const int32_t* ridx;
  const int32_t* status;
  const int32_t* v_ord;
  const int32_t* v_rep;
  const int32_t* triple;
  const int32_t* seq;   // may be null: 0
  const int32_t* deps;  // [m][n]
  const int32_t* dend;  // may be null: 0
  int32_t* outcome;
  int32_t* out_source;
  int32_t* out_triple;
  int32_t* out_ballot;
  int32_t* out_seq;
  int32_t* out_deps;
  int32_t* out_end;
  uint2* kv;            // (cell, message index)
  const uint2* sorted;
  uint8_t* flag;        // [m] 1 = a decision
  int32_t* decided;     // the compaction's (k_lr_*, through an LrBatch of its own)
  int32_t* num_decided;
};

__global__ void __launch_bounds__(256) k_rr_validate(const EpxState st, const RrBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n, to = b.to[i], L = b.leader[i], x = b.number[i];
  const int bo = b.b_ord[i], br = b.b_rep[i], q = b.ridx[i], s = b.status[i], vo = b.v_ord[i], vr = b.v_rep[i];
  bool ok = to >= 0 && to < n && L >= 0 && L < n && x >= 0 && x < st.num_instances && bo >= 0 && bo < (1 << 27) && br >= 0 &&
            br < n && q >= 0 && q < n && (s == 0 || s == CL_PRE_ACCEPTED || s == CL_ACCEPTED) &&
            ((vo == -1 && vr == -1) || (vo >= 0 && vo < (1 << 27) && vr >= 0 && vr < n));
  if (ok && s != 0) {  // a PreAcceptOk's rules (k_lr_validate)
    for (int l = 0; l < n; ++l) ok = ok && b.deps[(size_t)i * n + l] >= 0;
    const int end = b.dend ? b.dend[i] : 0;
    ok = ok && (end == 0 || (end >= x + 2 && b.deps[(size_t)i * n + L] == x));
  }
  if (!ok) epx_report(st.status, FPX_EINVAL, i);
  b.kv[i] = make_uint2(ok ? (uint32_t)(((size_t)to * n + L) * st.num_instances + x) : 0u, (uint32_t)i);
}

template <int N>
__global__ void __launch_bounds__(256) k_rr_walk(const EpxState st, const EpxLeader ls, const RrBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int j0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (j0 >= b.m) return;
  const uint2 e0 = b.sorted[j0];
  if (j0 > 0 && b.sorted[j0 - 1].x == e0.x) return;  // not a run head
  constexpr int F = (N - 1) / 2, SLOW = F + 1;  // Config.scala: slowQuorumSize = f + 1
  const size_t c = e0.x;
  const int to = (int)(c / ((size_t)N * st.num_instances));
  const int L = (int)((c / st.num_instances) % N), x = (int)(c % st.num_instances);
  const int4 h0 = ls.head[c];
  const int ballot = h0.y;
  bool live = (h0.x & 3) == LS_PREPARING && st.cl_status[c] != CL_COMMITTED && st.cl_ballot[c] == ballot;
  unsigned mask = ((unsigned)h0.x >> 8) & 0xffu, stat = ((unsigned)h0.x >> 16) & 0x3fffu;
  bool dirty = false;
  int32_t* const rows = ls.resp + c * N * (N + 2);
  int2* const prep = ls.prep + c * N;

  for (int j = j0; j < b.m; ++j) {
    const uint2 e = j == j0 ? e0 : b.sorted[j];
    if (e.x != e0.x) break;
    const int i = (int)e.y;
    const int mb = b.b_ord[i] * 8 + b.b_rep[i];
    int outcome = FPX_EPX_RC_IGNORED, src = -1, otr = -1;
    if (live && mb > ballot) {  // logger.checkLt(prepareOk.ballot, ballot) :1792
      outcome = FPX_EPX_RC_FATAL;
      if (atomicCAS(&st.status[0], 0, FPX_EFATAL_PROTOCOL) == 0) st.status[1] = i;
    } else if (live && mb == ballot) {
      const int q = b.ridx[i], s = b.status[i];
      // responses(replicaIndex) = prepareOk (:1796): a later answer of one sender replaces the earlier one
      int32_t* r = rows + q * (N + 2);
      int e_can = 0;
      r[0] = (s && b.seq) ? b.seq[i] : 0;
      const int in_end = (s && b.dend) ? b.dend[i] : 0;
#pragma unroll
      for (int l = 0; l < N; ++l) {
        int w = s ? b.deps[(size_t)i * N + l] : 0;
        if (l == L && s) own_column(in_end ? in_end : w, x, &w, &e_can);  // a cover of x and of x + 1 are one set
        r[1 + l] = w;
      }
      r[1 + N] = e_can;
      prep[q] = make_int2(b.v_ord[i] < 0 ? -1 : b.v_ord[i] * 8 + b.v_rep[i], b.triple[i]);
      mask |= 1u << q;
      stat = (stat & ~(3u << (2 * q))) | ((unsigned)s << (2 * q));
      dirty = true;
      if (__popc(mask) < SLOW) {
        outcome = FPX_EPX_RC_WAITING;  // :1800-1802
      } else {
        int maxvb = -2;  // :1806-1808 only the responses of the highest voteBallot count
        for (int p = 0; p < N; ++p)
          if ((mask >> p) & 1u) maxvb = imax(maxvb, prep[p].x);
        unsigned pre = 0, acc = 0;  // the PreAccepted / Accepted responses of that ballot
        for (int p = 0; p < N; ++p) {
          if (!((mask >> p) & 1u) || prep[p].x != maxvb) continue;
          const unsigned sp = (stat >> (2 * p)) & 3u;
          pre |= (sp == CL_PRE_ACCEPTED ? 1u : 0u) << p, acc |= (sp == CL_ACCEPTED ? 1u : 0u) << p;
        }
        // :1813 as written compares a CommandStatus with an Option and never matches; :1836 as written reads the Prepare's
        // ballot, the recovery's own
        if (b.as_intended && acc) src = __ffs(acc) - 1, outcome = FPX_EPX_RC_ACCEPT;
        const bool in_default = b.as_intended ? maxvb == L : ballot == L;  // Ballot(0, leader) encoded
        if (src < 0 && in_default) {
          // Util.popularItems(.., config.f) over the triples of everyone but `to` (:1833-1851); rows are canonical, so
          // equal sets are equal rows
          const unsigned cand = pre & ~(1u << to);
          for (int p = 0; p < N && src < 0; ++p) {
            if (!((cand >> p) & 1u)) continue;
            const int tp = prep[p].y;
            int same = 0;
            for (int p2 = 0; p2 < N; ++p2) {
              if (!((cand >> p2) & 1u)) continue;
              bool eq = prep[p2].y == tp;
              for (int l = 0; l < N + 2 && eq; ++l) eq = rows[p * (N + 2) + l] == rows[p2 * (N + 2) + l];
              same += eq ? 1 : 0;
            }
            if (same >= F) src = p, outcome = FPX_EPX_RC_ACCEPT;
          }
        }
        if (src < 0) {  // :1856-1867 start over, avoiding the fast path: with a pre-accepted command, else with a Noop
          if (pre) src = __ffs(pre) - 1, outcome = FPX_EPX_RC_PRE_ACCEPT;
          else outcome = FPX_EPX_RC_PRE_ACCEPT_NOOP;
        }
        if (src >= 0) otr = prep[src].y;
        live = false, mask = 0, stat = 0;  // the transition is the caller's next call (fpx_epx_lead / fpx_epx_lead_accept)
      }
    }
    const bool decided = outcome == FPX_EPX_RC_ACCEPT || outcome == FPX_EPX_RC_PRE_ACCEPT || outcome == FPX_EPX_RC_PRE_ACCEPT_NOOP;
    const bool triple_out = outcome == FPX_EPX_RC_ACCEPT;
    if (b.outcome) b.outcome[i] = outcome;
    if (b.out_source) b.out_source[i] = src;
    if (b.out_triple) b.out_triple[i] = otr;
    if (b.out_ballot) b.out_ballot[i] = decided ? ballot : -1;
    const int32_t* r = rows + (src < 0 ? 0 : src) * (N + 2);
    if (b.out_seq) b.out_seq[i] = triple_out ? r[0] : 0;
    if (b.out_deps) {
      for (int l = 0; l < N; ++l) b.out_deps[(size_t)i * N + l] = triple_out ? r[1 + l] : 0;
    }
    if (b.out_end) b.out_end[i] = triple_out ? r[1 + N] : 0;
    b.flag[i] = decided ? 1 : 0;
  }
  if (dirty) ls.head[c] = make_int4(live ? (int)(LS_PREPARING | (mask << 8) | (stat << 16)) : LS_NONE, ballot, -1, -1);
}

// ---- fpx_epx_lead_accept -----------------------------------------------------------------------------------------------
struct LaBatch {
  int m;
  const int32_t* leader;
  const int32_t* number;
  const int32_t* at;
  const int32_t* b_ord;
  const int32_t* key;      // -1 = Noop; null in the key-list form
  const int32_t* key_off;  // key-list form (else null): checked on the host
  const int32_t* keys;
  const uint8_t* is_set;
  const int32_t* triple;
  const int32_t* seq;   // may be null: 0
  const int32_t* deps;  // [m][n]; a row starting with -1: the triple is known by its id alone
  const int32_t* dend;  // may be null: 0
  uint32_t run_id;
};

__global__ void __launch_bounds__(256) k_la_validate(const EpxState st, const LaBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n, L = b.leader[i], x = b.number[i], bo = b.b_ord[i], at = b.at[i], k = b.key_off ? 0 : b.key[i];
  bool ok = L >= 0 && L < n && x >= 0 && x < st.num_instances && bo >= 0 && bo < (1 << 27) && at >= 0 && at < n && k >= -1 &&
            k < st.num_keys;
  if (ok && b.deps[(size_t)i * n] != -1) {  // fpx_epx_handle_commit's rules, as an Accept of the inbox
    const int end = b.dend ? b.dend[i] : 0;
    for (int l = 0; l < n; ++l) ok = ok && b.deps[(size_t)i * n + l] >= 0;
    ok = ok && !(end != 0 && (end <= x + 1 || b.deps[(size_t)i * n + L] > x));
  }
  if (ok) ok = atomicExch(&st.cl_stamp[(size_t)L * st.num_instances + x], b.run_id) != b.run_id;
  if (!ok) epx_report(st.status, FPX_EINVAL, i);
}

template <int N>
__global__ void __launch_bounds__(256) k_la_install(const EpxState st, const EpxLeader ls, const LaBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int r = b.at[i], L = b.leader[i], x = b.number[i], ballot = b.b_ord[i] * 8 + r;
  const size_t c = ((size_t)r * N + L) * st.num_instances + x;
  const int kind = st.cl_status[c];
  // :740-744 a CommittedEntry is logger.fatal; :749-757 logger.checkLe(entry.ballot / voteBallot, ballot)
  if (kind == CL_COMMITTED || (kind != CL_NONE && st.cl_ballot[c] > ballot) || (kind >= CL_PRE_ACCEPTED && st.cl_vote[c] > ballot)) {
    if (atomicCAS(&st.status[0], 0, FPX_EFATAL_PROTOCOL) == 0) st.status[1] = i;
    return;
  }
  st.cl_status[c] = CL_ACCEPTED, st.cl_ballot[c] = ballot, st.cl_vote[c] = ballot, st.cl_triple[c] = b.triple[i];  // :759-762
  int32_t* row = ls.resp + (c * N + r) * (N + 2);
  const bool by_id = b.deps[(size_t)i * N] == -1;
  int end = (b.dend && !by_id) ? b.dend[i] : 0;
  row[0] = b.seq ? b.seq[i] : 0;
#pragma unroll
  for (int l = 0; l < N; ++l) {
    int w = b.deps[(size_t)i * N + l];
    if (by_id) w = -1;
    else if (l == L) own_column(end ? end : w, x, &w, &end);
    st.cl_deps[c * N + l] = w, row[1 + l] = w;
  }
  st.cl_dend[c] = end, row[1 + N] = end;
  // updateConflictIndex (:763): the replica may never have seen the instance.  TopOne.put is a maximum, instances are
  // pairwise distinct and nothing of this call reads the index, so the order of the puts does not show
  index_put_cmd(st, r, b.key, b.key_off, b.keys, i, b.is_set[i], L, x);  // (every key of a list; a Noop, no keys: nothing)
  // Accepting with the replica's own AcceptOk, the triple in its row (:765-790)
  ls.head[c] = make_int4(ls_pack(LS_ACCEPTING, 0, b.is_set[i] ? 1 : 0, 1u << r), ballot, b.triple[i],
                         ls_key_word(b.key, b.key_off, b.keys, i));
}
