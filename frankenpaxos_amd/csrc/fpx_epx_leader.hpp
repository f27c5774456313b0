// fpx_epx_leader.hpp -- the leader half of EPaxos on the device (FPX_EPX_F_LEADER_STATE): Replica.leaderStates
// (epaxos/Replica.scala:499) beside the command log, fpx_epx_lead (transitionToPreAcceptPhase, :633-729) and
// fpx_epx_leader_replies (handlePreAcceptOk :1291-1419, preAcceptingSlowPath :796-813, transitionToAcceptPhase :732-793,
// handleAcceptOk :1514-1565, handleNack :1577-1630, the defaultToSlowPath timer :1015-1036, commit :815-831).
// Included by fpx_epaxos.hip inside its anonymous namespace, after the K7 kernels it reuses.
//
// The state of cell c = (replica r, leader L, number x), the command log's cell index:
//   head[c]   int4: x = phase | avoidFastPath << 2 | is_set << 3 | responses << 8 (bit q: replica q has answered)
//                   y = ballot (encoded as the command log's), z = triple id, w = key (-1 = Noop or a command without keys,
//                   FPX_EPX_KEY_LIST = two or more distinct keys: the caller holds the list by triple id; ls_key_word)
//   resp[c]   n rows of n + 2 ints, row q = what replica q answered: sequence number, n watermarks, values_end -- always
//             in the canonical form own_column gives.  Accepting keeps the triple's (sequence number, dependencies) in
//             row r, the replica's own.
// 16 + 4 n (n + 2) bytes per cell (76 / 156 / 268 B at n = 3 / 5 / 7), n * n * num_instances cells.
//
// A burst of replies:
//   k_lr_validate   every message checked before anything is applied; (cell, message index) pairs for the sort
//   k_rs_*          the stable radix sort of K5 on the cell bits: a cell's messages become one run, in delivery order
//   k_lr_walk<N>    one thread per run head walks the run against the cell: the liveness test against the replica's
//                   command-log entry (one gather), then message by message.  A run is n - 1 messages in normal
//                   operation; re-sent replies make it longer and it is walked sequentially all the same
//   k_lr_count / k_lr_bscan / k_lr_compact   decided_index = the indices with outcome 3 / 4 / 5, in message order
// Integer compares, max and atomics only; plain vector stores.
#pragma once

enum { LS_NONE = 0, LS_PRE_ACCEPTING = 1, LS_ACCEPTING = 2, LS_PREPARING = 3 };  // (Preparing: fpx_epx_recovery.hpp)

struct EpxLeader {
  int4* head;     // [n * n * num_instances]
  int32_t* resp;  // [n * n * num_instances][n][n + 2]
  int2* prep;     // [n * n * num_instances][n] FPX_EPX_F_RECOVERY (else null): a PrepareOk's (voteBallot, triple id)
};

__device__ __forceinline__ int ls_pack(int phase, int avoid, int is_set, unsigned mask) {
  return phase | (avoid << 2) | (is_set << 3) | (int)(mask << 8);
}

// head.w of message i's command: its key (key_off null), or for a key list the one distinct key / -1 for none /
// FPX_EPX_KEY_LIST for more
__device__ __forceinline__ int ls_key_word(const int32_t* key, const int32_t* key_off, const int32_t* keys, int i) {
  if (!key_off) return key[i];
  const int lo = key_off[i], hi = key_off[i + 1];
  if (lo == hi) return -1;
  for (int j = lo + 1; j < hi; ++j)
    if (keys[j] != keys[lo]) return FPX_EPX_KEY_LIST;
  return keys[lo];
}

// ---- fpx_epx_lead ------------------------------------------------------------------------------------------------------
struct LdBatch {
  int m;
  const int32_t* leader;
  const int32_t* number;
  const int32_t* b_ord;
  const int32_t* at;
  const int32_t* key;      // -1 = Noop; null in the key-list form
  const int32_t* key_off;  // key-list form (else null), as HpBatch's: checked on the host, P pairs, uniq from k_mk_pairs
  const int32_t* keys;
  const uint8_t* uniq;
  int P;
  const uint8_t* is_set;
  const int32_t* triple;
  const uint8_t* avoid;
  int32_t* deps;      // [m][n] out
  int32_t* dend;      // [m] out
  uint8_t* skip;      // [m] scratch: the reference would have died (:662-682)
  uint8_t* act;       // [n][m] K7's gate table
  uint2* kv;          // [n][m] K7's sort pairs; key lists: [n][P]
  const int32_t* reply_deps;  // [m][n][n] from k_hp_reply
  const int32_t* reply_end;   // [m][n]
  uint32_t run_id;
};

__global__ void __launch_bounds__(256) k_ld_validate(const EpxState st, const LdBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n, L = b.leader[i], x = b.number[i], bo = b.b_ord[i], at = b.at[i];
  const int k = b.key_off ? 0 : b.key[i];  // (key lists: checked on the host)
  bool ok = L >= 0 && L < n && x >= 0 && x < st.num_instances && bo >= 0 && bo < (1 << 27) && at >= 0 && at < n && k >= -1 &&
            k < st.num_keys;
  if (ok) ok = atomicExch(&st.cl_stamp[(size_t)L * st.num_instances + x], b.run_id) != b.run_id;
  if (!ok) epx_report(st.status, FPX_EINVAL, i);
}

// K7's gate for a led instance: only replica at[i] takes part, and it processes unless the reference would have died;
// one thread per (replica, message), replica-major
__global__ void __launch_bounds__(256) k_ld_gate(const EpxState st, const LdBatch b) {
  const int n = st.n;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)b.m * n) return;
  const int r = (int)(t / b.m), i = (int)(t % b.m);
  const int L = b.leader[i], x = b.number[i], k = b.key_off ? 0 : b.key[i];
  int act = HP_NONE;
  // (a malformed message is reported by k_ld_validate; here it only must not index out of bounds)
  if (r == b.at[i] && L >= 0 && L < n && x >= 0 && x < st.num_instances) {
    const int ballot = b.b_ord[i] * 8 + r;
    const size_t c = ((size_t)r * n + L) * st.num_instances + x;
    const int kind = st.cl_status[c];
    // :663-667 a CommittedEntry is logger.fatal; :672-681 logger.checkLe(entry.ballot / voteBallot, ballot)
    const bool refuse = kind == CL_COMMITTED || (kind != CL_NONE && st.cl_ballot[c] > ballot) ||
                        (kind >= CL_PRE_ACCEPTED && st.cl_vote[c] > ballot);
    // (reported by k_ld_install: K5's scan, which runs in between, stands back from any status that is set)
    b.skip[i] = refuse ? 1 : 0;
    if (!refuse) act = HP_PROCESS;
  }
  const size_t o = (size_t)r * b.m + i;
  b.act[o] = (uint8_t)act;
  const bool scanned = act == HP_PROCESS && k >= 0 && k < st.num_keys;
  const uint32_t flags = ((uint32_t)(b.is_set[i] ? 1 : 0) << EPX_SET_SHIFT) | ((uint32_t)(L & 7) << EPX_LEADER_SHIFT);
  if (b.key_off) {  // one pair per (message, distinct key), in array order; the payload is the pair index (as k_hp_gate)
    for (int j = b.key_off[i]; j < b.key_off[i + 1]; ++j)
      b.kv[(size_t)r * b.P + j] = make_uint2((scanned && b.uniq[j] ? (uint32_t)b.keys[j] : (uint32_t)st.num_keys) | flags, (uint32_t)j);
    return;
  }
  b.kv[o] = make_uint2((scanned ? (uint32_t)k : (uint32_t)st.num_keys) | flags, (uint32_t)i);
}

// the PreAccept's dependencies and the leader state PreAccepting with the replica's own PreAcceptOk (:697-728); the
// command-log entry and the conflict index are k_hp_reply's and k_hp_commit's
template <int N>
__global__ void __launch_bounds__(256) k_ld_install(const EpxState st, const EpxLeader ls, const LdBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int r = b.at[i];
  int out[N], end = 0;
#pragma unroll
  for (int l = 0; l < N; ++l) out[l] = 0;
  if (b.skip[i]) {
    if (atomicCAS(&st.status[0], 0, FPX_EFATAL_PROTOCOL) == 0) st.status[1] = i;
  } else {
#pragma unroll
    for (int l = 0; l < N; ++l) out[l] = b.reply_deps[((size_t)i * N + r) * N + l];
    end = b.reply_end[(size_t)i * N + r];
    const size_t c = ((size_t)r * N + b.leader[i]) * st.num_instances + b.number[i];
    ls.head[c] = make_int4(ls_pack(LS_PRE_ACCEPTING, b.avoid[i] ? 1 : 0, b.is_set[i] ? 1 : 0, 1u << r), b.b_ord[i] * 8 + r,
                           b.triple[i], ls_key_word(b.key, b.key_off, b.keys, i));
    int32_t* row = ls.resp + (c * N + r) * (N + 2);
    row[0] = 0;  // sequence numbers are 0 with top-k dependencies (:575-578, 599)
#pragma unroll
    for (int l = 0; l < N; ++l) row[1 + l] = out[l];
    row[1 + N] = end;
  }
  if (b.deps) {
#pragma unroll
    for (int l = 0; l < N; ++l) b.deps[(size_t)i * N + l] = out[l];
  }
  if (b.dend) b.dend[i] = end;
}

// ---- fpx_epx_leader_replies --------------------------------------------------------------------------------------------
enum { LR_PRE_ACCEPT_OK = 0, LR_ACCEPT_OK = 1, LR_NACK = 2, LR_SLOW_PATH_TIMER = 3 };
constexpr int LR_BLOCK = 1024;  // messages per workgroup of the compaction (4 per thread)

struct LrBatch {
  int m;
  const int32_t* kind;
  const int32_t* to;
  const int32_t* leader;
  const int32_t* number;
  const int32_t* b_ord;
  const int32_t* b_rep;
  const int32_t* ridx;
  const int32_t* seq;   // may be null: 0
  const int32_t* deps;  // [m][n]
  const int32_t* dend;  // may be null: 0
  int32_t* outcome;
  int32_t* out_seq;
  int32_t* out_deps;
  int32_t* out_end;
  int32_t* out_triple;
  int32_t* decided;
  int32_t* num_decided;
  uint2* kv;            // (cell, message index)
  const uint2* sorted;
  uint8_t* flag;        // [m] 1 = outcome 3 / 4 / 5
  uint32_t* bsum;       // [blocks]
  int blocks;
};

__global__ void __launch_bounds__(256) k_lr_validate(const EpxState st, const LrBatch b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.m) return;
  const int n = st.n, kind = b.kind[i], to = b.to[i], L = b.leader[i], x = b.number[i];
  bool ok = kind >= LR_PRE_ACCEPT_OK && kind <= LR_SLOW_PATH_TIMER && to >= 0 && to < n && L >= 0 && L < n && x >= 0 &&
            x < st.num_instances;
  if (ok && kind != LR_SLOW_PATH_TIMER) {
    const int bo = b.b_ord[i], br = b.b_rep[i], q = b.ridx[i];
    ok = bo >= 0 && bo < (1 << 27) && br >= 0 && br < n && q >= 0 && q < n;
  }
  if (ok && kind == LR_PRE_ACCEPT_OK) {
    for (int l = 0; l < n; ++l) ok = ok && b.deps[(size_t)i * n + l] >= 0;
    // explicit ids are the run number + 1 .. end - 1 above the instance, over the watermark `number`
    const int end = b.dend ? b.dend[i] : 0;
    ok = ok && (end == 0 || (end >= x + 2 && b.deps[(size_t)i * n + L] == x));
  }
  if (!ok) epx_report(st.status, FPX_EINVAL, i);
  b.kv[i] = make_uint2(ok ? (uint32_t)(((size_t)to * n + L) * st.num_instances + x) : 0u, (uint32_t)i);
}

template <int N>
struct LrCell {
  int32_t* row;  // the cell's response rows
  __device__ __forceinline__ int32_t* at(int q) const { return row + q * (N + 2); }
};

// preAcceptingSlowPath (:796-813): the max of the sequence numbers, the union of ALL responses' dependencies (the own
// one included).  Unions are taken on covers -- on the own-leader column the cover is values_end where there are explicit
// values, else the watermark -- and own_column brings the result back to the canonical form.
template <int N>
__device__ __forceinline__ void lr_union(const LrCell<N>& cell, unsigned mask, int L, int x, int* seq, int* w, int* end) {
  int s = 0;
#pragma unroll
  for (int l = 0; l < N; ++l) w[l] = 0;
  for (int q = 0; q < N; ++q) {
    if (!((mask >> q) & 1u)) continue;
    const int32_t* r = cell.at(q);
    s = imax(s, r[0]);
#pragma unroll
    for (int l = 0; l < N; ++l) w[l] = imax(w[l], (l == L && r[1 + N]) ? r[1 + N] : r[1 + l]);
  }
  int own = 0, e = 0;
#pragma unroll
  for (int l = 0; l < N; ++l)
    if (l == L) own = w[l];
  own_column(own, x, &own, &e);
#pragma unroll
  for (int l = 0; l < N; ++l)
    if (l == L) w[l] = own;
  *seq = s, *end = e;
}

template <int N>
__global__ void __launch_bounds__(256) k_lr_walk(const EpxState st, const EpxLeader ls, const LrBatch b) {
  if (st.status[0] == FPX_EINVAL) return;
  const int j0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (j0 >= b.m) return;
  const uint2 e0 = b.sorted[j0];
  if (j0 > 0 && b.sorted[j0 - 1].x == e0.x) return;  // not a run head
  constexpr int SLOW = (N - 1) / 2 + 1, FAST = N - 1;  // Config.scala: slowQuorumSize = f + 1, fastQuorumSize = n - 1
  const size_t c = e0.x;
  const int to = (int)(c / ((size_t)N * st.num_instances));
  const int L = (int)((c / st.num_instances) % N), x = (int)(c % st.num_instances);
  const int4 h0 = ls.head[c];
  int phase = h0.x & 3;
  const int avoid = (h0.x >> 2) & 1;
  unsigned mask = ((unsigned)h0.x >> 8) & 0xffu;
  const int ballot = h0.y, triple = h0.z;
  // The reference drops leaderStates(instance) when a PreAccept / Accept / Prepare of a higher ballot arrives (:1239-1242,
  // 1480-1483, 1645-1648) or the instance commits (:831).  Each of them leaves the replica's own entry committed or with
  // another ballot / vote ballot than the one led in, so the state is live exactly while the entry still shows it.
  // (A Preparing state -- fpx_epx_recovery.hpp -- moved `ballot` only: the vote ballot is not compared.)
  if (phase != LS_NONE && (st.cl_status[c] == CL_COMMITTED || st.cl_ballot[c] != ballot ||
                           (phase != LS_PREPARING && st.cl_vote[c] != ballot)))
    phase = LS_NONE;
  bool dirty = phase != (h0.x & 3);
  LrCell<N> cell{ls.resp + c * N * (N + 2)};

  for (int j = j0; j < b.m; ++j) {
    const uint2 e = j == j0 ? e0 : b.sorted[j];
    if (e.x != e0.x) break;
    const int i = (int)e.y, kind = b.kind[i];
    int outcome = FPX_EPX_IGNORED, oseq = 0, oend = 0, otr = -1, ow[N];
#pragma unroll
    for (int l = 0; l < N; ++l) ow[l] = 0;
    bool fatal = false, slow_path = false, commit = false;
    const int mb = kind == LR_SLOW_PATH_TIMER ? 0 : b.b_ord[i] * 8 + b.b_rep[i];
    if (kind == LR_PRE_ACCEPT_OK) {
      if (phase == LS_PRE_ACCEPTING && mb >= ballot) {  // :1295-1335
        if (mb > ballot) {
          fatal = true;  // logger.checkLt(preAcceptOk.ballot, ballot) :1333
        } else {
          const int q = b.ridx[i];
          int32_t* r = cell.at(q);  // responses(replicaIndex) = preAcceptOk (:1340): a later answer replaces the earlier one
          r[0] = b.seq ? b.seq[i] : 0;
          const int in_end = b.dend ? b.dend[i] : 0;
          int e_can = 0;
#pragma unroll
          for (int l = 0; l < N; ++l) {
            int w = b.deps[(size_t)i * N + l];
            if (l == L) own_column(in_end ? in_end : w, x, &w, &e_can);  // a cover of x and of x + 1 are one set
            r[1 + l] = w;
          }
          r[1 + N] = e_can;
          const int old_n = __popc(mask);
          mask |= 1u << q;
          dirty = true;
          const int new_n = __popc(mask);
          if (new_n < SLOW) {
            outcome = FPX_EPX_WAITING;  // :1345-1347
          } else if (!avoid && old_n < SLOW && SLOW < FAST) {
            outcome = FPX_EPX_START_SLOW_PATH_TIMER;  // :1353-1364
          } else if (avoid) {
            slow_path = true;  // :1369-1372
          } else if (new_n >= FAST) {
            // Util.popularItems over the (sequence number, dependencies) of everyone but `to`, threshold fastQuorumSize - 1
            // (:1382-1396); rows are canonical, so equal sets are equal rows
            int cand = -1;
            for (int p = 0; p < N && cand < 0; ++p) {
              if (p == to || !((mask >> p) & 1u)) continue;
              int same = 0;
              for (int p2 = 0; p2 < N; ++p2) {
                if (p2 == to || !((mask >> p2) & 1u)) continue;
                bool eq = true;
                for (int l = 0; l < N + 2; ++l) eq = eq && cell.at(p)[l] == cell.at(p2)[l];
                same += eq ? 1 : 0;
              }
              if (same >= FAST - 1) cand = p;
            }
            if (cand >= 0) {
              commit = true, outcome = FPX_EPX_FAST_COMMIT;  // :1401-1410
              oseq = cell.at(cand)[0], oend = cell.at(cand)[1 + N];
#pragma unroll
              for (int l = 0; l < N; ++l) ow[l] = cell.at(cand)[1 + l];
            } else {
              slow_path = true;  // :1411-1415
            }
          } else {
            outcome = FPX_EPX_WAITING;
          }
        }
      }
    } else if (kind == LR_ACCEPT_OK) {
      if (phase == LS_ACCEPTING && mb >= ballot) {  // :1518-1552
        if (mb > ballot) {
          fatal = true;  // logger.checkLt(acceptOk.ballot, ballot) :1550
        } else {
          mask |= 1u << b.ridx[i];  // :1554-1555
          dirty = true;
          if (__popc(mask) < SLOW) {
            outcome = FPX_EPX_WAITING;  // :1558-1560
          } else {
            commit = true, outcome = FPX_EPX_SLOW_COMMIT;  // :1563, the Accept's triple
            oseq = cell.at(to)[0], oend = cell.at(to)[1 + N];
#pragma unroll
            for (int l = 0; l < N; ++l) ow[l] = cell.at(to)[1 + l];
          }
        }
      }
    } else if (kind == LR_NACK) {
      atomicMax(&st.largest[to], mb);  // :1578, whatever follows
      outcome = (phase != LS_NONE && ballot < mb) ? FPX_EPX_NACK_RECOVER : FPX_EPX_NACK_IGNORED;  // :1580-1629
    } else {
      // the defaultToSlowPath timer (:1023-1031; any other state, Preparing too, is its logger.fatal); preAcceptingSlowPath checks responses.size >= slowQuorumSize (:801)
      if (phase == LS_PRE_ACCEPTING && __popc(mask) >= SLOW) slow_path = true;
      else fatal = true;
    }
    if (slow_path) {
      // transitionToAcceptPhase (:732-793): AcceptedEntry(ballot, ballot, triple) at `to`, Accepting with the own AcceptOk.
      // (Its checks :739-759 cannot fire on a live state, and updateConflictIndex :763 repeats fpx_epx_lead's put.)
      outcome = FPX_EPX_ACCEPT;
      lr_union<N>(cell, mask, L, x, &oseq, ow, &oend);
      st.cl_status[c] = CL_ACCEPTED, st.cl_ballot[c] = ballot, st.cl_vote[c] = ballot, st.cl_triple[c] = triple;
      int32_t* r = cell.at(to);
      r[0] = oseq, r[1 + N] = oend;
#pragma unroll
      for (int l = 0; l < N; ++l) st.cl_deps[c * N + l] = ow[l], r[1 + l] = ow[l];
      st.cl_dend[c] = oend;
      phase = LS_ACCEPTING, mask = 1u << to, dirty = true;
    }
    if (commit) {
      // commit (:815-831): CommittedEntry(triple) at `to`, the leader state goes.  The conflict index needs no write: the
      // instance and its command were put by fpx_epx_lead, and TopOne.put is a maximum (util/TopOne.scala:14-17) --
      // putting them again changes nothing.
      st.cl_status[c] = CL_COMMITTED, st.cl_ballot[c] = -1, st.cl_vote[c] = -1, st.cl_triple[c] = triple;
#pragma unroll
      for (int l = 0; l < N; ++l) st.cl_deps[c * N + l] = ow[l];
      st.cl_dend[c] = oend;
      phase = LS_NONE, mask = 0, dirty = true;
    }
    if (fatal) {
      outcome = FPX_EPX_FATAL;
      if (atomicCAS(&st.status[0], 0, FPX_EFATAL_PROTOCOL) == 0) st.status[1] = i;
    }
    const bool decided = slow_path || commit;
    if (decided) otr = triple;
    if (b.outcome) b.outcome[i] = outcome;
    if (b.out_seq) b.out_seq[i] = oseq;
    if (b.out_deps) {
#pragma unroll
      for (int l = 0; l < N; ++l) b.out_deps[(size_t)i * N + l] = ow[l];
    }
    if (b.out_end) b.out_end[i] = oend;
    if (b.out_triple) b.out_triple[i] = otr;
    b.flag[i] = decided ? 1 : 0;
  }
  if (dirty) ls.head[c] = make_int4(ls_pack(phase, avoid, (h0.x >> 3) & 1, mask), ballot, triple, h0.w);
}

// decided_index: the message indices with outcome 3 / 4 / 5 in message order -- counts per block of LR_BLOCK messages, an
// exclusive scan of the counts, then every block places its own
__device__ __forceinline__ uint32_t lr_flags4(const LrBatch& b, int first, uint32_t* f) {
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[k] = first + k < b.m ? b.flag[first + k] : 0u;
    v += f[k];
  }
  return v;
}

__global__ void __launch_bounds__(256) k_lr_count(const EpxState st, const LrBatch b) {
  __shared__ uint32_t sh[4];
  if (st.status[0] == FPX_EINVAL) return;
  uint32_t f[4];
  const uint32_t all = block_reduce<ScanSum, 256>(lr_flags4(b, blockIdx.x * LR_BLOCK + threadIdx.x * 4, f), sh);
  if (threadIdx.x == 0) b.bsum[blockIdx.x] = all;
}

// an array scan: workgroup r rewrites the `len` words of row r (rows `stride` words apart) to their exclusive scan and
// leaves the row's sum in total[r] (total may be null).  The compaction's block counts are one row, fpx_epx_recover's
// ranks n.
__global__ void __launch_bounds__(256) k_lr_bscan(const EpxState st, uint32_t* a, int len, size_t stride, int32_t* total) {
  __shared__ uint32_t lds[SCAN_ARRAY_LDS(256)];
  if (st.status[0] == FPX_EINVAL) return;
  const uint32_t all = scan_array_excl<ScanSum, 256, 1>(a + blockIdx.x * stride, len, lds);
  if (threadIdx.x == 0 && total) total[blockIdx.x] = (int32_t)all;
}

__global__ void __launch_bounds__(256) k_lr_compact(const EpxState st, const LrBatch b) {
  __shared__ uint32_t sh[4];
  if (st.status[0] == FPX_EINVAL) return;
  uint32_t f[4];
  const int first = blockIdx.x * LR_BLOCK + threadIdx.x * 4;
  const uint32_t v = lr_flags4(b, first, f);
  uint32_t at = block_excl_scan<ScanSum, 256>(v, b.bsum[blockIdx.x], sh);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (f[k]) b.decided[at++] = first + k;
}
