// epaxos_leader_host_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone, array-shaped restatement of the leader half of an
// EPaxos replica (fpx_epx_lead / fpx_epx_leader_replies of include/fpx.h) on one host thread.  Flat arrays indexed by
// (replica, leader, number), dependencies as per-leader covers, one message at a time in array order.  It shares no code
// with the library; tests/test_epaxos_leader_cpu.py builds it with -fsanitize=address,undefined, plays the generator's
// streams through it and compares every line with the reference-shaped Python model.  The acceptor half is not restated
// here: an acceptor-side call reaches this program as the state it left (ENTRY / SETINDEX / LARGEST lines).
//
//   epaxos/Replica.scala  :633-729 transitionToPreAcceptPhase   :1291-1419 handlePreAcceptOk   :796-813 preAcceptingSlowPath
//                         :732-793 transitionToAcceptPhase      :1514-1565 handleAcceptOk      :1577-1630 handleNack
//                         :1015-1036 the defaultToSlowPath timer                               :815-831 commit
//
// stdin (one op per line; LEAD / REPLIES are followed by their messages):
//   CFG n num_keys num_instances
//   LEAD m            then m x "leader number at ballot_ordering key is_set triple_id avoid_fast_path"
//   REPLIES m         then m x "kind to leader number ballot_ordering ballot_replica replica_index seq values_end w[0..n)"
//   ENTRY r L x kind ballot vote triple has_deps values_end w[0..n)
//   SETINDEX r key gets[0..n) sets[0..n)        LARGEST r ballot
//   READ r L x        INDEX r key               LARGESTQ r
//   BENCH instances slow_per_mille              (a measurement: 3 PreAcceptOks per instance at n = 5, one thread)
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

enum { ST_OK = 0, ST_EINVAL = 1, ST_EFATAL = 9 };
enum { CL_NONE = 0, CL_NO_COMMAND = 1, CL_PRE_ACCEPTED = 2, CL_ACCEPTED = 3, CL_COMMITTED = 4 };
enum { PH_NONE = 0, PH_PRE = 1, PH_ACC = 2 };
enum { O_IGNORED, O_WAITING, O_TIMER, O_FAST, O_ACCEPT, O_SLOW_COMMIT, O_NACK_RECOVER, O_NACK_IGNORED, O_FATAL };

struct Lead {
  int L, x, at, bo, key, is_set, tid, avoid;
};
struct Reply {
  int kind, to, L, x, bo, br, q, seq, end;
  int w[8];
};
struct Result {
  int outcome = O_IGNORED, seq = 0, end = 0, tid = -1;
  int w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

struct Host {
  int n = 0, keys = 0, ni = 0, slow = 0, fast = 0;
  std::vector<int> kind, ballot, vote, tid, deps, dend;       // the command log, per cell
  std::vector<int> gets, sets, largest;                       // the conflict index [n][keys][n], largestBallot [n]
  std::vector<int> phase, lballot, avoid, ltid, lkey, lset, mask, rows;  // leaderStates, per cell; rows [n][n + 2]

  void init(int n_, int keys_, int ni_) {
    n = n_, keys = keys_, ni = ni_, slow = (n - 1) / 2 + 1, fast = n - 1;
    const size_t c = (size_t)n * n * ni;
    kind.assign(c, 0), ballot.assign(c, -1), vote.assign(c, -1), tid.assign(c, -1), deps.assign(c * n, 0), dend.assign(c, 0);
    gets.assign((size_t)n * keys * n, 0), sets.assign((size_t)n * keys * n, 0);
    largest.resize(n);
    for (int r = 0; r < n; ++r) largest[r] = r;  // Ballot(0, index), Replica.scala:458
    phase.assign(c, 0), lballot.assign(c, -1), avoid.assign(c, 0), ltid.assign(c, -1), lkey.assign(c, -1), lset.assign(c, 0);
    mask.assign(c, 0), rows.assign(c * n * (n + 2), 0);
  }
  size_t cell(int r, int L, int x) const { return ((size_t)r * n + L) * ni + x; }
  int* row(size_t c, int q) { return &rows[(c * n + q) * (n + 2)]; }

  // the own-leader column of instance (L, x): the ids below `cover` without x itself
  static void canon(int cover, int x, int* w, int* end) {
    *w = cover <= x ? cover : x;
    *end = cover > x + 1 ? cover : 0;
  }

  int lead(const std::vector<Lead>& ms, std::vector<std::vector<int>>& out_w, std::vector<int>& out_end) {
    std::vector<std::pair<int, int>> seen;
    for (const Lead& m : ms) {
      if (m.L < 0 || m.L >= n || m.x < 0 || m.x >= ni || m.at < 0 || m.at >= n || m.bo < 0 || m.bo >= (1 << 27) || m.key < -1 ||
          m.key >= keys)
        return ST_EINVAL;
      seen.push_back({m.L, m.x});
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return ST_EINVAL;
    int status = ST_OK;
    for (const Lead& m : ms) {
      std::vector<int> w(n, 0);
      int end = 0;
      const size_t c = cell(m.at, m.L, m.x);
      const int b = m.bo * 8 + m.at;
      const bool dies = kind[c] == CL_COMMITTED || (kind[c] != CL_NONE && ballot[c] > b) || (kind[c] >= CL_PRE_ACCEPTED && vote[c] > b);
      if (dies) {  // :662-682
        status = ST_EFATAL;
      } else {
        if (m.key >= 0) {  // getTopOneConflicts: a get conflicts with the sets, a set with gets and sets
          const int* s = &sets[((size_t)m.at * keys + m.key) * n];
          const int* g = &gets[((size_t)m.at * keys + m.key) * n];
          for (int l = 0; l < n; ++l) w[l] = m.is_set ? std::max(s[l], g[l]) : s[l];
          canon(w[m.L], m.x, &w[m.L], &end);
          int* put = m.is_set ? &sets[((size_t)m.at * keys + m.key) * n] : &gets[((size_t)m.at * keys + m.key) * n];
          put[m.L] = std::max(put[m.L], m.x + 1);  // :694
        }
        kind[c] = CL_PRE_ACCEPTED, ballot[c] = b, vote[c] = b, tid[c] = m.tid, dend[c] = end;  // :684-693
        for (int l = 0; l < n; ++l) deps[c * n + l] = w[l];
        phase[c] = PH_PRE, lballot[c] = b, avoid[c] = m.avoid ? 1 : 0, ltid[c] = m.tid, lkey[c] = m.key, lset[c] = m.is_set ? 1 : 0;
        mask[c] = 1 << m.at;  // :712-728
        int* r = row(c, m.at);
        r[0] = 0, r[1 + n] = end;
        for (int l = 0; l < n; ++l) r[1 + l] = w[l];
      }
      out_w.push_back(w), out_end.push_back(end);
    }
    return status;
  }

  bool live(size_t c) const { return phase[c] != PH_NONE && kind[c] != CL_COMMITTED && ballot[c] == lballot[c] && vote[c] == lballot[c]; }

  void slow_path(size_t c, int to, int L, int x, Result& res) {
    std::vector<int> cover(n, 0);
    int seq = 0;
    for (int q = 0; q < n; ++q) {
      if (!((mask[c] >> q) & 1)) continue;
      const int* r = row(c, q);
      seq = std::max(seq, r[0]);
      for (int l = 0; l < n; ++l) cover[l] = std::max(cover[l], (l == L && r[1 + n]) ? r[1 + n] : r[1 + l]);
    }
    int end = 0;
    canon(cover[L], x, &cover[L], &end);
    kind[c] = CL_ACCEPTED, ballot[c] = lballot[c], vote[c] = lballot[c], tid[c] = ltid[c], dend[c] = end;
    int* r = row(c, to);
    r[0] = seq, r[1 + n] = end;
    for (int l = 0; l < n; ++l) deps[c * n + l] = cover[l], r[1 + l] = cover[l];
    phase[c] = PH_ACC, mask[c] = 1 << to;
    res.outcome = O_ACCEPT, res.seq = seq, res.end = end, res.tid = ltid[c];
    std::copy(cover.begin(), cover.end(), res.w);
  }

  void commit(size_t c, const int* r, int outcome, Result& res) {
    res.outcome = outcome, res.seq = r[0], res.end = r[1 + n], res.tid = ltid[c];
    std::copy(r + 1, r + 1 + n, res.w);
    kind[c] = CL_COMMITTED, ballot[c] = -1, vote[c] = -1, tid[c] = ltid[c], dend[c] = res.end;
    for (int l = 0; l < n; ++l) deps[c * n + l] = res.w[l];
    phase[c] = PH_NONE, mask[c] = 0;  // (the conflict index already holds the instance: lead put it)
  }

  int replies(const std::vector<Reply>& ms, std::vector<Result>& out, std::vector<int>& decided) {
    for (const Reply& m : ms) {
      bool ok = m.kind >= 0 && m.kind <= 3 && m.to >= 0 && m.to < n && m.L >= 0 && m.L < n && m.x >= 0 && m.x < ni;
      if (ok && m.kind != 3) ok = m.bo >= 0 && m.bo < (1 << 27) && m.br >= 0 && m.br < n && m.q >= 0 && m.q < n;
      if (ok && m.kind == 0) {
        for (int l = 0; l < n; ++l) ok = ok && m.w[l] >= 0;
        ok = ok && (m.end == 0 || (m.end >= m.x + 2 && m.w[m.L] == m.x));
      }
      if (!ok) return ST_EINVAL;
    }
    int status = ST_OK;
    out.assign(ms.size(), Result());
    for (size_t i = 0; i < ms.size(); ++i) {
      const Reply& m = ms[i];
      Result& res = out[i];
      const size_t c = cell(m.to, m.L, m.x);
      if (phase[c] != PH_NONE && !live(c)) phase[c] = PH_NONE, mask[c] = 0;  // the state went when the entry moved
      const int b = m.kind == 3 ? 0 : m.bo * 8 + m.br;
      if (m.kind == 0) {
        if (phase[c] != PH_PRE || b < lballot[c]) continue;
        if (b > lballot[c]) {
          res.outcome = O_FATAL, status = ST_EFATAL;
          continue;
        }
        const int old_n = __builtin_popcount(mask[c]);
        int* r = row(c, m.q);
        r[0] = m.seq;
        for (int l = 0; l < n; ++l) r[1 + l] = m.w[l];
        canon(m.end ? m.end : m.w[m.L], m.x, &r[1 + m.L], &r[1 + n]);
        mask[c] |= 1 << m.q;
        const int new_n = __builtin_popcount(mask[c]);
        if (new_n < slow) {
          res.outcome = O_WAITING;
        } else if (!avoid[c] && old_n < slow && slow < fast) {
          res.outcome = O_TIMER;
        } else if (avoid[c]) {
          slow_path(c, m.to, m.L, m.x, res);
        } else if (new_n >= fast) {
          int cand = -1;
          for (int p = 0; p < n && cand < 0; ++p) {
            if (p == m.to || !((mask[c] >> p) & 1)) continue;
            int same = 0;
            for (int p2 = 0; p2 < n; ++p2)
              if (p2 != m.to && ((mask[c] >> p2) & 1) && std::equal(row(c, p), row(c, p) + n + 2, row(c, p2))) ++same;
            if (same >= fast - 1) cand = p;
          }
          if (cand >= 0) commit(c, row(c, cand), O_FAST, res);
          else slow_path(c, m.to, m.L, m.x, res);
        } else {
          res.outcome = O_WAITING;
        }
      } else if (m.kind == 1) {
        if (phase[c] != PH_ACC || b < lballot[c]) continue;
        if (b > lballot[c]) {
          res.outcome = O_FATAL, status = ST_EFATAL;
          continue;
        }
        mask[c] |= 1 << m.q;
        if (__builtin_popcount(mask[c]) < slow) res.outcome = O_WAITING;
        else commit(c, row(c, m.to), O_SLOW_COMMIT, res);
      } else if (m.kind == 2) {
        largest[m.to] = std::max(largest[m.to], b);
        res.outcome = (phase[c] != PH_NONE && lballot[c] < b) ? O_NACK_RECOVER : O_NACK_IGNORED;
      } else {
        if (phase[c] == PH_PRE && __builtin_popcount(mask[c]) >= slow) slow_path(c, m.to, m.L, m.x, res);
        else res.outcome = O_FATAL, status = ST_EFATAL;
      }
      if (res.outcome == O_FAST || res.outcome == O_ACCEPT || res.outcome == O_SLOW_COMMIT) decided.push_back((int)i);
    }
    return status;
  }
};

int rd(int* v) { return scanf("%d", v) == 1; }

int bench(int instances, int slow_per_mille) {
  Host h;
  const int n = 5;
  h.init(n, 1, instances);
  std::vector<Lead> leads;
  for (int x = 0; x < instances; ++x) leads.push_back({x % n, x / n, x % n, 0, -1, 0, x, 0});
  std::vector<std::vector<int>> w;
  std::vector<int> e;
  if (h.lead(leads, w, e) != ST_OK) return 1;
  std::vector<Reply> burst;
  for (int k = 0; k < n - 2; ++k)
    for (int x = 0; x < instances; ++x) {
      Reply r{0, x % n, x % n, x / n, 0, x % n, (x % n + 1 + k) % n, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
      if (k == 0 && (x * 7919LL) % 1000 < slow_per_mille) r.w[(x + 1) % n] = 1;
      burst.push_back(r);
    }
  std::vector<Result> out;
  std::vector<int> decided;
  const auto t0 = std::chrono::steady_clock::now();
  const int st = h.replies(burst, out, decided);
  const auto t1 = std::chrono::steady_clock::now();
  long fast = 0;
  for (int i : decided) fast += out[i].outcome == O_FAST;
  printf("BENCH status %d messages %zu decided %zu fast %ld ms %.3f\n", st, burst.size(), decided.size(), fast,
         std::chrono::duration<double, std::milli>(t1 - t0).count());
  return 0;
}

}  // namespace

int main() {
  Host h;
  char op[32];
  while (scanf("%31s", op) == 1) {
    const std::string o(op);
    if (o == "CFG") {
      int n, k, ni;
      if (!rd(&n) || !rd(&k) || !rd(&ni)) return 2;
      h.init(n, k, ni);
    } else if (o == "BENCH") {
      int inst, spm;
      if (!rd(&inst) || !rd(&spm)) return 2;
      return bench(inst, spm);
    } else if (o == "LEAD") {
      int m;
      if (!rd(&m)) return 2;
      std::vector<Lead> ms(m);
      for (Lead& a : ms)
        if (!rd(&a.L) || !rd(&a.x) || !rd(&a.at) || !rd(&a.bo) || !rd(&a.key) || !rd(&a.is_set) || !rd(&a.tid) || !rd(&a.avoid)) return 2;
      std::vector<std::vector<int>> w;
      std::vector<int> e;
      const int st = h.lead(ms, w, e);
      printf("L %d\n", st);
      if (st != ST_EINVAL)
        for (int i = 0; i < m; ++i) {
          for (int l = 0; l < h.n; ++l) printf("%d ", w[i][l]);
          printf("%d\n", e[i]);
        }
    } else if (o == "REPLIES") {
      int m;
      if (!rd(&m)) return 2;
      std::vector<Reply> ms(m);
      for (Reply& a : ms) {
        if (!rd(&a.kind) || !rd(&a.to) || !rd(&a.L) || !rd(&a.x) || !rd(&a.bo) || !rd(&a.br) || !rd(&a.q) || !rd(&a.seq) || !rd(&a.end))
          return 2;
        for (int l = 0; l < h.n; ++l)
          if (!rd(&a.w[l])) return 2;
      }
      std::vector<Result> out;
      std::vector<int> decided;
      const int st = h.replies(ms, out, decided);
      if (st == ST_EINVAL) {
        printf("R %d 0\n", st);
        continue;
      }
      printf("R %d %zu\n", st, decided.size());
      for (const Result& r : out) {
        printf("%d %d %d %d", r.outcome, r.seq, r.end, r.tid);
        for (int l = 0; l < h.n; ++l) printf(" %d", r.w[l]);
        printf("\n");
      }
      for (int i : decided) printf("%d ", i);
      printf("\n");
    } else if (o == "ENTRY") {
      int r, L, x, has;
      if (!rd(&r) || !rd(&L) || !rd(&x)) return 2;
      const size_t c = h.cell(r, L, x);
      if (!rd(&h.kind[c]) || !rd(&h.ballot[c]) || !rd(&h.vote[c]) || !rd(&h.tid[c]) || !rd(&has) || !rd(&h.dend[c])) return 2;
      for (int l = 0; l < h.n; ++l)
        if (!rd(&h.deps[c * h.n + l])) return 2;
      if (!has) h.deps[c * h.n] = -1;
    } else if (o == "SETINDEX") {
      int r, k;
      if (!rd(&r) || !rd(&k)) return 2;
      for (int l = 0; l < h.n; ++l)
        if (!rd(&h.gets[((size_t)r * h.keys + k) * h.n + l])) return 2;
      for (int l = 0; l < h.n; ++l)
        if (!rd(&h.sets[((size_t)r * h.keys + k) * h.n + l])) return 2;
    } else if (o == "LARGEST") {
      int r, b;
      if (!rd(&r) || !rd(&b)) return 2;
      h.largest[r] = std::max(h.largest[r], b);
    } else if (o == "READ") {
      int r, L, x;
      if (!rd(&r) || !rd(&L) || !rd(&x)) return 2;
      const size_t c = h.cell(r, L, x);
      printf("C %d %d %d %d %d", h.kind[c], h.ballot[c], h.vote[c], h.tid[c], h.dend[c]);
      for (int l = 0; l < h.n; ++l) printf(" %d", h.deps[c * h.n + l]);
      const int ph = h.live(c) ? h.phase[c] : 0;
      printf(" | %d %d %d %d %d %d %d", ph, h.lballot[c], h.avoid[c], h.ltid[c], h.lkey[c], h.lset[c], ph ? h.mask[c] : 0);
      for (int q = 0; q < h.n; ++q)
        if (ph && ((h.mask[c] >> q) & 1)) {
          printf(" /%d", q);
          for (int l = 0; l < h.n + 2; ++l) printf(" %d", h.row(c, q)[l]);
        }
      printf("\n");
    } else if (o == "INDEX") {
      int r, k;
      if (!rd(&r) || !rd(&k)) return 2;
      printf("I");
      for (int l = 0; l < h.n; ++l) printf(" %d", h.gets[((size_t)r * h.keys + k) * h.n + l]);
      for (int l = 0; l < h.n; ++l) printf(" %d", h.sets[((size_t)r * h.keys + k) * h.n + l]);
      printf("\n");
    } else if (o == "LARGESTQ") {
      int r;
      if (!rd(&r)) return 2;
      printf("G %d\n", h.largest[r]);
    } else {
      fprintf(stderr, "unknown op %s\n", op);
      return 2;
    }
  }
  return 0;
}
