"""epaxos_recovery_model.py -- TEST INFRASTRUCTURE ONLY: the Preparing phase on top of tests/epaxos_leader_model.py, in the
shapes of the Scala: a Preparing object with a `responses` dict in leaderStates, dependencies as explicit sets, messages
handled ONE AT A TIME, and a state dropped EAGERLY where the reference drops it (LeaderModel's _yield_to / peer_commit).

    :969-996    transitionToPreparePhase (+ the self-addressed Prepare, handlePrepare :1632-1757)   -> recover
    :1759-1869  handlePrepareOk                                                                    -> prepare_oks
    :732-793    transitionToAcceptPhase with a triple the caller names                             -> lead_accept
    :1609-1617  handleNack, the Preparing case                                                     -> _one (kind 2)

`census` counts the branches taken, for tests/epaxos_recovery_streams.py.
"""
import collections

from oracle import epaxos_sets as ES
from tests import epaxos_leader_model as M
from tests.epaxos_leader_model import OK, EINVAL, EFATAL, MAX_ORDERING

RV_PREPARING, RV_COMMITTED, RV_FATAL = range(3)
RC_IGNORED, RC_WAITING, RC_ACCEPT, RC_PRE_ACCEPT, RC_PRE_ACCEPT_NOOP, RC_FATAL = range(6)
F_LEADER_STATE, F_RECOVERY = 1, 2
NOT_SEEN, PRE_ACCEPTED, ACCEPTED = 0, 2, 3        # PrepareOk.status, the codes of fpx_epx_prepare


def enc(b):
    return -1 if b == ES.NULL_BALLOT else b[0] * 8 + b[1]


class PrepareOk:
    def __init__(self, status, vote_ballot, triple_id, seq, deps):
        self.status, self.vote_ballot, self.triple_id, self.seq = status, vote_ballot, triple_id, seq
        self.deps = deps                                # frozenset of instances; None: the triple is known by its id alone

    def triple(self):
        return (self.triple_id, self.seq, self.deps)


class Preparing:
    def __init__(self, ballot, responses):
        self.ballot = ballot
        self.responses = responses                      # replicaIndex -> PrepareOk


class RecoveryModel(M.LeaderModel):
    def __init__(self, n, num_keys, num_instances):
        super().__init__(n, num_keys, num_instances)
        self.census = collections.Counter()

    # ---- transitionToPreparePhase at one replica, its own Prepare delivered at once ------------------------------------
    def recover(self, msgs):
        """msgs: (leader, number, at) in array order.  Returns (status, [(outcome, ballot ordering, own status, own vote
        ballot encoded, own triple id)])"""
        seen, count = set(), collections.Counter()
        for (L, x, at) in msgs:                                        # require(...): nothing applied
            if not (0 <= L < self.n and 0 <= x < self.num_instances and 0 <= at < self.n) or (L, x) in seen:
                return EINVAL, None
            seen.add((L, x))
            count[at] += 1
        for at, k in count.items():
            if self.replicas[at].largest_ballot[0] + k >= MAX_ORDERING:
                return EINVAL, None
        status, out = OK, []
        if max(count.values(), default=0) > 1:
            self.census["two_recoveries_at_one_replica"] += 1
        for (L, x, at) in msgs:
            inst, rep = (L, x), self.replicas[at]
            ballot = (rep.largest_ballot[0] + 1, at)                   # :972-975
            rep.largest_ballot = ballot
            e = rep.cmd_log.get(inst)
            if e is not None and e.kind == ES.COMMITTED:               # Prepare -> the Commit back -> commit clears the state
                self.leader_states[at].pop(inst, None)
                out.append((RV_COMMITTED, ballot[0], -1, -1, -1))
                self.census["recover_committed"] += 1
                continue
            if e is not None and e.ballot >= ballot:                   # largestBallot bounds it
                status = EFATAL
                out.append((RV_FATAL, ballot[0], -1, -1, -1))
                self.census["recover_fatal"] += 1
                continue
            if e is None or e.kind == ES.NO_COMMAND:                   # :1654-1669, :1686-1701
                self.census["recover_unseen" if e is None else "recover_no_command"] += 1
                rep.cmd_log[inst] = ES.Entry(ES.NO_COMMAND, ballot)
                own = PrepareOk(NOT_SEEN, ES.NULL_BALLOT, -1, 0, frozenset())
            else:                                                      # :1711-1743 only `ballot` moves
                self.census["recover_pre_accepted" if e.kind == ES.PRE_ACCEPTED else "recover_accepted"] += 1
                e.ballot = ballot
                own = PrepareOk(e.kind, e.vote_ballot, e.triple_id, 0, e.deps)
            self.leader_states[at][inst] = Preparing(ballot, {at: own})   # :977-995
            out.append((RV_PREPARING, ballot[0], own.status, enc(own.vote_ballot), own.triple_id))
        return status, out

    # ---- handlePrepareOk over a burst, message at a time ----------------------------------------------------------------
    def prepare_oks(self, msgs, as_intended=False):
        """msgs: (to, leader, number, ballot_ordering, ballot_replica, replica_index, status, vote_ordering, vote_replica,
        triple_id, sequence_number, watermarks, values_end).  Returns (status, [(outcome, source, triple id, ballot encoded,
        seq, deps or None [only for RC_ACCEPT; "by_id" where known by id alone])], decided indices)"""
        n = self.n
        for (to, L, x, bo, br, q, s, vo, vr, tid, seq, w, end) in msgs:
            ok = (0 <= to < n and 0 <= L < n and 0 <= x < self.num_instances and 0 <= bo < MAX_ORDERING and 0 <= br < n and
                  0 <= q < n and s in (NOT_SEEN, PRE_ACCEPTED, ACCEPTED) and
                  ((vo, vr) == (-1, -1) or (0 <= vo < MAX_ORDERING and 0 <= vr < n)))
            if ok and s != NOT_SEEN:
                ok = all(v >= 0 for v in w) and (end == 0 or (end >= x + 2 and w[L] == x))
            if not ok:
                return EINVAL, None, None
        status, out, decided = OK, [], []
        for i, (to, L, x, bo, br, q, s, vo, vr, tid, seq, w, end) in enumerate(msgs):
            if s == NOT_SEEN:
                ok = PrepareOk(s, (vo, vr), tid, 0, frozenset())       # (sequence number and dependencies are not read)
            else:
                ok = PrepareOk(s, (vo, vr), tid, seq, M.deps_from_message(n, (L, x), w, end))
            res = self._prepare_ok(to, (L, x), (bo, br), q, ok, as_intended)
            if res[0] == RC_FATAL:
                status = EFATAL
            if res[0] in (RC_ACCEPT, RC_PRE_ACCEPT, RC_PRE_ACCEPT_NOOP):
                decided.append(i)
            out.append(res)
        return status, out, decided

    def _prepare_ok(self, to, inst, ballot, q, ok, as_intended):
        nothing = (-1, -1, -1, 0, None)
        st = self.leader_states[to].get(inst)
        if not isinstance(st, Preparing):                              # :1764-1780
            self.census["ok_not_preparing"] += 1
            return (RC_IGNORED,) + nothing
        if ballot != st.ballot:                                        # :1785-1794
            if not ballot < st.ballot:
                self.census["ok_above"] += 1
                return (RC_FATAL,) + nothing                           # logger.checkLt :1792
            self.census["ok_stale"] += 1
            return (RC_IGNORED,) + nothing
        if q in st.responses:
            old = st.responses[q]
            same = (old.status, old.vote_ballot, old.triple()) == (ok.status, ok.vote_ballot, ok.triple())
            self.census["ok_duplicate" if same else "ok_replaced"] += 1
        self.census["ok_status_%d" % ok.status] += 1
        st.responses[q] = ok                                           # :1796
        if len(st.responses) < self.slow:                              # :1800
            return (RC_WAITING,) + nothing
        max_ballot = max(r.vote_ballot for r in st.responses.values())             # :1806-1808
        oks = {r: v for r, v in st.responses.items() if v.vote_ballot == max_ballot}
        tag = "_intended" if as_intended else "_as_written"
        del self.leader_states[to][inst]                               # the transition is the caller's next call
        if as_intended:                                                # :1813 (as written: never true)
            for r in sorted(oks):
                if oks[r].status == ACCEPTED:
                    self.census["accept_accepted" + tag] += 1
                    return (RC_ACCEPT, r, oks[r].triple_id, enc(st.ballot), oks[r].seq, oks[r].deps)
        default = (0, inst[0])
        in_default = (max_ballot == default) if as_intended else (st.ballot == default)    # :1836
        cands = [(r, v) for r, v in sorted(oks.items()) if v.status == PRE_ACCEPTED and in_default and r != to]
        for r, v in cands:                                             # Util.popularItems(.., config.f)
            if sum(1 for _, w in cands if w.triple() == v.triple()) >= self.f:
                self.census["accept_popular" + tag] += 1
                return (RC_ACCEPT, r, v.triple_id, enc(st.ballot), v.seq, v.deps)
        for r in sorted(oks):                                          # :1856-1867
            if oks[r].status == PRE_ACCEPTED:
                self.census["pre_accept" + tag] += 1
                return (RC_PRE_ACCEPT, r, oks[r].triple_id, enc(st.ballot), 0, None)
        self.census["noop" + tag] += 1
        return (RC_PRE_ACCEPT_NOOP, -1, -1, enc(st.ballot), 0, None)

    # ---- transitionToAcceptPhase with a given triple (:732-793) -----------------------------------------------------------
    def lead_accept(self, msgs):
        """msgs: (leader, number, at, ballot_ordering, key, is_set, triple_id, sequence_number, watermarks, values_end);
        watermarks[0] == -1: the triple is known by its id alone.  Returns the status"""
        seen = set()
        for (L, x, at, bo, key, is_set, tid, seq, w, end) in msgs:
            ok = (0 <= L < self.n and 0 <= x < self.num_instances and 0 <= at < self.n and 0 <= bo < MAX_ORDERING and
                  -1 <= key < self.num_keys and (L, x) not in seen)
            if ok and w[0] != -1:
                ok = all(v >= 0 for v in w) and not (end != 0 and (end <= x + 1 or w[L] > x))
            if not ok:
                return EINVAL
            seen.add((L, x))
        status = OK
        for (L, x, at, bo, key, is_set, tid, seq, w, end) in msgs:
            inst, ballot, rep = (L, x), (bo, at), self.replicas[at]
            e = rep.cmd_log.get(inst)
            if e is not None and (e.kind == ES.COMMITTED or e.ballot > ballot or                 # :740-757
                                  (e.kind in (ES.PRE_ACCEPTED, ES.ACCEPTED) and e.vote_ballot > ballot)):
                status = EFATAL
                self.census["lead_accept_fatal"] += 1
                continue
            deps = None if w[0] == -1 else M.deps_from_message(self.n, inst, w, end)
            rep.cmd_log[inst] = ES.Entry(ES.ACCEPTED, ballot, ballot, tid, deps)                 # :759-762
            if key >= 0:
                rep.index_put(key, bool(is_set), inst)                                           # :763
            self.leader_states[at][inst] = M.Accepting(ballot, key, bool(is_set), tid, (seq, deps), {at})
            self.census["lead_accept"] += 1
        return status

    # ---- handleNack: a Preparing state is a leader state like the other two (:1609-1617) --------------------------------
    def _one(self, kind, to, inst, ballot, q, seq, w, end):
        st = self.leader_states[to].get(inst)
        if isinstance(st, Preparing):
            if kind == M.NACK:
                self.census["nack_while_preparing"] += 1
                self.replicas[to].largest_ballot = max(self.replicas[to].largest_ballot, ballot)   # :1578
                return (M.NACK_RECOVER if st.ballot < ballot else M.NACK_IGNORED, 0, None, -1)
            self.census["reply_while_preparing"] += 1
        return super()._one(kind, to, inst, ballot, q, seq, w, end)

    def peer_prepare(self, instance, ballot, targets):
        for r in targets:
            st = self.leader_states[r].get(instance)
            if isinstance(st, Preparing) and ballot > st.ballot:
                self.census["prepare_while_preparing"] += 1
        return super().peer_prepare(instance, ballot, targets)
