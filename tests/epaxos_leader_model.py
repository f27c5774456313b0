"""epaxos_leader_model.py -- TEST INFRASTRUCTURE ONLY: a reference-shaped restatement of the LEADER half of an EPaxos
replica, on top of oracle/epaxos_sets.py (the acceptor half: cmdLog, conflict index, handlePreAccept / handleAccept /
handlePrepare / handleCommit).

It keeps the shapes of the Scala: `leaderStates` is a dict per replica (epaxos/Replica.scala:499) holding PreAccepting /
Accepting objects with a `responses` dict, dependencies are explicit SETS of instances, messages are handled ONE AT A TIME,
and a leader state is dropped EAGERLY where the reference drops it -- when a PreAccept / Accept / Prepare of a higher
ballot arrives (:1239-1242, 1480-1483, 1645-1648) and on commit (:831).  The device keeps no such hook: it tests the
replica's own command-log entry when replies arrive (include/fpx.h); the tests hold the two rules against each other.

    :633-729    transitionToPreAcceptPhase      -> lead
    :1291-1419  handlePreAcceptOk               -> kind 0       :796-813  preAcceptingSlowPath
    :1514-1565  handleAcceptOk                  -> kind 1       :732-793  transitionToAcceptPhase
    :1577-1630  handleNack                      -> kind 2       :815-831  commit
    :1015-1036  the defaultToSlowPath timer     -> kind 3
"""
from oracle import epaxos_sets as ES

OK, EINVAL, EFATAL = 0, 1, 9
PRE_ACCEPT_OK, ACCEPT_OK, NACK, SLOW_PATH_TIMER = 0, 1, 2, 3
(IGNORED, WAITING, START_SLOW_PATH_TIMER, FAST_COMMIT, ACCEPT, SLOW_COMMIT, NACK_RECOVER, NACK_IGNORED, FATAL) = range(9)
MAX_ORDERING = 1 << 27


class PreAccepting:
    def __init__(self, ballot, key, is_set, triple_id, responses, avoid_fast_path):
        self.ballot, self.key, self.is_set, self.triple_id = ballot, key, is_set, triple_id
        self.responses = responses                      # replicaIndex -> (sequenceNumber, frozenset of instances)
        self.avoid_fast_path = avoid_fast_path


class Accepting:
    def __init__(self, ballot, key, is_set, triple_id, triple, responses):
        self.ballot, self.key, self.is_set, self.triple_id = ballot, key, is_set, triple_id
        self.triple = triple                            # (sequenceNumber, frozenset of instances)
        self.responses = responses                      # a set of replica indices


def deps_from_message(n, instance, watermarks, values_end):
    """InstancePrefixSet.fromProto of a PreAcceptOk's dependencies: per leader the ids below the watermark, on the own-leader
    column also the explicit ids number + 1 .. values_end - 1; the instance itself is never a dependency (:582)"""
    L, x = instance
    s = set()
    for l in range(n):
        top = watermarks[l]
        if l == L and values_end:
            top = values_end
        s.update((l, y) for y in range(top))
    s.discard(instance)
    return frozenset(s)


class LeaderModel(ES.EPaxos):
    def __init__(self, n, num_keys, num_instances):
        super().__init__(n, num_keys)
        self.num_keys, self.num_instances = num_keys, num_instances
        self.slow, self.fast = self.f + 1, n - 1         # epaxos/Config.scala:8-9
        self.leader_states = [dict() for _ in range(n)]

    # ---- the acceptor half, with the eager drops of the reference ------------------------------------------------------
    def _yield_to(self, r, instance, ballot):
        st = self.leader_states[r].get(instance)
        if st is not None and ballot > st.ballot:
            del self.leader_states[r][instance]

    def peer_preaccept(self, instance, ballot, key, is_set, triple_id, deps_in, targets):
        out = {}
        for r in targets:
            rep = super().handle_preaccept(instance, ballot, key, is_set, triple_id, deps_in, [r])
            if rep[r][0] == "ok":
                self._yield_to(r, instance, ballot)      # :1239-1242 (only when the message is processed)
            out.update(rep)
        return out

    def peer_accept(self, instance, ballot, triple_id, targets, key=-1, is_set=False):
        before = {r: self.replicas[r].cmd_log.get(instance) for r in targets}
        res = super().accept(instance, ballot, triple_id, targets, key, is_set)
        for r in targets:
            if self.replicas[r].cmd_log.get(instance) is not before[r]:   # the Accept was taken in: :1480-1483
                self._yield_to(r, instance, ballot)
        if res[2]:                                       # committed at every replica: commit :831
            for r in range(self.n):
                self.leader_states[r].pop(instance, None)
        return res

    def peer_prepare(self, instance, ballot, targets):
        for r in targets:
            self._yield_to(r, instance, ballot)          # :1645-1648, before anything else
        return super().prepare(instance, ballot, targets)

    def peer_commit(self, instance, triple_id, deps, targets, key=-1, is_set=False):
        super().handle_commit(instance, triple_id, deps, targets, key, is_set)
        for r in targets:
            self.leader_states[r].pop(instance, None)    # commit :831

    # ---- transitionToPreAcceptPhase at one replica (:633-729) ----------------------------------------------------------
    def lead(self, msgs):
        """msgs: (leader, number, at, ballot_ordering, key, is_set, triple_id, avoid_fast_path) in array order.
        Returns (status, [frozenset of dependencies, or None where the message was skipped])"""
        seen = set()
        for (L, x, at, bo, key, is_set, tid, avoid) in msgs:           # require(...): nothing applied
            if not (0 <= L < self.n and 0 <= x < self.num_instances and 0 <= at < self.n and 0 <= bo < MAX_ORDERING and
                    -1 <= key < self.num_keys) or (L, x) in seen:
                return EINVAL, None
            seen.add((L, x))
        status, out = OK, []
        for (L, x, at, bo, key, is_set, tid, avoid) in msgs:
            inst, ballot, rep = (L, x), (bo, at), self.replicas[at]
            e = rep.cmd_log.get(inst)
            if e is not None and (e.kind == ES.COMMITTED or e.ballot > ballot or        # :663-667, checkLe :672-681
                                  (e.kind in (ES.PRE_ACCEPTED, ES.ACCEPTED) and e.vote_ballot > ballot)):
                status = EFATAL
                out.append(None)
                continue
            deps = frozenset(rep.compute_dependencies(inst, key, bool(is_set)))         # :640-641
            rep.cmd_log[inst] = ES.Entry(ES.PRE_ACCEPTED, ballot, ballot, tid, deps)    # :684-693
            if key >= 0:
                rep.index_put(key, bool(is_set), inst)                                  # :694
            self.leader_states[at][inst] = PreAccepting(ballot, key, bool(is_set), tid, {at: (0, deps)}, bool(avoid))  # :712-728
            out.append(deps)
        return status, out

    # ---- one burst of replies, message at a time ------------------------------------------------------------------------
    def replies(self, msgs):
        """msgs: (kind, to, leader, number, ballot_ordering, ballot_replica, replica_index, sequence_number, watermarks,
        values_end).  Returns (status, [(outcome, seq, deps or None, triple_id)], decided indices)"""
        n = self.n
        for (kind, to, L, x, bo, br, q, seq, w, end) in msgs:
            ok = kind in (0, 1, 2, 3) and 0 <= to < n and 0 <= L < n and 0 <= x < self.num_instances
            if ok and kind != SLOW_PATH_TIMER:
                ok = 0 <= bo < MAX_ORDERING and 0 <= br < n and 0 <= q < n
            if ok and kind == PRE_ACCEPT_OK:
                ok = all(v >= 0 for v in w) and (end == 0 or (end >= x + 2 and w[L] == x))
            if not ok:
                return EINVAL, None, None
        status, out, decided = OK, [], []
        for i, (kind, to, L, x, bo, br, q, seq, w, end) in enumerate(msgs):
            res = self._one(kind, to, (L, x), (bo, br), q, seq, w, end)
            if res[0] == FATAL:
                status = EFATAL
            if res[0] in (FAST_COMMIT, ACCEPT, SLOW_COMMIT):
                decided.append(i)
            out.append(res)
        return status, out, decided

    def _one(self, kind, to, inst, ballot, q, seq, w, end):
        states, rep = self.leader_states[to], self.replicas[to]
        st = states.get(inst)
        if kind == PRE_ACCEPT_OK:
            if not isinstance(st, PreAccepting):                       # :1296-1315
                return (IGNORED, 0, None, -1)
            if ballot != st.ballot:
                if not ballot < st.ballot:                             # logger.checkLt :1333
                    return (FATAL, 0, None, -1)
                return (IGNORED, 0, None, -1)
            old = len(st.responses)
            st.responses[q] = (seq, deps_from_message(self.n, inst, w, end))   # :1339-1341
            new = len(st.responses)
            if new < self.slow:                                        # :1345
                return (WAITING, 0, None, -1)
            if not st.avoid_fast_path and old < self.slow <= new and self.slow < self.fast:   # :1353-1364
                return (START_SLOW_PATH_TIMER, 0, None, -1)
            if st.avoid_fast_path and new >= self.slow:                # :1369-1372
                return self._slow_path(to, inst, st)
            if new >= self.fast:                                       # :1376-1417
                others = [v for r, v in st.responses.items() if r != to]
                cands = {v for v in others if others.count(v) >= self.fast - 1}   # Util.popularItems
                if cands:
                    assert len(cands) == 1                             # logger.checkEq :1402
                    s, deps = next(iter(cands))
                    self._commit(to, inst, st, deps)
                    return (FAST_COMMIT, s, deps, st.triple_id)
                return self._slow_path(to, inst, st)
            return (WAITING, 0, None, -1)
        if kind == ACCEPT_OK:
            if not isinstance(st, Accepting):                          # :1519-1535
                return (IGNORED, 0, None, -1)
            if ballot != st.ballot:
                if not ballot < st.ballot:                             # logger.checkLt :1550
                    return (FATAL, 0, None, -1)
                return (IGNORED, 0, None, -1)
            st.responses.add(q)                                        # :1554-1555
            if len(st.responses) < self.slow:                          # :1558
                return (WAITING, 0, None, -1)
            s, deps = st.triple
            self._commit(to, inst, st, deps)                           # :1563
            return (SLOW_COMMIT, s, deps, st.triple_id)
        if kind == NACK:
            rep.largest_ballot = max(rep.largest_ballot, ballot)       # :1578
            if st is None or st.ballot >= ballot:                      # :1580-1618
                return (NACK_IGNORED, 0, None, -1)
            return (NACK_RECOVER, 0, None, -1)                         # :1623-1629
        # the defaultToSlowPath timer fired (:1021-1032)
        if not isinstance(st, PreAccepting) or len(st.responses) < self.slow:   # logger.fatal :1024-1028, logger.check :801
            return (FATAL, 0, None, -1)
        return self._slow_path(to, inst, st)

    def _slow_path(self, to, inst, st):
        # preAcceptingSlowPath :796-813
        seq = max(s for s, _ in st.responses.values())
        deps = frozenset().union(*(d for _, d in st.responses.values()))
        # transitionToAcceptPhase :732-793 (its checks cannot fire: the entry still is the one lead() wrote)
        rep = self.replicas[to]
        e = rep.cmd_log.get(inst)
        assert e is not None and e.kind != ES.COMMITTED and e.ballot <= st.ballot and e.vote_ballot <= st.ballot
        rep.cmd_log[inst] = ES.Entry(ES.ACCEPTED, st.ballot, st.ballot, st.triple_id, deps)
        if st.key >= 0:
            rep.index_put(st.key, st.is_set, inst)                     # :763
        self.leader_states[to][inst] = Accepting(st.ballot, st.key, st.is_set, st.triple_id, (seq, deps), {to})
        return (ACCEPT, seq, deps, st.triple_id)

    def _commit(self, to, inst, st, deps):
        rep = self.replicas[to]                                        # commit :815-831
        rep.cmd_log[inst] = ES.Entry(ES.COMMITTED, triple_id=st.triple_id, deps=deps)
        if st.key >= 0:
            rep.index_put(st.key, st.is_set, inst)                     # :828
        del self.leader_states[to][inst]
