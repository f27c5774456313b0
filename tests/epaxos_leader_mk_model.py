"""epaxos_leader_mk_model.py -- TEST INFRASTRUCTURE ONLY: tests/epaxos_leader_model.py's transitionToPreAcceptPhase and
transitionToAcceptPhase with KEY LISTS, on the replicas of the multi-key set model (tests/epaxos_multikey_sets.py): the
dependencies are compute_dependencies over the command's keys and the put goes under every key.  The reply handling is
LeaderModel's own -- it never looks at keys: a leader state here keeps key = -1 (so the repeated puts of the slow path and of
commit, which are maxima that lead() already made, are left out) and the list in `keys`."""
from oracle import epaxos_sets as ES
from tests import epaxos_leader_model as LM
from tests import epaxos_multikey_sets as MK

KEY_LIST = -2                                  # FPX_EPX_KEY_LIST


def key_word(keys):
    """what the device's leader state stores for a key list"""
    distinct = set(keys)
    return -1 if not distinct else keys[0] if len(distinct) == 1 else KEY_LIST


class LeaderMkModel(LM.LeaderModel):
    def __init__(self, n, num_keys, num_instances):
        super().__init__(n, num_keys, num_instances)
        self.replicas = [MK.Replica(r, n, num_keys) for r in range(n)]

    def _valid(self, msgs, at_of):
        seen = set()
        for x in msgs:
            L, num, at, bo, keys = x[0], x[1], x[2], x[3], x[4]
            if not (0 <= L < self.n and 0 <= num < self.num_instances and 0 <= at < self.n and 0 <= bo < LM.MAX_ORDERING and
                    all(0 <= k < self.num_keys for k in keys)) or (L, num) in seen:
                return False
            seen.add((L, num))
        return True

    def refuses(self, inst, ballot, at):
        e = self.replicas[at].cmd_log.get(inst)
        return e is not None and (e.kind == ES.COMMITTED or e.ballot > ballot or
                                  (e.kind in (ES.PRE_ACCEPTED, ES.ACCEPTED) and e.vote_ballot > ballot))

    def lead(self, msgs):
        """msgs: (leader, number, at, ballot_ordering, keys, is_set, triple_id, avoid_fast_path) in array order.
        Returns (status, [frozenset of dependencies, or None where the message was skipped])"""
        if not self._valid(msgs, 2):
            return LM.EINVAL, None
        status, out = LM.OK, []
        for (L, x, at, bo, keys, is_set, tid, avoid) in msgs:
            inst, ballot, rep = (L, x), (bo, at), self.replicas[at]
            if self.refuses(inst, ballot, at):                                          # :663-667, checkLe :672-681
                status = LM.EFATAL
                out.append(None)
                continue
            deps = frozenset(rep.compute_dependencies(inst, tuple(keys), bool(is_set)))  # :640-641
            rep.cmd_log[inst] = ES.Entry(ES.PRE_ACCEPTED, ballot, ballot, tid, deps)    # :684-693
            rep.index_put(tuple(keys), bool(is_set), inst)                              # :694, under every key
            st = LM.PreAccepting(ballot, -1, bool(is_set), tid, {at: (0, deps)}, bool(avoid))
            st.keys = tuple(keys)
            self.leader_states[at][inst] = st                                           # :712-728
            out.append(deps)
        return status, out

    def lead_accept(self, msgs):
        """msgs: (leader, number, at, ballot_ordering, keys, is_set, triple_id, sequence_number, deps as a set or None).
        Returns the status"""
        if not self._valid(msgs, 2):
            return LM.EINVAL
        status = LM.OK
        for (L, x, at, bo, keys, is_set, tid, seq, deps) in msgs:
            inst, ballot, rep = (L, x), (bo, at), self.replicas[at]
            if self.refuses(inst, ballot, at):                                          # :740-744, checkLe :749-757
                status = LM.EFATAL
                continue
            deps = None if deps is None else frozenset(deps)
            rep.cmd_log[inst] = ES.Entry(ES.ACCEPTED, ballot, ballot, tid, deps)        # :759-762
            rep.index_put(tuple(keys), bool(is_set), inst)                              # :763
            st = LM.Accepting(ballot, -1, bool(is_set), tid, (seq, deps), {at})         # :765-790
            st.keys = tuple(keys)
            self.leader_states[at][inst] = st
        return status
