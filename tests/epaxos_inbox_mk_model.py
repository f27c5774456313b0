"""epaxos_inbox_mk_model.py -- TEST INFRASTRUCTURE ONLY: tests/epaxos_inbox_model.py's InboxModel restated over the multi-key
set model (tests/epaxos_multikey_sets.py): what a burst of peer messages with KEY LISTS must do at hosted EPaxos replicas, one
message at a time.

A message is (kind, to, leader, number, ballot_ordering, ballot_replica, keys, is_set, triple_id, watermarks, values_end) with
keys a tuple of keys -- repeats allowed, () behaves like a Noop (no conflicts, no put).  Result rows are InboxModel's."""
from oracle import epaxos_sets as ES
from tests import epaxos_inbox_model as IM
from tests import epaxos_leader_model as LM
from tests import epaxos_multikey_sets as MK

MAX_PAIRS = 1 << 23                        # FPX_EPX_MK_MAX_PAIRS


class InboxMkModel(MK.EPaxos):
    def __init__(self, n, num_keys, num_instances=1 << 20):
        super().__init__(n, num_keys)
        self.num_keys, self.num_instances = num_keys, num_instances

    # ---- Replica.handleAccept at replica `to` (:1421-1511) ------------------------------------------------------------------
    def handle_accept(self, instance, ballot, triple_id, deps, to, keys, is_set):
        """InboxModel.handle_accept; updateConflictIndex (:1503, :602-614) puts under EVERY key of the list"""
        rep = self.replicas[to]
        entry = rep.cmd_log.get(instance)
        if entry is not None:
            if entry.kind == ES.COMMITTED:
                return ("commit", entry.deps, entry.triple_id)
            if ballot < entry.ballot:
                return ("nack", rep.largest_ballot)
            if entry.kind == ES.ACCEPTED and ballot == entry.vote_ballot:
                return ("again",)
        if ballot > rep.largest_ballot:
            rep.largest_ballot = ballot
        rep.cmd_log.pop(instance, None)
        rep.cmd_log[instance] = ES.Entry(ES.ACCEPTED, ballot, ballot, triple_id, None if deps is None else frozenset(deps))
        rep.index_put(tuple(keys), is_set, instance)
        return ("ok",)

    # ---- argument checks of fpx_epx_replica_inbox_mk (include/fpx.h) ------------------------------------------------------------
    def valid(self, msg):
        keys = msg[6]
        if any(not (0 <= k < self.num_keys) for k in keys):            # the list rules hold for the whole CSR
            return False
        single = IM.InboxModel.valid(self, msg[:6] + (0,) + msg[7:])    # the message-level rules, with some key in range
        return single

    def inbox(self, msgs):
        if sum(len(x[6]) for x in msgs) > MAX_PAIRS or not all(self.valid(x) for x in msgs):
            return IM.EINVAL, None
        return IM.OK, [self.deliver(x) for x in msgs]

    def deliver(self, msg):
        kind, to, L, x, bo, br, keys, is_set, tid, w, end = msg
        keys = tuple(keys)
        inst, ballot, n = (L, x), (bo, br), self.n
        rep = self.replicas[to]
        given = None if (kind in (IM.IN_ACCEPT, IM.IN_COMMIT) and w[0] == -1) else LM.deps_from_message(n, inst, list(w), int(end))
        if kind == IM.IN_PRE_ACCEPT:
            r = self.handle_preaccept(inst, ballot, keys, bool(is_set), tid, given, [to])[to]
            if r[0] == "ok":
                return (IM.RI_PRE_ACCEPT_OK, -1, -1, r[1], r[2])
            if r[0] == "resend":
                return (IM.RI_PRE_ACCEPT_OK_AGAIN, -1, -1, r[1], r[2])
            if r[0] == "commit":
                return (IM.RI_COMMIT_BACK, -1, -1, r[1], r[2])
            if r[0] == "nack":
                return (IM.RI_NACK, IM.enc(r[1]), -1, IM.NO_DEPS, -1)
            return (IM.RI_IGNORED, -1, -1, IM.NO_DEPS, -1)
        if kind == IM.IN_ACCEPT:
            r = self.handle_accept(inst, ballot, tid, given, to, keys, bool(is_set))
            if r[0] == "commit":
                return (IM.RI_COMMIT_BACK, -1, -1, r[1], r[2])
            if r[0] == "nack":
                return (IM.RI_NACK, IM.enc(r[1]), -1, IM.NO_DEPS, -1)
            return (IM.RI_ACCEPT_OK_AGAIN if r[0] == "again" else IM.RI_ACCEPT_OK, -1, -1, IM.NO_DEPS, -1)
        if kind == IM.IN_COMMIT:
            self.handle_commit(inst, tid, given, [to], keys, bool(is_set))
            return (IM.RI_LEARNT, -1, -1, IM.NO_DEPS, -1)
        r = self.prepare(inst, ballot, [to])[to]                            # (a Prepare's list is not looked at)
        entry = rep.cmd_log.get(inst)
        if r[0] == "commit":
            return (IM.RI_COMMIT_BACK, -1, -1, entry.deps, entry.triple_id)
        if r[0] == "nack":
            return (IM.RI_NACK, IM.enc(r[1]), -1, IM.NO_DEPS, -1)
        _, status, vote, triple = r
        if status == ES.NONE:
            return (IM.RI_PREPARE_OK, -1, 0, IM.NO_DEPS, -1)
        return (IM.RI_PREPARE_OK, IM.enc(vote), status, entry.deps, triple)
