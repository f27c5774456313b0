"""epaxos_inbox_model.py -- TEST INFRASTRUCTURE ONLY: what a burst of peer messages at hosted EPaxos replicas must do, stated
on the set model of oracle/epaxos_sets.py one message at a time.  PreAccept, Prepare and Commit are that model's own
handle_preaccept / prepare / handle_commit with targets=[to]; handle_accept restates Replica.handleAccept
(epaxos/Replica.scala:1421-1511) at ONE replica, which the model only has inside its whole Accept phase.

A message is (kind, to, leader, number, ballot_ordering, ballot_replica, key, is_set, triple_id, watermarks, values_end);
watermarks[0] = -1 on an Accept or a Commit says "the triple is known by its id alone".
A result row is (outcome, out_ballot, out_status, deps, triple_id) with deps a frozenset of instances, None (the stored triple
is known by its id alone) or NO_DEPS (the reply carries none)."""
from oracle import epaxos_sets as ES
from tests import epaxos_leader_model as LM

IN_PRE_ACCEPT, IN_ACCEPT, IN_COMMIT, IN_PREPARE = 0, 1, 2, 3
(RI_IGNORED, RI_PRE_ACCEPT_OK, RI_PRE_ACCEPT_OK_AGAIN, RI_ACCEPT_OK, RI_ACCEPT_OK_AGAIN, RI_LEARNT, RI_PREPARE_OK, RI_NACK,
 RI_COMMIT_BACK) = range(9)
OUTCOME_NAMES = ("IGNORED", "PRE_ACCEPT_OK", "PRE_ACCEPT_OK_AGAIN", "ACCEPT_OK", "ACCEPT_OK_AGAIN", "LEARNT", "PREPARE_OK",
                 "NACK", "COMMIT_BACK")
NO_DEPS = "no-deps"
OK, EINVAL = 0, 1                          # FPX_OK, FPX_EINVAL

# every (kind, outcome) pair a message can end in
REACHABLE = {(IN_PRE_ACCEPT, o) for o in (RI_PRE_ACCEPT_OK, RI_PRE_ACCEPT_OK_AGAIN, RI_NACK, RI_COMMIT_BACK, RI_IGNORED)} | \
            {(IN_ACCEPT, o) for o in (RI_ACCEPT_OK, RI_ACCEPT_OK_AGAIN, RI_NACK, RI_COMMIT_BACK)} | \
            {(IN_COMMIT, RI_LEARNT)} | \
            {(IN_PREPARE, o) for o in (RI_PREPARE_OK, RI_NACK, RI_COMMIT_BACK)}


def enc(ballot):
    return -1 if ballot == ES.NULL_BALLOT else ballot[0] * 8 + ballot[1]


class InboxModel(ES.EPaxos):
    def __init__(self, n, num_keys, num_instances=1 << 20):
        super().__init__(n, num_keys)
        self.num_keys, self.num_instances = num_keys, num_instances

    # ---- Replica.handleAccept at replica `to` (:1421-1511) ------------------------------------------------------------------
    def handle_accept(self, instance, ballot, triple_id, deps, to, key, is_set):
        """deps: the Accept's dependencies as a set of instances, or None (the triple is known by its id alone).
        Returns ("commit", deps, triple id) | ("nack", largestBallot) | ("again",) | ("ok",)"""
        rep = self.replicas[to]
        entry = rep.cmd_log.get(instance)
        if entry is not None:                                              # cmdLog.get(accept.instance) match, :1425
            if entry.kind == ES.COMMITTED:                                 # :1464-1474 the Commit goes back, nothing else
                return ("commit", entry.deps, entry.triple_id)
            if ballot < entry.ballot:                                      # :1432, :1439, :1446 an old ballot: Nack(largestBallot)
                return ("nack", rep.largest_ballot)
            if entry.kind == ES.ACCEPTED and ballot == entry.vote_ballot:  # :1451-1461 answered already: AcceptOk again
                return ("again",)
        # (:1477-1484 leaderStates, :1490 timers: not the command log's)
        if ballot > rep.largest_ballot:                                    # :1487
            rep.largest_ballot = ballot
        rep.cmd_log.pop(instance, None)                                    # :1493
        rep.cmd_log[instance] = ES.Entry(ES.ACCEPTED, ballot, ballot, triple_id,                  # :1494-1502
                                         None if deps is None else frozenset(deps))
        if key >= 0:                                                       # :1503 updateConflictIndex (a Noop has no bytes)
            rep.index_put(key, is_set, instance)
        return ("ok",)

    # ---- argument checks of fpx_epx_replica_inbox (include/fpx.h) -----------------------------------------------------------
    def valid(self, msg):
        kind, to, L, x, bo, br, key, is_set, tid, w, end = msg
        n = self.n
        if kind not in (0, 1, 2, 3) or not (0 <= to < n and 0 <= L < n and 0 <= x < self.num_instances):
            return False
        if kind != IN_COMMIT and not (0 <= bo < (1 << 27) and 0 <= br < n):
            return False
        if kind != IN_PREPARE and not (-1 <= key < self.num_keys):
            return False
        if kind == IN_PRE_ACCEPT:
            if any(v < 0 for v in w):
                return False
            return w[L] <= x if end == 0 else (w[L] == x and end >= x + 2)
        if kind in (IN_ACCEPT, IN_COMMIT) and w[0] != -1:
            if any(v < 0 for v in w):
                return False
            return not (end != 0 and (end <= x + 1 or w[L] > x))
        return True

    # ---- one burst, message by message ------------------------------------------------------------------------------------------
    def inbox(self, msgs):
        if not all(self.valid(m) for m in msgs):
            return EINVAL, None
        return OK, [self.deliver(m) for m in msgs]

    def deliver(self, msg):
        kind, to, L, x, bo, br, key, is_set, tid, w, end = msg
        inst, ballot, n = (L, x), (bo, br), self.n
        rep = self.replicas[to]
        given = None if (kind in (IN_ACCEPT, IN_COMMIT) and w[0] == -1) else LM.deps_from_message(n, inst, list(w), int(end))
        if kind == IN_PRE_ACCEPT:
            r = self.handle_preaccept(inst, ballot, key, bool(is_set), tid, given, [to])[to]
            if r[0] == "ok":
                return (RI_PRE_ACCEPT_OK, -1, -1, r[1], r[2])
            if r[0] == "resend":
                return (RI_PRE_ACCEPT_OK_AGAIN, -1, -1, r[1], r[2])
            if r[0] == "commit":
                return (RI_COMMIT_BACK, -1, -1, r[1], r[2])
            if r[0] == "nack":
                return (RI_NACK, enc(r[1]), -1, NO_DEPS, -1)
            return (RI_IGNORED, -1, -1, NO_DEPS, -1)
        if kind == IN_ACCEPT:
            r = self.handle_accept(inst, ballot, tid, given, to, key, bool(is_set))
            if r[0] == "commit":
                return (RI_COMMIT_BACK, -1, -1, r[1], r[2])
            if r[0] == "nack":
                return (RI_NACK, enc(r[1]), -1, NO_DEPS, -1)
            return (RI_ACCEPT_OK_AGAIN if r[0] == "again" else RI_ACCEPT_OK, -1, -1, NO_DEPS, -1)
        if kind == IN_COMMIT:
            self.handle_commit(inst, tid, given, [to], key, bool(is_set))
            return (RI_LEARNT, -1, -1, NO_DEPS, -1)
        r = self.prepare(inst, ballot, [to])[to]
        entry = rep.cmd_log.get(inst)
        if r[0] == "commit":                                               # the Commit carries the stored triple (:1744-1755)
            return (RI_COMMIT_BACK, -1, -1, entry.deps, entry.triple_id)
        if r[0] == "nack":
            return (RI_NACK, enc(r[1]), -1, NO_DEPS, -1)
        _, status, vote, triple = r
        if status == ES.NONE:
            return (RI_PREPARE_OK, -1, 0, NO_DEPS, -1)
        return (RI_PREPARE_OK, enc(vote), status, entry.deps, triple)
