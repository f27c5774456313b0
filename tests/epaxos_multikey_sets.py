"""epaxos_multikey_sets.py -- test infrastructure: oracle/epaxos_sets.py's explicit-set restatement of EPaxos with
MULTI-KEY commands.  A command is a tuple of keys plus get / set; None is a Noop.

statemachine/KeyValueStore.scala:221-302 (typedTopKConflictIndex, k = 1) merges the per-key TopOne's of all of a
command's keys: a get with the sets of its keys, a set with their gets and sets (TopOne.mergeEquals, an element-wise
max); put records the instance under every key.  Zero keys merge nothing (the snapshots, which EPaxos never fills) and
put nothing; a repeated key merges and puts the same thing twice.  The handlers are oracle/epaxos_sets.py's, with the
key tuple where that file has one key.  Pure-Python loops: small cases only."""
from oracle.epaxos_sets import ACCEPTED, COMMITTED, PRE_ACCEPTED, Entry
from oracle import epaxos_sets as base


_PREFIXES = {}


def prefix_set(leader, top):
    """{(leader, x) : x < top}, built once: the sets below are unions of these (explicit sets still, only faster)"""
    s = _PREFIXES.get((leader, top))
    if s is None:
        s = _PREFIXES[(leader, top)] = frozenset((leader, x) for x in range(top))
    return s


class Replica(base.Replica):
    def top_one_conflicts(self, keys, is_set):
        merged = [0] * self.n
        for k in keys:
            merged = [max(a, b) for a, b in zip(merged, self.sets[k])]
            if is_set:
                merged = [max(a, b) for a, b in zip(merged, self.gets[k])]
        return merged

    def index_put(self, keys, is_set, instance):
        leader, number = instance
        for k in keys:
            row = (self.sets if is_set else self.gets)[k]
            row[leader] = max(row[leader], number + 1)

    def compute_dependencies(self, instance, keys, is_set):
        if keys is None:                                    # Noop (:592-593)
            return set()
        top = self.top_one_conflicts(keys, is_set)
        deps = set().union(*(prefix_set(l, top[l]) for l in range(self.n)))
        deps.discard(instance)                              # subtractOne (:582)
        return deps


class EPaxos(base.EPaxos):
    def __init__(self, n, num_keys):
        self.n, self.f = n, (n - 1) // 2
        self.replicas = [Replica(r, n, num_keys) for r in range(n)]

    def tick(self, leader, number, keys, is_set, resp_mask, rank, seen_mask=None, triple_id=None):
        """keys[i]: command i's key tuple; returns per message (fast, deps, leader_deps) with deps as sets"""
        m, n = len(leader), self.n
        seen_mask = resp_mask if seen_mask is None else seen_mask
        local = [[None] * n for _ in range(m)]
        for r, rep in enumerate(self.replicas):
            for i in sorted(range(m), key=lambda i: rank[r][i]):
                inst = (int(leader[i]), int(number[i]))
                if r != inst[0] and not (int(seen_mask[i]) >> r) & 1:
                    continue
                assert inst not in rep.cmd_log
                local[i][r] = rep.compute_dependencies(inst, tuple(keys[i]), bool(is_set[i]))
                rep.index_put(tuple(keys[i]), bool(is_set[i]), inst)
        out = []
        for i in range(m):
            L = int(leader[i])
            inst = (L, int(number[i]))
            D = local[i][L]
            answers = {r: local[i][r] | D for r in range(n) if r != L and (int(seen_mask[i]) >> r) & 1}
            first_quorum = [answers[r] for r in range(n) if (int(resp_mask[i]) >> r) & 1]
            fast = all(a == first_quorum[0] for a in first_quorum)
            deps = first_quorum[0] if fast else set().union(D, *first_quorum)
            tid = -1 if triple_id is None else int(triple_id[i])
            for r, rep in enumerate(self.replicas):
                if fast:
                    rep.cmd_log[inst] = Entry(COMMITTED, triple_id=tid, deps=frozenset(deps))
                elif r == L:
                    rep.cmd_log[inst] = Entry(PRE_ACCEPTED, (0, L), (0, L), tid, frozenset(D))
                elif r in answers:
                    rep.cmd_log[inst] = Entry(PRE_ACCEPTED, (0, L), (0, L), tid, frozenset(answers[r]))
            out.append((fast, deps, D))
        for rep in self.replicas:
            for i in range(m):
                rep.index_put(tuple(keys[i]), bool(is_set[i]), (int(leader[i]), int(number[i])))
        return out

    def handle_preaccept(self, instance, ballot, keys, is_set, triple_id, deps_in, targets):
        replies = {}
        for r in targets:
            rep = self.replicas[r]
            e = rep.cmd_log.get(instance)
            if e is not None:
                if e.kind == COMMITTED:
                    replies[r] = ("commit", e.deps, e.triple_id)
                    continue
                if ballot < e.ballot:
                    replies[r] = ("nack", rep.largest_ballot)
                    continue
                if e.kind == PRE_ACCEPTED and ballot == e.vote_ballot:
                    replies[r] = ("resend", e.deps, e.triple_id)
                    continue
                if e.kind == ACCEPTED and ballot == e.vote_ballot:
                    replies[r] = ("ignore",)
                    continue
            rep.largest_ballot = max(rep.largest_ballot, ballot)
            deps = rep.compute_dependencies(instance, keys, is_set) | set(deps_in)
            rep.cmd_log[instance] = Entry(PRE_ACCEPTED, ballot, ballot, triple_id, frozenset(deps))
            if keys is not None:
                rep.index_put(keys, is_set, instance)
            replies[r] = ("ok", frozenset(deps), triple_id)
        return replies

    def accept(self, instance, ballot, triple_id, targets, keys=None, is_set=False):
        """returns (fatal, replies, committed); keys None: a Noop, nothing to put"""
        P = ballot[1]
        prop = self.replicas[P]
        put = lambda rep: rep.index_put(keys, is_set, instance) if keys is not None else None
        e = prop.cmd_log.get(instance)
        if e is not None and (e.kind == COMMITTED or e.ballot > ballot or
                              (e.kind in (PRE_ACCEPTED, ACCEPTED) and e.vote_ballot > ballot)):
            return True, {}, False
        prop.cmd_log[instance] = Entry(ACCEPTED, ballot, ballot, triple_id, None)
        put(prop)
        replies = {P: ("ok",)}
        for r in targets:
            rep = self.replicas[r]
            e = rep.cmd_log.get(instance)
            if e is not None and e.kind == COMMITTED:
                replies[r] = ("commit",)
            elif e is not None and ballot < e.ballot:
                replies[r] = ("nack", rep.largest_ballot)
            elif e is not None and e.kind == ACCEPTED and ballot == e.vote_ballot:
                replies[r] = ("ok",)
            else:
                rep.largest_ballot = max(rep.largest_ballot, ballot)
                rep.cmd_log[instance] = Entry(ACCEPTED, ballot, ballot, triple_id, None)
                put(rep)
                replies[r] = ("ok",)
        committed = len([r for r, v in replies.items() if v[0] == "ok"]) >= self.f + 1
        if committed:
            for rep in self.replicas:
                rep.cmd_log[instance] = Entry(COMMITTED, triple_id=triple_id, deps=None)
                put(rep)
        return False, replies, committed

    def handle_commit(self, instance, triple_id, deps, targets, keys=None, is_set=False):
        for r in targets:
            rep = self.replicas[r]
            rep.cmd_log[instance] = Entry(COMMITTED, triple_id=triple_id, deps=None if deps is None else frozenset(deps))
            if keys is not None:
                rep.index_put(keys, is_set, instance)


def csr(key_lists):
    """[[k, ...], ...] -> (key_offsets[m + 1], keys) as the _mk entry points take them"""
    import numpy as np

    off = np.zeros(len(key_lists) + 1, np.int32)
    off[1:] = np.cumsum([len(k) for k in key_lists])
    keys = np.array([k for ks in key_lists for k in ks], np.int32)
    return off, keys
