"""Two independently written models of fpx_acceptor_inbox (include/fpx.h) for the tests:

  Sequential  a message at a time on oracle/multipaxos_maps.Acceptor objects (shaped like multipaxos/Acceptor.scala:95-254,
              one object per (group, index) with `round`, a `states` map and `maxVotedSlot`), plus the two read handlers
              (:222-254), which answer with maxVotedSlot and change nothing.
  Arrays      vectorised numpy on flat state: the messages of every acceptor brought together in delivery order, the
              round each meets as the exclusive running maximum of the earlier Phase1a / Phase2a rounds started at the
              acceptor's, accept = round >= that, maxVotedSlot likewise over the accepted slots, and the cells by
              last-accepted-writer-wins.

Both hold their state between bursts, refuse a bad burst as a whole (status 1, the lowest offending index, nothing
applied) and export the state as the arrays Context.read_scalars / read_state return.
"""
import numpy as np

from frankenpaxos_amd import wire
from oracle.multipaxos_maps import Acceptor

P2A, P1A, MSR, BMSR, OTHER = (wire.PHASE2A, wire.PHASE1A, wire.MAX_SLOT_REQUEST, wire.BATCH_MAX_SLOT_REQUEST,
                              wire.OTHER)
PHASE2B, NACK, PHASE1B = wire.PHASE2B, wire.NACK, wire.PHASE1B
MAX_ROUND = 2**30 - 2
EINVAL = 1


def entry_of(b, i):
    """(group, replica) of the acceptor message i was delivered to, or None"""
    g, a = int(b.group[i]), int(b.acceptor[i])
    if a < 0 or g < 0:
        return None
    if b.grid_cols:
        if a >= b.grid_cols or g * b.grid_cols + a >= b.R:
            return None
        return 0, g * b.grid_cols + a
    if a >= b.R or g >= b.groups:
        return None
    return g, a


def first_bad(b):
    for i in range(len(b)):
        k = int(b.kind[i])
        if k == OTHER:
            continue
        if k not in (P2A, P1A, MSR, BMSR):
            return i
        e = entry_of(b, i)
        if e is None:
            return i
        if k in (P2A, P1A) and not 0 <= int(b.round[i]) <= MAX_ROUND:
            return i
        if k == P2A and (not 0 <= int(b.slot[i]) < b.S or int(b.slot[i]) % b.groups != e[0]):
            return i
    return -1


class Sequential:
    def __init__(self, R, groups, S):
        self.R, self.groups, self.S = R, groups, S
        self.acceptors = {(g, r): Acceptor(g, r) for g in range(groups) for r in range(R)}

    def run(self, b):
        """-> (status, bad_index, reply_kind, reply_value)"""
        n = len(b)
        bad = first_bad(b)
        if bad >= 0:
            return EINVAL, bad, None, None
        rk, rv = np.zeros(n, np.int32), np.full(n, -1, np.int32)
        for i in range(n):
            k = int(b.kind[i])
            if k == OTHER:
                continue
            acc = self.acceptors[entry_of(b, i)]
            if k == P2A:
                out = acc.handle_phase2a(int(b.slot[i]), int(b.round[i]), int(b.value[i]))
                rk[i], rv[i] = (NACK, out[1]) if out[0] == "nack" else (PHASE2B, b.round[i])
            elif k == P1A:
                out = acc.handle_phase1a(int(b.round[i]))
                rk[i], rv[i] = (NACK, out[1]) if out[0] == "nack" else (PHASE1B, b.round[i])
            else:
                rk[i], rv[i] = MSR, acc.max_voted_slot          # Acceptor.scala:233, :250
        return 0, -1, rk, rv

    def scalars(self):
        pr = np.array([[self.acceptors[g, r].round for r in range(self.R)] for g in range(self.groups)], np.int32)
        mv = np.array([[self.acceptors[g, r].max_voted_slot for r in range(self.R)] for g in range(self.groups)], np.int32)
        return pr, mv

    def cells(self):
        vr, vv = np.full((self.S, self.R), -1, np.int32), np.full((self.S, self.R), -1, np.int32)
        for (g, r), acc in self.acceptors.items():
            for s, (round_, value) in acc.states.items():
                assert s % self.groups == g
                vr[s, r], vv[s, r] = round_, value
        return vr, vv


class Arrays:
    def __init__(self, R, groups, S):
        self.R, self.groups, self.S = R, groups, S
        self.promised = np.full(groups * R, -1, np.int64)
        self.max_voted = np.full(groups * R, -1, np.int64)
        self.vr, self.vv = np.full((S, R), -1, np.int32), np.full((S, R), -1, np.int32)

    def run(self, b):
        n = len(b)
        kind, slot, rnd = b.kind.astype(np.int64), b.slot.astype(np.int64), b.round.astype(np.int64)
        g, a = b.group.astype(np.int64), b.acceptor.astype(np.int64)
        live = kind != OTHER
        moves, reads = (kind == P2A) | (kind == P1A), (kind == MSR) | (kind == BMSR)
        if b.grid_cols:
            rep = g * b.grid_cols + a
            ok_idx = (a >= 0) & (g >= 0) & (a < b.grid_cols) & (rep < self.R)
            ent = rep
        else:
            ok_idx = (a >= 0) & (g >= 0) & (a < self.R) & (g < self.groups)
            ent = g * self.R + a
        bad = live & ~(moves | reads)
        bad |= live & ~ok_idx
        bad |= moves & ((rnd < 0) | (rnd > MAX_ROUND))
        p2a = kind == P2A
        bad |= p2a & ((slot < 0) | (slot >= self.S))
        bad |= p2a & ok_idx & (slot % self.groups != ent // self.R)
        if bad.any():
            return EINVAL, int(np.flatnonzero(bad)[0]), None, None
        rk, rv = np.zeros(n, np.int32), np.full(n, -1, np.int32)
        idx = np.flatnonzero(live)
        order = idx[np.argsort(ent[idx], kind="stable")]          # every acceptor's messages together, in delivery order
        keys = ent[order]
        starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]]) if len(order) else np.array([], np.int64)
        for lo, hi in zip(starts, np.r_[starts[1:], len(order)]):
            e, m = int(keys[lo]), order[lo:hi]
            r = np.where(moves[m], rnd[m], -1)
            met = np.maximum.accumulate(np.r_[self.promised[e], r])[:-1]      # exclusive, started at the acceptor's round
            acc = moves[m] & (r >= met)
            nack = moves[m] & ~acc
            rk[m[nack]], rv[m[nack]] = NACK, met[nack]
            rk[m[acc]] = np.where(kind[m[acc]] == P2A, PHASE2B, PHASE1B)
            rv[m[acc]] = r[acc]
            voted = acc & p2a[m]
            s = np.where(voted, slot[m], -1)
            seen = np.maximum.accumulate(np.r_[self.max_voted[e], s])[:-1]
            rd = reads[m]
            rk[m[rd]], rv[m[rd]] = MSR, seen[rd]
            self.promised[e] = max(self.promised[e], r.max())
            self.max_voted[e] = max(self.max_voted[e], s.max())
            w = m[voted]                                           # ascending index: a later assignment wins
            if len(w):
                # the last accepted Phase2a of every slot: the first occurrence in the reversed list
                sl, first = np.unique(slot[w][::-1], return_index=True)
                win = w[::-1][first]
                self.vr[sl, e % self.R], self.vv[sl, e % self.R] = b.round[win], b.value[win]
        return 0, -1, rk, rv

    def scalars(self):
        return (self.promised.reshape(self.groups, self.R).astype(np.int32),
                self.max_voted.reshape(self.groups, self.R).astype(np.int32))

    def cells(self):
        return self.vr.copy(), self.vv.copy()


def assert_same_state(a, b, what=""):
    for x, y, name in zip(a.scalars() + a.cells(), b.scalars() + b.cells(), ("promised", "max_voted", "vote_round", "vote_value")):
        np.testing.assert_array_equal(x, y, err_msg="%s %s" % (what, name))


def conditions(b, model_before, rk, rv):
    """what a burst reaches, as counts, from the replies of a model that started at `model_before`'s state (a Sequential
    BEFORE the burst ran; it is not changed): see tests/test_acceptor_inbox_cpu.py"""
    pr0, mv0 = model_before.scalars()
    twin = Sequential(model_before.R, model_before.groups, model_before.S)
    for key, acc in model_before.acceptors.items():
        t = twin.acceptors[key]
        t.round, t.max_voted_slot, t.states = acc.round, acc.max_voted_slot, dict(acc.states)
    st, _, rk2, rv2 = twin.run(b)
    assert st == 0 and (rk2 == rk).all() and (rv2 == rv).all()
    _, mv1 = twin.scalars()
    c = dict(nacks=0, rewritten_cells=0, equal_round_other_value=0, p1a_promised=0, p1a_nacked=0, p1a_then_nacked_p2a=0,
             reads_in_between=0)
    last = {}          # (entry, slot) -> (round, value) of the last accepted Phase2a of the burst
    raised_by_p1a = {}  # entry -> the round a Phase1a of this burst left it at (dropped when a Phase2a moves it on)
    for i in range(len(b)):
        k = int(b.kind[i])
        if k == OTHER:
            continue
        e = entry_of(b, i)
        if rk[i] == NACK:
            c["nacks"] += 1
            if k == P1A:
                c["p1a_nacked"] += 1
            elif raised_by_p1a.get(e) == rv[i]:
                c["p1a_then_nacked_p2a"] += 1
        elif k == P1A:
            c["p1a_promised"] += 1
            raised_by_p1a[e] = int(b.round[i])
        elif k == P2A:
            key = (e, int(b.slot[i]))
            if key in last:
                c["rewritten_cells"] += 1
                if last[key][0] == b.round[i] and last[key][1] != b.value[i]:
                    c["equal_round_other_value"] += 1
            last[key] = (int(b.round[i]), int(b.value[i]))
            if raised_by_p1a.get(e) is not None and b.round[i] > raised_by_p1a[e]:
                del raised_by_p1a[e]
        else:
            if rv[i] != mv0[e] and rv[i] != mv1[e]:
                c["reads_in_between"] += 1
    return c
