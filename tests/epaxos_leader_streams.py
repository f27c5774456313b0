"""epaxos_leader_streams.py -- TEST INFRASTRUCTURE ONLY: seeded streams of leader-side EPaxos traffic (lead calls, bursts of
PreAcceptOk / AcceptOk / Nack / timer events, and acceptor-side calls that take an instance away from its leader), the
runners that play a stream on a model or on the GPU context, and the dependency-set <-> watermark encoding.

A stream is a list of ops:
    ("lead", [(leader, number, at, ballot_ordering, key, is_set, triple_id, avoid_fast_path), ...])
    ("replies", [(kind, to, leader, number, ballot_ordering, ballot_replica, replica_index, seq, watermarks, values_end), ...])
    ("preaccept", (L, x), (bo, br), key, is_set, triple_id, watermarks, values_end, target)     fpx_epx_handle_preaccept
    ("accept", (L, x), (bo, br), triple_id, target, key, is_set)                                fpx_epx_accept
    ("prepare", (L, x), (bo, br), target)                                                       fpx_epx_prepare
    ("commit", (L, x), triple_id, watermarks, values_end, target, key, is_set)                  fpx_epx_handle_commit
The generator drives a LeaderModel of its own only to SHAPE the traffic (which ballot an instance is led in, what its
PreAccept's dependencies are); what a stream's results must be is decided by the models under test.
"""
import random

import numpy as np

from tests import epaxos_leader_model as M


def encode_deps(n, instance, deps):
    """a set of instances -> (watermarks[n], values_end) in the canonical form of include/fpx.h"""
    L, x = instance
    w, end = [0] * n, 0
    for l in range(n):
        col = sorted(y for (ll, y) in deps if ll == l)
        top = 0
        while top < len(col) and col[top] == top:
            top += 1
        rest = col[top:]
        if l == L and rest:
            assert top == x and rest == list(range(x + 1, rest[-1] + 1)), (instance, col)
            end = rest[-1] + 1
        else:
            assert not rest, (instance, l, col)
        w[l] = top
    return w, end


def decode_deps(n, instance, w, end):
    return M.deps_from_message(n, instance, list(w), int(end))


class _Shaper:
    def __init__(self, seed, n, num_keys, num_instances):
        self.rng = random.Random(seed)
        self.n, self.num_keys, self.num_instances = n, num_keys, num_instances
        self.model = M.LeaderModel(n, num_keys, num_instances)
        self.ops = []
        self.next_number = [0] * n
        self.triple = 1000

    def fresh(self, L):
        x = self.next_number[L]
        self.next_number[L] += 1
        assert x < self.num_instances
        return (L, x)

    def lead(self, msgs):
        self.ops.append(("lead", list(msgs)))
        return self.model.lead(msgs)[1]

    def ok(self, inst, at, ballot, q, w, end, seq=0):
        return (M.PRE_ACCEPT_OK, at, inst[0], inst[1], ballot[0], ballot[1], q, seq, list(w), end)

    def accept_ok(self, inst, at, ballot, q):
        return (M.ACCEPT_OK, at, inst[0], inst[1], ballot[0], ballot[1], q, 0, [0] * self.n, 0)

    def nack(self, inst, at, ballot, q):
        return (M.NACK, at, inst[0], inst[1], ballot[0], ballot[1], q, 0, [0] * self.n, 0)

    def timer(self, inst, at):
        return (M.SLOW_PATH_TIMER, at, inst[0], inst[1], 0, 0, 0, 0, [0] * self.n, 0)

    def bump(self, inst, w, end):
        """other dependencies than (w, end): one more id on a column that is not the instance's own"""
        l = self.rng.choice([c for c in range(self.n) if c != inst[0]])
        w2 = list(w)
        w2[l] += 1 + self.rng.randrange(2)
        return w2, end


SCENARIOS = ("agree", "disagree", "dup", "ballots", "nacks", "timer", "own", "own_column", "seq", "avoid", "early_accept_ok",
             "interfere_preaccept", "interfere_accept", "interfere_prepare", "interfere_commit", "late", "relead")


def make_stream(seed, n, num_keys=4, num_instances=64, per_round=None, rounds=2, scenarios=SCENARIOS):
    """rounds x (lead a batch, [take some instances away], one burst of replies)"""
    S = _Shaper(seed, n, num_keys, num_instances)
    rng = S.rng
    per_round = per_round or len(scenarios)
    slow, fast = (n - 1) // 2 + 1, n - 1
    for rnd in range(rounds):
        # ---- lead a batch: mostly a replica's own fresh instances in its default ballot; some at another replica in a higher
        # ballot, avoiding the fast path (what a recovery does)
        batch = []
        for j in range(per_round):
            sc = scenarios[(j + rnd) % len(scenarios)] if j < len(scenarios) else rng.choice(scenarios)
            L = rng.randrange(n)
            inst = S.fresh(L)
            at, bo, avoid = L, 0, sc == "avoid"
            if sc == "ballots" or rng.random() < 0.15:
                at, bo = rng.randrange(n), 1 + rng.randrange(3)
                avoid = avoid or rng.random() < 0.5
            key = -1 if rng.random() < 0.1 else rng.randrange(num_keys)
            S.triple += 1
            batch.append((sc, inst, at, (bo, at), key, rng.randrange(2), S.triple, int(avoid)))
        deps = S.lead([(i[0], i[1], at, b[0], key, s, t, a) for (_, i, at, b, key, s, t, a) in batch])
        per_instance, between = [], []
        for (sc, inst, at, ballot, key, is_set, tid, avoid), d in zip(batch, deps):
            w, end = encode_deps(n, inst, d)
            peers = [r for r in range(n) if r != at]
            rng.shuffle(peers)
            quorum = peers[:fast - 1]
            msgs = []
            if sc in ("agree", "avoid", "late", "relead"):
                msgs = [S.ok(inst, at, ballot, q, w, end) for q in quorum]
                if sc == "late":
                    msgs.append(S.ok(inst, at, ballot, peers[-1], w, end))           # after the decision: ignored
                    msgs.append(S.accept_ok(inst, at, ballot, peers[0]))
                    msgs.append(S.timer(inst, at))                                   # the timer after the decision: fatal
                if sc == "relead":
                    msgs = [S.nack(inst, at, (ballot[0] + 1, peers[0]), peers[0])] + msgs[:1]
            elif sc in ("disagree", "early_accept_ok"):
                msgs = [S.ok(inst, at, ballot, q, w, end) for q in quorum]
                msgs[-1] = S.ok(inst, at, ballot, quorum[-1], *S.bump(inst, w, end))
                if sc == "early_accept_ok":
                    msgs.insert(0, S.accept_ok(inst, at, ballot, quorum[0]))         # before the Accept phase: ignored
                msgs += [S.accept_ok(inst, at, ballot, q) for q in peers[:slow]]     # one more than needed: ignored
            elif sc == "dup":
                w2, e2 = S.bump(inst, w, end)
                first, last = ((w2, e2), (w, end)) if rng.random() < 0.5 else ((w, end), (w2, e2))
                msgs = [S.ok(inst, at, ballot, quorum[0], *first), S.ok(inst, at, ballot, quorum[0], *last)]
                msgs += [S.ok(inst, at, ballot, q, w, end) for q in quorum[1:]]
                msgs.append(S.ok(inst, at, ballot, quorum[0], *last))
            elif sc == "ballots":
                msgs = [S.ok(inst, at, (ballot[0] - 1, ballot[1]), quorum[0], w, end),    # stale: ignored
                        S.ok(inst, at, (ballot[0] + 1, ballot[1]), quorum[0], w, end),    # too large: checkLt
                        S.accept_ok(inst, at, (ballot[0] + 1, ballot[1]), quorum[0], ),
                        S.ok(inst, at, ballot, quorum[0], *S.bump(inst, w, end))]
                msgs += [S.ok(inst, at, ballot, q, w, end) for q in quorum[1:]]
                msgs += [S.accept_ok(inst, at, (ballot[0] - 1, ballot[1]), peers[0]),
                         S.accept_ok(inst, at, (ballot[0] + 2, 0), peers[0])]
                msgs += [S.accept_ok(inst, at, ballot, q) for q in peers[:slow - 1]]
            elif sc == "nacks":
                other = ((inst[0] + 1) % n, num_instances - 1)                            # never led
                msgs = [S.nack(other, at, (5, rng.randrange(n)), peers[0]),
                        S.nack(inst, at, ballot, peers[0]),                               # not above the ballot led in
                        S.nack(inst, at, (ballot[0] + 2, peers[0]), peers[0]),
                        S.ok(inst, at, ballot, quorum[0], w, end)]
            elif sc == "timer":
                msgs = [S.timer(inst, at)]                                                # before a slow quorum: logger.check
                msgs += [S.ok(inst, at, ballot, q, w, end) for q in quorum[:slow - 1]]
                msgs += [S.timer(inst, at), S.timer(inst, at)]
                msgs += [S.accept_ok(inst, at, ballot, q) for q in peers[:slow - 1]]
            elif sc == "own":
                w2, e2 = S.bump(inst, w, end)
                msgs = [S.ok(inst, at, ballot, at, w2, e2)]                               # replaces the leader's own response
                msgs += [S.ok(inst, at, ballot, q, w, end) for q in quorum]
            elif sc == "own_column":
                # agreement that holds only because a cover of x and of x + 1 are the same set on the own column
                L, x = inst
                covers = [x, x + 1]
                msgs = []
                for j, q in enumerate(quorum):
                    w2 = list(w)
                    w2[L] = covers[j % 2]
                    msgs.append(S.ok(inst, at, ballot, q, w2, 0))
            elif sc == "seq":
                msgs = [S.ok(inst, at, ballot, q, w, end, seq=(3 if j == 0 else 0)) for j, q in enumerate(quorum)]
                msgs += [S.accept_ok(inst, at, ballot, q) for q in peers[:slow - 1]]
            else:  # interfere_*: the instance is taken away from its leader between lead and the replies
                high = (ballot[0] + 1, peers[0])
                if sc == "interfere_preaccept":
                    between.append(("preaccept", inst, high, key, is_set, tid + 500, [0] * n, 0, at))
                elif sc == "interfere_accept":
                    between.append(("accept", inst, high, tid + 500, at, key, is_set))
                elif sc == "interfere_prepare":
                    between.append(("prepare", inst, high, at))
                else:
                    between.append(("commit", inst, tid, w, end, at, key, is_set))
                msgs = [S.ok(inst, at, ballot, q, w, end) for q in quorum]
                msgs += [S.nack(inst, at, high, peers[0]), S.accept_ok(inst, at, ballot, peers[0])]
            per_instance.append(msgs)
        rng.shuffle(between)
        for op in between:
            S.ops.append(op)
            run_op(S.model, op)
        # one burst: the instances' messages interleaved, each instance's own order kept
        burst, cursors = [], [0] * len(per_instance)
        live = [k for k, msgs in enumerate(per_instance) if msgs]
        while live:
            k = rng.choice(live)
            burst.append(per_instance[k][cursors[k]])
            cursors[k] += 1
            if cursors[k] == len(per_instance[k]):
                live.remove(k)
        S.ops.append(("replies", burst))
        S.model.replies(burst)
        # lead again, in a higher ballot, what a Nack stopped (scenario "relead")
        again = []
        for (sc, inst, at, ballot, key, is_set, tid, avoid) in batch:
            if sc == "relead":
                again.append((inst, at, (ballot[0] + 2, at), key, is_set, tid, 1))
        if again:
            deps = S.lead([(i[0], i[1], at, b[0], key, s, t, a) for (i, at, b, key, s, t, a) in again])
            burst = []
            for (inst, at, ballot, key, is_set, tid, avoid), d in zip(again, deps):
                if d is None:                            # (n = 3: the one answer after the Nack already committed it)
                    continue
                w, end = encode_deps(n, inst, d)
                peers = [r for r in range(n) if r != at]
                burst += [S.ok(inst, at, ballot, q, w, end) for q in peers[:slow - 1]]
                burst += [S.accept_ok(inst, at, ballot, q) for q in peers[:slow - 1]]
            S.ops.append(("replies", burst))
            S.model.replies(burst)
            # and once more on a committed instance: transitionToPreAcceptPhase dies (:663-667)
            inst, at, ballot, key, is_set, tid, avoid = again[0]
            S.lead([(inst[0], inst[1], at, ballot[0] + 1, key, is_set, tid, 0)])
    return S.ops


# ---- runners ---------------------------------------------------------------------------------------------------------------
def run_op(model, op):
    """one op on a LeaderModel; lead / replies results in encoded (array) form"""
    n = model.n
    kind = op[0]
    if kind == "lead":
        st, deps = model.lead(op[1])
        if st == M.EINVAL:
            return (st, None)
        rows = []
        for msg, d in zip(op[1], deps):
            rows.append(([0] * n, 0) if d is None else encode_deps(n, (msg[0], msg[1]), d))
        return (st, rows)
    if kind == "replies":
        st, out, decided = model.replies(op[1])
        if st == M.EINVAL:
            return (st, None, None)
        rows = []
        for msg, (outcome, seq, d, tid) in zip(op[1], out):
            w, end = ([0] * n, 0) if d is None else encode_deps(n, (msg[2], msg[3]), d)
            rows.append((outcome, seq, w, end, tid))
        return (st, rows, decided)
    if kind == "preaccept":
        _, inst, ballot, key, is_set, tid, w, end, target = op
        model.peer_preaccept(inst, ballot, key, bool(is_set), tid, decode_deps(n, inst, w, end), [target])
    elif kind == "accept":
        _, inst, ballot, tid, target, key, is_set = op
        model.peer_accept(inst, ballot, tid, [target], key, bool(is_set))
    elif kind == "prepare":
        _, inst, ballot, target = op
        model.peer_prepare(inst, ballot, [target])
    elif kind == "commit":
        _, inst, tid, w, end, target, key, is_set = op
        model.peer_commit(inst, tid, decode_deps(n, inst, w, end), [target], key, bool(is_set))
    else:
        raise ValueError(kind)
    return None


def run_model(model, ops):
    return [run_op(model, op) for op in ops]


def burst_arrays(n, msgs):
    """the arrays of fpx_epx_leader_replies for a list of message tuples"""
    cols = list(zip(*[m[:8] for m in msgs])) if msgs else [[]] * 8
    a = [np.asarray(c, np.int32) for c in cols]
    deps = np.asarray([m[8] for m in msgs], np.int32).reshape(len(msgs), n)
    dend = np.asarray([m[9] for m in msgs], np.int32)
    return a + [deps, dend]


def run_gpu_op(epx, op):
    """the same op on a frankenpaxos_amd.EPaxos context (leader_state=True), results in the form run_op gives"""
    n = epx.n
    kind = op[0]
    if kind == "lead":
        cols = [np.asarray(c, np.int32) for c in zip(*op[1])]
        st, deps, dend = epx.lead(cols[0], cols[1], cols[2], cols[3], cols[4], cols[5].astype(np.uint8), cols[6],
                                  cols[7].astype(np.uint8))
        if st == M.EINVAL:
            return (st, None)
        return (st, [([int(v) for v in deps[i]], int(dend[i])) for i in range(len(op[1]))])
    if kind == "replies":
        a = burst_arrays(n, op[1])
        st, outcome, oseq, odeps, oend, otr, dec = epx.leader_replies(*a)
        if st == M.EINVAL:
            return (st, None, None)
        rows = [(int(outcome[i]), int(oseq[i]), [int(v) for v in odeps[i]], int(oend[i]), int(otr[i])) for i in range(len(op[1]))]
        return (st, rows, [int(v) for v in dec])
    one = lambda v: np.asarray([v], np.int32)
    if kind == "preaccept":
        _, inst, ballot, key, is_set, tid, w, end, target = op
        epx.handle_preaccept(one(inst[0]), one(inst[1]), one(ballot[0]), one(ballot[1]), one(key), [is_set], one(tid),
                             np.asarray([w], np.int32), one(end), [1 << target])
    elif kind == "accept":
        _, inst, ballot, tid, target, key, is_set = op
        epx.accept(one(inst[0]), one(inst[1]), one(ballot[0]), one(ballot[1]), one(tid), [1 << target], one(key), [is_set])
    elif kind == "prepare":
        _, inst, ballot, target = op
        epx.prepare(one(inst[0]), one(inst[1]), one(ballot[0]), one(ballot[1]), [1 << target])
    elif kind == "commit":
        _, inst, tid, w, end, target, key, is_set = op
        epx.handle_commit(one(inst[0]), one(inst[1]), one(tid), [1 << target], one(key), [is_set], np.asarray([w], np.int32),
                          one(end))
    else:
        raise ValueError(kind)
    return None


def run_gpu(epx, ops):
    return [run_gpu_op(epx, op) for op in ops]


def touched(ops, step=1):
    """the (replica, instance) cells a stream can have written (every step-th of them), and the keys it names"""
    cells, keys = set(), set()
    for op in ops:
        if op[0] == "lead":
            for msg in op[1]:
                cells.add((msg[2], (msg[0], msg[1])))
                keys.add(msg[4])
        elif op[0] == "replies":
            for msg in op[1]:
                cells.add((msg[1], (msg[2], msg[3])))
        elif op[0] == "preaccept":
            cells.add((op[8], op[1]))
        elif op[0] == "accept":
            cells.add((op[4], op[1])), cells.add((op[2][1], op[1]))
        elif op[0] == "prepare":
            cells.add((op[3], op[1]))
        elif op[0] == "commit":
            cells.add((op[5], op[1]))
    return sorted(cells)[::step], sorted(k for k in keys if k >= 0)


def model_state(model, ops, step=1):
    """what the GPU readbacks show, from a LeaderModel: per touched cell the command-log entry (kind, ballot, vote ballot,
    triple id), its dependencies (or None: known by id) and the leader state; per replica largestBallot; per (replica, key)
    the conflict index"""
    n = model.n
    enc = lambda b: -1 if b == (-1, -1) else b[0] * 8 + b[1]
    cells, keys = touched(ops, step)
    out = {}
    for (r, inst) in cells:
        e = model.replicas[r].cmd_log.get(inst)
        if e is None:
            entry, deps = (0, -1, -1, -1), None
        else:
            entry = (e.kind, enc(e.ballot), enc(e.vote_ballot), e.triple_id)
            deps = None if e.deps is None else encode_deps(n, inst, e.deps)
        st = model.leader_states[r].get(inst)
        if st is None:
            ls = (0,)
        elif isinstance(st, M.PreAccepting):
            resp = {q: (s,) + tuple(x for x in _flat(encode_deps(n, inst, d))) for q, (s, d) in st.responses.items()}
            ls = (1, enc(st.ballot), int(st.avoid_fast_path), st.triple_id, st.key, int(st.is_set), resp)
        else:
            s, d = st.triple
            ls = (2, enc(st.ballot), st.triple_id, st.key, int(st.is_set), sorted(st.responses),
                  (s,) + tuple(_flat(encode_deps(n, inst, d))))
        out[(r, inst)] = (entry, deps, ls)
    largest = [enc(rep.largest_ballot) for rep in model.replicas]
    index = {(r, k): (list(model.replicas[r].gets[k]), list(model.replicas[r].sets[k])) for r in range(n) for k in keys}
    return out, largest, index


def _flat(we):
    return list(we[0]) + [we[1]]


def gpu_state(epx, ops, step=1):
    n = epx.n
    cells, keys = touched(ops, step)
    out = {}
    largest = [None] * n
    for (r, inst) in cells:
        kind, ballot, vote, tid, lg = epx.read_cmdlog(r, inst[0], inst[1])
        largest[r] = lg
        d, dend = epx.read_cmdlog_deps(r, inst[0], inst[1])
        deps = None if (kind == 0 or d[0] == -1) else ([int(v) for v in d], dend)
        if kind == 0:
            ballot = vote = tid = -1
        head, resp = epx.read_leader_state(r, inst[0], inst[1])
        phase, lb, avoid, ltid, key, is_set, mask = head[:7]
        if phase == 0:
            ls = (0,)
        elif phase == 1:
            ls = (1, lb, avoid, ltid, key, is_set,
                  {q: tuple(int(v) for v in resp[q]) for q in range(n) if (mask >> q) & 1})
        else:
            ls = (2, lb, ltid, key, is_set, [q for q in range(n) if (mask >> q) & 1], tuple(int(v) for v in resp[r]))
        out[(r, inst)] = ((kind, ballot, vote, tid), deps, ls)
    for r in range(n):
        if largest[r] is None:
            largest[r] = epx.read_cmdlog(r, 0, 0)[4]
    index = {}
    for r in range(n):
        for k in keys:
            g, s = epx.read_index(r, k)
            index[(r, k)] = ([int(v) for v in g], [int(v) for v in s])
    return out, largest, index
