"""epaxos_inbox_streams.py -- TEST INFRASTRUCTURE ONLY: seeded bursts of peer messages for fpx_epx_replica_inbox (PreAccept,
Accept, Commit, Prepare, interleaved, instances and keys repeated), their packing into the call's arrays, the census of what
a burst exercises, and the readback of the state a burst touched from the model and from the GPU context.

A message is the tuple of tests/epaxos_inbox_model.py:
    (kind, to, leader, number, ballot_ordering, ballot_replica, key, is_set, triple_id, watermarks, values_end)
"""
import random

import numpy as np

from oracle import epaxos_sets as ES
from tests import epaxos_inbox_model as IM
from tests.epaxos_leader_streams import decode_deps, encode_deps  # noqa: F401  (the encoding is shared)


def _deps(rng, n, inst, span, kind):
    """dependencies of a valid shape for the message kind: (watermarks, values_end)"""
    L, x = inst
    if kind in (IM.IN_ACCEPT, IM.IN_COMMIT) and rng.random() < 0.3:
        return [-1] + [0] * (n - 1), 0                       # the triple is known by its id alone
    w = [rng.randrange(span + 1) for _ in range(n)]
    end = 0
    roll = rng.random()
    if roll < 0.4:
        w[L] = rng.randrange(x + 1)                          # a plain watermark, not above the instance
    elif roll < 0.8 or kind == IM.IN_PRE_ACCEPT:
        w[L], end = x, x + 2 + rng.randrange(3)              # explicit ids above the instance
    else:
        w[L] = x + 1 + rng.randrange(3)                      # a cover above the instance (a Commit's / an Accept's may)
    return w, end


def make_burst(seed, n, m, num_keys=4, num_instances=64, hot_key=None, hot_to=None, first_triple=1000, max_ordering=3):
    """m messages: scripts of 1 .. 9 messages on one cell (to, leader, number) each, interleaved with every script's own
    order kept.  Cells come from a pool small enough that instances repeat across scripts and across receivers."""
    rng = random.Random(seed)
    span = max(2, min(num_instances, max(4, m // 8)))
    scripts, total, tid = [], 0, first_triple
    while total < m:
        inst = (rng.randrange(n), rng.randrange(span))
        to = rng.randrange(n) if hot_to is None else hot_to
        key = -1 if rng.random() < 0.1 else rng.randrange(num_keys)
        if hot_key is not None:
            key = hot_key
        is_set = rng.randrange(2)
        length = min(m - total, 1 + min(rng.randrange(9), rng.randrange(9)))
        script = []
        for _ in range(length):
            kind = rng.choices((IM.IN_PRE_ACCEPT, IM.IN_ACCEPT, IM.IN_COMMIT, IM.IN_PREPARE), (40, 25, 10, 25))[0]
            if script and rng.random() < 0.4:                # a re-sent message, or the next phase in the same ballot
                bo, br = script[-1][4], script[-1][5]
            else:
                bo, br = rng.randrange(max_ordering + 1), rng.randrange(n)
            tid += 1
            w, end = _deps(rng, n, inst, span, kind)
            script.append((kind, to, inst[0], inst[1], bo, br, key, is_set, tid, w, end))
        scripts.append(script)
        total += length
    burst, cursors = [], [0] * len(scripts)
    live = list(range(len(scripts)))
    while live:
        k = rng.choice(live)
        burst.append(scripts[k][cursors[k]])
        cursors[k] += 1
        if cursors[k] == len(scripts[k]):
            live.remove(k)
    return burst


def long_run(n, length, key=1):
    """`length` messages on ONE cell, every kind and outcome among them: ballots climb slowly, so most messages repeat or
    fall behind; the Commit comes late"""
    rng = random.Random(length)
    to, inst = 1, (0, 3)
    out = []
    for j in range(length):
        kind = (IM.IN_PRE_ACCEPT, IM.IN_PRE_ACCEPT, IM.IN_ACCEPT, IM.IN_ACCEPT, IM.IN_PREPARE, IM.IN_PRE_ACCEPT)[j % 6]
        if j == length - 20:
            kind = IM.IN_COMMIT
        bo = max(0, j // 12 - rng.randrange(2))
        w, end = _deps(rng, n, inst, 8, kind)
        out.append((kind, to, inst[0], inst[1], bo, rng.randrange(n), key, j & 1, 5000 + j, w, end))
    return out


def pack(n, msgs):
    """the arrays of EPaxos.replica_inbox, in its argument order"""
    m = len(msgs)
    cols = list(zip(*[x[:9] for x in msgs])) if msgs else [[]] * 9
    a = [np.asarray(c, np.int32) for c in cols]
    a[7] = a[7].astype(np.uint8)
    deps = np.asarray([x[9] for x in msgs], np.int32).reshape(m, n)
    dend = np.asarray([x[10] for x in msgs], np.int32)
    return a + [deps, dend]


def decode_outputs(n, msgs, outs):
    """(outcome, out_ballot, out_status, out_deps, out_values_end, out_triple) arrays -> rows like the model's.  A reply without
    dependencies must carry zeros / 0: anything else decodes to a marker no model row equals."""
    outcome, ob, os_, odeps, oend, otr = outs
    rows = []
    for i, msg in enumerate(msgs):
        o = int(outcome[i])
        inst = (msg[2], msg[3])
        carries = o in (IM.RI_PRE_ACCEPT_OK, IM.RI_PRE_ACCEPT_OK_AGAIN, IM.RI_COMMIT_BACK) or (o == IM.RI_PREPARE_OK and int(os_[i]) > 0)
        w = [int(v) for v in odeps[i]]
        if not carries:
            d = IM.NO_DEPS if (not any(w) and int(oend[i]) == 0) else ("garbage", tuple(w), int(oend[i]))
        elif w[0] == -1:
            d = None if (all(v == -1 for v in w) and int(oend[i]) == 0) else ("garbage", tuple(w), int(oend[i]))
        else:
            d = decode_deps(n, inst, w, int(oend[i]))
        rows.append((o, int(ob[i]), int(os_[i]), d, int(otr[i])))
    return rows


# ---- state readback ---------------------------------------------------------------------------------------------------------
def touched(msgs, num_keys):
    cells = sorted({(x[1], (x[2], x[3])) for x in msgs})
    keys = sorted({x[6] for x in msgs if x[0] != IM.IN_PREPARE and 0 <= x[6] < num_keys})
    return cells, keys


def model_state(model, cells, keys):
    out = {}
    for (r, inst) in cells:
        e = model.replicas[r].cmd_log.get(inst)
        if e is None:
            out[(r, inst)] = ((0, -1, -1, -1), None)
        else:
            deps = e.deps if e.kind >= ES.PRE_ACCEPTED else None
            out[(r, inst)] = ((e.kind, IM.enc(e.ballot), IM.enc(e.vote_ballot), e.triple_id), deps)
    largest = [IM.enc(rep.largest_ballot) for rep in model.replicas]
    index = {(r, k): (list(model.replicas[r].gets[k]), list(model.replicas[r].sets[k])) for r in range(model.n) for k in keys}
    return out, largest, index


def gpu_state(epx, cells, keys, raw=False):
    """raw: the dependencies as stored (watermarks, values_end), for bit-for-bit comparisons between two contexts"""
    n = epx.n
    out = {}
    for (r, inst) in cells:
        kind, ballot, vote, tid, _ = epx.read_cmdlog(r, inst[0], inst[1])
        d, dend = epx.read_cmdlog_deps(r, inst[0], inst[1])
        if raw:
            deps = ([int(v) for v in d], dend)
        elif kind < ES.PRE_ACCEPTED or d[0] == -1:
            deps = None
        else:
            deps = decode_deps(n, inst, [int(v) for v in d], dend)
        if kind == 0:
            ballot = vote = tid = -1
        out[(r, inst)] = ((kind, ballot, vote, tid), deps)
    largest = [epx.read_cmdlog(r, 0, 0)[4] for r in range(n)]
    index = {}
    for r in range(n):
        for k in keys:
            g, s = epx.read_index(r, k)
            index[(r, k)] = ([int(v) for v in g], [int(v) for v in s])
    return out, largest, index


# ---- what a burst exercises -----------------------------------------------------------------------------------------------------
def census(n, num_keys, msgs, num_instances=1 << 20):
    """plays the burst on a fresh InboxModel and counts: pairs[(kind, outcome)], longest_run (messages on one cell),
    multi_to (instances that reach two receivers), conflict_from[kind] (processed PreAccepts with a conflict that a message
    of that kind put earlier in the burst), deps_from_burst[outcome] (replies answered from an entry that an earlier message
    of the burst wrote), nack_raised (Nacks whose largestBallot an earlier message of the burst raised)"""
    model = IM.InboxModel(n, num_keys, num_instances)
    start_largest = [IM.enc(rep.largest_ballot) for rep in model.replicas]
    pairs, conflict_from, deps_from_burst = {}, {0: 0, 1: 0, 2: 0}, {}
    runs, receivers, writer = {}, {}, {}
    origin = {}                      # (to, key, is_set, leader) -> (value, kind of the message that put it)
    nack_raised = 0
    for i, msg in enumerate(msgs):
        kind, to, L, x, bo, br, key, is_set, tid, w, end = msg
        cell = (to, L, x)
        runs[cell] = runs.get(cell, 0) + 1
        receivers.setdefault((L, x), set()).add(to)
        row = model.deliver(msg)
        outcome = row[0]
        pairs[(kind, outcome)] = pairs.get((kind, outcome), 0) + 1
        if outcome == IM.RI_PRE_ACCEPT_OK and key >= 0:
            seen = set()
            for l in range(n):
                best = (0, None)
                for t in ((1,) if not is_set else (0, 1)):   # a get conflicts with sets, a set with gets and sets
                    v = origin.get((to, key, t, l), (0, None))
                    if v[0] > best[0]:
                        best = v
                if best[1] is not None:
                    seen.add(best[1])
            for k in seen:
                conflict_from[k] += 1
        if outcome in (IM.RI_PRE_ACCEPT_OK, IM.RI_ACCEPT_OK, IM.RI_LEARNT):
            if key >= 0:
                o = (to, key, int(bool(is_set)), L)
                if x + 1 > origin.get(o, (0, None))[0]:
                    origin[o] = (x + 1, kind)
            writer[cell] = i
        elif row[3] is not IM.NO_DEPS and cell in writer:
            deps_from_burst[outcome] = deps_from_burst.get(outcome, 0) + 1
        if outcome == IM.RI_NACK and row[1] > start_largest[to]:
            nack_raised += 1
    return {"pairs": pairs, "longest_run": max(runs.values()) if runs else 0,
            "multi_to": sum(1 for v in receivers.values() if len(v) >= 2), "conflict_from": conflict_from,
            "deps_from_burst": deps_from_burst, "nack_raised": nack_raised}
