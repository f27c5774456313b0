"""epaxos_inbox_mk_streams.py -- TEST INFRASTRUCTURE ONLY: tests/epaxos_inbox_streams.py for fpx_epx_replica_inbox_mk: seeded
bursts of peer messages whose commands carry KEY LISTS, their packing into the call's arrays, and the census of what a burst
exercises.  The decoding of the outputs and the state readback are that file's (re-exported here).

A message is the tuple of tests/epaxos_inbox_mk_model.py:
    (kind, to, leader, number, ballot_ordering, ballot_replica, keys, is_set, triple_id, watermarks, values_end)
"""
import random

import numpy as np

from tests import epaxos_inbox_model as IM
from tests import epaxos_inbox_mk_model as MM
from tests.epaxos_inbox_streams import _deps, decode_outputs, gpu_state, model_state  # noqa: F401


def key_list(rng, num_keys, hot_key=None):
    """0 .. 5 keys drawn WITH replacement (so keys repeat inside a list, on purpose); about one list in ten is empty"""
    if hot_key is None and rng.random() < 0.1:
        return ()
    keys = [rng.randrange(num_keys) for _ in range(1 + rng.randrange(5))]
    if hot_key is not None:
        keys[rng.randrange(len(keys))] = hot_key
    return tuple(keys)


def make_burst(seed, n, m, num_keys=4, num_instances=64, hot_key=None, hot_to=None, first_triple=1000, max_ordering=3,
               one_key=False):
    """tests/epaxos_inbox_streams.make_burst with a key list per script: scripts of 1 .. 9 messages on one cell (to, leader,
    number), interleaved with every script's own order kept; a script's messages share the list.  one_key: every list has
    exactly one key (the single-key call's domain without its Noops)"""
    rng = random.Random(seed)
    span = max(2, min(num_instances, max(4, m // 8)))
    scripts, total, tid = [], 0, first_triple
    while total < m:
        inst = (rng.randrange(n), rng.randrange(span))
        to = rng.randrange(n) if hot_to is None else hot_to
        keys = (rng.randrange(num_keys),) if one_key else key_list(rng, num_keys, hot_key)
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
            script.append((kind, to, inst[0], inst[1], bo, br, keys, is_set, tid, w, end))
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


def distinct_instances(msgs):
    """the burst without the later messages of any instance (what the per-kind entry points require)"""
    seen, out = set(), []
    for x in msgs:
        if (x[2], x[3]) not in seen:
            seen.add((x[2], x[3]))
            out.append(x)
    return out


def with_pairs(msgs, pairs, num_keys=4):
    """the burst with its LAST message's list padded or cut (and lists before it emptied, from the end) so that the
    burst has exactly `pairs` keys"""
    msgs = list(msgs)
    have = sum(len(x[6]) for x in msgs)
    j = len(msgs) - 1
    while have > pairs and j >= 0:                           # drop keys from the end
        cut = min(len(msgs[j][6]), have - pairs)
        msgs[j] = msgs[j][:6] + (msgs[j][6][:len(msgs[j][6]) - cut],) + msgs[j][7:]
        have -= cut
        j -= 1
    if have < pairs:
        last = msgs[-1]
        pad = tuple((3 * q + 1) % num_keys for q in range(pairs - have))
        msgs[-1] = last[:6] + (tuple(last[6]) + pad,) + last[7:]
    assert sum(len(x[6]) for x in msgs) == pairs
    return msgs


def single_key_form(msgs):
    """a burst whose lists have at most one key -> the messages of tests/epaxos_inbox_streams.py (no key: a Noop)"""
    assert all(len(x[6]) <= 1 for x in msgs)
    return [x[:6] + (x[6][0] if x[6] else -1,) + x[7:] for x in msgs]


def csr(msgs):
    off = np.zeros(len(msgs) + 1, np.int32)
    off[1:] = np.cumsum([len(x[6]) for x in msgs])
    keys = np.asarray([k for x in msgs for k in x[6]], np.int32)
    return off, keys


def pack(n, msgs):
    """the arguments of EPaxos.replica_inbox_mk, in its order (the key lists as the CSR pair of arrays)"""
    m = len(msgs)
    col = lambda j, t=np.int32: np.asarray([x[j] for x in msgs], t)
    deps = np.asarray([x[9] for x in msgs], np.int32).reshape(m, n)
    return [col(0), col(1), col(2), col(3), col(4), col(5), csr(msgs), col(7, np.uint8), col(8), deps, col(10)]


def all_keys(num_keys):
    return list(range(num_keys))


def cells_of(msgs):
    return sorted({(x[1], (x[2], x[3])) for x in msgs})


# ---- what a burst exercises -----------------------------------------------------------------------------------------------------
def census(n, num_keys, msgs, num_instances=1 << 20):
    """plays the burst on a fresh InboxMkModel and counts: pairs[(kind, outcome)]; processed (PreAccepts that were processed);
    cross_key -- the processed PreAccepts with at least two distinct keys whose dependency on some column is raised by a put
    made EARLIER IN THE SAME BURST under a key that is not the first of their list (what only the merge over a command's pairs
    can get right); repeated (commands with a key repeated inside their list); empty (commands without keys); max_keys"""
    model = MM.InboxMkModel(n, num_keys, num_instances)
    pairs = {}
    put = {}                          # (to, key, is_set, leader) -> the highest number + 1 put in this burst
    processed = cross_key = repeated = empty = max_keys = 0
    for msg in msgs:
        kind, to, L, x, bo, br, keys, is_set, tid, w, end = msg
        outcome = model.deliver(msg)[0]
        pairs[(kind, outcome)] = pairs.get((kind, outcome), 0) + 1
        if kind != IM.IN_PREPARE:
            repeated += len(set(keys)) < len(keys)
            empty += not keys
            max_keys = max(max_keys, len(keys))
        if outcome == IM.RI_PRE_ACCEPT_OK:
            processed += 1
            types = (0, 1) if is_set else (1,)               # a get conflicts with sets, a set with gets and sets
            seen = lambda k, l: max(put.get((to, k, t, l), 0) for t in types)
            distinct = list(dict.fromkeys(keys))
            if len(distinct) >= 2 and any(max(seen(k, l) for k in distinct[1:]) > seen(distinct[0], l) for l in range(n)):
                cross_key += 1
        if outcome in (IM.RI_PRE_ACCEPT_OK, IM.RI_ACCEPT_OK, IM.RI_LEARNT):
            for k in keys:
                o = (to, k, int(bool(is_set)), L)
                put[o] = max(put.get(o, 0), x + 1)
    return {"pairs": pairs, "processed": processed, "cross_key": cross_key, "repeated": repeated, "empty": empty,
            "max_keys": max_keys}
