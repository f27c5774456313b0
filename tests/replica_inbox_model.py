"""Two reference models of fpx_replica_inbox (include/fpx.h), written independently of each other:

  sequential(...)  message at a time, shaped like multipaxos/Replica.scala: a dict log, a dict of deferred lists,
                   handleChosen / executeLog / handleDeferrableRead / executeRead, and an event list of
                   (read index, entries executed, reply_slot) in the order the reads run
  arrays(...)      the closed form the kernels use: first occurrence per slot, np.maximum.accumulate, searchsorted

Both take the log before the burst as (present[S] uint8, values[S] int32, W0, num_chosen) and return a Result.  A burst
with a bad Chosen slot gives Result(status=EINVAL, bad_index=lowest) and nothing else."""
from dataclasses import dataclass, field

import numpy as np

from frankenpaxos_amd import wire

EINVAL = 1
CHOSEN = wire.CHOSEN
DEFERRABLE = set(wire.DEFERRABLE_READS)
EVENTUAL = set(wire.EVENTUAL_READS)
BATCHES = {wire.READ_REQUEST_BATCH, wire.SEQUENTIAL_READ_REQUEST_BATCH, wire.EVENTUAL_READ_REQUEST_BATCH}
NOT_A_READ, STILL_DEFERRED = -2, -1

CLASSES = ("below_w0", "after_earlier_chosen", "released", "released_by_hole_fill", "shared_slot", "under_present_slot",
           "still_deferred_in_range", "beyond_num_slots", "minus_one", "eventual", "batch", "duplicate_chosen", "masked")


@dataclass
class Result:
    status: int = 0
    bad_index: int = -1
    exec_count: np.ndarray = None
    reply_slot: np.ndarray = None
    order: np.ndarray = None            # the reads that ran in run order, then the still-deferred ones in index order
    counts: tuple = None                # (reads, ran, W0, W1)
    num_chosen: int = 0
    present: np.ndarray = None
    values: np.ndarray = None
    classes: dict = field(default_factory=dict)

    @property
    def w1(self):
        return self.counts[3]

    def still_deferred(self):
        return self.order[self.counts[1]:self.counts[0]]


def _mask(mask, n):
    return np.ones(n, np.uint8) if mask is None else np.asarray(mask, np.uint8)


def _first_bad(kind, slot, mask, S):
    for i in range(len(kind)):
        if mask[i] and kind[i] == CHOSEN and not 0 <= slot[i] < S:
            return i
    return -1


def sequential(present, values, w0, num_chosen, kind, slot, value, mask=None):
    S, n = len(present), len(kind)
    mask = _mask(mask, n)
    bad = _first_bad(kind, slot, mask, S)
    if bad >= 0:
        return Result(status=EINVAL, bad_index=bad)
    cls = dict.fromkeys(CLASSES, 0)
    log = {int(s): int(values[s]) for s in np.flatnonzero(present)}
    deferred = {}                       # slot -> the reads waiting for it, in arrival order
    events = []
    state = dict(wm=int(w0), nc=int(num_chosen))
    exec_count = np.full(n, NOT_A_READ, np.int32)
    reply_slot = np.full(n, NOT_A_READ, np.int32)

    def execute_read(i, executed):
        events.append((i, executed, state["wm"] - 1))      # ReadReply.slot = executedWatermark - 1

    def execute_log():
        ran, released = 0, 0
        while state["wm"] in log:
            s = state["wm"]
            ran += 1                                        # executeCommandBatchOrNoop(slot, ...)
            for i in deferred.pop(s, ()):                   # processDeferredReads: the watermark has not moved yet
                execute_read(i, s + 1)
                released += 1
            state["wm"] += 1
        cls["released"] += released
        if ran >= 2:
            cls["released_by_hole_fill"] += released

    for i in range(n):
        k, r = int(kind[i]), int(slot[i])
        if not mask[i]:
            cls["masked"] += 1
            continue
        if k == CHOSEN:
            if r in log:
                cls["duplicate_chosen"] += 1
                continue
            log[r] = int(value[i])
            state["nc"] += 1
            execute_log()
        elif k in DEFERRABLE or k in EVENTUAL:
            cls["batch"] += k in BATCHES
            if k in EVENTUAL:
                cls["eventual"] += 1
                execute_read(i, state["wm"])
                continue
            cls["minus_one"] += r == -1
            if r >= state["wm"]:
                waiting = deferred.setdefault(r, [])
                waiting.append(i)
                cls["shared_slot"] += len(waiting) == 2
                cls["under_present_slot"] += r in log
                exec_count[i] = reply_slot[i] = STILL_DEFERRED
                continue
            cls["below_w0"] += r < w0
            cls["after_earlier_chosen"] += r >= w0
            execute_read(i, state["wm"])
    for i, executed, reply in events:
        exec_count[i], reply_slot[i] = executed, reply
    left = sorted(i for waiting in deferred.values() for i in waiting)
    for i in left:
        cls["still_deferred_in_range"] += slot[i] < S
        cls["beyond_num_slots"] += slot[i] >= S
    out_p, out_v = np.zeros(S, np.uint8), np.full(S, -1, np.int32)
    for s, v in log.items():
        out_p[s], out_v[s] = 1, v
    order = np.array([e[0] for e in events] + left, np.int32)
    return Result(0, -1, exec_count, reply_slot, order, (len(order), len(events), int(w0), state["wm"]), state["nc"],
                  out_p, out_v, cls)


def arrays(present, values, w0, num_chosen, kind, slot, value, mask=None):
    S, n = len(present), len(kind)
    kind, slot, value = (np.asarray(a, np.int64) for a in (kind, slot, value))
    live = _mask(mask, n) != 0
    idx = np.arange(n)
    is_chosen = live & (kind == CHOSEN)
    bad = idx[is_chosen & ((slot < 0) | (slot >= S))]
    if len(bad):
        return Result(status=EINVAL, bad_index=int(bad[0]))
    present0 = np.asarray(present) != 0
    ci = idx[is_chosen]
    ci = ci[~present0[slot[ci]]]                            # the Chosens of slots that were absent
    put_slot, first = np.unique(slot[ci], return_index=True)     # first occurrence per slot (ci is increasing)
    put_by = np.full(S, -1, np.int64)
    put_by[put_slot] = ci[first]
    out_p, out_v = present0.copy(), np.asarray(values, np.int32).copy()
    out_p[put_slot], out_v[put_slot] = True, value[ci[first]]
    w1 = int(w0)
    if len(put_slot):
        holes = np.flatnonzero(~out_p[w0:])
        w1 = int(w0) + (int(holes[0]) if len(holes) else S - int(w0))
    executed_by = np.maximum.accumulate(put_by[w0:w1]) if w1 > w0 else np.zeros(0, np.int64)
    deferrable = live & np.isin(kind, list(DEFERRABLE))
    eventual = live & np.isin(kind, list(EVENTUAL))
    reads = deferrable | eventual
    w_at = w0 + np.searchsorted(executed_by, idx, side="left")  # W(i): the slots executed by messages before i
    r = np.where(deferrable, slot, -1)
    at_once = reads & (r < w_at)
    released = reads & ~at_once & (r < w1)
    exec_count = np.full(n, NOT_A_READ, np.int64)
    reply_slot = np.full(n, NOT_A_READ, np.int64)
    exec_count[reads], reply_slot[reads] = STILL_DEFERRED, STILL_DEFERRED
    exec_count[at_once], reply_slot[at_once] = w_at[at_once], w_at[at_once] - 1
    exec_count[released], reply_slot[released] = r[released] + 1, r[released] - 1
    ran = idx[reads & (exec_count >= 0)]
    ran = ran[np.lexsort((ran, exec_count[ran]))]
    left = idx[reads & (exec_count < 0)]
    order = np.concatenate([ran, left]).astype(np.int32)
    return Result(0, -1, exec_count.astype(np.int32), reply_slot.astype(np.int32), order,
                  (len(order), len(ran), int(w0), w1), int(num_chosen) + len(put_slot), out_p.astype(np.uint8), out_v)


def assert_same(a, b, what=""):
    assert (a.status, a.bad_index) == (b.status, b.bad_index), what
    if a.status:
        return
    assert tuple(a.counts) == tuple(b.counts) and a.num_chosen == b.num_chosen, (what, a.counts, b.counts)
    for name in ("exec_count", "reply_slot", "order", "present", "values"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg="%s %s" % (what, name))
