"""Seeded bursts of a MultiPaxos replica's inbox for the fpx_replica_inbox tests: a log state before the burst (an executed
prefix, and slots that are in the log above the watermark) and n messages -- Chosens that mostly walk up the log with
local disorder (holes that a later Chosen fills, so that several slots execute at once), duplicates, one slot that is
never chosen (everything above it stays unexecuted), and reads aimed around the slot being chosen at that moment, below
the old watermark, at -1, far above, and past num_slots; other kinds and masked-out messages in between."""
from dataclasses import dataclass

import numpy as np

from frankenpaxos_amd import wire

SEEDS = (1, 2, 3)
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 3000)
DEFERRABLE = list(wire.DEFERRABLE_READS)
EVENTUAL = list(wire.EVENTUAL_READS)


@dataclass
class Burst:
    num_slots: int
    init_slot: np.ndarray       # the log before the burst: 0 .. W0 - 1 and some slots above W0 (never W0 itself)
    init_value: np.ndarray
    w0: int
    kind: np.ndarray
    slot: np.ndarray
    value: np.ndarray
    mask: np.ndarray

    def arrays(self):
        return self.kind, self.slot, self.value, self.mask

    def state(self):
        """(present, values, W0, num_chosen) before the burst"""
        present, values = np.zeros(self.num_slots, np.uint8), np.full(self.num_slots, -1, np.int32)
        present[self.init_slot], values[self.init_slot] = 1, self.init_value
        return present, values, self.w0, len(self.init_slot)


def make(seed, n, num_slots=4096):
    rng = np.random.default_rng(seed * 1000003 + n)
    w0 = int(rng.integers(5, 40))
    is_chosen = rng.random(n) < 0.55
    nc = int(is_chosen.sum())
    assert w0 + 2 * nc + 64 <= num_slots
    # the Chosens' slots: W0, W0 + 1, ... in an order disturbed by up to ~6 places, one of them never chosen (the watermark
    # stops there); a tenth of the Chosens repeat a slot chosen earlier in the burst
    nu = nc - nc // 10
    never = w0 + (4 * nu) // 5
    uniq = w0 + np.argsort(np.arange(nu) + rng.uniform(0, 6, nu), kind="stable")
    target = [int(s) for s in np.where(uniq == never, w0 + nu, uniq)]
    for _ in range(nc - nu):
        at = int(rng.integers(1, len(target) + 1))
        target.insert(at, target[int(rng.integers(0, at))])
    above = np.array([s for s in range(w0 + 1, w0 + nc + 8) if s != never and rng.random() < 0.15], np.int64)
    init_slot = np.concatenate([np.arange(w0), above]).astype(np.int32)
    kind, slot, value = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    done, seen = 0, set()
    for i in range(n):
        if is_chosen[i]:
            kind[i], slot[i], value[i] = wire.CHOSEN, target[done], 5000 + i
            seen.add(target[done])
            done += 1
            continue
        u = rng.random()
        if u < 0.08:                                        # not for this path
            kind[i], slot[i] = (wire.OTHER, wire.PHASE2A, wire.CHOSEN_NOOP_RANGE)[int(rng.integers(0, 3))], rng.integers(-5, 50)
        elif u < 0.25:
            kind[i], slot[i] = EVENTUAL[int(rng.integers(0, 2))], -1
        else:
            kind[i] = DEFERRABLE[int(rng.integers(0, 4))]
            v = rng.random()
            here = w0 + len(seen)                             # about where the log is being filled
            if v < 0.12:
                slot[i] = rng.integers(0, w0)
            elif v < 0.2:
                slot[i] = -1
            elif v < 0.7:
                slot[i] = here + rng.integers(-8, 9)
            elif v < 0.8:
                slot[i] = here + 2                          # several reads under one slot
            elif v < 0.9:
                slot[i] = rng.integers(never, num_slots)
            else:
                slot[i] = (num_slots, num_slots + 7, 2**31 - 1)[int(rng.integers(0, 3))]
    mask = (rng.random(n) >= 0.05).astype(np.uint8)
    chosen = np.flatnonzero(is_chosen)
    mask[chosen[np.unique(slot[chosen], return_index=True)[1]]] = 1     # (the first Chosen of every slot is delivered)
    return Burst(num_slots, init_slot, (1000 + init_slot).astype(np.int32), w0, kind, slot, value, mask)


def resubmit(burst, k, deferred):
    """the messages of burst[k:] behind the reads of burst[:k] that are still deferred (their indices, in hand-back
    order): the arrays, and for each new position the index in the whole burst"""
    idx = np.concatenate([np.asarray(deferred, np.int64), np.arange(k, len(burst.kind))]).astype(np.int64)
    return (burst.kind[idx], burst.slot[idx], burst.value[idx], burst.mask[idx]), idx
