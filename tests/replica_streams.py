"""Bursts of a Mencius replica's inbox -- Chosen and ChosenNoopRange interleaved, in delivery order -- for
fpx_replica_chosen_msgs[_dev]: the stream generator, a dictionary-based restatement of the two handlers and executeLog
(mencius/Replica.scala:402-420, 464-485, 331-371; written from the Scala, independent of oracle/fpx_oracle.c), and the
oracle driven message by message, which is the reference of tests/test_gpu_replica_msgs.py."""
import numpy as np

CHOSEN, CHOSEN_NOOP_RANGE, PHASE2B = 4, 8, 2          # include/fpx_wire.h
NOOP = -1

# (num_leader_groups, num_slots) of the random streams, and their committed seeds
SHAPES = ((1, 4096), (3, 4096), (256, 1 << 16))
SEEDS = (1, 2, 3)
BURSTS = 8


class Replica:
    """the second restatement: log as a dict, one message at a time"""

    def __init__(self, num_leader_groups):
        self.L = num_leader_groups
        self.log = {}
        self.executed_watermark = 0
        self.num_chosen = 0
        self._prefix = 0

    def execute_log(self):                                         # Replica.scala:331-371
        while self.executed_watermark in self.log:
            self.executed_watermark += 1

    def chosen(self, slot, value):                                 # :402-420
        if slot in self.log:
            return                                                 # redundantly chosen: executeLog is not reached
        self.log[slot] = value
        self.num_chosen += 1
        self.execute_log()

    def chosen_noop_range(self, start, end):                       # :464-485
        for slot in range(start, end, self.L):
            if slot in self.log:
                return                                             # leaves the handler: no executeLog
            self.log[slot] = NOOP
            self.num_chosen += 1
        self.execute_log()

    def handle_one(self, k, s, e, v, m):
        if m and k == CHOSEN:
            self.chosen(int(s), int(v))
        elif m and k == CHOSEN_NOOP_RANGE:
            self.chosen_noop_range(int(s), int(e))

    def handle(self, burst):
        for msg in zip(*burst):
            self.handle_one(*msg)

    def prefix(self):
        """the first hole of the log (nothing is ever removed: the search resumes where it stopped)"""
        while self._prefix in self.log:
            self._prefix += 1
        return self._prefix

    def arrays(self, S):
        vals, pres = np.full(S, -1, np.int32), np.zeros(S, np.uint8)
        for s, v in self.log.items():
            vals[s], pres[s] = v, 1
        return vals, pres


def burst_of(msgs):
    """[(kind, slot, slot_end, value, mask)] -> the five arrays of one call"""
    if not msgs:
        return tuple(np.zeros(0, t) for t in (np.int32, np.int32, np.int32, np.int32, np.uint8))
    k, s, e, v, m = zip(*msgs)
    return (np.array(k, np.int32), np.array(s, np.int32), np.array(e, np.int32), np.array(v, np.int32),
            np.array(m, np.uint8))


def C(slot, value, mask=1):
    return (CHOSEN, slot, 0, value, mask)


def R(start, end, mask=1):
    return (CHOSEN_NOOP_RANGE, start, end, 12345, mask)             # (the value of a range is ignored)


def stream(L, S, seed, bursts=BURSTS):
    """8 bursts of at most 4096 messages: fresh and repeated Chosens, a run of Chosens at the head of the log, ranges of
    random start and length (empty ones, ends off the stride), repeats of earlier ranges, other kinds, a 10 % mask.  The
    traffic of burst b falls into a window that moves up the log, so that ranges still find free stretches late in the
    stream; every other burst ends with a range that starts at the first hole of the log and is cut two positions later:
    its Noops extend the prefix and the watermark stays behind."""
    rng = np.random.default_rng(1000 * L + seed)
    model = Replica(L)
    W = S // bursts
    seen_slots, seen_ranges, out = [0], [(0, 0)], []
    for b in range(bursts):
        lo, hi = max(0, (b - 1) * W), min(S, (b + 1) * W)
        n = int(rng.integers(2500, 4090))
        msgs = []
        for _ in range(n):
            u = rng.random()
            mask = 0 if rng.random() < 0.10 else 1
            if u < 0.30:
                msgs.append(C(int(rng.integers(lo, hi)), int(rng.integers(0, 1 << 30)), mask))
            elif u < 0.42:
                msgs.append(C(seen_slots[int(rng.integers(len(seen_slots)))], int(rng.integers(0, 1 << 30)), mask))
            elif u < 0.60:
                msgs.append(C(min(S - 1, model.prefix() + int(rng.integers(0, 3))), int(rng.integers(0, 1 << 30)), mask))
            elif u < 0.85:
                start = int(rng.integers(lo, hi))
                count = int(rng.integers(0, 12))
                end = min(S, start + count * L - (int(rng.integers(0, L)) if count and rng.random() < 0.5 else 0))
                msgs.append(R(start, end, mask))
            elif u < 0.97:
                msgs.append(R(*seen_ranges[int(rng.integers(len(seen_ranges)))], mask))
            else:
                msgs.append((PHASE2B, int(rng.integers(0, S)), 0, 7, mask))
            m = msgs[-1]
            if m[0] == CHOSEN:
                seen_slots.append(m[1])
            elif m[0] == CHOSEN_NOOP_RANGE:
                seen_ranges.append((m[1], m[2]))
            model.handle_one(*m)
        if b % 2 == 1:
            p = model.prefix()
            if p + 3 * L <= S:
                tail = [C(p + 2 * L, 77), R(p, p + 3 * L)]
                msgs += tail
                model.handle(burst_of(tail))
        out.append(burst_of(msgs))
    return out


def oracle_burst(ref, burst, S, L):
    """the reference: the oracle handles the burst one message at a time.  Returns (executed_watermark, num_chosen) and
    what the burst was made of, judged by the oracle's own answers"""
    _, before = ref.replica_read_log(0, S)
    wm, nc = ref.replica_chosen([], [])[1:]
    stats = dict(truncated=0, full=0, redundant=0, own=0)
    for k, s, e, v, m in zip(*burst):
        if not m:
            continue
        if k == CHOSEN:
            st, wm, nc2 = ref.replica_chosen([int(s)], [int(v)])
            assert st == 0
            stats["redundant"] += nc2 == nc
            nc = nc2
        elif k == CHOSEN_NOOP_RANGE:
            st, wm, nc2 = ref.replica_chosen_noop_range(int(s), int(e))
            assert st == 0
            count = len(range(int(s), int(e), L))
            if nc2 - nc == count:
                stats["full"] += 1
            else:
                stats["truncated"] += 1
                stats["own"] += not before[int(s) + (nc2 - nc) * L]    # stopped by a slot that this burst put
            nc = nc2
    vals, pres = ref.replica_read_log(0, S)
    prefix = int(np.argmin(pres)) if not pres.all() else S
    stats["lag"] = int(wm < prefix)
    return (wm, nc), (vals, pres), stats


def assert_not_vacuous(total, scalars):
    """the conditions every committed (L, seed) meets: `total` = the sums of oracle_burst's figures over a stream"""
    assert total["truncated"] >= 20 and total["full"] >= 20, total
    assert total["redundant"] >= 50 and total["own"] >= 5, total
    assert total["lag"] >= 1, total                       # a burst left executed_watermark below the contiguous prefix
    assert scalars[0] > 0
