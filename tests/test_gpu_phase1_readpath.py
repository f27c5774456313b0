"""Phase-1 recovery (k_quorum_max_slot, k_phase1b_scan<G>), the acceptor's Phase1b.info, the read path
(k_max_voted_in) and the replica log (k_log_ingest / k_log_scan / k_log_range_first / k_log_range_fill) at every
lanes-per-slot width, past every launch's grid cap and on Mencius and grid geometries -- against two references that
share no code with the kernels: the C oracle, driven by the same script, and a plain numpy restatement of each
operation on the (S, R) arrays a context reads back.  Every comparison is exact integer equality.

The numpy restatement is pinned on the oracle by the CPU tests at the top (small sizes, the same scripts), so the
second opinion of the GPU tests is a trusted one.  The GPU tests prove by arithmetic or on the reference that they
reach the cell they are about: the width G, a second pass of a grid-stride loop, a partial last quad, more than one
workgroup of k_quorum_max_slot, the position of the hole.  The grid caps are restated here from the launch code
(fpx_api.hip: launch_p1b, fpx_replica_chosen_dev, fpx_replica_chosen_noop_range); num_cus is taken from torch's
multi_processor_count, the same hipDeviceProp_t::multiProcessorCount fpx_create stores in ctx->num_cus.
"""
import numpy as np
import pytest

from tests import workloads as W

gpu_test = pytest.mark.gpu

# the lanes-per-slot width of every R under test, written out by the rule "the smallest power of two with 4 G >= R"
# (each of the seven widths at its lowest and its highest R; a partial last quad wherever R % 4 != 0)
EXPECT_G = {3: 1, 4: 1, 5: 2, 8: 2, 9: 4, 13: 4, 16: 4, 17: 8, 32: 8, 33: 16, 61: 16, 64: 16, 65: 32, 100: 32, 128: 32,
            129: 64, 253: 64, 256: 64}
GRIDS = {4: (2, 2), 8: (2, 4), 9: (3, 3), 16: (4, 4), 32: (4, 8), 33: (3, 11), 64: (8, 8), 65: (5, 13), 100: (10, 10),
         128: (8, 16), 129: (3, 43), 253: (11, 23), 256: (16, 16)}
BIG_R = {1: 3, 2: 5, 4: 13, 8: 17, 16: 61, 32: 65, 64: 253}      # past the grid cap: one R per width, all partial quads


# =====================================================================================================================
# CPU-only reference helpers
# =====================================================================================================================
def lanes(R):
    G = 1
    while 4 * G < R:
        G *= 2
    return G


def pack_bits(mat):
    """bool [n, R] -> uint64 [n, 4] (W.bits_from_bool without its n x 256 bytes: the big cases have 2^21 rows)"""
    n, R = mat.shape
    out = np.zeros((n, 4), np.uint64)
    for j in range(R):
        out[:, j >> 6] |= mat[:, j].astype(np.uint64) << np.uint64(j & 63)
    return out


def acceptors(n, R, members):
    """n equal target masks: exactly the acceptors `members`"""
    row = np.zeros((1, R), bool)
    row[0, list(members)] = True
    return np.repeat(pack_bits(row), n, axis=0)


class NpState:
    """The acceptors' votes as plain arrays (read_state / read_scalars of either backend) and the operations under
    test restated on them."""

    def __init__(self, be, L=1, A=1):
        self.vr, self.vv, _ = be.read_state()
        _, self.mv = be.read_scalars()
        self.S, self.R = self.vr.shape
        self.L, self.A = L, A

    def groups(self, s):
        s = np.asarray(s)
        return (s % self.L) * self.A + (s // self.L) % self.A

    def scan(self, wm, q, cap):
        """(max_slot, safe_round, safe_value) of Leader.handlePhase1b: max_slot from max_voted and the watermark,
        count = min(cap, max_slot - wm + 1), safe_round the maximum vote round over the quorum of the slot's group,
        safe_value the value at the lowest acceptor that holds it, -1 if nobody voted"""
        qb = W.bool_from_bits(np.asarray(q, np.uint64).reshape(-1, 4), self.R)     # bits >= R fall off here
        cand = self.mv[qb]
        cand = cand[cand >= wm]
        mx = int(cand.max()) if len(cand) else -1
        count = max(0, min(cap, mx - wm + 1))
        s = np.arange(wm, wm + count)
        rr = np.where(qb[self.groups(s)], self.vr[wm:wm + count], -1).reshape(count, self.R)
        sr = rr.max(axis=1)
        sv = np.where(sr >= 0, self.vv[s, rr.argmax(axis=1)], -1)                    # argmax: the first = lowest r
        return mx, sr.astype(np.int32), sv.astype(np.int32)

    def max_contributors(self, wm, q):
        """the groups that hold the acceptor whose max_voted IS max_slot"""
        qb = W.bool_from_bits(np.asarray(q, np.uint64).reshape(-1, 4), self.R)
        mx = self.scan(wm, q, 0)[0]
        return set(np.nonzero((qb & (self.mv == mx)).any(axis=1))[0].tolist()) if mx >= 0 else set()

    def voted(self, group, r, first, count):
        s = np.arange(first, first + count)
        return s[(self.groups(s) == group) & (self.vr[first:first + count, r] != -1)]

    def max_voted_in(self, group, r, first, count):
        s = self.voted(group, r, first, count)
        return int(s.max()) if len(s) else -1

    def info(self, group, r, wm):
        s = self.voted(group, r, wm, self.S - wm) if wm < self.S else np.zeros(0, np.int64)
        return s.astype(np.int32), self.vr[s, r], self.vv[s, r]


class NpLog:
    """Replica.handleChosen / handleChosenNoopRange / executeLog on two arrays"""

    def __init__(self, S, stride=1):
        self.present = np.zeros(S + 1, np.uint8)        # (one absent slot behind the log ends every walk)
        self.value = np.full(S, -1, np.int32)
        self.S, self.stride, self.wm, self.num = S, stride, 0, 0

    def _execute(self):
        while self.present[self.wm]:                    # (in strides: a plain loop over 2^21 slots is seconds)
            rest = self.present[self.wm:self.wm + 65536]
            gap = np.flatnonzero(rest == 0)
            self.wm += int(gap[0]) if len(gap) else len(rest)

    def replica_chosen(self, slot, value, mask=None):
        slot, value = np.asarray(slot), np.asarray(value)
        if mask is not None:
            slot, value = slot[np.asarray(mask) != 0], value[np.asarray(mask) != 0]
        u, at = np.unique(slot, return_index=True)      # delivery order: the first message of a slot wins
        new = self.present[u] == 0
        self.value[u[new]] = value[at[new]]
        self.present[u[new]] = 1
        self.num += int(new.sum())
        self._execute()
        return 0, self.wm, self.num

    def replica_chosen_noop_range(self, start, end):
        pos = np.arange(start, end, self.stride)
        there = np.flatnonzero(self.present[pos])
        first = int(there[0]) if len(there) else len(pos)
        self.value[pos[:first]] = -1
        self.present[pos[:first]] = 1
        self.num += first
        if first == len(pos):                           # the handler ran to its end: executeLog
            self._execute()
        return 0, self.wm, self.num

    def replica_read_log(self, first, count):
        return self.value[first:first + count], self.present[first:first + count]


# ---- the state every small case scans ----------------------------------------------------------------------------
def recovery_script(S, R, L, A, seed):
    """Votes in [0, S): the lower half from the adversarial stream (Mencius: a plain stream in two rounds with thrifty
    targets), then, in rounds above every round of the stream, single-acceptor votes that put the highest round of a
    slot at acceptor 0, at R - 1 (the last real cell of a partial quad) and at the last cell of the last whole quad
    before it; two acceptors voting DIFFERENT values in one round (a leader never does that; the scan's answer is
    the lowest index, include/fpx.h) inside one quad and across lanes; the same single votes in the upper half, where
    nobody else voted, with untouched slots between them; and one vote each of acceptor 0 and R - 1 near S."""
    half = S // 2
    assert half >= 256
    if L == 1:
        ops = W.adversarial_script(half, R, R // 2 + 1, seed, epochs=8, fused=True, ngroups=A)
    else:
        rng, ops = np.random.default_rng(seed), []
        for rnd in (0, 1):
            slot = rng.permutation(half)[: half // 2].astype(np.int32)
            tgt = W.bits_from_bool(W.random_subsets(rng, len(slot), R, 1, R))
            ops.append(("fused", slot, np.full(len(slot), rnd, np.int32), W.steady_values(slot), tgt))
    hi = 1 + max([int(op[2].max()) for op in ops if op[0] == "fused"] + [op[2] for op in ops if op[0] == "phase1a"])
    qe = 4 * ((R - 1) // 4) - 1
    k = np.arange(12, dtype=np.int32)

    def single(acc, slots, off):
        slots = slots.astype(np.int32)
        ops.append(("fused", slots, np.full(len(slots), hi, np.int32), 500000 + off + slots, acceptors(len(slots), R, [acc])))

    def tie(a, b, slots):
        slots = slots.astype(np.int32)
        rr = np.full(len(slots), hi + 1, np.int32)
        ops.append(("phase2a", slots, rr, 700000 + slots, acceptors(len(slots), R, [a])))
        ops.append(("phase2a", slots, rr, 800000 + slots, acceptors(len(slots), R, [b])))

    for base, step in ((40, 13), (half + 6, 7)):
        single(0, base + step * k, 0)
        single(R - 1, base + 1 + step * k, 100000)
        if qe > 0:
            single(qe, base + 2 + step * k, 200000)
    tie(0, 1, 45 + 13 * k)
    tie(1, R - 1, 46 + 13 * k)
    tie(0, 1, half + 4 + 7 * k[:4])
    single(0, np.array([S - 9]), 0)
    single(R - 1, np.array([S - 3]), 100000)
    return ops


def quorum_masks(R, ng, rng):
    """the quorum masks of a scan, the same set of acceptors in every group unless the name says otherwise"""
    def every(members):
        return acceptors(ng, R, members)
    lastquad = range(4 * ((R - 1) // 4), R)
    out = {"first": every([0]), "last": every([R - 1]), "all": every(range(R)), "lastquad": every(lastquad),
           "random": pack_bits(W.random_subsets(rng, ng, R, 1, R)), "random2": pack_bits(W.random_subsets(rng, ng, R, 1, R))}
    if R < 256:   # acceptor 0 and every bit at or above R: names no acceptor, ignored (include/fpx.h)
        over = np.zeros((1, 256), bool)
        over[0, 0] = True
        over[0, R:] = True
        out["first+beyond"] = np.repeat(pack_bits(over), ng, axis=0)
    for g in sorted({0, ng // 3, ng - 1}) if ng > 1 else ():
        one = np.zeros((ng, 4), np.uint64)
        one[g] = every(range(R))[0]
        out["group%d" % g] = one
    return out


def same_scan(backends, st, wm, q, cap):
    want = st.scan(wm, q, cap)
    for be in backends:
        got = be.leader_phase1b_scan(wm, q, cap)
        assert got[0] == 0 and got[1] == want[0], (wm, cap, got[:2], want[0])
        np.testing.assert_array_equal(got[2], want[1], err_msg="safe_round wm %d cap %d" % (wm, cap))
        np.testing.assert_array_equal(got[3], want[2], err_msg="safe_value wm %d cap %d" % (wm, cap))
    return want


def check_scans(backends, st, masks):
    """every backend against the numpy restatement: the watermarks around one wavefront pass of the width (Q slots),
    the caps around it, every mask; returns the groups that decided max_slot"""
    Q = 64 // lanes(st.R)
    names = list(masks)
    top = st.scan(0, masks["all"], 0)[0]
    assert top > st.S // 2
    contributors = set()
    wms = sorted({0, 1, max(Q - 1, 0), Q, Q + 1, st.S // 3 + 5, top, top + 1})
    for wi, wm in enumerate(wms):
        for ci in range(6):
            q = masks[names[(wi * 5 + ci) % len(names)]]
            count = max(0, st.scan(wm, q, 0)[0] - wm + 1)
            cap = (0, 1, max(Q - 1, 0), Q + 1, max(count - 1, 0), count)[ci]
            same_scan(backends, st, wm, q, cap)
            contributors |= st.max_contributors(wm, q)
    assert same_scan(backends, st, top + 1, masks["all"], st.S)[0] == -1         # empty: nothing at or above it
    # every mask over the whole range.  "first+beyond" among them is the check that a backend ignores quorum bits at and
    # above R: the restatement drops them (bool_from_bits), so it answers what it answers for "first".  On the device
    # the cells those bits name are the padding of a partial last quad, and they are not all -1: a vote of every real
    # acceptor of the quad is stored as one whole int4, padding included, and the lower half of the state is full of
    # such votes, in rounds above acceptor 0's and in slots it did not vote in -- the `r0 + k < g.R` of the reduction is
    # what keeps them out.
    for name in names:
        for wm in (0, Q + 1):
            same_scan(backends, st, wm, masks[name], st.S)
            contributors |= st.max_contributors(wm, masks[name])
    return contributors


def assert_kinds(st):
    """the scanned range holds every kind of slot the scan has a branch for"""
    R, vr = st.R, st.vr
    nvot = (vr != -1).sum(axis=1)
    assert (nvot[: st.S - 3] == 0).any()                                     # nobody voted
    assert ((vr[:, 0] == -1) & (nvot > 0)).any()                              # only acceptors outside {0} voted
    assert ((vr[:, R - 1] == -1) & (nvot > 0)).any()
    top = vr.max(axis=1)
    sole = (vr == top[:, None]).sum(axis=1) == 1
    qe = 4 * ((R - 1) // 4) - 1
    for acc in [0, R - 1] + ([qe] if qe > 0 else []):                         # the highest round at this acceptor, others below
        assert ((vr[:, acc] == top) & sole & (nvot > 1)).any(), acc
    tied = (vr == top[:, None]) & (top[:, None] >= 0)
    two = tied.sum(axis=1) == 2
    differ = np.array([len(set(st.vv[s][tied[s]].tolist())) == 2 for s in np.nonzero(two)[0]])
    rows = np.nonzero(two)[0][differ]
    assert len(rows) and (tied[rows][:, :2].all(axis=1)).any()                # a tie inside the first quad
    if R > 4:
        assert (tied[rows][:, 1] & tied[rows][:, R - 1]).any()                # a tie across lanes


def check_info(backends, st, ng, wms):
    for g in sorted({0, 1 % ng, ng // 2, ng - 1}):
        for r in sorted({0, st.R // 2, st.R - 1}):
            for wm in wms:
                want = st.info(g, r, wm)
                for be in backends:
                    for x, y in zip(be.acceptor_phase1b_info(g, r, wm), want):
                        np.testing.assert_array_equal(x, y, err_msg="info group %d acceptor %d from %d" % (g, r, wm))


def only_first_and_only_last(st, group, r):
    """two windows of acceptor r's column: one whose only vote is in its first slot, one whose only vote is in its last"""
    v = st.voted(group, r, 0, st.S)
    gaps = np.nonzero(np.diff(v) >= 3)[0]
    assert len(gaps), "no two votes of acceptor %d with a gap between them" % r
    i = gaps[len(gaps) // 2]
    return (int(v[i]), int(v[i + 1] - v[i])), (int(v[i]) + 1, int(v[i + 1] - v[i]))


def check_max_voted_in(gpu, st, ng):
    """fpx_acceptor_max_voted_in against the numpy restatement; returns the number of windows that held a vote"""
    S, R = st.S, st.R
    hits = 0

    def same(g, r, first, count):
        want = st.max_voted_in(g, r, first, count)
        got = gpu.acceptor_max_voted_in(g, r, first, count)
        assert got == want, (g, r, first, count, got, want)
        return want

    for g in sorted({0, ng // 2, ng - 1}):
        for r in (0, R - 1):
            assert same(g, r, 0, S) == (st.voted(g, r, 0, S).max() if len(st.voted(g, r, 0, S)) else -1)
            for count in (1, 63, 64, 65, 255, 256, 257, 4097):
                for first in (0, 64, 100, 4096 - 37, S - count):              # at and off multiples of 64; ending at S
                    if 0 <= first and first + count <= S:
                        hits += same(g, r, first, count) >= 0
            # no vote at all: the untouched slots above the upper half's single votes
            lo = S // 2 + 6 + 7 * 12
            assert st.max_voted_in(g, r, lo, S - 9 - lo) == -1 and same(g, r, lo, S - 9 - lo) == -1
            if len(st.voted(g, r, 0, S)) > 1:
                (f1, c1), (f2, c2) = only_first_and_only_last(st, g, r)
                assert same(g, r, f1, c1) == f1 and len(st.voted(g, r, f1, c1)) == 1
                assert same(g, r, f2, c2) == f2 + c2 - 1 and len(st.voted(g, r, f2, c2)) == 1
    if ng > 1:
        # a window that holds votes of acceptor 0 of the OTHER groups only: one short of the period of the group
        # pattern (a group recurs every L * A slots), started behind a slot of the group
        period = st.L * st.A
        seen = 0
        for g in sorted({0, ng // 2, ng - 1}):
            for first in range(40, 40 + 3 * ng):
                if st.groups(first - 1) == g and (st.vr[first:first + period - 1, 0] != -1).any():
                    assert not (st.groups(np.arange(first, first + period - 1)) == g).any()
                    assert same(g, 0, first, period - 1) == -1
                    seen += 1
                    break
        assert seen > 0
    return hits


def log_sizes(num_cus):
    """slots one pass of each replica-log kernel covers (fpx_api.hip): k_log_ingest runs min(ceil(n / 256), num_cus * 8,
    4096) workgroups of 256, k_log_scan num_cus * 4, k_log_range_first / _fill min(ceil(count / 256), num_cus * 8)"""
    return min(num_cus * 8, 4096) * 256, num_cus * 4 * 256, num_cus * 8 * 256


def host_runs(slot):
    """The launches the host form of replica_chosen makes of the live messages of one batch, restated from split_runs
    (fpx_api.hip): it drops the masked-out messages, then delivers the rest in runs back to back and starts a new run
    at every message whose slot the current run holds already.  Returns the length of every run."""
    runs, seen = [0], set()
    for s in slot.tolist():
        if s in seen:
            runs.append(0)
            seen = set()
        seen.add(s)
        runs[-1] += 1
    return runs


def log_holes(logs, ING, SCAN):
    """Batches that leave a single hole (a) in the scan's first pass, (b) in the first slot of its second pass, (c) in the
    last slot below largestKey, each from a nonzero watermark that is not a multiple of 256, and the batch that fills
    it; the first batch reaches k_log_ingest as ONE launch of more records than one pass of it and carries duplicates
    of the batch before (each slot once, with another value, ignored) and masked-out messages for absent slots
    (ignored; the host form drops them before the launch, the device mask is test_replica_log_past_the_caps's)."""
    rng = np.random.default_rng(21)

    def step(slot, value=None, mask=None):
        slot = np.asarray(slot, np.int32)
        value = W.steady_values(slot) if value is None else value
        got = [lg.replica_chosen(slot, value, mask) for lg in logs]
        assert all(g == got[-1] for g in got), got
        return got[-1]

    def run(lo, n, hole):
        assert lo % 256 != 0 and lo > 0
        s = lo + rng.permutation(n)
        return s[s != hole]

    w0 = 777
    assert step(rng.permutation(w0)) == (0, w0, w0)
    n1 = ING + 5001
    hole = w0 + min(1234, SCAN // 2)
    assert hole - w0 < SCAN                                                # (a): inside the first pass
    dup = rng.choice(w0, 300, replace=False)                               # no slot twice in the batch: the host cuts nothing
    ghost = w0 + n1 + 10 + np.arange(500)
    new = run(w0, n1, hole)
    slot = np.concatenate([new, dup[:200], ghost])
    value = np.concatenate([W.steady_values(new), np.full(200, 7, np.int32), np.full(500, 9, np.int32)])
    mask = np.concatenate([np.ones(n1 - 1 + 200, np.uint8), np.zeros(500, np.uint8)])
    order = rng.permutation(len(slot))                                     # ... and 100 of the duplicates go last
    slot = np.concatenate([slot[order], dup[200:]])
    value = np.concatenate([value[order], np.full(100, 7, np.int32)])
    mask = np.concatenate([mask[order], np.ones(100, np.uint8)])
    runs = host_runs(slot[mask != 0])
    assert len(runs) == 1 and runs[0] > ING                                # one launch, and k_log_ingest strides in it
    late = np.flatnonzero(mask != 0)[ING:]                                 # what its threads take in their second pass:
    assert (slot[late] < w0).any() and (slot[late] >= w0).any()            # duplicates and new records
    assert step(slot, value, mask) == (0, hole, w0 + n1 - 1)
    top = w0 + n1
    assert step([hole]) == (0, top, top)
    n2 = SCAN + 3001
    hole = top + SCAN                                                      # (b): the first slot of the second pass
    assert step(run(top, n2, hole)) == (0, hole, top + n2 - 1)
    top += n2
    assert step([hole]) == (0, top, top)
    n3 = 2 * SCAN + 778
    hole = top + n3 - 2                                                    # (c): the last slot below largestKey
    assert hole - top > 2 * SCAN
    assert step(run(top, n3, hole)) == (0, hole, top + n3 - 1)
    top += n3
    assert step([hole]) == (0, top, top)
    return top


def dev_batches(ING, SCAN, S):
    """Two batches for the device form of replica_chosen, which validates and ingests a batch as it stands: it names
    no slot twice and no slot outside the log, masked out or not.  The first is longer than one pass of k_log_ingest,
    lacks a slot its threads would take in their second pass (the hole) and carries masked-out messages for slots that
    are absent: for the hole, as the very last message, and for slots nothing ever fills.  The second fills the hole,
    repeats 500 slots of the first with another value and adds more than one pass of k_log_scan.  Returns (hole, end
    of the first, end of the second) and the batches as (slot, value, mask)."""
    rng = np.random.default_rng(4)
    n = ING + 2001
    hole = ING + 5
    end = n + SCAN + 300
    live = rng.permutation(n)
    live = live[live != hole]
    ghost = np.concatenate([[hole], end + 10 + np.arange(400)])
    first = np.concatenate([live, ghost])
    mask = np.concatenate([np.ones(len(live), np.uint8), np.zeros(len(ghost), np.uint8)])
    order = rng.permutation(len(first))
    j = int(np.flatnonzero(order == len(live))[0])
    order[j], order[-1] = order[-1], order[j]                             # the hole's goes last
    first, mask = first[order].astype(np.int32), mask[order]
    assert (mask[:ING] != 0).any() and (mask[:ING] == 0).any()            # both kinds of message in the first pass of
    assert (mask[ING:] != 0).any() and (mask[ING:] == 0).any()            # k_log_ingest's threads and in their second
    assert int(mask.sum()) > ING and first.max() < S and len(np.unique(first)) == len(first)
    second = np.concatenate([[hole], live[:500], n + rng.permutation(SCAN + 300)]).astype(np.int32)
    assert len(np.unique(second)) == len(second)
    vals = [np.where(mask != 0, W.steady_values(first), 77).astype(np.int32),
            np.concatenate([[41], np.full(500, 3, np.int32), W.steady_values(second[501:])]).astype(np.int32)]
    return (hole, n, end), [(first, vals[0], mask), (second, vals[1], None)]


def log_noop_ranges(logs, RANGE, L):
    """Noop ranges of more positions than one pass of k_log_range_first (stride L): the first position already in the
    log in the first pass, in the second pass, at the last position and nowhere.  A range that stops early executes
    nothing, though it is contiguous with the watermark."""
    N = RANGE + 1501

    def same(name, *a):
        got = [getattr(lg, name)(*a) for lg in logs]
        assert all(g == got[-1] for g in got), (name, a, got)
        return got[-1]

    def slot(pos, lg=0):
        return lg + pos * L

    x0 = 333
    s0 = np.concatenate([slot(np.arange(x0)), slot(np.arange(x0), L - 1)]) if L > 1 else np.arange(x0)
    same("replica_chosen", s0.astype(np.int32), W.steady_values(s0))
    wm = same("replica_chosen", np.array([slot(x0 + 100)], np.int32), np.array([5], np.int32))[1]
    assert wm == (slot(x0) if L > 1 else x0)
    st, w, num = same("replica_chosen_noop_range", slot(x0), slot(x0 + N))               # stops in the first pass
    assert (st, w, num) == (0, wm, len(s0) + 1 + 100)
    x1 = x0 + 101
    wm = same("replica_chosen", np.array([slot(x1 + RANGE + 7)], np.int32), np.array([6], np.int32))[1]
    assert wm == (slot(x0) + 1 if L > 1 else x1)           # this handler does execute what the range before left
    st, w, num2 = same("replica_chosen_noop_range", slot(x1), slot(x1 + N))              # stops in the second pass
    assert (st, w, num2 - num) == (0, wm, 1 + RANGE + 7)
    x2 = x1 + RANGE + 8
    wm = same("replica_chosen", np.array([slot(x2 + N - 1)], np.int32), np.array([8], np.int32))[1]
    assert wm == (slot(x0) + 1 if L > 1 else x2)
    st, w, num3 = same("replica_chosen_noop_range", slot(x2), slot(x2 + N))              # stops at the last position
    assert (st, w, num3 - num2) == (0, wm, 1 + N - 1)
    x3 = x2 + N
    if L == 1:
        st, w, num4 = same("replica_chosen_noop_range", x3, x3 + N)                      # runs to its end: executeLog
        assert (st, w, num4 - num3) == (0, x3 + N, N)
        return x3 + N
    # Mencius: the last leader group skips its slots from the watermark on -- nothing of it is in the log, the range runs
    # to its end and executeLog stops at leader group 0's first absent slot
    n1 = x3 - x0 + 50
    assert n1 > RANGE
    st, w, num4 = same("replica_chosen_noop_range", slot(x0, L - 1), slot(x0 + n1, L - 1))
    assert (st, num4 - num3) == (0, n1) and w == (slot(x3) if L == 2 else slot(x0, 1))
    return slot(x0 + n1, L - 1)


# =====================================================================================================================
# CPU: the numpy restatement pinned on the oracle
# =====================================================================================================================
def geometry(name):
    return {"mencius8x2": dict(num_replicas=3, f=1, num_groups=2, num_leader_groups=8),
            "mencius256": dict(num_replicas=3, f=1, num_groups=1, num_leader_groups=256),
            "grid16": dict(num_replicas=4, num_groups=16, quorum_kind=2, grid_rows=2, grid_cols=2)}[name]


def test_width_table_covers_every_lane_count():
    for R, G in EXPECT_G.items():
        assert lanes(R) == G and 4 * G >= R and (G == 1 or 2 * G < R)
    for G in (1, 2, 4, 8, 16, 32, 64):
        rs = [R for R in EXPECT_G if EXPECT_G[R] == G]
        assert max(2 * G + 1, 3) in rs and 4 * G in rs                 # the lowest and the highest R of the width
        assert any(R % 4 for R in rs) and any(R % 4 == 0 for R in rs)  # with and without a partial last quad
        assert lanes(BIG_R[G]) == G and BIG_R[G] % 4


@pytest.mark.parametrize("R,kw", [(3, dict(f=1)), (5, dict(quorum_kind=1, ballot_mode=1)), (13, dict(f=6)),
                                  (33, dict(quorum_kind=1)), (65, dict(quorum_kind=2, grid_rows=5, grid_cols=13)),
                                  (3, geometry("mencius8x2")), (3, geometry("mencius256")), (4, geometry("grid16"))])
def test_numpy_restatement_matches_oracle(oracle, R, kw):
    L, A = kw.get("num_leader_groups", 1), kw.get("num_groups", 1)
    S = 8192 if L == 256 else 1024
    kw = dict(kw, num_replicas=R)
    ref = oracle.System(oracle.make_config(num_slots=S, tally_ways=8, **kw))
    W.run_script(ref, recovery_script(S, R, L, A, 100 + R + L))
    st = NpState(ref, L, A)
    masks = quorum_masks(R, L * A, np.random.default_rng(R))
    assert_kinds(st)
    check_scans([ref], st, masks)
    check_info([ref], st, L * A, (0, 17, S // 2 - 1, S - 3, S - 1))
    # max_voted_in has no oracle entry point: held to the oracle's read_acceptor column and to its Phase1b.info
    rng = np.random.default_rng(7)
    for g in sorted({0, L * A - 1}):
        for r in (0, R - 1):
            col = ref.read_acceptor(g, r)[2]
            sl = ref.acceptor_phase1b_info(g, r, 0)[0]
            for first, count in [(0, S), (S - 1, 1)] + [(int(a), int(b)) for a, b in zip(rng.integers(0, S // 2, 40), rng.integers(1, S // 2, 40))]:
                hit = np.nonzero(col[first:first + count] != -1)[0]
                want = first + int(hit[-1]) if len(hit) else -1
                inside = sl[(sl >= first) & (sl < first + count)]
                assert st.max_voted_in(g, r, first, count) == want == (int(inside[-1]) if len(inside) else -1)


@pytest.mark.parametrize("L", [1, 2])
def test_numpy_log_matches_oracle(oracle, L):
    S = 1 << 15
    ref = oracle.System(oracle.make_config(num_slots=S, num_replicas=3, f=1, num_leader_groups=L))
    mine = NpLog(S, L)
    if L == 1:
        top = log_holes([ref, mine], 2048, 1024)
        a, b = ref.replica_read_log(0, S), mine.replica_read_log(0, S)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        assert top < S
        ref, mine = oracle.System(oracle.make_config(num_slots=S, num_replicas=3, f=1)), NpLog(S, 1)
        (hole, n, end), batches = dev_batches(2048, 1024, S)
        got = [ref.replica_chosen(*b) for b in batches]
        assert got == [mine.replica_chosen(*b) for b in batches] == [(0, hole, n - 1), (0, end, end)]
        a, b = ref.replica_read_log(0, S), mine.replica_read_log(0, S)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        ref, mine = oracle.System(oracle.make_config(num_slots=S, num_replicas=3, f=1)), NpLog(S, 1)
    assert log_noop_ranges([ref, mine], 2048, L) <= S
    a, b = ref.replica_read_log(0, S), mine.replica_read_log(0, S)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert b[1].sum() == mine.num


# =====================================================================================================================
# GPU
# =====================================================================================================================
@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()  # raises if libfpx.so is missing: no fallback
    return frankenpaxos_amd


def num_cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def both(fa, oracle, **kw):
    return fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))


def small_state(fa, oracle, S, R, kw, seed):
    """a GPU context and the oracle after the same recovery script, the numpy state read back from the GPU context
    (and equal, cell for cell, to the oracle's)"""
    L, A = kw.get("num_leader_groups", 1), kw.get("num_groups", 1)
    gpu, ref = both(fa, oracle, num_slots=S, tally_ways=8, **dict(kw, num_replicas=R))
    script = recovery_script(S, R, L, A, seed)
    W.assert_same_outputs(W.run_script(gpu, script), W.run_script(ref, script))
    W.assert_same_state(gpu, ref)
    widths = {k[0] for k in gpu.vote_launch_census()["cells"]}
    assert widths == {EXPECT_G[R]}, widths          # ctx->lanes_per_slot, which picks k_phase1b_scan<G> too
    return gpu, ref, NpState(gpu, L, A)


def width_cases():
    """(R, ballot mode, quorum): the ballot mode alternates with R, so that every width runs each kind of quorum with
    scalar and with per-slot ballots"""
    out = []
    for i, R in enumerate(EXPECT_G):
        out.append((R, i % 2, dict(f=(R - 1) // 2)))
        out.append((R, 1 - i % 2, dict(quorum_kind=1)))
        if R in GRIDS:
            out.append((R, R % 2, dict(quorum_kind=2, grid_rows=GRIDS[R][0], grid_cols=GRIDS[R][1])))
    return out


@gpu_test
@pytest.mark.parametrize("R,ballot_mode,kw", width_cases())
def test_scan_at_every_width(fa, oracle, R, ballot_mode, kw):
    """case 1: k_phase1b_scan<G> for every G at its lowest and highest R, with and without a partial last quad, both
    ballot modes, threshold / simple-majority / grid quorums"""
    S = 2048
    gpu, ref, st = small_state(fa, oracle, S, R, dict(kw, ballot_mode=ballot_mode), 31 + R)
    masks = quorum_masks(R, 1, np.random.default_rng(R))
    assert_kinds(st)
    check_scans([gpu, ref], st, masks)
    check_info([gpu, ref], st, 1, (0, 17, S // 2 - 1, S - 3, S - 1))
    gpu.close()


@gpu_test
@pytest.mark.parametrize("G", sorted(BIG_R))
def test_scan_past_the_grid_cap(fa, oracle, G):
    """case 2: launch_p1b caps the grid at num_cus * 16 workgroups of 4 wavefronts, each taking Q = 64 / G slots a pass;
    the scanned count here is more than two whole passes plus a ragged remainder, with distinctive votes in the first
    slot of the second and of the third pass, in the ragged tail and in the last slot.  The state is held to the
    oracle by the outputs of every call and by state_digest; the oracle scans it too."""
    R, Q = BIG_R[G], 64 // G
    assert lanes(R) == G
    per_pass = num_cus() * 16 * 4 * Q
    wm = 5
    count = 2 * per_pass + 3 * Q + Q // 2
    assert count > 2 * per_pass and (Q == 1 or count % Q != 0)
    S = wm + count
    gpu, ref = both(fa, oracle, num_slots=S, num_replicas=R, quorum_kind=1, ballot_mode=G.bit_length() % 2, tally_ways=8)
    rng = np.random.default_rng(G)
    marks = np.array(sorted({wm + per_pass, wm + 2 * per_pass, S - 1} | set(range(S - 1 - count % Q, S))), np.int32)
    for rnd, slot, tgt in ((0, np.nonzero(rng.random(S) < 0.5)[0], None), (1, np.nonzero(rng.random(S) < 0.3)[0], None),
                           (7, marks, acceptors(len(marks), R, [R - 1]))):
        slot = slot.astype(np.int32)
        tgt = pack_bits(W.random_subsets(rng, len(slot), R, 1, R)) if tgt is None else tgt
        val = W.steady_values(slot) if rnd < 7 else 900000 + slot
        a = gpu.phase2_fused(slot, np.full(len(slot), rnd, np.int32), val, tgt)
        b = ref.phase2_fused(slot, np.full(len(slot), rnd, np.int32), val, tgt)
        assert a[0] == b[0] == 0
        for x, y in zip(a[1:], b[1:]):
            np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    assert {k[0] for k in gpu.vote_launch_census()["cells"]} == {G}
    st = NpState(gpu)
    masks = quorum_masks(R, 1, rng)
    for name, w, cap in (("all", wm, S), ("last", wm, S), ("random", wm + Q + 1, S), ("lastquad", wm, count - 1)):
        q = masks[name] | masks["last"] if name == "random" else masks[name]
        mx, sr, sv = same_scan([gpu, ref], st, w, q, cap)
        assert mx == S - 1 and len(sr) == min(cap, S - w) and len(sr) > 2 * per_pass
        at = marks[marks - w < len(sr)] - w          # acceptor R - 1 is in every one of these quorums: its round-7 votes win
        assert len(at) >= 2 and (sr[at] == 7).all() and (sv[at] == 900000 + w + at).all()
    gpu.close()


@gpu_test
@pytest.mark.parametrize("name", ["mencius8x2", "mencius256", "grid16"])
def test_scan_and_info_on_geometries(fa, oracle, row_layout, name):
    """case 3: leader-group-major rows, one quorum mask per (leader group, acceptor group), and more acceptors than one
    workgroup of k_quorum_max_slot"""
    kw = geometry(name)
    R, L, A = kw["num_replicas"], kw.get("num_leader_groups", 1), kw.get("num_groups", 1)
    S = 8192
    gpu, ref, st = small_state(fa, oracle, S, R, kw, 100 + R + L)
    masks = quorum_masks(R, L * A, np.random.default_rng(R + L))
    assert_kinds(st)
    contributors = check_scans([gpu, ref], st, masks)
    assert len(contributors) >= 2, contributors                      # max_slot came from more than one group
    if name == "mencius256":
        assert L * A * R > 256 and max(contributors) * R >= 256       # ... one of them in a later workgroup
    check_info([gpu, ref], st, L * A, (0, 17, S // 2 - 1, S - 3, S - 1))
    gpu.close()


@gpu_test
@pytest.mark.parametrize("R,kw", [(3, dict(f=1)), (5, dict(quorum_kind=1, ballot_mode=1)), (13, dict(f=6)),
                                  (33, dict(quorum_kind=1)), (65, dict(quorum_kind=1, ballot_mode=1)), (253, dict(f=126)),
                                  (3, geometry("mencius8x2")), (3, geometry("mencius256")), (4, geometry("grid16"))])
def test_max_voted_in_matches_numpy(fa, oracle, row_layout, R, kw):
    """case 4: the read path's window maximum, which the oracle has no entry point for, against the numpy restatement
    (pinned on the oracle's columns by test_numpy_restatement_matches_oracle) on a state that equals the oracle's
    cell for cell; again after recycle_slots over part of the windows"""
    S = 8192
    L, A = kw.get("num_leader_groups", 1), kw.get("num_groups", 1)
    gpu, ref, st = small_state(fa, oracle, S, R, kw, 100 + R + L)
    assert check_max_voted_in(gpu, st, L * A) > 10
    for g, r, first, count in ((L * A, 0, 0, 1), (-1, 0, 0, 1), (0, R, 0, 1), (0, -1, 0, 1), (0, 0, -1, 1), (0, 0, 0, -1),
                               (0, 0, S - 1, 2), (0, 0, S, 1)):
        with pytest.raises(fa.FpxError) as e:
            gpu.acceptor_max_voted_in(g, r, first, count)
        assert e.value.status == fa.FPX_EINVAL
    gpu.recycle_slots(64, S // 4 + 100)
    ref.recycle_slots(64, S // 4 + 100)
    W.assert_same_state(gpu, ref)
    after = NpState(gpu, L, A)
    assert (after.vr[64:64 + S // 4 + 100] == -1).all() and (st.vr[64:64 + S // 4 + 100] != -1).any()
    for g in sorted({0, L * A - 1}):
        for r in (0, R - 1):
            for first, count in ((0, S), (0, 64), (0, 65), (40, 257), (100, 4097), (64, S // 4 + 100), (64, S // 4 + 101),
                                 (S // 4, S // 2)):
                assert gpu.acceptor_max_voted_in(g, r, first, count) == after.max_voted_in(g, r, first, count)
    gpu.close()


def same_log(gpu, ref, mine, S):
    va, pa = gpu.replica_read_log(0, S)
    for other in (ref, mine):
        vb, pb = other.replica_read_log(0, S)
        np.testing.assert_array_equal(pa, pb)
        np.testing.assert_array_equal(va, vb)


@gpu_test
def test_replica_log_past_the_caps(fa, oracle):
    """case 5: one batch that reaches k_log_ingest as a single launch of more records than one pass of it (log_holes
    asserts both), with duplicates of the batch before and a mask; the deciding hole in the first pass of k_log_scan,
    in the first slot of its second pass and in the last slot below largestKey; then the _dev form on a torch stream
    with nothing synchronised between two ingests, the first of them longer than a pass again and with a device mask
    (the host form drops masked-out messages before it launches), the second with duplicates of the first"""
    import torch

    ING, SCAN, _ = log_sizes(num_cus())
    S = 1 << int(ING + 3 * SCAN + 12000).bit_length()
    gpu, ref = both(fa, oracle, num_slots=S, num_replicas=3, f=1)
    mine = NpLog(S)
    top = log_holes([gpu, ref, mine], ING, SCAN)
    assert top < S and gpu.replica_state() == (top, top)
    same_log(gpu, ref, mine, S)
    assert gpu.replica_chosen(np.array([S], np.int32), np.array([1], np.int32))[0] == fa.FPX_EINVAL
    gpu.close()

    gpu, ref = both(fa, oracle, num_slots=S, num_replicas=3, f=1)
    mine = NpLog(S)
    dev = torch.device("cuda:0")
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    (hole, n, end), batches = dev_batches(ING, SCAN, S)
    t = [tuple(None if a is None else torch.from_numpy(a).to(dev) for a in svm) for svm in batches]
    torch.cuda.current_stream().synchronize()
    for s, v, m in t:
        gpu.replica_chosen_dev(s, v, m)
    assert gpu.sync() == 0
    for s, v, m in batches:
        want = ref.replica_chosen(s, v, m)
        assert want == mine.replica_chosen(s, v, m)
        assert m is None or want == (0, hole, n - 1)                      # the masked-out message left the hole open
    assert gpu.replica_state() == want[1:] == (end,) * 2
    same_log(gpu, ref, mine, S)
    gpu.set_stream(None)
    gpu.close()


@gpu_test
@pytest.mark.parametrize("L", [1, 2])
def test_replica_noop_ranges_past_the_caps(fa, oracle, L):
    """case 5, the noop ranges: more positions than one pass of k_log_range_first / k_log_range_fill, stride 1 and, on a
    Mencius context, stride L"""
    _, SCAN, RANGE = log_sizes(num_cus())
    S = 1 << int(L * (3 * RANGE + 6000)).bit_length()
    gpu, ref = both(fa, oracle, num_slots=S, num_replicas=3, f=1, num_leader_groups=L)
    mine = NpLog(S, L)
    end = log_noop_ranges([gpu, ref, mine], RANGE, L)
    assert end <= S and gpu.replica_state()[0] > SCAN      # the last executeLog walked more than one pass of k_log_scan
    same_log(gpu, ref, mine, S)
    gpu.close()
