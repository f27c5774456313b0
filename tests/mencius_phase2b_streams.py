"""Streams of per-acceptor Phase2b and Phase2bNoopRange messages for fpx_mencius_proxy_phase2b_msgs
(tests/test_gpu_mencius_phase2b_msgs.py runs them on the GPU, tests/test_mencius_phase2b_msgs_cpu.py checks on the
reference models alone that they are not vacuous).

A stream opens a set of single slots and a set of noop ranges -- among the ranges one of length 0 (no row), one of length
1, one that ends at S, two rounds of one range, and two length-1 ranges whose key meets a single-slot tally (one opened
after the slot: swallowed, mencius/ProxyLeader.scala:259-266; one opened before it: the slot's Phase2b's are ignored,
:327-333).  Every acceptor group of a range gets the votes of a random subset of its acceptors, drawn independently per
group with a size uniform in 0 .. R -- for one range in three uniform in f + 1 .. R instead, so that with three acceptor
groups (every group must reach f + 1) enough ranges still complete; 10 % of the votes are sent twice.  The range messages
are laid out range-major (the votes of a range adjacent), acceptor-major, or in a random permutation; the Phase2b's of a
tests/phase2b_streams.py-style stream (entries with vote subsets of size uniform in 0 .. R, 10 % duplicates, the same
layout) are interleaved at random positions, both halves keeping their order, and the whole is cut to exactly n.

Two reference models: rows_path (a Python fold of a burst into rows, then proxy_phase2b / proxy_phase2b_noop_ranges of
the oracle or of a second context -- the contract of include/fpx.h) and maps_run (oracle/mencius_maps.py message at a
time)."""
import numpy as np

PHASE2B, RANGE = 2, 7  # FPX_WIRE_PHASE2B, FPX_WIRE_PHASE2B_NOOP_RANGE

# the smallest shapes at which each code path can go wrong; all FPX_BALLOT_ACCEPTOR
SHAPES = {
    "a1r3": dict(num_slots=4096, num_replicas=3, num_groups=1, num_leader_groups=8, f=1),   # BASELINE config 5's shape
    "a2r3": dict(num_slots=4096, num_replicas=3, num_groups=2, num_leader_groups=4, f=1),   # the group index matters
    "a3r5": dict(num_slots=4096, num_replicas=5, num_groups=3, num_leader_groups=2, f=2),   # every group must reach f + 1
    "r256": dict(num_slots=512, num_replicas=256, num_groups=1, num_leader_groups=2, f=127),  # bits in all four words
}
LAYOUTS = ("range_major", "acceptor_major", "random")
LENGTHS = (1, 63, 64, 65, 257, 20000)  # the wavefront and workgroup edges; many workgroups
MAX_RANGES = 1200                      # the range table of these shapes holds 2048 live entries


def _votes(rng, entries, groups, R, f, strong_every=0):
    """(entry, group, bit) per vote: per (entry, group) a random subset of a size uniform in 0 .. R (f + 1 .. R for every
    strong_every-th entry), 10 % of the votes twice"""
    ent, grp, bit = [], [], []
    for e in range(entries):
        for g in range(groups):
            lo = f + 1 if strong_every and e % strong_every == 0 else 0
            k = int(rng.integers(lo, R + 1))
            for b in rng.choice(R, size=k, replace=False):
                ent.append(e), grp.append(g), bit.append(int(b))
    ent, grp, bit = np.array(ent, np.int64), np.array(grp, np.int64), np.array(bit, np.int64)
    dup = rng.random(len(ent)) < 0.10
    return np.concatenate([ent, ent[dup]]), np.concatenate([grp, grp[dup]]), np.concatenate([bit, bit[dup]])


def _order(rng, layout, ent, bit):
    if layout == "random":
        return rng.permutation(len(ent))
    return np.argsort(ent if layout == "range_major" else bit, kind="stable")


class Stream:
    """single_slot / single_round / single_value and range_start / range_end / range_round: what to open (open_all);
    kind / group_index / acceptor_index / slot / slot_end / round: the n messages; swallowed: the keys of the ranges
    that a single-slot tally holds"""

    def __init__(self, shape, n, layout, seed):
        kw = SHAPES[shape]
        rng = np.random.default_rng(seed)
        S, R, A, L, f = kw["num_slots"], kw["num_replicas"], kw["num_groups"], kw["num_leader_groups"], kw["f"]
        self.kw, self.shape = kw, shape
        per_range = A * (R / 2.0 + (f + 1) / 6.0) * 1.1         # votes of a range, on average
        want_ranges = int(min(MAX_RANGES, max(8, np.ceil(0.4 * n / per_range))))
        # ---- the ranges: the directed ones first --------------------------------------------------------------------
        sA, sB, sC = (int(x) for x in rng.choice(np.arange(8, S - 64), size=3, replace=False))
        # length 0, length 1, ends at S, two rounds of one range, and the two whose key meets a single-slot tally
        ranges = [(sA, sA, 0), (sA, sA + 1, 0), (S - 37, S, 0), (S - 90, S - 50, 0), (S - 90, S - 50, 1), (sB, sB + 1, 0),
                  (sC, sC + 1, 0)]
        keys = set(ranges)
        while len(ranges) < want_ranges:
            start = int(rng.integers(0, S - 1))
            length = int(rng.choice([0, 2, 3, 5, 9, 17, 40]))  # (length 1 only where directed: its key is a slot's)
            key = (start, min(S, start + length), int(rng.integers(0, 2)) if len(ranges) % 16 == 0 else 0)
            if key not in keys:
                keys.add(key), ranges.append(key)
        self.range_start = np.array([k[0] for k in ranges], np.int32)
        self.range_end = np.array([k[1] for k in ranges], np.int32)
        self.range_round = np.array([k[2] for k in ranges], np.int32)
        self.swallowed = {(sB, sB + 1, 0)}
        self.shadowed = {(sC, 0)}                              # single slots held by a length-1 range
        r_ent, r_grp, r_bit = _votes(rng, len(ranges), A, R, f, strong_every=3)
        o = _order(rng, layout, r_ent, r_bit)
        r_ent, r_grp, r_bit = r_ent[o], r_grp[o], r_bit[o]
        # ---- the single slots: (slots[e % nslots], round e // nslots), as tests/phase2b_streams.py ----------------------
        free = np.setdiff1d(np.arange(S), [sA, sB, sC])
        need = max(0, n - len(r_ent)) + 8
        entries = int(np.ceil(need / (0.55 * R))) + 2
        while True:
            entries = min(entries, 3 * len(free))
            nslots = min(len(free), entries)
            slots = rng.choice(free, size=nslots, replace=False)
            oslot = [sB, sC] + [int(slots[e % nslots]) for e in range(entries)]
            oround = [0, 0] + [e // nslots for e in range(entries)]
            p_ent, _, p_bit = _votes(rng, len(oslot), 1, R, f)
            if len(p_ent) >= need or entries == 3 * len(free):
                break
            entries += max(2, entries // 10)
        o = _order(rng, layout, p_ent, p_bit)[:need]
        p_ent, p_bit = p_ent[o], p_bit[o]
        self.single_slot, self.single_round = np.array(oslot, np.int32), np.array(oround, np.int32)
        self.single_value = (1000 + np.arange(len(oslot))).astype(np.int32)
        # ---- interleave, both halves in their order, and cut to n ------------------------------------------------------
        total = len(r_ent) + len(p_ent)
        is_range = np.zeros(total, bool)
        is_range[rng.choice(total, size=len(r_ent), replace=False)] = True
        kind = np.where(is_range, RANGE, PHASE2B).astype(np.int32)
        slot, end, rnd = np.zeros(total, np.int32), np.full(total, -1, np.int32), np.zeros(total, np.int32)
        grp, acc = np.zeros(total, np.int32), np.zeros(total, np.int32)
        slot[is_range], end[is_range], rnd[is_range] = self.range_start[r_ent], self.range_end[r_ent], self.range_round[r_ent]
        grp[is_range], acc[is_range] = r_grp, r_bit
        ps = self.single_slot[p_ent]
        slot[~is_range], rnd[~is_range], acc[~is_range] = ps, self.single_round[p_ent], p_bit
        grp[~is_range] = (ps // L) % A                         # the slot's acceptor group (the library ignores it)
        assert total >= n, "the window has no room for %d messages" % n
        self.kind, self.group_index, self.acceptor_index = kind[:n], grp[:n], acc[:n]
        self.slot, self.slot_end, self.round = slot[:n], end[:n], rnd[:n]
        self.n = n

    def decoded(self, lo=0, hi=None):
        """messages [lo, hi) as fpx_wire_mencius_decode_proxy_leader_inbound leaves them"""
        hi = self.n if hi is None else hi
        return {k: getattr(self, k)[lo:hi].copy() for k in ("kind", "group_index", "acceptor_index", "slot", "slot_end", "round")}

    def range_keys(self):
        return list(zip(self.range_start.tolist(), self.range_end.tolist(), self.range_round.tolist()))


def open_all(sys_, st):
    """the stream's opens on a context or on the oracle's System: the single slots (all but the one a length-1 range holds),
    the ranges, then that slot -- a duplicate, like the range whose key the other directed slot holds"""
    held = np.array([(int(s), int(r)) in st.shadowed for s, r in zip(st.single_slot, st.single_round)])
    rc, new = sys_.proxy_open(st.single_slot[~held], st.single_round[~held], st.single_value[~held])
    assert rc == 0 and new.all()
    rc, new = sys_.proxy_open_noop_ranges(st.range_start, st.range_end, st.range_round)
    assert rc == 0 and [bool(x) for x in new] == [k not in st.swallowed for k in st.range_keys()]
    rc, new = sys_.proxy_open(st.single_slot[held], st.single_round[held], st.single_value[held])
    assert rc == 0 and not new.any()


def fold(d, kw):
    """the burst folded into rows, in order of first appearance, a message whose bit is no member left out:
    (first index, slot, round, bits[4]) per Phase2b row and (first index, start, end, round, bits[A][4]) per range row"""
    R, A = kw["num_replicas"], kw["num_groups"]
    prow, rrow = {}, {}
    for i, (k, g, a, s, e, r) in enumerate(zip(*(d[x].tolist() for x in
                                                 ("kind", "group_index", "acceptor_index", "slot", "slot_end", "round")))):
        if not 0 <= a < R:
            continue
        if k == PHASE2B:
            row = prow.setdefault((s, r), (i, np.zeros(4, np.uint64)))
            row[1][a >> 6] |= np.uint64(1 << (a & 63))
        elif k == RANGE:
            row = rrow.setdefault((s, e, r), (i, np.zeros((A, 4), np.uint64)))
            row[1][g, a >> 6] |= np.uint64(1 << (a & 63))
    return ([(i, s, r, b) for (s, r), (i, b) in prow.items()], [(i, s, e, r, b) for (s, e, r), (i, b) in rrow.items()])


def rows_path(sys_, d, kw, phase2b=True, ranges=True):
    """the contract: the folded rows through proxy_phase2b and proxy_phase2b_noop_ranges of `sys_` (the oracle's System
    or a second context), each row's outcome at the index of its first member message:
    (status, newly_chosen, chosen_round, chosen_value)"""
    n = len(d["kind"])
    ch, cr, cv = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    prows, rrows = fold(d, kw)
    status = 0
    if phase2b and prows:
        at = np.array([p[0] for p in prows])
        st, pch, pcr, pcv = sys_.proxy_phase2b([p[1] for p in prows], [p[2] for p in prows], np.stack([p[3] for p in prows]))
        status = status or st
        ch[at], cr[at], cv[at] = pch, pcr, pcv
    if ranges and rrows:
        at = np.array([p[0] for p in rrows])
        st, rch = sys_.proxy_phase2b_noop_ranges([p[1] for p in rrows], [p[2] for p in rrows], [p[3] for p in rrows],
                                                 np.stack([p[4] for p in rrows]))
        status = status or st
        rch = np.asarray(rch, np.uint8)
        ch[at] = rch
        cr[at] = np.where(rch != 0, np.array([p[3] for p in rrows], np.int32), -1)
    return status, ch, cr, cv


def chosen_keys(d, ch):
    """the keys (start, end, round) of the flagged messages of a burst; a Phase2b's key is (slot, slot + 1, round)"""
    out = []
    for i in np.nonzero(ch)[0].tolist():
        s, r = int(d["slot"][i]), int(d["round"][i])
        out.append((s, int(d["slot_end"][i]) if d["kind"][i] == RANGE else s + 1, r))
    return out


def maps_run(mencius_maps, st):
    """the stream message at a time through oracle/mencius_maps.py's ProxyLeader: (chosen keys in order, the deciding
    message's index per chosen key, {key: 1 Pending / 2 Done} of every opened key)"""
    kw = st.kw
    pl = mencius_maps.ProxyLeader(kw["f"] + 1, kw["num_groups"])
    held = [(int(s), int(r)) in st.shadowed for s, r in zip(st.single_slot, st.single_round)]
    singles = list(zip(st.single_slot.tolist(), st.single_round.tolist(), st.single_value.tolist()))
    for (s, r, v), h in zip(singles, held):
        if not h:
            assert pl.handle_phase2a(s, r, v)
    for k in st.range_keys():
        assert pl.handle_phase2a_noop_range(*k) == (k not in st.swallowed)
    for (s, r, v), h in zip(singles, held):
        if h:
            assert not pl.handle_phase2a(s, r, v)
    chosen, decided = [], {}
    for i, (k, g, a, s, e, r) in enumerate(zip(st.kind.tolist(), st.group_index.tolist(), st.acceptor_index.tolist(),
                                               st.slot.tolist(), st.slot_end.tolist(), st.round.tolist())):
        out = pl.handle_phase2b(s, r, a) if k == PHASE2B else pl.handle_phase2b_noop_range(s, e, r, g, a)
        assert out != "fatal"
        if out is not None:
            key = (s, s + 1, r) if k == PHASE2B else (s, e, r)
            chosen.append(key)
            decided[key] = i
    states = {key: 2 if v == "done" else 1 for key, v in pl.states.items()}
    return chosen, decided, states
