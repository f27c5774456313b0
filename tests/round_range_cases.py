"""The scripts and the case lists of the round-range tests (plain numpy, no GPU): tests/test_round_range_cpu.py proves
on the oracle alone that each of them commutes with the lift of tests/workloads.py, tests/test_gpu_round_range.py plays
them lifted on the kernels.

Every script is written in small rounds; lift_bases(script) then moves it so that its highest round is MAX_ROUND =
2^30 - 2 ("top"), or so that its rounds straddle 2^24 or 2^29."""
import numpy as np

from tests import range_batches as RB
from tests import workloads as W

DELIVERY = {"dense": 0, "masks": 1, "scattered": 2, "packed": 3}      # the census's mode
WIDTHS = (3, 17, 32, 129, 256)                                          # G = 1, 8, 8, 64, 64


def lanes(R):
    G = 1
    while 4 * G < R:
        G *= 2
    return G


def deliveries_of(R):
    """the packed walk takes rows of 253 ... 256 cells only (include/fpx.h)"""
    return ("dense", "masks", "scattered", "packed") if R >= 253 else ("dense", "masks", "scattered")


def vote_matrix():
    """(R, ballot_mode, delivery, fused, base): every width with each of its deliveries, ballot mode and fused / k1k2
    alternating so that all their pairs occur (test_round_range_cpu.test_vote_matrix_covers_the_pairs), all at base
    "top"; then one case per width at "24" or "29" """
    out = []
    for w, R in enumerate(WIDTHS):
        for j, dl in enumerate(deliveries_of(R)):
            bm = (j + w) % 2
            fu = (j // 2 + w + (j == 1)) % 2 == 0
            out.append((R, bm, dl, fu, "top"))
            if dl == "packed":           # one width has it: both ballot modes and both pipelines there
                out.append((R, 1 - bm, dl, not fu, "top"))
    for w, R in enumerate(WIDTHS):
        out.append((R, (w + 1) % 2, ("masks", "dense", "scattered")[w % 3], w % 2 == 1, ("24", "29")[w % 2]))
    return out


def adversarial_rounds(seed, epochs):
    """the rounds W.adversarial_script(.., seed, epochs) goes through (they depend on nothing else)"""
    return W.script_rounds(W.adversarial_script(epochs, 1, 1, seed, epochs=epochs))


def seed_with_rounds(seed, epochs, at_least=3):
    """the first seed from `seed` on whose adversarial script changes leaders often enough for `at_least` rounds: with a
    ballot per cell that is what leaves lazy promises outstanding (ps 2) and Nacks that carry a round"""
    while len(adversarial_rounds(seed, epochs)) < at_least:
        seed += 1
    return seed


def vote_script(R, delivery, fused, per=3000, epochs=6, seed=0):
    """(S, script): two batches of fresh slots in round 0 with no Phase1a before them (a ballot per cell: ps 1), one of
    several workgroups and one solo; then the adversarial stream -- leader changes, Phase1a's with partial targets,
    Nacks, re-proposals, duplicate Phase2b's when unfused -- in batches of `per` messages, every second one cut into
    solo launches.  "packed" delivers to runs of neighbouring acceptors (W.run_subsets)"""
    G = lanes(R)
    solo_n = 32 if G == 64 else 400
    S_adv = per * epochs
    S = S_adv + 4096
    subsets = W.run_subsets if delivery == "packed" else W.random_subsets
    rng = np.random.default_rng(seed)
    kind = "fused" if fused else "k1k2"
    script = []
    for lo, n in ((S_adv, 3000), (S_adv + 3000, solo_n)):
        slot = np.arange(lo, lo + n, dtype=np.int32)
        tgt = None if delivery == "dense" else W.bits_from_bool(subsets(rng, n, R, max(1, R // 2), R))
        op = (kind, slot, np.zeros(n, np.int32), W.steady_values(slot), tgt)
        script.append(op if fused else op + (rng.random(n) < 0.1,))
    seed = seed_with_rounds(seed, epochs)
    script += W.shaped(W.adversarial_script(S_adv, R, R // 2 + 1, seed, epochs=epochs, fused=fused, subsets=subsets),
                     delivery, 2, solo_n)
    return S, script


def whole(n, r):
    return np.full(n, r, np.int32)


def records_script(R, S=4096):
    """dense G = 64 with a ballot per cell, where whole-group chunks keep one (round, value) record per row: rounds 0 ... 8,
    so that at base "top" round 8 is MAX_ROUND.  In order: every row compact in round 0; a partial-target vote over compact
    rows (the record expands into cells); a lazy promise from slot 2050 on and a dense batch across it (steady chunks, the
    mixed chunk at 2048, rows that Nack in every cell); rows voted in round 7 = MAX_ROUND - 1 and then in round 8 =
    MAX_ROUND (their uniform ballot rows then hold MAX_ROUND); the tallies forgotten and the equal-round re-vote at 8"""
    f = (R - 1) // 2
    slot, _, val = W.steady_stream(S)
    rng = np.random.default_rng(R)
    tgt = W.bits_from_bool(W.random_subsets(rng, 1000, R, f + 1, f + 1))
    return [("phase1a", 0, 0, 0, None), ("flush",),
            ("fused", slot, whole(S, 0), val, None),
            ("fused", slot[1000:2000], whole(1000, 2), val[1000:2000] + 1, tgt),
            ("phase1a", 0, 5, 2050, None),
            ("fused", slot[1024:3072], whole(2048, 3), val[1024:3072] + 7, None),
            ("flush",),
            ("fused", slot[:1023], whole(1023, 6), val[:1023], None),
            ("phase1a", 0, 7, 0, None), ("flush",),
            ("fused", slot, whole(S, 7), val + 4, None),
            ("fused", slot, whole(S, 8), val + 5, None),
            ("forget", 0, S),
            ("fused", slot, whole(S, 8), val + 5, None),
            ("fused", slot[100:200], whole(100, 7), val[100:200], None)]      # stale by one: Nack round MAX_ROUND


def phase1a_script(R, S=8192):
    """device-resident steps with a ballot per cell: round 4 is MAX_ROUND at base "top".  A lazy promise at round 3 =
    MAX_ROUND - 1 on some acceptors; Phase2a's below it (Nack round 3), at it and above it (4), each of several
    workgroups so that a fold is pending when the next Phase1a arrives; Phase1a's at an equal round, below (Nack) and
    with a watermark above 0"""
    slot = np.arange(S, dtype=np.int32)
    val = W.steady_values(slot)
    some = W.bits_from_bool(np.arange(R)[None, :] % 3 == 0)[0]
    q = S // 4
    return [("phase1a", 0, 0, 0, None),
            ("fused", slot[:q], whole(q, 0), val[:q], None),
            ("phase1a", 0, 3, 0, some),
            ("fused", slot[q:2 * q], whole(q, 2), val[q:2 * q], None),          # below: the promised third Nacks in 3
            ("phase1a", 0, 3, 0, None),
            ("fused", slot[2 * q:3 * q], whole(q, 3), val[2 * q:3 * q], None),  # at it
            ("fused", slot[3 * q:], whole(q, 4), val[3 * q:], None),            # above it: raises the bound to MAX_ROUND
            ("phase1a", 0, 4, 0, None),                                         # equal to what the fold raised
            ("phase1a", 0, 3, 0, None),                                         # below: Nack
            ("phase1a", 0, 4, q + 1, some),
            ("fused", slot[:q], whole(q, 4), val[:q] + 1, None),
            ("fused", slot[q:2 * q], whole(q, 3), val[q:2 * q] + 1, None)]      # stale by one everywhere


def tally_script(R, ways=8, S=1024):
    """tally keys up to round 5 (MAX_ROUND at "top") through open / phase2a / phase2b: with 8 ways, six live rounds of one
    slot; with one way (the oracle has no such limit, so the script never holds two rounds of a slot) each round is
    forgotten before the next is opened.  Then in both: a key at round 5 that is Done, a Phase2b for it (ignored), the
    lower slots forgotten, the same (slot, round) unknown there, and opened again"""
    n = 64
    slot = np.arange(n, dtype=np.int32) * 3
    val = W.steady_values(slot)
    few = W.bits_from_bool(np.arange(R)[None, :].repeat(n, 0) < max(1, R // 4))     # below every quorum
    ops = [("phase1a", 0, 0, 0, None)]
    for r in (0, 1, 2, 3, 4):
        ops += [("open", slot, whole(n, r), val + r), ("phase2a", slot, whole(n, r), val + r, few)]
        if ways == 1:
            ops += [("phase2b", slot, whole(n, r), few), ("forget", 0, S)]
    ops += [("open", slot, whole(n, 5), val + 5)]
    ops += [("k1k2", slot, whole(n, 5), val + 5, None, np.arange(n) % 2 == 0)]      # known: not new; chosen, Done at 5
    if ways > 1:
        ops += [("phase2b", slot, whole(n, 4), few)]                                # Pending at MAX_ROUND - 1
    ops += [("phase2b", slot, whole(n, 5), few)]                                    # Done at MAX_ROUND: ignored
    ops += [("forget", 0, 96)]
    ops += [("phase2b", slot, whole(n, 5), few)]                                    # unknown for the slots below 96
    ops += [("open", slot, whole(n, 5), val + 6), ("phase2b", slot, whole(n, 5), few)]
    return ops


def range_geometry():
    return dict(L=4, A=2, R=5, f=2, rows=RB.span_straddlers_rows(4) + 144)


def range_script():
    """(S, script): the four range shapes of tests/range_batches.py, dense, with target masks and after a competing
    leader's Phase1a, in rounds up to 25 (MAX_ROUND at "top"); a command in the first slot of a length-one range of the
    same round (the KEY_RANGE shadow) in both orders; the table collected (rehash) with such entries in it and filled
    again with 900 ranges"""
    g = range_geometry()
    L, A, R, f = g["L"], g["A"], g["R"], g["f"]
    S = L * g["rows"]
    rng = np.random.default_rng(11)
    ops = [("phase1a", grp, 0, 0, None) for grp in range(L * A)]
    for lap, delivery in enumerate(("dense", "masks", "nacks")):
        rounds = [lg % 3 + 10 * lap for lg in range(L)]
        if delivery == "nacks":
            for grp in range(0, L * A, 2):
                ops.append(("phase1a", grp, 25, 0, W.bits_from_bool(W.random_subsets(rng, 1, R, 1, R // 2))[0]))
        batches = [RB.residue_batch(S, L, rounds), RB.overlap_batch(S, L, rounds)[:3], RB.aligned_runs(L, 144, rounds),
                   RB.span_straddlers(L, rounds)]
        for k, (start, end, rnd) in enumerate(batches):
            tm = RB.target_masks(len(start), A, R, f) if delivery == "masks" else None
            ops.append(("ranges" if (k + lap) % 2 == 0 else "ranges_k1k2", start, end, rnd, tm))
        if lap == 1:
            ops.append(("forget", 0, S // 2))
    # the shadow: slot s of leader group 1 in round 25, as a command first and as the range [s, s + 1) first
    for s, first in ((S - L + 1, "command"), (S - 2 * L + 1, "range")):
        cmd = ("fused", np.array([s], np.int32), whole(1, 25), np.array([77], np.int32), None)
        rge = ("ranges", np.array([s], np.int32), np.array([s + 1], np.int32), whole(1, 25), None)
        ops += [cmd, rge, rge] if first == "command" else [rge, cmd, cmd]
    ops.append(("forget", S // 2, S - S // 2))
    start, end, rnd = RB.many_ranges(S, L, 900, [25] * L)     # n A R > 8192: four launches in place of the chain
    ops.append(("ranges", start, end, rnd, None))
    return S, ops


def range_keys(script):
    """every (start, end, round) a script's range ops carry"""
    keys = set()
    for op in script:
        if op[0].startswith("ranges"):
            keys |= {(int(s), int(e), int(r)) for s, e, r in zip(op[1], op[2], op[3])}
    return sorted(keys)


def recovery_script(R, S=2048):
    """votes in several rounds per slot up to round 9 (MAX_ROUND at "top"), some slots voted by one acceptor only; values
    that the map sends to negative numbers and to -1; then the recovery scan at two watermarks, Phase1b.info of two
    acceptors, and the replica's log fed with the chosen values (negative ones and -1 among them)"""
    f = (R - 1) // 2
    slot = np.arange(S, dtype=np.int32)
    val = W.steady_values(slot)
    rng = np.random.default_rng(R + 9)
    ops = [("phase1a", 0, 0, 0, None)]
    for r, (lo, hi) in ((0, (0, S)), (4, (0, S // 2)), (8, (S // 4, S // 2)), (9, (0, 64))):
        n = hi - lo
        tgt = W.bits_from_bool(W.random_subsets(rng, n, R, 1, R))
        # (the highest round carries the slots' own values: the edge values, -1 among them, are then the safe ones)
        ops.append(("fused", slot[lo:hi], whole(n, r), val[lo:hi] + (r if r < 9 else 0), tgt))
    quorum = np.ones((1, R), bool)
    quorum[0, 0] = False
    ops += [("p1b_scan", 0, W.bits_from_bool(quorum), S), ("p1b_scan", 100, W.bits_from_bool(quorum), S),
            ("p1b_info", 0, 0, 0), ("p1b_info", 0, R - 1, 37)]
    order = rng.permutation(512).astype(np.int32)
    ops += [("chosen", order[:300], val[order[:300]]), ("read_log", 0, 512), ("chosen", order[300:], val[order[300:]]),
            ("read_log", 0, 600)]
    return ops


def sharded_script(S=4096, R=256):
    """the replica-sharded step of tests/test_gpu_sharding_world2.py as a script: everybody promises round 0, 100 acceptors
    spread over the ranks promise round 4 (MAX_ROUND at "top"); a step in round 3 that those Nack with 4, then one in
    round 4 in which everybody asked votes.  k1k2 without duplicates: the sharded entry point is open + K1 + K2"""
    rng = np.random.default_rng(77)
    slot, _, val = W.steady_stream(S)
    ahead = W.bits_from_bool(W.random_subsets(rng, 1, R, 100, 100))[0]
    ops = [("phase1a", 0, 0, 0, None), ("phase1a", 0, 4, 0, ahead)]
    for r in (3, 4):
        tgt = W.bits_from_bool(W.random_subsets(rng, S, R, 120, 256))
        ops.append(("k1k2", slot, whole(S, r), val, tgt, np.zeros(S, bool)))
    return ops


def script_families():
    """name -> (config keywords, script, keep_noop): what the CPU test proves the relation for, at sizes the oracle plays
    in a moment"""
    fam = {}
    for R, dl, fu in ((3, "masks", True), (17, "dense", False), (256, "packed", True), (129, "scattered", False)):
        for bm in (0, 1):
            S, script = vote_script(R, dl, fu, per=300, epochs=6, seed=R)
            fam["vote-%d-%s-%d-%d" % (R, dl, fu, bm)] = (dict(num_slots=S, num_replicas=R, quorum_kind=1, ballot_mode=bm,
                                                              tally_ways=8), script, False)
    fam["records"] = (dict(num_slots=4096, num_replicas=129, f=64, ballot_mode=1, tally_ways=8), records_script(129), False)
    fam["phase1a"] = (dict(num_slots=8192, num_replicas=17, f=8, ballot_mode=1, tally_ways=8), phase1a_script(17), False)
    for ways in (1, 8):
        fam["tally-%d" % ways] = (dict(num_slots=1024, num_replicas=5, f=2, tally_ways=ways), tally_script(5, ways), False)
    g = range_geometry()
    S, script = range_script()
    fam["ranges"] = (dict(num_slots=S, num_replicas=g["R"], num_groups=g["A"], num_leader_groups=g["L"], f=g["f"],
                          tally_ways=8), script, True)
    for bm in (0, 1):
        fam["sharded-%d" % bm] = (dict(num_slots=4096, num_replicas=256, f=127, ballot_mode=bm, tally_ways=8), sharded_script(),
                                  False)
    fam["recovery"] = (dict(num_slots=2048, num_replicas=5, f=2, tally_ways=8), recovery_script(5), False)
    return fam
