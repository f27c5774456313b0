"""The lift of tests/workloads.py (rounds r -> r + base, values through a bijection of int32) on the CPU oracle alone:
run(lift(script)) == lift(run(script)) for every script family tests/test_gpu_round_range.py plays on the kernels.  This
proves the helper and the scripts, not the kernels: the oracle has no round limit and no packed key words.

No base is rounded down to a multiple of num_leaders: the scripts take their rounds from next_classic_round BEFORE the
lift, and no output or state array carries a leader index (Nack routing by round -> leader is the caller's,
include/fpx.h), so no assertion here or on the GPU depends on round -> leader."""
import itertools

import numpy as np
import pytest

from tests import round_range_cases as RC
from tests import workloads as W

FAMILIES = RC.script_families()


def play(oracle, kw, script):
    ref = oracle.System(oracle.make_config(**kw))
    out = W.run_script(ref, script)
    S = kw["num_slots"]
    tallies = {s: ref.read_tally(s) for s in range(0, S, max(1, S // 97))}
    ranges = {k: ref.read_range_tally(*k) for k in RC.range_keys(script)} if kw.get("num_leader_groups", 1) > 1 else {}
    return out, W.snapshot(ref), tallies, ranges


def test_value_map_is_a_bijection_that_reaches_the_edges():
    for keep_noop in (False, True):
        vmap = W.ValueMap(keep_noop=keep_noop)
        src = W.steady_values(np.array(W.EDGE_SLOTS))
        edges = np.array(W.EDGE_VALUES, np.int32)
        if keep_noop:
            src, edges = src[edges != -1], edges[edges != -1]
            assert vmap(np.array([-1]))[0] == -1
        np.testing.assert_array_equal(vmap(src), edges)
        rng = np.random.default_rng(1)
        v = np.concatenate([rng.integers(-2 ** 31, 2 ** 31, 200000).astype(np.int32), np.array(list(vmap.table), np.int32),
                            np.array(W.EDGE_VALUES, np.int32), src])
        v = np.unique(v)
        assert len(np.unique(vmap(v))) == len(v)
        moved = vmap(v) != (v.view(np.uint32) ^ np.uint32(0x80000000)).view(np.int32)
        assert set(v[moved].tolist()) <= set(vmap.table)       # v ^ 0x80000000 everywhere but in the transpositions


def test_the_bases_are_pinned():
    """top: the script's highest round lands exactly on 2^30 - 2; 24 / 29: a middle round lands on 2^24 - 1 / 2^29 - 1 and
    a later round of the script lies above it"""
    assert W.MAX_ROUND == 2 ** 30 - 2
    for name, (kw, script, _) in FAMILIES.items():
        rounds = W.script_rounds(script)
        assert len(rounds) >= 3 and rounds[0] == 0, name
        bases = W.lift_bases(script)
        assert set(bases) == {"top", "24", "29"}
        lifted = W.script_rounds(W.lift_script(script, bases["top"], W.identity_values))
        assert lifted[-1] == W.MAX_ROUND and lifted[0] == bases["top"] and len(lifted) == len(rounds), name
        for key, bit in (("24", 24), ("29", 29)):
            lifted = W.script_rounds(W.lift_script(script, bases[key], W.identity_values))
            assert (1 << bit) - 1 in lifted and lifted[-1] >= 1 << bit and lifted[0] < 1 << bit, (name, key)


@pytest.mark.parametrize("base", ["top", "24", "29"])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_the_oracle_commutes_with_the_lift(oracle, name, base):
    kw, script, keep_noop = FAMILIES[name]
    vmap = W.ValueMap(keep_noop=keep_noop)
    b = W.lift_bases(script)[base]
    out, snap, tallies, ranges = play(oracle, kw, script)
    lout, lsnap, ltallies, lranges = play(oracle, kw, W.lift_script(script, b, vmap))
    W.assert_same_outputs(lout, W.lift_outputs(out, b, vmap))
    W.assert_same_snapshot(lsnap, W.lift_snapshot(snap, b, vmap))
    assert ltallies == {s: W.lift_tally(t, b, vmap) for s, t in tallies.items()}
    assert any(t for t in tallies.values()) or ranges
    assert len(ranges) == len(lranges)
    for (s, e, r), (state, bits) in ranges.items():
        lstate, lbits = lranges[(s, e, r + b)]
        assert lstate == state
        np.testing.assert_array_equal(lbits, bits)


@pytest.mark.parametrize("name", ["vote-3-masks-1-1", "vote-17-dense-0-0", "tally-8", "ranges", "recovery"])
def test_negative_control_unlifted_outputs_do_not_match(oracle, name):
    """lifting the script but not the outputs (or not the snapshot) must fail: the comparison sees rounds and values"""
    kw, script, keep_noop = FAMILIES[name]
    vmap = W.ValueMap(keep_noop=keep_noop)
    b = W.lift_bases(script)["top"]
    out, snap, _, _ = play(oracle, kw, script)
    lout, lsnap, _, _ = play(oracle, kw, W.lift_script(script, b, vmap))
    with pytest.raises(AssertionError):
        W.assert_same_outputs(lout, out)
    with pytest.raises(AssertionError):
        W.assert_same_snapshot(lsnap, snap)
    with pytest.raises(AssertionError):                       # rounds lifted, values not
        W.assert_same_snapshot(lsnap, W.lift_snapshot(snap, b, W.identity_values))
    with pytest.raises(AssertionError):                       # values lifted, rounds one short
        W.assert_same_outputs(lout, W.lift_outputs(out, b - 1, vmap))


def test_the_scripts_reach_what_they_are_about(oracle):
    """Nack rounds, Chosen values at the literal edge values, votes at MAX_ROUND over votes at MAX_ROUND - 1, unknown
    (slot, round) after a forget, a safe value of -1 with a vote: present in the oracle's lifted outputs"""
    kw, script, _ = FAMILIES["vote-3-masks-1-1"]
    vmap = W.ValueMap()
    b = W.lift_bases(script)["top"]
    out, snap, _, _ = play(oracle, kw, W.lift_script(script, b, vmap))
    nack = np.concatenate([o[5] for o in out if o[0] == "fused"])
    chosen_values = np.concatenate([o[4][o[2] == 1] for o in out if o[0] == "fused"])
    assert nack.max() >= W.MAX_ROUND - 2 and (nack == -1).any()
    assert len(chosen_values) and set(W.EDGE_VALUES) <= set(snap["vote_value"][snap["vote_round"] >= 0].tolist())
    assert snap["vote_round"].max() == W.MAX_ROUND and snap["ballot"].max() == W.MAX_ROUND
    assert (snap["vote_value"][snap["vote_round"] >= 0] < 0).any()

    kw, script, _ = FAMILIES["vote-17-dense-0-0"]              # dense: every slot is chosen, the edge values among them
    out, _, _, _ = play(oracle, kw, W.lift_script(script, W.lift_bases(script)["top"], vmap))
    assert set(W.EDGE_VALUES) <= set(np.concatenate([o[10][o[8] == 1] for o in out if o[0] == "k1k2"]).tolist())

    kw, script, _ = FAMILIES["records"]
    b = W.lift_bases(script)["top"]
    out, snap, _, _ = play(oracle, kw, W.lift_script(script, b, vmap))
    assert (snap["vote_round"] == W.MAX_ROUND).all() and (snap["ballot"] == W.MAX_ROUND).all()
    assert (out[-1][5] == W.MAX_ROUND).all() and not out[-1][2].any()          # stale by one: every acceptor Nacks
    assert (out[5][5][out[5][1] >= 0] >= -1).all() and (out[5][5] == b + 5).any()  # the lazy promise Nacks in round 5

    kw, script, _ = FAMILIES["tally-8"]
    b = W.lift_bases(script)["top"]
    out, _, tallies, _ = play(oracle, kw, W.lift_script(script, b, vmap))
    assert [o[1] for o in out if o[0] == "phase2b"] == [0, 0, 2, 0]           # FPX_EFATAL_UNKNOWN_SLOTROUND after the forget
    assert max(r for t in tallies.values() for r, _, _, _ in t) == W.MAX_ROUND
    assert max(len(t) for t in tallies.values()) >= 5

    kw, script, _ = FAMILIES["recovery"]
    b = W.lift_bases(script)["top"]
    out, _, _, _ = play(oracle, kw, W.lift_script(script, b, vmap))
    _, st, mx, sr, sv = [o for o in out if o[0] == "p1b_scan"][0]
    assert st == 0 and sr.max() == W.MAX_ROUND and (sv[sr >= 0] < -1).any()
    assert sr[5] == W.MAX_ROUND and sv[5] == -1               # a safe value of -1 WITH a vote (slot 5 carries the edge -1)


    # Phase1a: a promise at the round the fold raised (MAX_ROUND, equal: multipaxos promises an equal round again,
    # Acceptor.scala:155 and include/fpx.h -- the script relies on the oracle here, not on a Nack), a Nack below it, Nack
    # rounds MAX_ROUND - 1 and MAX_ROUND from stale Phase2a's
    kw, script, _ = FAMILIES["phase1a"]
    b = W.lift_bases(script)["top"]
    out, snap, _, _ = play(oracle, kw, W.lift_script(script, b, vmap))
    bits = lambda w: int(W.bool_from_bits(np.asarray(w)[None, :], 17)[0].sum())
    p1a = [(op[2] + b, bits(o[2]), bits(o[3])) for op, o in zip(script, out) if op[0] == "phase1a"]
    assert p1a == [(b, 17, 0), (W.MAX_ROUND - 1, 6, 0), (W.MAX_ROUND - 1, 17, 0), (W.MAX_ROUND, 17, 0), (W.MAX_ROUND - 1, 0, 17),
                   (W.MAX_ROUND, 6, 0)]
    assert set(out[3][5].tolist()) == {W.MAX_ROUND - 1} and out[3][2].all()    # below the lazy promise: its third Nacks
    assert set(out[11][5].tolist()) == {W.MAX_ROUND} and not out[11][2].any()  # stale by one everywhere
    assert (snap["ballot"] == W.MAX_ROUND).all()

    # ranges: a length-one range and the single-slot key of the same (slot, round), in both orders -- whoever comes second
    # is swallowed -- and both kinds of entry at MAX_ROUND
    kw, script, _ = FAMILIES["ranges"]
    vnoop = W.ValueMap(keep_noop=True)
    b = W.lift_bases(script)["top"]
    lifted = W.lift_script(script, b, vnoop)
    out, _, _, _ = play(oracle, kw, lifted)
    one = [(k, op) for k, op in enumerate(lifted) if op[0] in ("fused", "ranges") and len(op[1]) == 1]
    assert [op[0] for _, op in one] == ["fused", "ranges", "ranges", "ranges", "fused", "fused"]
    assert all(int(np.atleast_1d(op[3] if op[0] == "ranges" else op[2])[0]) == W.MAX_ROUND for _, op in one)
    assert one[0][1][1][0] == one[1][1][1][0] and one[3][1][1][0] == one[4][1][1][0]       # the same slot
    k = one[0][0]
    assert out[k][2][0] == 1 and out[k][3][0] == W.MAX_ROUND                 # the command first: chosen ...
    assert out[k + 1][5][0] == 0 and not out[k + 1][2].any()                  # ... and the range swallowed: not new, no votes
    assert out[k + 3][5][0] == 1 and out[k + 3][6][0] == 1                    # the range first: new and chosen ...
    assert out[k + 4][2][0] == 0 and out[k + 4][3][0] == -1                   # ... and the command swallowed
    assert sum(int(o[5].sum()) for o in out if o[0] == "ranges") > 900        # the refill after the rehash is new


def test_vote_matrix_covers_the_pairs():
    """the GPU file's vote cases: every width with each delivery it has, both ballot modes and both pipelines; every pair
    of (ballot mode, delivery), (ballot mode, fused), (delivery, fused); ps 0 / 1 / 2 follow from the ballot mode (a
    ballot per cell: fresh batches first, then Phase1a's); bases 24 and 29 at some width of every G"""
    cases = RC.vote_matrix()
    top = [c for c in cases if c[4] == "top"]
    assert {RC.lanes(R) for R in RC.WIDTHS} == {1, 8, 64} and RC.WIDTHS == (3, 17, 32, 129, 256)
    for R in RC.WIDTHS:
        mine = [c for c in top if c[0] == R]
        assert {c[2] for c in mine} == set(RC.deliveries_of(R)), R
        assert {c[1] for c in mine} == {0, 1} and {c[3] for c in mine} == {True, False}, R
    dls = set(RC.DELIVERY)
    assert {(c[1], c[2]) for c in top} == set(itertools.product((0, 1), dls))
    assert {(c[1], c[3]) for c in top} == set(itertools.product((0, 1), (True, False)))
    assert {(c[2], c[3]) for c in top} == set(itertools.product(dls, (True, False)))
    for G in (1, 8, 64):
        assert {c[4] for c in cases if RC.lanes(c[0]) == G} >= {"top"} and \
            {c[4] for c in cases if RC.lanes(c[0]) == G} & {"24", "29"}
    assert {c[4] for c in cases} == {"top", "24", "29"}
    assert len(set(cases)) == len(cases) <= 24
