"""tests/range_batches.py on the CPU: the builders keep their promises (each asserts them itself; here at every geometry
tests/test_gpu_range_matrix.py uses), and the oracle's fused form of every batch is its single-message handlers in array
order -- the new shapes are well defined on the reference side before the GPU is compared with it."""
import itertools

import numpy as np
import pytest

from tests import range_batches as RB
from tests import test_gpu_range_matrix as M
from tests import workloads as W

GEOMS = [(4, 1, 3, 1), (5, 1, 4, 1), (3, 2, 5, 2), (7, 3, 8, 3), (2, 1, 9, 4), (3, 1, 32, 15), (2, 4, 100, 49)]
ROWS = 144


def batches(L, S=None):
    S = L * ROWS if S is None else S
    rounds = [lg % 3 for lg in range(L)]
    return {
        "residue": RB.residue_batch(S, L, rounds),
        "overlap": RB.overlap_batch(S, L, rounds)[:3],
        "aligned": RB.aligned_runs(L, ROWS, rounds),
        "straddle": RB.span_straddlers(L, rounds),
        "many": RB.many_ranges(S, L, 150, rounds),
    }


@pytest.mark.parametrize("L", [2, 3, 4, 5, 7, 128])
def test_builders_keep_their_promises(L):
    for name, (start, end, rnd) in batches(L).items():
        assert start.dtype == end.dtype == rnd.dtype == np.int32 and len(start) == len(end) == len(rnd) > 0
        assert (end <= L * ROWS).all() and (start <= end).all(), name
        for lg in range(L):          # the run contract: one round per leader group
            assert len(set(rnd[start % L == lg].tolist())) <= 1, name
    # a window that is no whole number of rows (S % L != 0): the same promises, end == S included
    S = L * ROWS - 1
    start, end, rnd = RB.residue_batch(S, L)
    assert S in end and {int(x) % L for x in end - start} == set(range(L))
    RB.overlap_batch(S, L)


def test_overlap_batch_duplicates_sit_where_they_are_asked():
    start, end, rnd, dups = RB.overlap_batch(5 * ROWS, 5)
    assert dups[-1] == (0, len(start) - 1) and dups[0][1] == dups[0][0] + 1
    plain = RB.overlap_batch(5 * ROWS, 5, duplicates=False)
    assert plain[3] == [] and len(plain[0]) == len(start) - 2 and RB.distinct_keys(*plain[:3])
    ov = RB.overlaps(*plain[:2], 5)
    assert ov.sum() == 5 * 4 and (~ov).sum() == 5 * 4      # overlapping by a row and nested / disjoint and touching


def test_aligned_runs_and_span_straddlers_by_hand():
    start, end, rnd = RB.aligned_runs(4, ROWS)
    ja, jb = RB.rows_of(start, end, 4)
    assert sorted(set((jb - ja + 1).tolist())) == list(range(1, 10))
    start, end, rnd = RB.span_straddlers(16)
    ja, jb = RB.rows_of(start, end, 16)
    assert list(zip(ja.tolist(), jb.tolist()))[:5] == [(0, 0), (5, 7), (5, 8), (7, 7), (7, 8)]
    assert not RB.overlaps(start, end, 16).any()          # enough leader groups: every range alone in its rows
    assert RB.overlaps(*RB.span_straddlers(2)[:2], 2).sum() == 0 and RB.span_straddlers_rows(2) == 144


@pytest.mark.parametrize("L,A,R,f", GEOMS)
def test_oracle_fused_form_of_every_batch_is_the_singles_in_order(oracle, L, A, R, f):
    """as test_oracle_batched_ranges_are_the_singles_in_order: dense, with target masks that leave acceptor groups below
    quorum, and after a competing leader's Phase1a on a few acceptors"""
    S = L * ROWS
    kw = dict(num_slots=S, num_replicas=R, num_groups=A, num_leader_groups=L, f=f, tally_ways=8)
    rng = np.random.default_rng(L * 100 + R)
    for name, (start, end, rnd) in batches(L).items():
        for delivery in ("dense", "masks", "nacks"):
            a, b = oracle.System(oracle.make_config(**kw)), oracle.System(oracle.make_config(**kw))
            n = len(start)
            tm = None
            if delivery == "masks":
                tm = RB.target_masks(n, A, R, f)
            if delivery == "nacks":
                for g in range(0, L * A, 2):
                    t = W.bits_from_bool(W.random_subsets(rng, 1, R, 1, max(1, R // 2)))[0]
                    for x in (a, b):
                        assert x.acceptor_phase1a(g, 7, 0, t)[0] == 0
            st, vb, nb, nr, new, ch = a.noop_ranges_fused(start, end, rnd, tm)
            assert st == 0
            for i in range(n):
                s, e, r = int(start[i]), int(end[i]), int(rnd[i])
                st1, fresh = b.proxy_open_noop_range(s, e, r)
                assert st1 == 0 and fresh == new[i], (name, i)
                if fresh:
                    st2, vb1, nb1, nr1 = b.acceptor_phase2a_noop_range(s, e, r, None if tm is None else tm[i])
                    np.testing.assert_array_equal(vb1, vb[i])
                    np.testing.assert_array_equal(nb1, nb[i])
                    assert nr1 == nr[i]
                    assert b.proxy_phase2b_noop_range(s, e, r, vb1) == (0, ch[i])
                else:
                    assert ch[i] == 0 and not vb[i].any() and not nb[i].any() and nr[i] == -1
            np.testing.assert_array_equal(a.state_digest(), b.state_digest())
            W.assert_same_state(a, b)
            if delivery == "dense":
                assert ch.sum() == new.sum() > 0
            if delivery == "masks":
                assert 0 < ch.sum() < new.sum(), name       # some acceptor groups stayed below quorum
            if delivery == "nacks":
                assert (nr == 7).any(), name


def test_oracle_ranges_on_a_replica_shard(oracle):
    """replica_base = 60, 8 of 72 replicas: the vote bits straddle a 64-bit word"""
    kw = dict(num_slots=64, num_replicas=8, num_leader_groups=2, f=3, replica_base=60, replicas_total=72)
    s = oracle.System(oracle.make_config(**kw))
    st, vb, nb, nr, new, ch = s.noop_ranges_fused([0], [10], [0])
    assert st == 0 and new[0] == 1 and [int(x) for x in vb[0, 0]] == [0xf000000000000000, 0xf, 0, 0]


def test_gpu_case_list_covers_every_form_and_fill_branch():
    """the case list of tests/test_gpu_range_matrix.py: every census form is some case's target, and so is
    every (fill form, quads per row Q = 1 / 2 / more, A == 1 / A > 1, overlap or none) -- every shape case runs the
    batches without a shared row (residue, aligned) and those with (overlap, straddle at small L)"""
    forms = {"open_only", "acceptors_only", "tally_only", "rehash"}      # test_shard, test_table_*
    forms |= {c[3] for c in M.CHAIN_CASES} | {c[1] for c in M.BAND_CASES}
    have = set()
    for _, (L, A, R, f), fills in M.shape_cases():
        q = min((R + 3) // 4, 3)
        for fill, overlap in itertools.product(fills, (False, True)):
            if fill == "fill_lg":
                assert R <= 32
            have.add((fill, q, A > 1, overlap))
            forms.add(fill)
    assert forms == set(M.FORMS), set(M.FORMS) - forms
    want = set(itertools.product(("fill_lg", "fill_sweep", "fill_range"), (1, 2, 3), (False, True), (False, True)))
    assert want <= have, sorted(want - have)
    for L in {g[0] for g in M.GEOMS}:
        b = M.shape_batches(L * M.ROWS, L, [0] * L)
        assert not RB.overlaps(*b["residue"][:2], L).any() and RB.overlaps(*b["overlap"][:2], L).any()
    assert any(not M.chain_admits(n, A, R) for n, A, R, _ in M.CHAIN_CASES)
    for n, A, R, form in M.CHAIN_CASES:
        assert M.chain_admits(n, A, R) == (form == "chain")
