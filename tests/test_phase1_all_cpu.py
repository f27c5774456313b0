"""The batched Phase1b.info (fpx_acceptor_phase1b_info_all: every selected acceptor's votes from the watermark on, the
entries' runs back to back) restated in numpy on the arrays read_state() returns, and pinned on the oracle's
per-acceptor acceptor_phase1b_info entry by entry.  tests/test_gpu_phase1_all.py holds the device pass to this
restatement as well as to the oracle and to the single-acceptor path; it shares no code with the kernels.

The file also keeps the list of GPU cases and asserts that the list reaches every lanes-per-slot width and both row
layouts.
"""
import numpy as np
import pytest

from tests import workloads as W
from tests.test_gpu_phase1_readpath import lanes, pack_bits

# ---- the cases tests/test_gpu_phase1_all.py runs ------------------------------------------------------------------
WIDTH_RS = (3, 5, 13, 17, 61, 65, 253, 4, 256)       # one R per width with a partial last quad, plus 4 and 256
ROW_LAYOUTS = ("leader-group-major", "slot-major")   # the params of conftest's row_layout fixture
GEOMETRIES = {
    "groups4": dict(num_replicas=4, num_groups=4, quorum_kind=2, grid_rows=2, grid_cols=2),
    "mencius4x2": dict(num_replicas=3, f=1, num_groups=2, num_leader_groups=4),   # both layouts (row_layout)
}
P1I_TILE, P1I_CHUNK = 64, 4                          # fpx_phase1_info.hpp


def group_of(s, L, A):
    s = np.asarray(s)
    return (s % L) * A + (s // L) % A


def selection(masks, ng, R, base=0):
    """uint64 [ng, 4] mask words -> bool [ng, R]: bit base + r of group g's words (None = all)"""
    if masks is None:
        return np.ones((ng, R), bool)
    bits = W.bool_from_bits(np.asarray(masks, np.uint64).reshape(ng, 4), 256)
    return bits[:, base:base + R]


def info_all(vr, vv, L, A, wm, sel=None):
    """(offsets, slot, vote_round, vote_value): per entry e = g * R + r, the ascending slots >= max(wm, 0) of group g in
    which acceptor r holds a vote; unselected entries are empty"""
    S, R = vr.shape
    ng = L * A
    s = np.arange(S)
    grp = group_of(s, L, A)
    off, sl = [0], []
    for g in range(ng):
        rows = s[(grp == g) & (s >= max(wm, 0))]
        for r in range(R):
            hit = rows[vr[rows, r] != -1] if (sel is None or sel[g, r]) else rows[:0]
            sl.append(hit)
            off.append(off[-1] + len(hit))
    sl = np.concatenate(sl) if sl else np.zeros(0, np.int64)
    ent = np.repeat(np.arange(ng * R), np.diff(off))
    return (np.asarray(off, np.int64), sl.astype(np.int32), vr[sl, ent % R].astype(np.int32),
            vv[sl, ent % R].astype(np.int32))


def small_script(S, R, L, A, seed):
    if L == 1:
        return W.adversarial_script(S // 2, R, R // 2 + 1, seed, epochs=8, fused=True, ngroups=A)
    rng, ops = np.random.default_rng(seed), []
    for rnd in (0, 1):
        slot = rng.permutation(S)[: S // 2].astype(np.int32)
        tgt = W.bits_from_bool(W.random_subsets(rng, len(slot), R, 1, R))
        ops.append(("fused", slot, np.full(len(slot), rnd, np.int32), W.steady_values(slot), tgt))
    return ops


@pytest.mark.parametrize("R,kw", [(3, dict(f=1)), (5, dict(quorum_kind=1, ballot_mode=1)),
                                  (4, dict(num_groups=4, quorum_kind=2, grid_rows=2, grid_cols=2)),
                                  (3, dict(f=1, num_groups=2, num_leader_groups=4))])
def test_numpy_info_all_matches_oracle_entry_by_entry(oracle, R, kw):
    S = 1024
    L, A = kw.get("num_leader_groups", 1), kw.get("num_groups", 1)
    ng = L * A
    ref = oracle.System(oracle.make_config(num_slots=S, num_replicas=R, tally_ways=8, **kw))
    W.run_script(ref, small_script(S, R, L, A, 11 + R + L))
    vr, vv, _ = ref.read_state()
    rng = np.random.default_rng(R)
    subset = rng.random((ng, R)) < 0.5
    subset[0, 0] = True
    total0 = 0
    for wm in (-3, 0, 17, 64 * ng, S // 2 - 1, S - 1, S, S + 5):
        for sel in (None, subset):
            off, sl, r_, v_ = info_all(vr, vv, L, A, wm, sel)
            assert len(off) == ng * R + 1 and off[0] == 0 and off[-1] == len(sl) == len(r_) == len(v_)
            for g in range(ng):
                for r in range(R):
                    e = g * R + r
                    got = (sl[off[e]:off[e + 1]], r_[off[e]:off[e + 1]], v_[off[e]:off[e + 1]])
                    want = ref.acceptor_phase1b_info(g, r, wm) if (sel is None or sel[g, r]) else (np.zeros(0, np.int32),) * 3
                    for x, y in zip(got, want):
                        np.testing.assert_array_equal(x, y, err_msg="entry (%d, %d) from %d" % (g, r, wm))
            if wm == 0 and sel is None:
                total0 = int(off[-1])
    assert total0 > S // 8                                  # the scripts leave something to report
    assert info_all(vr, vv, L, A, S, None)[0][-1] == 0


def test_selection_follows_the_target_mask_bits():
    m = np.zeros((2, 4), np.uint64)
    m[0, 0] = np.uint64(0b101)
    m[1, 1] = np.uint64(1) << np.uint64(3)                  # bit 67
    sel = selection(m, 2, 5)
    assert sel.tolist() == [[True, False, True, False, False], [False] * 5]
    assert selection(m, 2, 4, base=64)[1].tolist() == [False, False, False, True]   # replica_base 64: bit 64 + r
    assert selection(None, 2, 3).all()
    np.testing.assert_array_equal(pack_bits(sel)[:, 0], m[:, 0])


def test_gpu_case_list_reaches_every_width_and_both_layouts():
    assert {lanes(R) for R in WIDTH_RS} == {1, 2, 4, 8, 16, 32, 64}
    for G in (1, 2, 4, 8, 16, 32, 64):
        assert any(lanes(R) == G and R % 4 for R in WIDTH_RS)         # each width with a partial last quad
    assert 4 in WIDTH_RS and 256 in WIDTH_RS
    # leader-group-major rows exist for Mencius contexts of at most 32 acceptors whose window is a whole number of rounds
    # over the leader groups (make_geom); the Mencius geometry runs under the row_layout fixture = both layouts
    m = GEOMETRIES["mencius4x2"]
    assert m["num_leader_groups"] > 1 and m["num_replicas"] <= 32 and 4096 % m["num_leader_groups"] == 0
    assert set(ROW_LAYOUTS) == {"leader-group-major", "slot-major"}
    assert GEOMETRIES["groups4"]["num_groups"] == 4 and GEOMETRIES["groups4"].get("num_leader_groups", 1) == 1
