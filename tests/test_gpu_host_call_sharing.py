"""The host-pointer entry points of an fpx_ctx carve every array of a call out of ONE staging buffer (host_call,
csrc/fpx_host.hpp): calls of different shapes follow each other on one context, so the buffer grows, is reused larger than
needed and is laid out differently by every call.  Each call here is checked the way its own parity test checks it --
against the oracle's System, driven message at a time where the oracle has no burst form (the helpers are those tests'),
or against the message-at-a-time model from the context's own state -- and at the end the whole state equals the oracle's.

Run on the MI355X box: python -m pytest tests -m gpu
"""
import numpy as np
import pytest

from frankenpaxos_amd import wire
from tests import acceptor_inbox_model as AM
from tests import acceptor_inbox_streams as AS
from tests import mencius_acceptor_inbox_streams as MAS
from tests import mencius_phase2b_streams as MPS
from tests import range_batches as RB
from tests import replica_streams as RPS
from tests import workloads as W
from tests.test_gpu_acceptor_inbox import call as acceptor_inbox_call
from tests.test_gpu_acceptor_inbox import one_by_one
from tests.test_gpu_mencius_acceptor_inbox import one_by_one as mencius_one_by_one
from tests.test_gpu_phase2b_msgs import rows_path
from tests.test_gpu_replica_inbox import run as replica_inbox_burst

pytestmark = pytest.mark.gpu
EINVAL = 1
SIZES = (1, 257, 3, 4095, 2)      # grows, is reused larger than needed, grows again, is reused
MULTIPAXOS = dict(num_slots=2048, num_replicas=5, f=2, ballot_mode=0, tally_ways=8)
MENCIUS = dict(num_slots=4096, num_replicas=3, num_groups=2, num_leader_groups=4, f=1, ballot_mode=0, tally_ways=8)


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


def both(fa, oracle, kw):
    return fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))


def same(tag, got, want):
    assert got[0] == want[0] == 0, (tag, got[0], want[0])
    W.assert_same_outputs([(tag,) + tuple(got)], [(tag,) + tuple(want)])


def subsets(rng, n, R):
    """a non-empty set of the R acceptors per message"""
    m = np.zeros((n, 4), np.uint64)
    m[:, 0] = rng.integers(1, 1 << R, n).astype(np.uint64)
    return m


def last_round(b):
    sel = np.isin(b.kind, (AM.P2A, AM.P1A))
    return int(b.round[sel].max()) if sel.any() else 0


def acceptor_burst(gpu, ref, b, with_group=True):
    st, rk, rv = gpu.acceptor_inbox(*b.arrays()[:5], b.group if with_group else None, b.grid_cols)
    assert st == 0, gpu.error_detail()
    want_kind, want_value = one_by_one(ref, b)
    np.testing.assert_array_equal(rk, want_kind)
    np.testing.assert_array_equal(rv, want_value)


def test_multipaxos_calls_of_five_sizes_interleaved_on_one_context(fa, oracle):
    gpu, ref = both(fa, oracle, MULTIPAXOS)
    S, R = MULTIPAXOS["num_slots"], MULTIPAXOS["num_replicas"]
    rng = np.random.default_rng(20261021)
    round0 = 1
    for k, n in enumerate(SIZES):
        odd = k % 2 == 1          # the optional inputs are there in every other pass: another layout again
        slot = rng.integers(0, S, n).astype(np.int32)             # (repeats: the host cuts these batches into runs)
        rnd = (round0 + (np.arange(n) >= (2 * n + 2) // 3)).astype(np.int32)
        val = (slot * 7 + rnd).astype(np.int32)
        tgt = subsets(rng, n, R) if odd else None
        votes = gpu.acceptor_phase2a(slot, rnd, val, tgt)
        same("phase2a", votes, ref.acceptor_phase2a(slot, rnd, val, tgt))
        same("open", gpu.proxy_open(slot, rnd, val), ref.proxy_open(slot, rnd, val))
        same("phase2b", gpu.proxy_phase2b(slot, rnd, votes[1]), ref.proxy_phase2b(slot, rnd, votes[1]))
        burst = AS.make(k + 1, n, R=R, S=S, round0=round0 + 2, up=min(0.02, 8.0 / n))
        acceptor_burst(gpu, ref, burst, with_group=odd)
        j = rng.integers(0, n, n)
        d = dict(kind=np.full(n, wire.PHASE2B, np.int32), group_index=np.zeros(n, np.int32),
                 acceptor_index=rng.integers(0, R, n).astype(np.int32), slot=slot[j].copy(), round=rnd[j].copy())
        same("phase2b_msgs", gpu.proxy_phase2b_msgs(d["acceptor_index"], d["slot"], d["round"], kind=d["kind"] if odd else None,
                                                    group_index=d["group_index"] if odd else None),
             rows_path(wire, ref, d, 0))
        u = rng.random(n)
        kind = np.where(u < 0.55, wire.CHOSEN, np.where(u < 0.7, wire.EVENTUAL_READ_REQUEST, wire.READ_REQUEST)).astype(np.int32)
        rslot = np.where(kind == wire.CHOSEN, rng.integers(0, S, n), rng.integers(-1, S + 8, n)).astype(np.int32)
        rvalue, rmask = (5000 + np.arange(n)).astype(np.int32), (rng.random(n) >= 0.05 if odd else np.ones(n, bool))
        replica_inbox_burst(gpu, kind, rslot, rvalue, rmask.astype(np.uint8) if odd else None)
        sel = (kind == wire.CHOSEN) & rmask                       # the oracle's replica sees the burst's Chosens one by one
        st, wm, nc = ref.replica_chosen(rslot[sel], rvalue[sel])
        assert st == 0 and (wm, nc) == gpu.replica_state()
        round1 = max(int(rnd.max()), last_round(burst)) + 1
        fslot = (rng.integers(0, S, n) if n > S else rng.permutation(S)[:n]).astype(np.int32)   # (4095 > S: a replay)
        frnd, fval = np.full(n, round1, np.int32), (fslot * 7 + round1).astype(np.int32)
        ftgt = None if odd else subsets(rng, n, R)
        same("fused", gpu.phase2_fused(fslot, frnd, fval, ftgt), ref.phase2_fused(fslot, frnd, fval, ftgt))
        round0 = round1 + 1
    W.assert_same_state(gpu, ref, tally_slots=range(0, S, 97))
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    gpu.close()


def test_mencius_calls_of_five_sizes_interleaved_on_one_context(fa, oracle):
    gpu, ref = both(fa, oracle, MENCIUS)
    S, R, A, L, f = (MENCIUS[k] for k in ("num_slots", "num_replicas", "num_groups", "num_leader_groups", "f"))
    rng = np.random.default_rng(20261022)
    round0, keys = 1, []
    for k, n in enumerate(SIZES):
        odd = k % 2 == 1
        # the ranges of a pass come from a pool of at most 100 (the range table holds 2048 live entries), so the batch
        # repeats keys; the last third is one round on: the host cuts the batch there (one round per leader group and run)
        pool = min(n, 100)
        row = rng.integers(0, S // L - 8, pool)
        pstart = (row * L + np.arange(pool) % L).astype(np.int32)
        pend = np.minimum(S, pstart + 1 + rng.integers(0, 5 * L, pool)).astype(np.int32)
        j = rng.integers(0, pool, n)
        start, end = pstart[j].copy(), pend[j].copy()
        rnd = (round0 + (np.arange(n) >= (2 * n + 2) // 3)).astype(np.int32)
        tgt = RB.target_masks(n, A, R, f) if odd else None
        same("ranges", gpu.noop_ranges_fused(start, end, rnd, tgt), ref.noop_ranges_fused(start, end, rnd, tgt))
        keys += list(zip(start.tolist(), end.tolist(), rnd.tolist()))[:: max(1, n // 16)]
        burst = MAS.make(k + 1, n, L=L, A=A, R=R, S=S, round0=round0 + 2, up=min(0.02, 8.0 / n))
        st, rk, rv = gpu.mencius_acceptor_inbox(*burst.arrays())
        assert st == 0, gpu.error_detail()
        want_kind, want_value = mencius_one_by_one(ref, burst)
        np.testing.assert_array_equal(rk, want_kind)
        np.testing.assert_array_equal(rv, want_value)
        # Phase2bNoopRanges for the ranges of this pass, one acceptor each, some of them after the range is Done
        j = rng.integers(0, n, n)
        d = dict(kind=np.full(n, wire.PHASE2B_NOOP_RANGE, np.int32), group_index=rng.integers(0, A, n).astype(np.int32),
                 acceptor_index=rng.integers(0, R, n).astype(np.int32), slot=start[j].copy(), slot_end=end[j].copy(),
                 round=rnd[j].copy())
        same("mencius_phase2b_msgs", gpu.mencius_proxy_phase2b_msgs(d["acceptor_index"], d["slot"], d["round"], kind=d["kind"],
                                                                    group_index=d["group_index"], slot_end=d["slot_end"]),
             MPS.rows_path(ref, d, MENCIUS))
        msgs = []
        for _ in range(n):
            u, mask = rng.random(), 0 if rng.random() < 0.10 else 1
            if u < 0.5:
                msgs.append(RPS.C(int(rng.integers(0, S)), int(rng.integers(0, 1 << 30)), mask))
            elif u < 0.9:
                s0 = int(rng.integers(0, S))
                msgs.append(RPS.R(s0, min(S, s0 + int(rng.integers(0, 12)) * L), mask))
            else:
                msgs.append((wire.PHASE2B, int(rng.integers(0, S)), 0, 7, mask))
        chosen = RPS.burst_of(msgs)
        st, wm, nc = gpu.replica_chosen_msgs(*chosen[:4], chosen[4] if odd or not chosen[4].all() else None)
        scalars, (vals, pres), _ = RPS.oracle_burst(ref, chosen, S, L)
        assert st == 0 and (wm, nc) == scalars
        got_vals, got_pres = gpu.replica_read_log(0, S)
        np.testing.assert_array_equal(got_pres, pres)
        np.testing.assert_array_equal(got_vals[pres != 0], vals[pres != 0])
        sel = np.isin(burst.kind, (wire.PHASE2A, wire.PHASE2A_NOOP_RANGE, wire.PHASE1A))
        round0 = max(int(rnd.max()), int(burst.round[sel].max()) if sel.any() else 0) + 1
    W.assert_same_state(gpu, ref)
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    for key in keys:
        got, want = gpu.read_range_tally(*key), ref.read_range_tally(*key)
        assert got[0] == want[0], key
        np.testing.assert_array_equal(got[1], want[1], err_msg=str(key))
    gpu.close()


def test_the_fused_step_replays_from_staging_behind_a_larger_call(fa, oracle):
    """n = 300 on pageable arrays, one slot twice with rising rounds: the device answers FPX_EORDER to the one validated
    run and the host replays its cuts from the inputs it staged once -- in a buffer that a 4095-message inbox burst
    left larger and laid out otherwise.  Equal to message-at-a-time delivery in the oracle."""
    gpu, ref = both(fa, oracle, MULTIPAXOS)
    S, R = MULTIPAXOS["num_slots"], MULTIPAXOS["num_replicas"]
    burst = AS.make(7, 4095, R=R, S=S, up=8.0 / 4095)
    acceptor_burst(gpu, ref, burst)
    n, rnd0 = 300, last_round(burst) + 1
    slot = np.random.default_rng(5).permutation(S)[:n].astype(np.int32)
    slot[n - 1] = slot[10]
    rnd = np.full(n, rnd0, np.int32)
    rnd[n - 1] = rnd0 + 1
    val = (slot * 7 + rnd).astype(np.int32)
    got = gpu.phase2_fused(slot, rnd, val)
    same("fused", got, ref.phase2_fused(slot, rnd, val))
    assert got[1][10] and got[1][n - 1] and got[2][n - 1] == rnd0 + 1      # chosen in both rounds, in array order
    W.assert_same_state(gpu, ref, tally_slots=[int(slot[10]), int(slot[0])])
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    gpu.close()


def test_a_refused_burst_leaves_the_replies_alone_behind_a_larger_call(fa):
    """one bad message: the held replies stay in the context's host buffer, the caller's arrays keep their sentinel (-9,
    written by Context.acceptor_inbox); status and fpx_error_detail are the device form's, which stages nothing"""
    big, good = AS.make(3, 3000, R=5, S=2048), AS.make(4, 600, R=5, S=2048)
    gpu = fa.Context(fa.make_config(**MULTIPAXOS))
    st, rk, rv = acceptor_inbox_call(gpu, big, False)
    assert st == 0 and (rk != -9).all()
    before = gpu.state_digest()
    what, bad, at = AS.spoiled(good)[0]
    st_dev, _, _ = acceptor_inbox_call(gpu, bad, True)
    detail_dev = gpu.error_detail()
    st, rk, rv = acceptor_inbox_call(gpu, bad, False)
    assert st == st_dev == EINVAL and gpu.error_detail() == detail_dev and detail_dev[0] == at, (what, st, gpu.error_detail())
    assert (rk == -9).all() and (rv == -9).all(), what
    np.testing.assert_array_equal(gpu.state_digest(), before)
    st, rk, rv = acceptor_inbox_call(gpu, good, False)                         # and the next call is served
    assert st == 0 and (rk != -9).all()
    gpu.close()
