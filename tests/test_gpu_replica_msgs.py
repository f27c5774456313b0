"""fpx_replica_chosen_msgs / _dev (include/fpx.h): a burst of a Mencius replica's inbox, Chosens and ChosenNoopRanges
interleaved, ingested in one device call -- against the oracle handling the same messages ONE BY ONE
(replica_chosen([slot], [value]) / replica_chosen_noop_range(start, end)): the status, (executed_watermark,
num_chosen) and the whole log after every burst, equal.  The pinned cases also spell their expected log out by hand.
The streams are tests/replica_streams.py.

Run on the MI355X box: python -m pytest tests -m gpu
"""
import ctypes as C

import numpy as np
import pytest

from tests import replica_streams as RS
from tests.replica_streams import C as Ch, R as Rg
from tests.test_jni_shim import jvm  # noqa: F401  (the mock JVM fixture)

pytestmark = pytest.mark.gpu
EINVAL = 1
S0, L0 = 4096, 4


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


def pair(fa, oracle, S=S0, L=L0, **more):
    kw = dict(num_slots=S, num_replicas=3, num_leader_groups=L, f=1, **more)
    return fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))


def same_log(gpu, want_vals, want_pres):
    vals, pres = gpu.replica_read_log(0, gpu.S)
    np.testing.assert_array_equal(pres, want_pres)
    np.testing.assert_array_equal(vals, want_vals)


def run(gpu, ref, msgs, dev=False):
    """one burst on both sides; returns (executed_watermark, num_chosen) and the oracle's figures"""
    burst = RS.burst_of(msgs) if isinstance(msgs, list) else msgs
    S, L = gpu.S, gpu.cfg.num_leader_groups
    want, (vals, pres), stats = RS.oracle_burst(ref, burst, S, L)
    if dev:
        import torch

        d = [torch.from_numpy(a).cuda() for a in burst]
        gpu.replica_chosen_msgs_dev(*d)
        assert gpu.sync() == 0
        got = gpu.replica_state()
    else:
        st, wm, nc = gpu.replica_chosen_msgs(*burst)
        assert st == 0
        got = (wm, nc)
        assert got == gpu.replica_state()
    assert got == want
    same_log(gpu, vals, pres)
    return got, stats


def by_hand(S, log):
    vals, pres = np.full(S, -1, np.int32), np.zeros(S, np.uint8)
    for s, v in log.items():
        vals[s], pres[s] = v, 1
    return vals, pres


# ---------------------------------------------------------------------------------------------------------------------
# pinned cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True])
def test_chosens_only(fa, oracle, dev):
    gpu, ref = pair(fa, oracle)
    assert run(gpu, ref, [Ch(7, 70)], dev)[0] == (0, 1)
    got, _ = run(gpu, ref, [Ch(5, 50), Ch(5, 51),                   # the same slot twice: the lower index wins
                            Ch(7, 71),                              # present before the burst
                            Ch(0, 10, mask=0),                      # masked out
                            (RS.PHASE2B, 1, 0, 13, 1),              # another kind in the middle
                            Ch(1, 11), Ch(0, 12)], dev)
    assert got == (2, 4)
    same_log(gpu, *by_hand(S0, {7: 70, 5: 50, 1: 11, 0: 12}))
    gpu.close()


def test_one_range_on_a_fresh_log_equals_the_single_range_entry_point(fa, oracle):
    gpu, ref = pair(fa, oracle)
    twin = fa.Context(gpu.cfg)
    log = {}
    for start, end, wm in ((2, 41, 0),       # the end is not on the stride: 2, 6, ... 38
                           (8, 8, 0),        # empty
                           (0, 4, 1)):       # slot 0: the prefix executes
        got, _ = run(gpu, ref, [Rg(start, end)])
        st, twm, tnc = twin.replica_chosen_noop_range(start, end)
        log.update({s: -1 for s in range(start, end, L0)})
        assert st == 0 and got == (twm, tnc) == (wm, len(log))
        same_log(gpu, *twin.replica_read_log(0, S0))
        same_log(gpu, *by_hand(S0, log))
    gpu.close(), twin.close()


TRUNCATION = [Ch(49, 490),        # 0
              Rg(0, 40),          # 1  class 0: 0 4 8 12 16, cut by slot 20, present before the burst
              Rg(41, 61),         # 2  class 1: 41 45, cut by slot 49, put by message 0
              Rg(2, 18),          # 3  class 2: 2 6 10 14, runs to its end although message 4 wants slot 10
              Ch(10, 100)]        # 4  redundant: slot 10 holds Noop
TRUNCATION_LOG = {20: 200, 49: 490, 0: -1, 4: -1, 8: -1, 12: -1, 16: -1, 41: -1, 45: -1, 2: -1, 6: -1, 10: -1, 14: -1}


@pytest.mark.parametrize("dev", [False, True])
def test_truncation_by_old_slots_and_earlier_messages_only(fa, oracle, dev):
    gpu, ref = pair(fa, oracle)
    run(gpu, ref, [Ch(20, 200)], dev)
    got, stats = run(gpu, ref, TRUNCATION, dev)
    assert got == (1, 13) and stats["truncated"] == 2 and stats["own"] == 1 and stats["redundant"] == 1
    same_log(gpu, *by_hand(S0, TRUNCATION_LOG))
    gpu.close()


def test_chains_in_one_residue_class(fa, oracle):
    gpu, ref = pair(fa, oracle)
    run(gpu, ref, [Ch(12, 120)])
    got, stats = run(gpu, ref, [Rg(0, 40),       # A: 0 4 8, stopped at position 3 by the old slot 12
                                Rg(16, 40),      # B: starts beyond it and fills what A dropped: 16 ... 36
                                Rg(0, 40),       # A again: stopped at position 0
                                Rg(1, 41)])      # another class over the same interval: 1 5 ... 37, unaffected
    log = {12: 120}
    log.update({s: -1 for s in (0, 4, 8)})
    log.update({s: -1 for s in range(16, 40, 4)})
    log.update({s: -1 for s in range(1, 41, 4)})
    assert got == (2, 20) and stats["truncated"] == 2 and stats["full"] == 2
    same_log(gpu, *by_hand(S0, log))
    gpu.close()


@pytest.mark.parametrize("catch_up", ["empty range", "chosen"])
def test_the_lagging_watermark(fa, oracle, catch_up):
    gpu, ref = pair(fa, oracle)
    assert run(gpu, ref, [Ch(0, 1), Ch(1, 2), Ch(2, 3), Ch(11, 9), Ch(12, 8)])[0] == (3, 5)
    # the burst ends with a truncated range whose Noop at slot 3 extends the prefix: counted, not executed
    assert run(gpu, ref, [Ch(2, 5), Rg(3, 15)])[0] == (3, 7)
    vals, pres = gpu.replica_read_log(0, 16)
    assert pres.tolist() == [1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0] and vals[3] == vals[7] == -1
    assert run(gpu, ref, [])[0] == (3, 7)                           # an empty burst
    assert run(gpu, ref, [Ch(1, 99), Ch(3, 98)])[0] == (3, 7)       # only redundant Chosens
    assert run(gpu, ref, [Rg(4, 16)])[0] == (3, 9)                  # only another truncated range: 4 8, cut by 12
    if catch_up == "empty range":
        assert run(gpu, ref, [Rg(9, 9)])[0] == (5, 9)
    else:
        assert run(gpu, ref, [Ch(5, 55)])[0] == (6, 10)
    gpu.close()


def test_loops_that_iterate_one_long_range(fa, oracle):
    S, L = 1 << 16, 3
    gpu, ref = pair(fa, oracle, S, L)
    cut = 1 + 3 * 19990
    got, stats = run(gpu, ref, [Ch(cut, 5), Rg(1, 1 + 3 * 20000), Ch(0, 6)])
    assert got == (2, 19992) and stats["truncated"] == 1 and stats["own"] == 1
    gpu.close()


def test_loops_that_iterate_every_class_and_many_chosens(fa, oracle):
    S, L = 1 << 16, 256
    gpu, ref = pair(fa, oracle, S, L)
    rng = np.random.default_rng(5)
    msgs = [Ch(int(s), int(v)) for s, v in zip(rng.integers(0, S, 1 << 15), rng.integers(0, 1 << 30, 1 << 15))]
    for c in range(L):
        msgs.insert(int(rng.integers(0, len(msgs) + 1)), Rg(c + L * (c % 7), S - L * (c % 5)))
    got, stats = run(gpu, ref, msgs, dev=True)
    assert stats["truncated"] + stats["full"] == L and stats["truncated"] > 100 and stats["redundant"] > 1000
    # the same messages backwards: every Chosen is redundant and every range is cut where it was, or at once -- no message
    # reaches executeLog
    got2, stats = run(gpu, ref, msgs[::-1])
    assert got2 == got and stats["full"] == 0
    gpu.close()


def test_ranges_listed_from_offsets_that_went_through_the_carry(fa, oracle):
    """n = 1024 * 256 + 3 * 256 + 57 messages are 1028 workgroups of k_rm_claim: k_rm_offsets (scan_array_excl of
    fpx_scan.hpp, 1024 counts a step) takes two steps, and the ranges behind message 1024 * 256 get their list places from
    offsets that carry the first step's total.  Those are the ranges of classes 0 .. 15; the Chosens of their classes keep
    to rows 200 and up, so every one of them still finds its first slot free and puts a run of Noops"""
    S, L, tail = 1 << 16, 256, 16
    n, first_step = 1024 * 256 + 3 * 256 + 57, 1024 * 256
    gpu, ref = pair(fa, oracle, S, L)
    rng = np.random.default_rng(6)
    slots = rng.integers(0, S, n - L)
    low = (slots % L < tail) & (slots // L < 200)                    # rows 0 .. 199 of those classes -> 200 .. 255
    slots[low] = slots[low] % L + L * (200 + (slots[low] // L) % 56)
    msgs = [Ch(int(s), int(v)) for s, v in zip(slots, rng.integers(0, 1 << 30, n - L))]
    ranges = {c: Rg(c + L * (c % 7), S - L * (c % 5)) for c in range(L)}
    for c in range(tail, L):
        msgs.insert(int(rng.integers(0, len(msgs) + 1)), ranges[c])
    for c in range(tail):
        msgs.insert(int(rng.integers(first_step + 8, len(msgs) + 1)), ranges[c])
    assert len(msgs) == n
    behind = [m for m in msgs[first_step:] if m[0] == RS.CHOSEN_NOOP_RANGE and m[1] % L < tail]
    assert len(behind) == tail
    got, stats = run(gpu, ref, msgs, dev=True)
    assert stats["truncated"] + stats["full"] == L and stats["redundant"] > 1000
    vals, pres = gpu.replica_read_log(0, S)
    for m in behind:                                                # (run() has compared the whole log with the oracle's)
        assert pres[m[1]] and vals[m[1]] == RS.NOOP and pres[m[1] + L] and vals[m[1] + L] == RS.NOOP
    gpu.close()


def test_refusal(fa, oracle):
    import torch

    gpu, ref = pair(fa, oracle)
    run(gpu, ref, [Ch(3, 30), Rg(0, 8)])
    vals, pres = gpu.replica_read_log(0, S0)
    scalars = gpu.replica_state()
    msgs = [Ch(40, 1), Rg(1, 30), Ch(41, 2), Rg(3, 40), Ch(42, 3), Ch(S0, 4), Rg(2, 50), Ch(5, 6), Rg(60, 60), Rg(8, S0 + 1),
            Ch(44, 7), Rg(0, 100)]
    st, wm, nc = gpu.replica_chosen_msgs(*RS.burst_of(msgs))
    assert st == EINVAL and gpu.error_detail()[0] == 5 and (wm, nc) == scalars == gpu.replica_state()
    same_log(gpu, vals, pres)
    # the _dev form: FPX_EINVAL at fpx_sync, lowest index first; a negative start
    d = [torch.from_numpy(a).cuda() for a in RS.burst_of(msgs[:3] + [Rg(-4, 8)] + msgs[4:])]
    gpu.replica_chosen_msgs_dev(*d)
    assert gpu.sync() == EINVAL and gpu.error_detail()[0] == 3 and gpu.replica_state() == scalars
    same_log(gpu, vals, pres)
    # masked out, the bad messages do not count
    bad_masked = [m[:4] + (0,) if i in (5, 9) else m for i, m in enumerate(msgs)]
    twin, tref = pair(fa, oracle)
    run(twin, tref, [Ch(3, 30), Rg(0, 8)])
    run(twin, tref, bad_masked)
    # the same burst without the two: equals the oracle -- the claim table was left clean
    good = [m for i, m in enumerate(msgs) if i not in (5, 9)]
    got, _ = run(gpu, ref, good)
    assert got == twin.replica_state()
    same_log(gpu, *twin.replica_read_log(0, S0))
    # refused at once: NULL arrays with n > 0; n = 0 changes nothing
    lib, h, p = fa.lib(), gpu._h, d[0].data_ptr()
    for k in range(4):
        args = [None if j == k else p for j in range(4)]
        assert lib.fpx_replica_chosen_msgs_dev(h, 4, *args, None) == EINVAL
        assert lib.fpx_replica_chosen_msgs(h, 4, *[None if a is None else vals.ctypes.data for a in args], None, None, None) == EINVAL
    assert lib.fpx_replica_chosen_msgs_dev(h, -1, p, p, p, p, None) == EINVAL
    assert lib.fpx_replica_chosen_msgs_dev(h, 0, None, None, None, None, None) == 0
    assert gpu.sync() == 0 and gpu.replica_state() == got
    assert gpu.replica_chosen_msgs([], [], [], []) == (0,) + got
    gpu.close(), twin.close()


def test_the_claim_table_is_counted_and_kept(fa, oracle):
    gpu, ref = pair(fa, oracle)
    before = gpu.device_bytes
    run(gpu, ref, [Ch(1, 1)])
    after = gpu.device_bytes
    assert after - before == 4 * S0
    run(gpu, ref, [Rg(0, 64)])
    assert gpu.device_bytes == after
    gpu.close()


def test_band_to_log_on_the_device(fa, oracle):
    """fpx_mencius_band_fused_dev's outputs, laid out as include/fpx.h describes, go straight into
    fpx_replica_chosen_msgs_dev on the same stream: no copy, no host step in between"""
    import torch

    from tests import range_batches as RB

    L, rows, R = 4, 40, 3
    kw = dict(num_slots=S0, num_replicas=R, num_leader_groups=L, f=1, ballot_mode=fa.FPX_BALLOT_ACCEPTOR)
    gpu, ref = fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    # leader groups 0 and 1 propose in their slots of rows 0 .. 39, groups 2 and 3 skip theirs (two ranges each)
    slot = (np.arange(rows)[:, None] * L + np.arange(2)[None, :]).reshape(-1).astype(np.int32)
    value = (np.arange(len(slot)) + 100).astype(np.int32)
    start, end = (np.array(x, np.int32) for x in zip(RB.row_range(L, 2, 0, 19, extra=1), RB.row_range(L, 3, 0, 29),
                                                     RB.row_range(L, 2, 20, 39), RB.row_range(L, 3, 30, 39)))
    n, k = len(slot), len(start)
    tm = RB.target_masks(k, 1, R, 1)                                # every third range stays below quorum: not chosen
    dev = torch.device("cuda:0")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    zeros = lambda m, t: torch.zeros(m, dtype=t, device=dev)
    d_slots = d(np.concatenate([slot, start]))                      # d_slot | d_slot_start
    d_flags = zeros(n + k, torch.uint8)                             # d_chosen | d_range_chosen
    d_values = torch.full((n + k,), -1, dtype=torch.int32, device=dev)   # d_chosen_value + k spare words
    d_kind = d(np.array([RS.CHOSEN] * n + [RS.CHOSEN_NOOP_RANGE] * k, np.int32))
    d_ends = d(np.concatenate([np.zeros(n, np.int32), end]))
    rr, rnd = d(np.zeros(n, np.int32)), d(np.zeros(k, np.int32))
    gpu.mencius_band_fused_dev(d_slots[:n], rr, d(value), None, d_flags[:n], zeros(n, torch.int32), d_values[:n],
                               zeros(n, torch.int32), d_slots[n:], d_ends[n:], rnd, d(tm.view(np.int64)),
                               torch.zeros((k, 1, 4), dtype=torch.int64, device=dev),
                               torch.zeros((k, 1, 4), dtype=torch.int64, device=dev), zeros(k, torch.int32),
                               zeros(k, torch.uint8), d_flags[n:], independent=False)
    gpu.replica_chosen_msgs_dev(d_kind, d_slots, d_ends, d_values, d_flags)
    assert gpu.sync() == 0
    b1 = ref.phase2_fused(slot, np.zeros(n, np.int32), value, None)
    b2 = ref.noop_ranges_fused(start, end, np.zeros(k, np.int32), tm)
    assert b1[0] == b2[0] == 0 and b1[1].all() and 0 < b2[5].sum() < k
    np.testing.assert_array_equal(d_flags.cpu().numpy(), np.concatenate([b1[1], b2[5]]).astype(np.uint8))
    for s, v in zip(slot[b1[1].astype(bool)], b1[3][b1[1].astype(bool)]):
        ref.replica_chosen([int(s)], [int(v)])
    for s, e in zip(start[b2[5].astype(bool)], end[b2[5].astype(bool)]):
        ref.replica_chosen_noop_range(int(s), int(e))
    assert gpu.replica_state() == ref.replica_chosen([], [])[1:] and gpu.replica_state()[1] > n
    same_log(gpu, *ref.replica_read_log(0, S0))
    gpu.close()


def test_the_jni_native_on_the_mock_jvm(fa, oracle, jvm):  # noqa: F811
    cfg = np.array([S0, 3, 1, L0, 1, 0, 0, 0, 2, 0, 4, 0, 0, 0, 0], np.int32)   # the 15 fpx_config fields
    h = jvm.call("create", C.c_int64, jvm.arr(cfg))
    assert h > 0
    ref = oracle.System(oracle.make_config(num_slots=S0, num_replicas=3, num_leader_groups=L0, f=1))
    state = jvm.arr(np.zeros(2, np.int32))

    def native(msgs, short=None):
        k, s, e, v, m = RS.burst_of(msgs)
        arrs = [k, s, e, v, m.view(np.int8)]
        if short is not None:
            arrs[short] = arrs[short][:-1]
        return jvm.call("replicaChosenMsgs", C.c_int32, h, len(msgs), *[jvm.arr(a) for a in arrs], state)

    for msgs in ([Ch(20, 200)], TRUNCATION):
        want, (vals, pres), _ = RS.oracle_burst(ref, RS.burst_of(msgs), S0, L0)
        assert native(msgs) == 0 and tuple(jvm.read(state, np.int32, 2)) == want
    got_v, got_p = np.zeros(S0, np.int32), np.zeros(S0, np.uint8)
    assert fa.lib().fpx_replica_read_log(C.c_void_p(h), 0, S0, got_v.ctypes.data, got_p.ctypes.data) == 0
    np.testing.assert_array_equal(got_v, vals)
    np.testing.assert_array_equal(got_p, pres)
    np.testing.assert_array_equal(got_v, by_hand(S0, TRUNCATION_LOG)[0])
    for short in range(5):                                          # a short array is refused before native code runs
        assert native([Ch(100, 1), Rg(101, 140)], short) == EINVAL
    assert native([Ch(100, 1)]) == 0 and tuple(jvm.read(state, np.int32, 2)) == (1, 14)
    assert jvm.call("destroy", C.c_int32, h) == 0


# ---------------------------------------------------------------------------------------------------------------------
# random streams
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", RS.SEEDS)
@pytest.mark.parametrize("L,S", RS.SHAPES)
def test_random_streams_equal_the_oracle_after_every_burst(fa, oracle, L, S, seed):
    gpu, ref = pair(fa, oracle, S, L)
    total = dict(truncated=0, full=0, redundant=0, own=0, lag=0)
    for b, burst in enumerate(RS.stream(L, S, seed)):
        got, stats = run(gpu, ref, burst, dev=b % 2 == 1)
        for k in total:
            total[k] += stats[k]
    RS.assert_not_vacuous(total, got)
    gpu.close()
