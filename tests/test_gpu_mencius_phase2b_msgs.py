"""fpx_mencius_proxy_phase2b_msgs / _dev and fpx_mencius_phase2b_tick (include/fpx.h): a burst of per-acceptor Phase2b and
Phase2bNoopRange messages tallied on the device without a host fold -- against the rows path (the burst folded into rows in
Python, then proxy_phase2b / proxy_phase2b_noop_ranges: flags on the oracle, state on a second context), against
fpx_proxy_phase2b_msgs_dev for the Phase2b half, and against oracle/mencius_maps.py message at a time (the same keys
chosen, each once, the same Pending / Done entries).  The streams are tests/mencius_phase2b_streams.py.

Run on the MI355X box: python -m pytest tests -m gpu
"""
import ctypes as C

import numpy as np
import pytest

from tests import mencius_phase2b_streams as MS
from tests.test_jni_shim import jvm  # noqa: F401  (the mock JVM fixture)

pytestmark = pytest.mark.gpu
EINVAL, EUNKNOWN, ECAPACITY = 1, 2, 5
FIELDS = ("kind", "group_index", "acceptor_index", "slot", "slot_end", "round")


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()
    return frankenpaxos_amd


@pytest.fixture(scope="module")
def models():
    from oracle import mencius_maps, pyoracle

    pyoracle.build()
    return pyoracle, mencius_maps


def context(fa, kw):
    import torch

    gpu = fa.Context(fa.make_config(**kw))
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)  # the uploads below are torch's
    return gpu


def dev_call(gpu, d, with_kind=True, with_end=True, with_group=True):
    """fpx_mencius_proxy_phase2b_msgs_dev + fpx_sync: (status, newly_chosen, chosen_round, chosen_value)"""
    import torch

    dev = torch.device("cuda:0")
    n = len(d["slot"])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    ch = torch.full((max(n, 1),), 77, dtype=torch.uint8, device=dev)[:n]
    cr = torch.full((max(n, 1),), 77, dtype=torch.int32, device=dev)[:n]
    cv = torch.full((max(n, 1),), 77, dtype=torch.int32, device=dev)[:n]
    gpu.mencius_proxy_phase2b_msgs_dev(t["acceptor_index"], t["slot"], t["round"], kind=t["kind"] if with_kind else None,
                                       group_index=t["group_index"] if with_group else None,
                                       slot_end=t["slot_end"] if with_end else None, newly_chosen=ch, chosen_round=cr,
                                       chosen_value=cv)
    st = gpu.sync()
    return st, ch.cpu().numpy(), cr.cpu().numpy(), cv.cpu().numpy()


def phase2b_msgs_dev(gpu, d):
    """the MultiPaxos call on the same arrays (it skips the range messages): (status, flags, rounds, values)"""
    import torch

    dev = torch.device("cuda:0")
    n = len(d["slot"])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    ch = torch.zeros(n, dtype=torch.uint8, device=dev)
    cr = torch.zeros(n, dtype=torch.int32, device=dev)
    cv = torch.zeros(n, dtype=torch.int32, device=dev)
    gpu.proxy_phase2b_msgs_dev(t["acceptor_index"], t["slot"], t["round"], kind=t["kind"], newly_chosen=ch, chosen_round=cr,
                               chosen_value=cv)
    st = gpu.sync()
    return st, ch.cpu().numpy(), cr.cpu().numpy(), cv.cpu().numpy()


def same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def check_against_the_models(gpu, st, got, mencius_maps):
    """the keys chosen and every opened key's Pending / Done state equal oracle/mencius_maps.py message at a time"""
    chosen, _, states = MS.maps_run(mencius_maps, st)
    assert sorted(got) == sorted(chosen) and len(set(got)) == len(got)
    for k in st.range_keys():
        if k not in st.swallowed:
            assert gpu.read_range_tally(*k)[0] == states[k], k
    for s in sorted(set(st.single_slot.tolist())):
        for rnd, state, value, bits in gpu.read_tally(s):
            if (s, rnd) not in st.shadowed:
                assert states[(s, s + 1, rnd)] - 1 == state, (s, rnd)   # read_tally: 0 Pending, 1 Done


@pytest.mark.parametrize("layout", MS.LAYOUTS)
@pytest.mark.parametrize("shape", sorted(MS.SHAPES))
def test_the_device_tally_equals_the_rows_path_and_the_reference(fa, models, shape, layout):
    pyoracle, mencius_maps = models
    kw = MS.SHAPES[shape]
    n = MS.LENGTHS[-1]
    st = MS.Stream(shape, n, layout, seed=100)
    gpu, ref = context(fa, kw), context(fa, kw)
    # the stream cut into bursts of every length (entries stay Pending in between, complete later, get votes after Done),
    # then once more as one burst
    cuts = [0] + np.cumsum(MS.LENGTHS[:-1]).tolist() + [n]
    for bursts in (list(zip(cuts[:-1], cuts[1:])), [(0, n)]):
        assert [hi - lo for lo, hi in bursts][:5] in (list(MS.LENGTHS[:5]), [n])
        gpu.reset(), ref.reset()
        orc = pyoracle.System(pyoracle.make_config(**kw))
        for s in (gpu, ref, orc):
            MS.open_all(s, st)
        got = []
        for lo, hi in bursts:
            d = st.decoded(lo, hi)
            rc, ch, cr, cv = dev_call(gpu, d)
            # 1. the rows path on the oracle: flags, rounds and values at the same indices
            wrc, wch, wcr, wcv = MS.rows_path(orc, d, kw)
            assert rc == 0 and wrc == 0
            same((ch, cr, cv), (wch, wcr, wcv))
            # 2. a second context: the folded range rows through fpx_proxy_phase2b_noop_ranges, the Phase2b half
            # through fpx_proxy_phase2b_msgs_dev -- the same outputs, the same state
            rrc, rch, rcr, rcv = MS.rows_path(ref, d, kw, phase2b=False)
            prc, pch, pcr, pcv = phase2b_msgs_dev(ref, d)
            assert rrc == 0 and prc == 0
            is_p = d["kind"] == MS.PHASE2B
            same((ch[is_p], cr[is_p], cv[is_p]), (pch[is_p], pcr[is_p], pcv[is_p]))
            same((ch[~is_p], cr[~is_p], cv[~is_p]), (rch[~is_p], rcr[~is_p], rcv[~is_p]))
            np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
            got += MS.chosen_keys(d, ch)
        for k in st.range_keys():
            a, b = gpu.read_range_tally(*k), ref.read_range_tally(*k)
            assert a[0] == b[0], k
            np.testing.assert_array_equal(a[1], b[1])
        # 3. the reference, message at a time
        check_against_the_models(gpu, st, got, mencius_maps)
    gpu.close(), ref.close()


@pytest.mark.parametrize("shape", ["a2r3", "r256"])
def test_a_mixed_burst_equals_its_two_halves_called_separately_in_either_order(fa, shape):
    st = MS.Stream(shape, 20000, "random", seed=21)
    d = st.decoded()
    is_p = d["kind"] == MS.PHASE2B
    only_p, only_r = {k: v.copy() for k, v in d.items()}, {k: v.copy() for k, v in d.items()}
    only_p["kind"][~is_p] = 0
    only_r["kind"][is_p] = 0
    mixed = context(fa, st.kw)
    MS.open_all(mixed, st)
    rc, ch, cr, cv = dev_call(mixed, d)
    assert rc == 0 and ch[is_p].any() and ch[~is_p].any()
    for order in ((only_p, only_r), (only_r, only_p)):
        split = context(fa, st.kw)
        MS.open_all(split, st)
        out = [dev_call(split, half) for half in order]
        assert out[0][0] == 0 and out[1][0] == 0
        # a half reports nothing at the other half's messages
        assert (out[0][1] & out[1][1]).sum() == 0
        same((ch, np.maximum(out[0][2], out[1][2]), np.maximum(out[0][3], out[1][3])), (out[0][1] | out[1][1], cr, cv))
        np.testing.assert_array_equal(mixed.state_digest(), split.state_digest())
        split.close()
    mixed.close()


@pytest.mark.parametrize("what", ["group", "end_below_start", "past_S", "acceptor256", "negative_acceptor"])
def test_a_bad_message_is_einval_nothing_is_applied_and_the_claim_words_stay_clean(fa, models, what):
    pyoracle, _ = models
    st = MS.Stream("a2r3", 20000, "random", seed=32)
    gpu, orc = context(fa, st.kw), pyoracle.System(pyoracle.make_config(**st.kw))
    MS.open_all(gpu, st), MS.open_all(orc, st)
    before = gpu.state_digest()
    d = st.decoded()
    bad = {k: v.copy() for k, v in d.items()}
    ranges = np.nonzero(d["kind"] == MS.RANGE)[0]
    at = [int(ranges[len(ranges) // 2]), int(ranges[len(ranges) // 5])]     # the lower index is the one named
    if what == "group":
        bad["group_index"][at] = [st.kw["num_groups"], -1]
    elif what == "end_below_start":
        bad["slot_end"][at] = bad["slot"][at] - 1
    elif what == "past_S":
        bad["slot_end"][at] = st.kw["num_slots"] + 1
    elif what == "acceptor256":
        bad["acceptor_index"][at] = 256
    else:
        bad["acceptor_index"][at] = -1
    rc, ch, cr, cv = dev_call(gpu, bad)
    assert rc == EINVAL and gpu.error_detail()[0] == min(at)
    assert not ch.any() and (cr == -1).all() and (cv == -1).all()
    np.testing.assert_array_equal(gpu.state_digest(), before)
    # a correct call straight after gives the right result: no claim word was left behind by the refused call
    rc, ch, cr, cv = dev_call(gpu, d)
    wrc, wch, wcr, wcv = MS.rows_path(orc, d, st.kw)
    assert rc == 0 and wrc == 0 and wch[d["kind"] == MS.RANGE].sum() > 0
    same((ch, cr, cv), (wch, wcr, wcv))
    gpu.close()


def test_an_unopened_range_is_unknown_at_the_lowest_index_and_a_non_member_bit_contributes_nothing(fa, models):
    pyoracle, _ = models
    st = MS.Stream("a2r3", 20000, "random", seed=31)
    gpu, ref = context(fa, st.kw), context(fa, st.kw)
    orc = pyoracle.System(pyoracle.make_config(**st.kw))
    for s in (gpu, ref, orc):
        MS.open_all(s, st)
    d = st.decoded()
    ranges = np.nonzero(d["kind"] == MS.RANGE)[0]
    lo, hi = int(ranges[len(ranges) // 10]), int(ranges[-3])      # different workgroups, far apart
    d["round"][[lo, hi]] = 9                                      # never opened
    # messages of a non-member acceptor: an unopened range among them (never reported), and the FIRST message of an
    # opened range (never its owner: the outcome moves to the range's next message)
    first = int(ranges[0])
    d["acceptor_index"][first] = 200
    ghost = int(ranges[3])
    d["acceptor_index"][ghost], d["round"][ghost] = 77, 11
    assert ghost < lo and first < lo
    rc, ch, cr, cv = dev_call(gpu, d)
    assert rc == EUNKNOWN and gpu.error_detail() == (lo, int(d["slot"][lo]), 9)
    assert not ch[first] and not ch[ghost]
    # every other message was applied: the rows path without the two unknown ones (its fold leaves non-members out)
    d2 = {k: v.copy() for k, v in d.items()}
    d2["kind"][[lo, hi]] = 0
    wrc, wch, wcr, wcv = MS.rows_path(orc, d2, st.kw)
    assert wrc == 0 and wch.sum() > 0
    same((ch, cr, cv), (wch, wcr, wcv))
    assert MS.rows_path(ref, d2, st.kw)[0] == 0
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    gpu.close(), ref.close()


def test_twenty_thousand_votes_for_one_range_cost_what_any_burst_costs(fa):
    """the O(n) claim: every message of the burst bids for ONE entry and ORs into its four words, in random acceptor order
    (runs of neighbouring lanes with one destination word are short: most votes are an atomic of their own)"""
    kw = MS.SHAPES["r256"]
    n, R = 20000, kw["num_replicas"]
    rng = np.random.default_rng(9)
    gpu, ref = context(fa, kw), context(fa, kw)
    for s in (gpu, ref):
        assert s.proxy_open_noop_ranges([10], [300], [2])[0] == 0
    acc = rng.integers(0, R, size=n).astype(np.int32)
    acc[:100] = np.arange(100)                          # (below the quorum of 128 for a while)
    d = dict(kind=np.full(n, MS.RANGE, np.int32), group_index=np.zeros(n, np.int32), acceptor_index=acc,
             slot=np.full(n, 10, np.int32), slot_end=np.full(n, 300, np.int32), round=np.full(n, 2, np.int32))
    # first too few votes: Pending, with exactly these bits; then all of them: chosen at the burst's first message
    few = {k: v[:100].copy() for k, v in d.items()}
    rc, ch, cr, cv = dev_call(gpu, few)
    assert rc == 0 and not ch.any()
    state, bits = gpu.read_range_tally(10, 300, 2)
    assert state == 1 and [int(w) for w in bits[0]] == [2 ** 64 - 1, 2 ** 36 - 1, 0, 0]
    rc, ch, cr, cv = dev_call(gpu, d)
    assert rc == 0 and ch[0] == 1 and ch.sum() == 1 and cr[0] == 2 and (cv == -1).all() and (cr[1:] == -1).all()
    assert MS.rows_path(ref, few, kw)[0] == 0 and MS.rows_path(ref, d, kw)[1][0] == 1
    assert gpu.read_range_tally(10, 300, 2)[0] == 2
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    # Done: further votes change nothing
    rc, ch, cr, cv = dev_call(gpu, d)
    assert rc == 0 and not ch.any()
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    gpu.close(), ref.close()


@pytest.mark.parametrize("shape,n", [("a1r3", 257), ("a3r5", 20000), ("r256", 20000)])
def test_the_host_form_equals_the_device_form(fa, shape, n):
    st = MS.Stream(shape, n, "random", seed=34)
    a, b = context(fa, st.kw), context(fa, st.kw)
    MS.open_all(a, st), MS.open_all(b, st)
    total = 0
    for lo, hi in [(0, n // 2), (n // 2, n)]:
        d = st.decoded(lo, hi)
        rc, ch, cr, cv = dev_call(a, d)
        hrc, hch, hcr, hcv = b.mencius_proxy_phase2b_msgs(d["acceptor_index"], d["slot"], d["round"], kind=d["kind"],
                                                          group_index=d["group_index"], slot_end=d["slot_end"])
        assert rc == 0 and hrc == 0
        total += int(ch.sum())
        same((ch, cr, cv), (hch, hcr, hcv))
        np.testing.assert_array_equal(a.state_digest(), b.state_digest())
    assert total > 0
    # the host form's errors: the status comes back from the call itself
    d = st.decoded()
    at = int(np.nonzero(d["kind"] == MS.RANGE)[0][-1])
    d["group_index"][at] = st.kw["num_groups"]
    before = b.state_digest()
    assert b.mencius_proxy_phase2b_msgs(d["acceptor_index"], d["slot"], d["round"], kind=d["kind"],
                                        group_index=d["group_index"], slot_end=d["slot_end"])[0] == EINVAL
    assert b.error_detail()[0] == at
    np.testing.assert_array_equal(b.state_digest(), before)
    a.close(), b.close()


def test_null_kind_null_slot_end_other_kinds_and_an_empty_burst(fa, models):
    pyoracle, _ = models
    st = MS.Stream("a2r3", 257, "random", seed=33)
    gpu, ref = context(fa, st.kw), context(fa, st.kw)
    orc = pyoracle.System(pyoracle.make_config(**st.kw))
    for s in (gpu, ref, orc):
        MS.open_all(s, st)
    d = st.decoded()
    rng = np.random.default_rng(5)
    other = rng.random(st.n) < 0.3
    d["kind"][other] = rng.choice([0, 1, 3, 5, 6, 8], size=int(other.sum()))
    d["slot"][other & (rng.random(st.n) < 0.5)] = -1      # what the decoder leaves in fields that do not apply
    rc, ch, cr, cv = dev_call(gpu, d)
    wrc, wch, wcr, wcv = MS.rows_path(orc, d, st.kw)
    assert rc == 0 and wrc == 0 and not ch[other].any() and wch.sum() > 0
    same((ch, cr, cv), (wch, wcr, wcv))
    assert MS.rows_path(ref, d, st.kw)[0] == 0
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    # kind == NULL: every message is a Phase2b; slot_end == NULL is fine then, and with a kind array without ranges
    p = {k: v[d["kind"] == MS.PHASE2B].copy() for k, v in st.decoded().items()}
    gpu.reset(), ref.reset()
    MS.open_all(gpu, st), MS.open_all(ref, st)
    rc, ch, cr, cv = dev_call(gpu, p, with_kind=False, with_end=False, with_group=False)
    prc, pch, pcr, pcv = phase2b_msgs_dev(ref, p)
    assert rc == 0 and prc == 0 and pch.sum() > 0
    same((ch, cr, cv), (pch, pcr, pcv))
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    before = gpu.state_digest()
    assert dev_call(gpu, p, with_end=False)[0] == 0       # (Done entries ignore the second delivery)
    # ... but a range message without a slot_end array is refused
    assert dev_call(gpu, st.decoded(), with_end=False)[0] == EINVAL
    # n == 0
    assert dev_call(gpu, st.decoded(0, 0))[0] == 0
    z = np.zeros(0, np.int32)
    assert gpu.mencius_proxy_phase2b_msgs(z, z, z)[0] == 0
    assert gpu.mencius_phase2b_tick(z, z, z)[:2] == (0, 0)
    np.testing.assert_array_equal(gpu.state_digest(), before)
    gpu.close(), ref.close()


# ---- the tick: decoded arrays to records ------------------------------------------------------------------------------
def expected_records(orc, d, kw):
    wrc, wch, wcr, wcv = MS.rows_path(orc, d, kw)
    assert wrc == 0
    return [(int(d["kind"][i]), int(d["slot"][i]), int(d["slot_end"][i]) if d["kind"][i] == MS.RANGE else -1, int(wcr[i]),
             int(wcv[i])) for i in np.nonzero(wch)[0].tolist()]


def tick(gpu, d, out_cap=None):
    return gpu.mencius_phase2b_tick(d["acceptor_index"], d["slot"], d["round"], kind=d["kind"], group_index=d["group_index"],
                                    slot_end=d["slot_end"], out_cap=out_cap)


def test_the_tick_gives_the_flagged_messages_as_records_in_message_order(fa, models):
    pyoracle, _ = models
    st = MS.Stream("a2r3", 3000, "random", seed=41)
    gpu, ref = context(fa, st.kw), context(fa, st.kw)
    orc = pyoracle.System(pyoracle.make_config(**st.kw))
    for s in (gpu, ref, orc):
        MS.open_all(s, st)
    before = gpu.state_digest()
    # a refused tick applies nothing
    bad = st.decoded()
    bad["acceptor_index"][1234] = 256
    rc, count, recs = tick(gpu, bad)
    assert rc == EINVAL and count == 0 and recs == [] and gpu.error_detail()[0] == 1234
    np.testing.assert_array_equal(gpu.state_digest(), before)
    # the first half: every record; the second half with too small an out: the tick is applied, the count is exact
    d = st.decoded(0, 1500)
    want = expected_records(orc, d, st.kw)
    assert {w[0] for w in want} == {MS.PHASE2B, MS.RANGE}
    rc, count, recs = tick(gpu, d)
    assert rc == 0 and count == len(want) and recs == want
    assert MS.rows_path(ref, d, st.kw)[0] == 0
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    d = st.decoded(1500, 3000)
    want = expected_records(orc, d, st.kw)
    assert len(want) > 1
    rc, count, recs = tick(gpu, d, out_cap=len(want) - 1)
    assert rc == ECAPACITY and count == len(want) and recs == want[:-1]
    assert MS.rows_path(ref, d, st.kw)[0] == 0
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    gpu.close(), ref.close()


def test_the_jni_natives_give_the_same_tick(fa, models, jvm):  # noqa: F811
    pyoracle, _ = models
    st = MS.Stream("a3r5", 3000, "random", seed=45)
    gpu, ref = context(fa, st.kw), context(fa, st.kw)
    orc = pyoracle.System(pyoracle.make_config(**st.kw))
    for s in (gpu, ref, orc):
        MS.open_all(s, st)
    h = gpu._h.value if hasattr(gpu._h, "value") else int(gpu._h)
    n = 1500
    # menciusProxyPhase2bMsgs on the first half
    d = st.decoded(0, n)
    wrc, wch, wcr, wcv = MS.rows_path(orc, d, st.kw)
    arrs = [jvm.arr(d[k]) for k in FIELDS]
    ch, cr, cv = jvm.arr(np.zeros(n, np.int8)), jvm.arr(np.zeros(n, np.int32)), jvm.arr(np.zeros(n, np.int32))
    assert jvm.call("menciusProxyPhase2bMsgs", C.c_int32, C.c_int64(h), n, *arrs, ch, cr, cv) == 0
    assert wrc == 0 and wch.sum() > 0
    same((jvm.read(ch, np.int8, n), jvm.read(cr, np.int32, n), jvm.read(cv, np.int32, n)), (wch.view(np.int8), wcr, wcv))
    # menciusPhase2bTick on the second
    d = st.decoded(n, 2 * n)
    want = expected_records(orc, d, st.kw)
    arrs = [jvm.arr(d[k]) for k in FIELDS]
    outs = [jvm.arr(np.full(n, -77, np.int32)) for _ in range(5)]
    cnt = jvm.arr(np.zeros(1, np.int32))
    assert jvm.call("menciusPhase2bTick", C.c_int32, C.c_int64(h), n, *arrs, *outs, n, cnt) == 0
    count = int(jvm.read(cnt, np.int32, 1)[0])
    assert count == len(want) and {w[0] for w in want} == {MS.PHASE2B, MS.RANGE}
    assert list(zip(*[jvm.read(o, np.int32, count).tolist() for o in outs])) == want
    assert MS.rows_path(ref, st.decoded(0, n), st.kw)[0] == 0 and MS.rows_path(ref, d, st.kw)[0] == 0
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    gpu.close(), ref.close()
