"""fpx_acceptor_phase1b_info_all[_dev] and fpx_acceptor_phase1: the Phase1b.info of every selected acceptor in one
device pass (csrc/fpx_phase1_info.hpp), against three references -- the untouched single-acceptor path
(fpx_acceptor_phase1b_info), the C oracle, and the numpy restatement of tests/test_phase1_all_cpu.py.  Every comparison
is exact integer equality.

The count kernel's grid cap is restated from the launch code (fpx_api.hip, enqueue_p1i): one wavefront per unit of
P1I_CHUNK tiles of 64 slots of one group, four wavefronts to a workgroup, at most num_cus * 8 workgroups.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import workloads as W
from tests.test_gpu_phase1_readpath import EXPECT_G, acceptors, lanes, num_cus, pack_bits, recovery_script
from tests.test_jni_shim import jvm  # noqa: F401  (the mock JVM fixture)
from tests.test_phase1_all_cpu import GEOMETRIES, P1I_CHUNK, P1I_TILE, WIDTH_RS, info_all, selection

pytestmark = pytest.mark.gpu
EINVAL, ECAPACITY = 1, 5
SENTINEL = -7


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()  # raises if libfpx.so is missing: no fallback
    return frankenpaxos_amd


def both(fa, oracle, **kw):
    return fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))


def geom(kw):
    return kw.get("num_leader_groups", 1), kw.get("num_groups", 1)


def watermarks(S, ng):
    return (-3, 0, 17, P1I_TILE * ng, S - 1, S, S + 5)


def slices(res, e):
    off, sl, vr, vv = res
    return sl[off[e]:off[e + 1]], vr[off[e]:off[e + 1]], vv[off[e]:off[e + 1]]


def same(got, want, what=""):
    for k, (x, y) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(x, y, err_msg="%s [%d]" % (what, k))


def check_everything(gpu, ref, L, A, wms, entries=None):
    """the batched result at every watermark: whole against the numpy restatement of the state the GPU reads back, and
    entry by entry against the single-acceptor path and the oracle"""
    vr, vv, _ = gpu.read_state()
    ng, R = L * A, gpu.R
    total = 0
    for wm in wms:
        got = gpu.acceptor_phase1b_info_all(wm)
        same(got, info_all(vr, vv, L, A, wm), "wm %d" % wm)
        for e in (range(ng * R) if entries is None else entries):
            g, r = divmod(e, R)
            same(slices(got, e), gpu.acceptor_phase1b_info(g, r, wm), "single (%d, %d) wm %d" % (g, r, wm))
            if ref is not None:
                same(slices(got, e), ref.acceptor_phase1b_info(g, r, wm), "oracle (%d, %d) wm %d" % (g, r, wm))
        total += int(got[0][-1])
    return total


def run_both(gpu, ref, script):
    W.assert_same_outputs(W.run_script(gpu, script), W.run_script(ref, script))


# ---- widths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", WIDTH_RS)
def test_every_entry_at_every_width(fa, oracle, R):
    S = 2048
    gpu, ref = both(fa, oracle, num_slots=S, num_replicas=R, f=(R - 1) // 2, ballot_mode=R % 2, tally_ways=8)
    run_both(gpu, ref, recovery_script(S, R, 1, 1, 31 + R))
    assert {k[0] for k in gpu.vote_launch_census()["cells"]} == {EXPECT_G[R]} == {lanes(R)}
    assert check_everything(gpu, ref, 1, 1, watermarks(S, 1)) > S
    gpu.close()


# ---- geometries -----------------------------------------------------------------------------------------------------
def test_groups_grid(fa, oracle):
    kw, S = GEOMETRIES["groups4"], 4096
    gpu, ref = both(fa, oracle, num_slots=S, tally_ways=8, **kw)
    run_both(gpu, ref, recovery_script(S, kw["num_replicas"], 1, 4, 9))
    assert check_everything(gpu, ref, 1, 4, watermarks(S, 4)) > S // 4
    gpu.close()


def test_mencius_both_layouts(fa, oracle, row_layout):
    kw, S = GEOMETRIES["mencius4x2"], 4096 + 8 * 5          # a ragged last tile: S is no multiple of 64 x groups
    L, A = geom(kw)
    assert S % (P1I_TILE * L * A) != 0 and S % L == 0
    gpu, ref = both(fa, oracle, num_slots=S, tally_ways=8, **kw)
    run_both(gpu, ref, recovery_script(S, kw["num_replicas"], L, A, 19))
    assert check_everything(gpu, ref, L, A, watermarks(S, L * A)) > S // 8
    gpu.close()


def test_interleaved_rows(fa, oracle):
    old = os.environ.get("FPX_INTERLEAVE")
    os.environ["FPX_INTERLEAVE"] = "1"                      # read by fpx_create (make_geom)
    try:
        S = 2048 + 37
        gpu, ref = both(fa, oracle, num_slots=S, num_replicas=3, f=1, tally_ways=8)
    finally:
        if old is None:
            del os.environ["FPX_INTERLEAVE"]
        else:
            os.environ["FPX_INTERLEAVE"] = old
    run_both(gpu, ref, recovery_script(S, 3, 1, 1, 3))
    assert check_everything(gpu, ref, 1, 1, watermarks(S, 1)) > S
    gpu.close()


def test_replica_shard_mask_bits(fa, oracle):
    """a shard of acceptors 64 .. 76 of 96: the mask bit of local acceptor r is replica_base + r"""
    S, R, base, total = 2048, 13, 64, 96
    gpu = fa.Context(fa.make_config(num_slots=S, num_replicas=R, f=47, replica_base=base, replicas_total=total, tally_ways=8))
    rng = np.random.default_rng(4)
    slot = np.arange(S, dtype=np.int32)
    tgt = W.bits_from_bool(W.random_subsets(rng, S, total, 30, 96))
    assert gpu.acceptor_phase2a(slot, np.zeros(S, np.int32), W.steady_values(slot), tgt)[0] == 0
    vr, vv, _ = gpu.read_state()
    assert check_everything(gpu, None, 1, 1, (0, 17, S - 1)) > S
    m = np.zeros((1, 4), np.uint64)
    m[0, 1] = np.uint64(0b1000000000101)                    # bits 64, 66, 76: local acceptors 0, 2, 12
    m[0, 0] = np.uint64(0b101)                              # acceptors 0 and 2 of ANOTHER shard: not ours
    sel = selection(m, 1, R, base)
    assert np.nonzero(sel[0])[0].tolist() == [0, 2, 12]
    got = gpu.acceptor_phase1b_info_all(5, m)
    same(got, info_all(vr, vv, 1, 1, 5, sel))
    for r in range(R):
        want = gpu.acceptor_phase1b_info(0, r, 5) if sel[0, r] else (np.zeros(0, np.int32),) * 3
        same(slices(got, r), want)
    gpu.close()


# ---- past the grid cap --------------------------------------------------------------------------------------------
def test_past_the_count_grid_cap(fa, oracle):
    R = 3
    units_per_pass = num_cus() * 8 * 4                      # wavefronts of a full grid; one unit each per pass
    S = (units_per_pass + 3) * P1I_CHUNK * P1I_TILE + 2 * P1I_TILE + 9
    gpu, ref = both(fa, oracle, num_slots=S, num_replicas=R, f=1, tally_ways=8)
    rng = np.random.default_rng(8)
    second = units_per_pass * P1I_CHUNK * P1I_TILE          # the first slot a wavefront's SECOND unit holds
    marks = np.array([0, second - 1, second, second + 1, S - 1], np.int32)
    for rnd, slot, tgt in ((0, np.nonzero(rng.random(S) < 0.4)[0], None), (3, marks, acceptors(len(marks), R, [R - 1]))):
        slot = slot.astype(np.int32)
        tgt = pack_bits(W.random_subsets(rng, len(slot), R, 1, R)) if tgt is None else tgt
        a = gpu.phase2_fused(slot, np.full(len(slot), rnd, np.int32), W.steady_values(slot), tgt)
        b = ref.phase2_fused(slot, np.full(len(slot), rnd, np.int32), W.steady_values(slot), tgt)
        assert a[0] == b[0] == 0
    for wm in (0, second - 70):
        got = gpu.acceptor_phase1b_info_all(wm)
        for r in range(R):
            want = ref.acceptor_phase1b_info(0, r, wm)
            same(slices(got, r), want, "acceptor %d wm %d" % (r, wm))
            same(slices(got, r), gpu.acceptor_phase1b_info(0, r, wm))
        sl, vr, _ = slices(got, R - 1)
        assert set(marks[marks >= wm].tolist()) <= set(sl.tolist()) and sl[-1] == S - 1 and vr[-1] == 3
    gpu.close()


# ---- hand-built vote patterns ----------------------------------------------------------------------------------------
def test_hand_built_patterns(fa, oracle):
    """acceptor 0 never votes, 1 votes in every slot of its group, 2 only in the window's last slot, 3 in every other slot
    of its group; two groups, a ragged last tile"""
    R, A = 5, 2
    S = 2048 + 2 * 11 + 1
    assert S % (P1I_TILE * A) != 0
    gpu, ref = both(fa, oracle, num_slots=S, num_replicas=R, num_groups=A, f=2, tally_ways=8)
    s = np.arange(S, dtype=np.int32)
    plan = [(1, s), (2, s[-1:]), (3, s[(s // A) % 2 == 0]), (4, s[s % 7 == 3])]
    for acc, slot in plan:
        for be in (gpu, ref):
            st = be.acceptor_phase2a(slot, np.full(len(slot), acc, np.int32), 1000 * acc + slot, acceptors(len(slot), R, [acc]))
            assert st[0] == 0
    wms = watermarks(S, A) + (2 * P1I_TILE * A - 1, 2 * P1I_TILE * A + 1)
    assert check_everything(gpu, ref, 1, A, wms) > S
    off, sl, vr, vv = gpu.acceptor_phase1b_info_all(0)
    last_group = (S - 1) % A
    for g in range(A):
        mine = s[s % A == g]
        assert off[g * R + 1] == off[g * R]                                                       # no vote
        np.testing.assert_array_equal(slices((off, sl, vr, vv), g * R + 1)[0], mine)               # every slot
        assert slices((off, sl, vr, vv), g * R + 2)[0].tolist() == ([S - 1] if g == last_group else [])
        np.testing.assert_array_equal(slices((off, sl, vr, vv), g * R + 3)[0], mine[(mine // A) % 2 == 0])
    gpu.close()


# ---- masks ---------------------------------------------------------------------------------------------------------
def test_masks(fa, oracle):
    kw, S = GEOMETRIES["mencius4x2"], 2048
    L, A = geom(kw)
    ng, R = L * A, kw["num_replicas"]
    gpu, ref = both(fa, oracle, num_slots=S, tally_ways=8, **kw)
    run_both(gpu, ref, recovery_script(S, R, L, A, 23))
    vr, vv, _ = gpu.read_state()
    full = gpu.acceptor_phase1b_info_all(17, None)
    ones = np.full((ng, 4), ~np.uint64(0), np.uint64)       # all ones: also every bit outside the members
    same(gpu.acceptor_phase1b_info_all(17, ones), full)
    zero = gpu.acceptor_phase1b_info_all(17, np.zeros((ng, 4), np.uint64))
    assert not zero[0].any() and len(zero[0]) == ng * R + 1 and len(zero[1]) == 0
    one = np.zeros((ng, 4), np.uint64)
    one[ng - 1, 0] = np.uint64(1 << (R - 1))
    rng = np.random.default_rng(6)
    subset = pack_bits(rng.random((ng, R)) < 0.5)
    assert len({tuple(x) for x in subset.tolist()}) > 2     # a different subset per group
    # bits outside the members: fpx_acceptor_phase1a never looks at them (its kernels test bit base + r, r < R only)
    outside = subset.copy()
    outside[:, 0] |= ~np.uint64(0) << np.uint64(R)
    outside[:, 1:] = ~np.uint64(0)
    for m in (one, subset, outside):
        sel = selection(m, ng, R)
        got = gpu.acceptor_phase1b_info_all(17, m)
        same(got, info_all(vr, vv, L, A, 17, sel))
        for e in range(ng * R):
            g, r = divmod(e, R)
            want = ref.acceptor_phase1b_info(g, r, 17) if sel[g, r] else (np.zeros(0, np.int32),) * 3
            same(slices(got, e), want)
            if sel[g, r]:
                same(slices(got, e), slices(full, e))
    same(gpu.acceptor_phase1b_info_all(17, outside), gpu.acceptor_phase1b_info_all(17, subset))
    assert gpu.acceptor_phase1b_info_all(17, one)[0][-1] == len(ref.acceptor_phase1b_info(ng - 1, R - 1, 17)[0]) > 0
    # ... and Phase1a treats the same words the same way: the promised bits are the members' bits only
    pa = gpu.acceptor_phase1a(0, 900, 0, outside[0])
    pb = ref.acceptor_phase1a(0, 900, 0, outside[0])
    assert pa[0] == pb[0] == 0
    np.testing.assert_array_equal(pa[1], pb[1])
    assert W.bool_from_bits(pa[1][None, :], 256)[0, R:].sum() == 0
    gpu.close()


# ---- the _dev form: capacity, ordering, refusals ----------------------------------------------------------------------
class Dev:
    def __init__(self, gpu, cap):
        import torch
        self.t = torch
        E = gpu.ngroups * gpu.R
        self.off = torch.full((E + 1,), SENTINEL, dtype=torch.int64, device="cuda")
        self.rec = [torch.full((max(cap, 1),), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
        self.tot = torch.full((2,), SENTINEL, dtype=torch.int64, device="cuda")
        self.cap = cap

    def call(self, gpu, wm, masks=None, cap=None):
        cap = self.cap if cap is None else cap
        rec = self.rec if cap > 0 else [None] * 3
        gpu.acceptor_phase1b_info_all_dev(wm, masks, cap, self.off, rec[0], rec[1], rec[2], self.tot)

    def host(self):
        return (self.off.cpu().numpy(), [r.cpu().numpy() for r in self.rec], self.tot.cpu().numpy())


def test_dev_capacity(fa, oracle):
    S, R = 2048, 13
    gpu, ref = both(fa, oracle, num_slots=S, num_replicas=R, f=6, tally_ways=8)
    run_both(gpu, ref, recovery_script(S, R, 1, 1, 44))
    want = gpu.acceptor_phase1b_info_all(17)
    total = int(want[0][-1])
    mid = int(want[0][5] + (want[0][6] - want[0][5]) // 2)  # inside acceptor 5's run
    assert want[0][5] < mid < want[0][6] and total > mid > 0
    for cap in (0, total - 1, total, mid):
        d = Dev(gpu, cap + 16)
        d.call(gpu, 17, cap=cap)
        st = gpu.sync()
        off, rec, tot = d.host()
        assert st == (0 if cap >= total else ECAPACITY), (cap, st)
        np.testing.assert_array_equal(off, want[0])                            # offsets and totals in full
        assert tot.tolist() == [total, min(total, cap)]
        for k in range(3):
            np.testing.assert_array_equal(rec[k][:cap], want[1 + k][:cap])     # exactly the first cap records
            assert (rec[k][cap:] == SENTINEL).all()                            # nothing beyond them
        # the code was per call: the next _dev call applies normally
        d2 = Dev(gpu, total)
        d2.call(gpu, 17)
        assert gpu.sync() == 0
        off, rec, tot = d2.host()
        same((off, rec[0], rec[1], rec[2]), want)
        assert tot.tolist() == [total, total]
    gpu.close()


def test_dev_ordering_and_refusal(fa, oracle):
    import torch
    S, R = 4096, 65
    gpu, ref = both(fa, oracle, num_slots=S, num_replicas=R, quorum_kind=1, ballot_mode=1, tally_ways=8)
    run_both(gpu, ref, recovery_script(S, R, 1, 1, 5))
    # directly behind a fused step with a ballot per cell, nothing in between: the step's fold is still pending
    slot = np.arange(S // 2, S // 2 + 1500, dtype=np.int32)
    rnd = np.full(len(slot), 2000, np.int32)
    ts, tr, tv = (torch.from_numpy(x).cuda() for x in (slot, rnd, W.steady_values(slot).astype(np.int32)))
    ch, cr, cv = torch.zeros(len(slot), dtype=torch.uint8, device="cuda"), torch.zeros_like(ts), torch.zeros_like(ts)
    d = Dev(gpu, S * R)
    gpu.phase2_fused_dev(ts, tr, tv, None, ch, cr, cv)
    d.call(gpu, 100)
    assert gpu.sync() == 0
    assert ref.phase2_fused(slot, rnd, W.steady_values(slot))[0] == 0
    off, rec, tot = d.host()
    for e in range(R):
        want = ref.acceptor_phase1b_info(0, e, 100)
        same(tuple(x[off[e]:off[e + 1]] for x in rec), want, "behind the fused step, acceptor %d" % e)
    assert tot[0] == off[-1] >= 1500 * R
    # after recycling the middle of the window
    gpu.recycle_slots(S // 4, S // 2)
    ref.recycle_slots(S // 4, S // 2)
    d.call(gpu, 100)
    assert gpu.sync() == 0
    off, rec, tot = d.host()
    for e in range(R):
        want = ref.acceptor_phase1b_info(0, e, 100)
        same(tuple(x[off[e]:off[e + 1]] for x in rec), want, "after recycle, acceptor %d" % e)
        assert not ((want[0] >= S // 4) & (want[0] < 3 * S // 4)).any()
    # a refused run in front (a malformed tick decoded on the device): nothing but {0, 0} and offsets[0]
    from frankenpaxos_amd import wire
    msgs = [wire.encode_proxy_leader_phase2a(s, 2001, None) for s in range(8)]
    msgs[3] = msgs[3][:-1]                                 # truncated
    buf, offs = wire.pack(msgs)
    d3 = Dev(gpu, S * R)
    gpu.wire_decode_dev("proxy_leader_inbound", torch.from_numpy(buf).cuda(), torch.from_numpy(offs).cuda(),
                        buf_len=int(offs[-1]))
    d3.call(gpu, 100)
    assert gpu.sync() == EINVAL
    off, rec, tot = d3.host()
    assert tot.tolist() == [0, 0] and off[0] == 0 and (off[1:] == SENTINEL).all()
    assert all((r == SENTINEL).all() for r in rec)
    d3.call(gpu, 100)                                      # and the next call applies normally
    assert gpu.sync() == 0
    assert d3.host()[2].tolist() == d.host()[2].tolist() and d3.host()[2][0] > 0
    gpu.close()


# ---- fpx_acceptor_phase1 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ballot_mode", [0, 1])
@pytest.mark.parametrize("name", ["plain", "mencius4x2"])
def test_acceptor_phase1(fa, oracle, ballot_mode, name):
    kw = dict(num_replicas=5, f=2) if name == "plain" else GEOMETRIES[name]
    L, A = geom(kw)
    ng, R, S = L * A, kw["num_replicas"], 2048
    gpu, ref = both(fa, oracle, num_slots=S, ballot_mode=ballot_mode, tally_ways=8, **kw)
    run_both(gpu, ref, recovery_script(S, R, L, A, 61))
    hi = 5000
    # some acceptors are ahead already: they will Nack
    ahead = acceptors(1, R, [1])[0]
    for be in (gpu, ref):
        assert be.acceptor_phase1a(0, hi + 7, 0, ahead)[0] == 0
    if ng == 1:
        masks = acceptors(1, R, [0, 1, 3])
    else:  # Mencius: only leader group 0's acceptors (its A acceptor groups) are addressed
        masks = np.zeros((ng, 4), np.uint64)
        masks[:A] = acceptors(A, R, range(R))
    for wm in (0, 300):
        rnd = hi + (1 if wm else 0)                         # both below the round acceptor 1 of group 0 is in already
        pb, nb, off, sl, vr, vv = gpu.acceptor_phase1(rnd, wm, masks)
        for g in range(ng):
            if masks[g].any():
                st, wp, wn = ref.acceptor_phase1a(g, rnd, wm, masks[g])
                assert st == 0
            else:
                wp = wn = np.zeros(4, np.uint64)
            np.testing.assert_array_equal(pb[g], wp, err_msg="promised bits of group %d" % g)
            np.testing.assert_array_equal(nb[g], wn, err_msg="nack bits of group %d" % g)
        prom = selection(pb, ng, R)
        assert prom.any() and selection(nb, ng, R)[0, 1] and not prom[0, 1]
        for e in range(ng * R):
            g, r = divmod(e, R)
            want = ref.acceptor_phase1b_info(g, r, wm) if prom[g, r] else (np.zeros(0, np.int32),) * 3
            same(slices((off, sl, vr, vv), e), want, "entry (%d, %d)" % (g, r))
        assert off[-1] > 0
    W.assert_same_state(gpu, ref)
    # a stale-round fused step afterwards is Nacked identically
    slot = np.arange(0, 64, dtype=np.int32)
    a = gpu.phase2_fused(slot, np.full(64, 3, np.int32), W.steady_values(slot))
    b = ref.phase2_fused(slot, np.full(64, 3, np.int32), W.steady_values(slot))
    assert a[0] == b[0] == 0
    same(a[1:], b[1:])
    assert (b[4] >= 0).any()                                # Nack rounds were reported
    W.assert_same_state(gpu, ref)
    gpu.close()


# ---- argument errors, JNI ----------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing(fa):
    gpu = fa.Context(fa.make_config(num_slots=2048, num_replicas=3, f=1))
    L, h = gpu.L, gpu._h
    before = gpu.state_digest()
    off = np.full(4, SENTINEL, np.int64)
    rec = np.full(8, SENTINEL, np.int32)
    k = C.c_int64(SENTINEL)
    o, r = off.ctypes.data, rec.ctypes.data
    for fn, args in (
            (L.fpx_acceptor_phase1b_info_all_dev, (None, 0, None, 0, o, None, None, None, o)),
            (L.fpx_acceptor_phase1b_info_all_dev, (h, 0, None, -1, o, r, r, r, o)),
            (L.fpx_acceptor_phase1b_info_all_dev, (h, 0, None, 0, None, None, None, None, o)),
            (L.fpx_acceptor_phase1b_info_all_dev, (h, 0, None, 0, o, None, None, None, None)),
            (L.fpx_acceptor_phase1b_info_all_dev, (h, 0, None, 4, o, r, None, r, o)),
            (L.fpx_acceptor_phase1b_info_all, (None, 0, None, 0, o, None, None, None, C.byref(k))),
            (L.fpx_acceptor_phase1b_info_all, (h, 0, None, -1, o, r, r, r, C.byref(k))),
            (L.fpx_acceptor_phase1b_info_all, (h, 0, None, 0, None, None, None, None, C.byref(k))),
            (L.fpx_acceptor_phase1b_info_all, (h, 0, None, 0, o, None, None, None, None)),
            (L.fpx_acceptor_phase1b_info_all, (h, 0, None, 4, o, None, r, r, C.byref(k))),
            (L.fpx_acceptor_phase1, (None, 1, 0, None, None, None, 0, o, None, None, None, C.byref(k))),
            (L.fpx_acceptor_phase1, (h, 1, 0, None, None, None, -1, o, r, r, r, C.byref(k))),
            (L.fpx_acceptor_phase1, (h, 1, 0, None, None, None, 0, None, None, None, None, C.byref(k))),
            (L.fpx_acceptor_phase1, (h, 1, 0, None, None, None, 0, o, None, None, None, None)),
            (L.fpx_acceptor_phase1, (h, 1, 0, None, None, None, 4, o, r, r, None, C.byref(k)))):
        assert fn(*args) == EINVAL, args
    assert gpu.sync() == 0 and k.value == SENTINEL and (off == SENTINEL).all() and (rec == SENTINEL).all()
    np.testing.assert_array_equal(gpu.state_digest(), before)       # the refused fpx_acceptor_phase1 promised nothing
    assert gpu.read_scalars()[0].max() == -1
    gpu.close()


def test_jni_acceptor_phase1_all(fa, oracle, jvm):
    kw = GEOMETRIES["groups4"]
    S, R, ng = 2048, kw["num_replicas"], 4
    cfgs = [fa.make_config(num_slots=S, tally_ways=8, **kw) for _ in range(2)]
    a, b = fa.Context(cfgs[0]), fa.Context(cfgs[1])
    script = recovery_script(S, R, 1, 4, 15)
    W.assert_same_outputs(W.run_script(a, script), W.run_script(b, script))
    masks = pack_bits(np.random.default_rng(3).random((ng, R)) < 0.7)
    want = a.acceptor_phase1(7000, 40, masks)
    total, E = len(want[3]), ng * R
    assert total > 0
    h = C.c_int64(b._h.value if hasattr(b._h, "value") else int(b._h))
    call = lambda *x: jvm.call("acceptorPhase1All", C.c_int64, h, 7000, 40, *x)
    tm, bits, off = jvm.arr(masks.reshape(-1).view(np.int64)), jvm.arr(np.zeros(8 * ng, np.int64)), jvm.arr(np.zeros(E + 1, np.int64))
    sl, vr, vv = (jvm.arr(np.zeros(total, np.int32)) for _ in range(3))
    short_i, short_l = jvm.arr(np.zeros(total - 1, np.int32)), jvm.arr(np.zeros(E, np.int64))
    assert call(ng, tm, bits, total, off, short_i, vr, vv) == -EINVAL          # a short record array
    assert call(ng, tm, bits, total, short_l, sl, vr, vv) == -EINVAL           # short offsets
    assert call(ng, tm, jvm.arr(np.zeros(8 * ng - 1, np.int64)), total, off, sl, vr, vv) == -EINVAL
    assert call(ng + 1, tm, bits, total, off, sl, vr, vv) == -EINVAL           # not the handle's groups
    assert call(ng, tm, bits, -1, off, sl, vr, vv) == -EINVAL
    assert b.read_scalars()[0].max() < 7000                                    # the refused calls promised nothing
    assert call(ng, tm, bits, total, off, sl, vr, vv) == total
    gb = jvm.read(bits, np.int64, 8 * ng).view(np.uint64)
    np.testing.assert_array_equal(gb[:4 * ng].reshape(ng, 4), want[0])
    np.testing.assert_array_equal(gb[4 * ng:].reshape(ng, 4), want[1])
    np.testing.assert_array_equal(jvm.read(off, np.int64, E + 1), want[2])
    for o, w in zip((sl, vr, vv), want[3:]):
        np.testing.assert_array_equal(jvm.read(o, np.int32, total), w)
    W.assert_same_state(a, b)
    a.close(), b.close()
