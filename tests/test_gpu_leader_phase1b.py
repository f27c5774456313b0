"""fpx_leader_phase1b_msgs[_dev] on the GPU against tests/leader_phase1b_model.py: the hand-written cases and every
FPX_EINVAL condition through both forms, random streams (tests/phase1b_streams.py), capacity, the sizing call, the
"apply nothing" state, and the device-to-device path from fpx_acceptor_phase1b_info_all_dev -- whole and replica-sharded
-- against fpx_leader_phase1b_scan."""
import ctypes as C

import numpy as np
import pytest

from tests import phase1b_streams as PS
from tests import workloads as W
from tests.leader_phase1b_model import PHASE1B, flatten, handle_burst
from tests.test_jni_shim import jvm  # noqa: F401  (the mock JVM fixture)

pytestmark = pytest.mark.gpu
WORDS = 8  # FPX_P1B_RESULT_WORDS


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    return frankenpaxos_amd


def held_words(held, ngroups):
    w = np.zeros((ngroups, 4), np.uint64)
    for g, b in held:
        w[g, b >> 6] |= np.uint64(1) << np.uint64(b & 63)
    return w


def call_kw(kw):
    return dict(leader_group=kw.get("leader_group", 0), recover_slot=kw.get("recover_slot", -1),
                flags=1 if kw.get("all_rows") else 0, grid_cols=kw.get("grid_cols", 0))


def run_host(ctx, kw, arrs, cap=None):
    st, res = ctx.leader_phase1b_msgs(kw["round_"], kw["watermark"], arrs["msg_round"], arrs["acceptor_index"], arrs["offsets"],
                                      arrs["info_slot"], arrs["info_vote_round"], arrs["info_value_id"], kind=arrs["kind"],
                                      group_index=arrs["group_index"], cap=cap, **call_kw(kw))
    return st, res, ctx.error_detail()[0]


def run_dev(ctx, kw, arrs, cap):
    """the device form: (status at sync, result dict like the host form's, error index, raw output bytes)"""
    import torch

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = {k: dev(v) for k, v in arrs.items()}
    result = torch.full((WORDS,), -1, dtype=torch.int64, device="cuda")
    out = [torch.full((max(cap, 1),), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    held = torch.zeros(ctx.ngroups * 4, dtype=torch.int64, device="cuda")
    ctx.leader_phase1b_msgs_dev(kw["round_"], kw["watermark"], t["msg_round"], t["acceptor_index"], t["offsets"], t["info_slot"],
                                t["info_vote_round"], t["info_value_id"], result, kind=t["kind"], group_index=t["group_index"],
                                cap=cap, out_slot=out[0] if cap else None, safe_round=out[1] if cap else None,
                                safe_value=out[2] if cap else None, held_bits=held, **call_kw(kw))
    st = ctx.sync()
    idx = ctx.error_detail()[0]
    r = result.cpu().numpy()
    o = [x.cpu().numpy() for x in out]
    res = {"complete": int(r[0]), "decided_at": int(r[1])}
    if r[0] == 1:
        w = int(r[5])
        res.update(count=int(r[2]), max_slot=int(r[3]), next_slot=int(r[4]), written=w, out_slot=o[0][:w], safe_round=o[1][:w],
                   safe_value=o[2][:w], held_bits=held.cpu().numpy().view(np.uint64).reshape(ctx.ngroups, 4))
    raw = b"".join(x.tobytes() for x in [r] + o)
    return st, res, idx, raw


def same(st, res, idx, want, ngroups):
    assert st == want.status, (st, want.status)
    if want.status in (1, 9):
        assert idx == want.err_index
    if want.complete is None:
        assert res["complete"] == -1               # nothing was written
        return
    assert res["complete"] == want.complete and res["decided_at"] == want.decided_at
    if want.complete != 1:
        return
    assert (res["count"], res["max_slot"], res["next_slot"]) == (want.count, want.max_slot, want.next_slot)
    assert res["written"] == len(want.out_slot)
    np.testing.assert_array_equal(res["out_slot"], np.array(want.out_slot, np.int32))
    np.testing.assert_array_equal(res["safe_round"], np.array(want.safe_round, np.int32))
    np.testing.assert_array_equal(res["safe_value"], np.array(want.safe_value, np.int32))
    np.testing.assert_array_equal(res["held_bits"], held_words(want.held, ngroups))


@pytest.mark.parametrize("name", sorted(PS.hand_cases()))
def test_hand_written_cases_both_forms(fa, name):
    cfg, geo, kw, msgs, exp = PS.hand_cases()[name]
    want = handle_burst(geo, msgs=msgs, **kw)
    for k, v in exp.items():
        assert getattr(want, k) == v, k
    ctx = fa.Context(fa.make_config(**cfg))
    arrs = flatten(msgs)
    same(*run_host(ctx, kw, arrs), want, ctx.ngroups)
    cap = want.count or 0
    st, res, idx, _ = run_dev(ctx, kw, arrs, cap)
    same(st, res, idx, want, ctx.ngroups)
    ctx.close()


@pytest.mark.parametrize("name", sorted(PS.einval_cases()))
def test_every_einval_condition_both_forms(fa, name):
    cfg, geo, kw, msgs, index, off_bad = PS.einval_cases()[name]
    want = handle_burst(geo, msgs=msgs, offsets_bad_at=off_bad, **kw)
    assert (want.status, want.err_index) == (1, index)
    arrs = flatten(msgs)
    if off_bad is not None:
        arrs = PS.break_offsets(arrs, name)
    ctx = fa.Context(fa.make_config(**cfg))
    same(*run_host(ctx, kw, arrs, cap=8), want, ctx.ngroups)
    st, res, idx, _ = run_dev(ctx, kw, arrs, 8)
    same(st, res, idx, want, ctx.ngroups)
    # the refusal left the context usable: the good prefix of the hand-written case (a) decides
    cfg_a, geo_a, kw_a, msgs_a, _ = PS.hand_cases()["a_basic"]
    if cfg == cfg_a:
        same(*run_host(ctx, kw_a, flatten(msgs_a)), handle_burst(geo_a, msgs=msgs_a, **kw_a), ctx.ngroups)
    ctx.close()


def test_arguments_refused_at_once(fa):
    cfg, geo, kw, msgs, _ = PS.hand_cases()["a_basic"]
    ctx = fa.Context(fa.make_config(**cfg))
    a = flatten(msgs)
    L = fa.lib()
    res = np.full(WORDS, -1, np.int64)
    p = lambda x: x.ctypes.data

    def call(round_=4, wm=1, lg=0, rec=-1, flags=0, n=3, grid_cols=0, cap=0, result=res):
        return L.fpx_leader_phase1b_msgs(ctx._h, round_, wm, lg, rec, flags, n, p(a["kind"]), p(a["msg_round"]), p(a["group_index"]),
                                         p(a["acceptor_index"]), p(a["offsets"]), p(a["info_slot"]), p(a["info_vote_round"]),
                                         p(a["info_value_id"]), grid_cols, cap, None, None, None, None if result is None else p(result), None)

    assert call() == 5 and res[0] == 1 and res[2] == 5          # the sizing call: FPX_ECAPACITY, count written
    for bad in (dict(n=-1), dict(cap=-1), dict(round_=-1), dict(round_=2 ** 30 - 1), dict(wm=-1), dict(rec=-2), dict(lg=1),
                dict(flags=2), dict(grid_cols=-1), dict(grid_cols=257), dict(cap=4), dict(result=None)):
        assert call(**bad) == 1, bad
    ctx.close()


@pytest.mark.parametrize("shape,seed", [(s, seed) for s in sorted(PS.SHAPES) for seed in PS.SEEDS])
def test_random_streams_against_the_model(fa, shape, seed):
    s = PS.Stream(shape, seed)
    ctx = fa.Context(fa.make_config(**s.cfg))
    arrs = flatten(s.msgs)
    kw = dict(round_=s.round, watermark=s.watermark)
    same(*run_host(ctx, kw, arrs), s.want, ctx.ngroups)                       # sizing call, then cap = count
    st, res, idx, raw = run_dev(ctx, kw, arrs, s.want.count)
    same(st, res, idx, s.want, ctx.ngroups)
    assert run_dev(ctx, kw, arrs, s.want.count)[3] == raw                     # the same burst again: the same bytes
    # cap < count: FPX_ECAPACITY, the first cap entries exact (cap not a multiple of 64 either)
    cap = s.want.count // 2 + 3
    short = handle_burst(s.geo, s.round, s.watermark, s.msgs, cap=cap)
    assert short.status == 5 and len(short.out_slot) == cap
    same(*run_host(ctx, kw, arrs, cap=cap), short, ctx.ngroups)
    st, res, idx, _ = run_dev(ctx, kw, arrs, cap)
    same(st, res, idx, short, ctx.ngroups)
    # a shorter burst is not complete yet; the longer one is
    part = s.msgs[: s.want.decided_at]
    same(*run_host(ctx, kw, flatten(part)), handle_burst(s.geo, s.round, s.watermark, part), ctx.ngroups)
    ctx.close()


def test_apply_nothing_state_writes_complete_only(fa):
    import torch

    cfg, geo, kw, msgs, _ = PS.hand_cases()["a_basic"]
    ctx = fa.Context(fa.make_config(**cfg))
    # a _dev batch that breaks the run contract (one slot twice) puts the context into the state
    slot = torch.tensor([3, 3], dtype=torch.int32, device="cuda")
    one = torch.ones(2, dtype=torch.int32, device="cuda")
    ctx.phase2_fused_dev(slot, one, one)
    arrs = flatten(msgs)
    t = {k: torch.from_numpy(v).cuda() for k, v in arrs.items()}
    result = torch.full((WORDS,), -1, dtype=torch.int64, device="cuda")
    out = [torch.full((8,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    ctx.leader_phase1b_msgs_dev(4, 1, t["msg_round"], t["acceptor_index"], t["offsets"], t["info_slot"], t["info_vote_round"],
                                t["info_value_id"], result, kind=t["kind"], group_index=t["group_index"], cap=8,
                                out_slot=out[0], safe_round=out[1], safe_value=out[2])
    assert ctx.sync() == 6                                              # FPX_EORDER, from the vote batch
    assert result.cpu().tolist() == [0] + [-1] * (WORDS - 1)
    assert all((o.cpu().numpy() == -7).all() for o in out)
    st, res, idx, _ = run_dev(ctx, kw, arrs, 5)                         # after the sync the context answers again
    same(st, res, idx, handle_burst(geo, msgs=msgs, **kw), ctx.ngroups)
    ctx.close()


# ---- device to device ------------------------------------------------------------------------------------------------
def info_all_dev(ctx, wm, cap):
    import torch

    E = ctx.ngroups * ctx.R
    off = torch.zeros(E + 1, dtype=torch.int64, device="cuda")
    rec = [torch.zeros(max(cap, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")
    ctx.acceptor_phase1b_info_all_dev(wm, None, cap, off, rec[0], rec[1], rec[2], tot)
    return off, rec, tot


def headers_on_device(quorum, R, base, round_):
    """kind / msg_round / group / acceptor of the E entries of one context, from the quorum's mask [ngroups, total]:
    an entry outside the quorum is not a Phase1b"""
    import torch

    q = torch.from_numpy(quorum).cuda()
    ng = q.shape[0]
    e = torch.arange(ng * R, device="cuda")
    grp, acc = (e // R).to(torch.int32), (base + e % R).to(torch.int32)
    kind = torch.where(q[grp.long(), acc.long()], PHASE1B, 0).to(torch.int32)
    return kind, torch.full_like(kind, round_), grp, acc


def recover_dev(ctx, wm, round_, hdr, off, rec, cap):
    import torch

    result = torch.full((WORDS,), -1, dtype=torch.int64, device="cuda")
    out = [torch.full((cap,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    ctx.leader_phase1b_msgs_dev(round_, wm, hdr[1], hdr[3], off, rec[0], rec[1], rec[2], result, kind=hdr[0], group_index=hdr[2],
                                cap=cap, out_slot=out[0], safe_round=out[1], safe_value=out[2])
    assert ctx.sync() == 0
    r = result.cpu().numpy()
    assert r[0] == 1
    return int(r[3]), out[1].cpu().numpy()[: r[5]], out[2].cpu().numpy()[: r[5]], out[0].cpu().numpy()[: r[5]]


def test_info_all_feeds_the_leader_without_a_host_read(fa, oracle):
    S, R, A, wm = 4096, 8, 2, 1000
    kw = dict(num_slots=S, num_replicas=R, num_groups=A, f=3, tally_ways=8)
    ctx, ref = fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))
    script = W.adversarial_script(S // 2, R, R // 2 + 1, 5, epochs=8, fused=True, ngroups=A)
    W.run_script(ctx, script), W.run_script(ref, script)
    rng = np.random.default_rng(3)
    # exactly f + 1 of every group: the handler decides at the (f + 1)-th and ignores what follows, the scan takes its whole mask
    quorum = W.random_subsets(rng, A, R, 4, 4)
    off, rec, tot = info_all_dev(ctx, wm, S * R * A)
    hdr = headers_on_device(quorum, R, 0, 9)
    mx, sr, sv, sl = recover_dev(ctx, wm, 9, hdr, off, rec, S)
    for scan in (ctx.leader_phase1b_scan(wm, W.bits_from_bool(quorum), S), ref.leader_phase1b_scan(wm, W.bits_from_bool(quorum), S)):
        assert scan[0] == 0 and scan[1] == mx and mx > wm
        np.testing.assert_array_equal(sr, scan[2])
        np.testing.assert_array_equal(sv, scan[3])
    np.testing.assert_array_equal(sl, np.arange(wm, mx + 1))
    assert (sr >= 0).any() and (sr < 0).any()
    ctx.close()


def test_two_replica_shards_recover_what_the_whole_group_would(fa, oracle):
    """replica_base 0 and 4 of 8: no context sees a quorum's rows, so the scan cannot be used; the two shards' info
    passes, concatenated as messages, can"""
    import torch

    S, R, wm = 4096, 8, 100
    whole = oracle.System(oracle.make_config(num_slots=S, num_replicas=R, f=3, tally_ways=8))
    shards = [fa.Context(fa.make_config(num_slots=S, num_replicas=4, f=3, replica_base=b, replicas_total=R, tally_ways=8))
              for b in (0, 4)]
    rng = np.random.default_rng(8)
    slot, _, val = W.steady_stream(S // 2)
    for r in (1, 2, 4):
        keep = rng.random(len(slot)) < 0.7
        sl, vl = slot[keep], val[keep] + r
        rr = np.full(len(sl), r, np.int32)
        tgt = W.bits_from_bool(W.random_subsets(rng, len(sl), R, 1, R))
        for be in [whole] + shards:
            be.proxy_open(sl, rr, vl)
            assert be.acceptor_phase2a(sl, rr, vl, tgt)[0] == 0
    quorum = np.zeros((1, R), bool)
    quorum[0, [1, 2, 4, 7]] = True                                        # f + 1 acceptors, two in each shard
    parts = [(info_all_dev(sh, wm, S * 4), headers_on_device(quorum, 4, b, 9)) for sh, b in zip(shards, (0, 4))]
    (off0, rec0, tot0), h0 = parts[0]
    (off1, rec1, tot1), h1 = parts[1]
    n0 = int(tot0[0])                                                     # (sizes the concatenation; the records stay on the device)
    off = torch.cat([off0[:-1], off1 + off0[-1]])
    rec = [torch.cat([a[:n0], b[: int(tot1[0])]]) for a, b in zip(rec0, rec1)]
    hdr = [torch.cat([a, b]) for a, b in zip(h0, h1)]
    mx, sr, sv, _ = recover_dev(shards[1], wm, 9, hdr, off, rec, S)
    scan = whole.leader_phase1b_scan(wm, W.bits_from_bool(quorum), S)
    assert scan[1] == mx and mx > wm
    np.testing.assert_array_equal(sr, scan[2])
    np.testing.assert_array_equal(sv, scan[3])
    assert len(set(sr.tolist())) > 2
    for sh in shards:
        sh.close()


def test_the_jni_native_on_the_mock_jvm(fa, jvm):  # noqa: F811
    cfg, geo, kw, msgs, _ = PS.hand_cases()["a_basic"]
    want = handle_burst(geo, msgs=msgs, **kw)
    c = fa.make_config(**cfg)
    h = jvm.call("create", C.c_int64, jvm.arr(np.array([getattr(c, f) for f, _ in c._fields_], np.int32)))
    assert h > 0
    a = flatten(msgs)
    scalars = jvm.arr(np.array([4, 1, 0, -1, 0, 0], np.int32))
    result, held = jvm.arr(np.zeros(WORDS, np.int64)), jvm.arr(np.zeros(4, np.int64))
    outs = [jvm.arr(np.zeros(5, np.int32)) for _ in range(3)]
    ins = lambda: [jvm.arr(a[k]) for k in ("kind", "msg_round", "group_index", "acceptor_index", "offsets", "info_slot",
                                           "info_vote_round", "info_value_id")]
    st = jvm.call("leaderPhase1bMsgs", C.c_int32, h, scalars, 3, *ins(), 5, *outs, result, held)
    assert st == 0
    r = jvm.read(result, np.int64, WORDS)
    assert list(r[:6]) == [1, want.decided_at, want.count, want.max_slot, want.next_slot, 5]
    np.testing.assert_array_equal(jvm.read(outs[0], np.int32, 5), want.out_slot)
    np.testing.assert_array_equal(jvm.read(outs[1], np.int32, 5), want.safe_round)
    np.testing.assert_array_equal(jvm.read(outs[2], np.int32, 5), want.safe_value)
    assert jvm.read(held, np.int64, 4)[0] == 3
    short = ins()
    short[5] = jvm.arr(a["info_slot"][:-1])                               # fewer records than the offsets promise
    assert jvm.call("leaderPhase1bMsgs", C.c_int32, h, scalars, 3, *short, 5, *outs, result, held) == 1
    assert jvm.call("destroy", C.c_int32, h) == 0
