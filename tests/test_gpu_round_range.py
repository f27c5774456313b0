"""The vote, tally, range, Phase1a and recovery kernels at the ends of the round range (include/fpx.h: rounds 0 ...
2^30 - 2, any int32 value_id), where the packed key words, the row records and the cross-lane maxima could lose a bit
without any other test noticing: every other GPU test stays below round a few hundred and value 2^31.

Every case plays a script of tests/round_range_cases.py LIFTED (tests/workloads.py: rounds r -> r + base so that the
highest is MAX_ROUND or the rounds straddle 2^24 / 2^29; values through a bijection of int32 that reaches INT32_MIN, -2,
-1, 0, 2^30 - 1, 2^30, 2^31 - 1) and asserts
  1. every output equal to the CPU oracle's, which has no round limit and no packed keys;
  2. the whole state, sampled tallies and the digest equal to the oracle's;
  3. outputs and state equal to the lift of what a second context gives for the unlifted script -- this one needs no
     oracle (tests/test_round_range_cpu.py proves the relation for the oracle alone);
and, through a census, that the launch form the case is about ran."""
import numpy as np
import pytest

from tests import round_range_cases as RC
from tests import workloads as W

pytestmark = pytest.mark.gpu

EINVAL, UNKNOWN = 1, 2
BAD_ROUNDS = (W.MAX_ROUND + 1, 2 ** 31 - 1, -1, W.INT32_MIN)


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()  # raises if libfpx.so is missing: no fallback
    return frankenpaxos_amd


def cells(ctx, **want):
    keys = ("G", "mode", "ps", "fused", "form")
    return {k: v for k, v in ctx.vote_launch_census()["cells"].items()
            if all(k[keys.index(name)] == val for name, val in want.items())}


def tallies_of(be, S):
    return {s: be.read_tally(s) for s in range(0, S, max(1, S // 97))}


def run_lifted(fa, oracle, kw, script, base, flags=0, keep_noop=False, play=W.run_script, before_readback=None):
    """the three assertions of the module docstring; returns the context that played the lifted script (census intact)"""
    vmap = W.ValueMap(keep_noop=keep_noop)
    b = W.lift_bases(script)[base]
    lifted = W.lift_script(script, b, vmap)
    assert W.script_rounds(lifted)[-1] == W.MAX_ROUND or base != "top"
    gpu, plain = fa.Context(fa.make_config(flags=flags, **kw)), fa.Context(fa.make_config(flags=flags, **kw))
    ref = oracle.System(oracle.make_config(**kw))
    S = kw["num_slots"]
    out_gpu, out_ref = play(gpu, lifted), W.run_script(ref, lifted)
    W.assert_same_outputs(out_gpu, out_ref)
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    if before_readback:
        before_readback(gpu)
    W.assert_same_state(gpu, ref, tally_slots=range(0, S, max(1, S // 97)))
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    keys = RC.range_keys(lifted)
    for key in keys:
        a, r = gpu.read_range_tally(*key), ref.read_range_tally(*key)
        assert a[0] == r[0], key
        np.testing.assert_array_equal(a[1], r[1])
    # the metamorphic half: the same contexts' answers to the unlifted script, lifted
    out_plain = play(plain, script)
    W.assert_same_outputs(out_gpu, W.lift_outputs(out_plain, b, vmap))
    W.assert_same_snapshot(W.snapshot(gpu), W.lift_snapshot(W.snapshot(plain), b, vmap))
    assert tallies_of(gpu, S) == {s: W.lift_tally(t, b, vmap) for s, t in tallies_of(plain, S).items()}
    for s, e, r in RC.range_keys(script):
        a, p = gpu.read_range_tally(s, e, r + b), plain.read_range_tally(s, e, r)
        assert a[0] == p[0], (s, e, r)
        np.testing.assert_array_equal(a[1], p[1])
    plain.close()
    return gpu


# ---------------------------------------------------------------------------------------------------------------------
# vote and tally: widths x ballot modes x deliveries x fused / k1k2, forms solo and grid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,ballot_mode,delivery,fused,base", RC.vote_matrix())
def test_vote_and_tally(fa, oracle, R, ballot_mode, delivery, fused, base):
    G, mode = RC.lanes(R), RC.DELIVERY[delivery]
    S, script = RC.vote_script(R, delivery, fused, per=3000, epochs=6, seed=R * 16 + ballot_mode * 8 + mode)
    kw = dict(num_slots=S, num_replicas=R, quorum_kind=1, ballot_mode=ballot_mode, tally_ways=8)
    flags = fa.FPX_F_SCATTERED_TARGETS if delivery == "scattered" else 0
    gpu = run_lifted(fa, oracle, kw, script, base, flags=flags)
    census = gpu.vote_launch_census()
    if delivery == "packed":
        assert cells(gpu, G=G, mode=3, fused=int(fused)), census        # the packed walk took fresh rows ...
        mode = 1                                                       # ... and the row-at-a-time walk the others
    for ps in ((0,) if ballot_mode == 0 else (1, 2)):
        for form in ("solo", "grid"):
            assert cells(gpu, G=G, mode=mode, ps=ps, fused=int(fused), form=form), (ps, form, census)
    assert all(k[0] == G for k in census["cells"]), census
    gpu.close()


# ---------------------------------------------------------------------------------------------------------------------
# the steady front pass and the row records (dense G = 64, a ballot per cell)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,base", [(129, "top"), (256, "top"), (256, "24"), (129, "29")])
def test_steady_rows_and_their_records(fa, oracle, R, base):
    kw = dict(num_slots=4096, num_replicas=R, f=(R - 1) // 2, ballot_mode=1, tally_ways=8)
    seen = {}

    def audit(gpu):
        seen["rows"] = gpu.vote_summary_audit()
        seen["ballots"] = gpu.ballot_summary_audit()

    gpu = run_lifted(fa, oracle, kw, RC.records_script(R), base, before_readback=audit)
    fresh, as_cells, compact = seen["rows"]
    # every row went compact in the dense rounds 7 and 8 and stayed so through the equal-round re-vote; the last batch's
    # 100 rows Nack in every cell, which writes their records out into cells
    assert (fresh, as_cells, compact) == (0, 100, 3996), seen
    uniform, mixed, bad = seen["ballots"]
    assert bad == 0 and uniform == 4096, seen                                    # every ballot row uniform (in round 8)
    for ps in (1, 2):
        assert cells(gpu, G=64, mode=0, ps=ps, fused=1, form="grid"), gpu.vote_launch_census()
    assert cells(gpu, G=64, mode=1, fused=1)
    gpu.close()


# ---------------------------------------------------------------------------------------------------------------------
# Phase1a and the deferred fold: device-resident steps
# ---------------------------------------------------------------------------------------------------------------------
def play_on_device(ctx, script):
    """run_script through the _dev entry points, nothing read back until the end: folds stay pending between steps"""
    import torch

    dev = torch.device("cuda:0")
    d = lambda a, view=None: torch.from_numpy(np.ascontiguousarray(a) if view is None else np.ascontiguousarray(a).view(view)).to(dev)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    held = []
    for op in script:
        if op[0] == "phase1a":
            _, g, rnd, wm, tgt = op
            pb, nb = (torch.zeros(4, dtype=torch.int64, device=dev) for _ in range(2))
            ctx.acceptor_phase1a_dev(g, rnd, wm, None if tgt is None else d(tgt, np.int64), pb, nb)
            held.append(("phase1a", pb, nb))
        elif op[0] == "fused":
            _, slot, rr, val, tgt = op
            n = len(slot)
            o = [torch.zeros(n, dtype=torch.uint8, device=dev)] + [torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(3)]
            ctx.phase2_fused_dev(d(slot), d(rr), d(val), None if tgt is None else d(tgt, np.int64), *o)
            held.append(("fused",) + tuple(o))
        else:
            raise ValueError(op[0])
    st = ctx.sync()
    out = []
    for h in held:
        if h[0] == "phase1a":
            out.append(("phase1a", st, h[1].cpu().numpy().view(np.uint64), h[2].cpu().numpy().view(np.uint64)))
        elif h[0] == "fused":
            out.append(("fused", st) + tuple(t.cpu().numpy() for t in h[1:]))
    return out


@pytest.mark.parametrize("R,split,base", [(3, False, "top"), (17, False, "top"), (200, False, "top"), (17, True, "top"),
                                          (200, True, "top"), (200, False, "29")])
def test_phase1a_and_the_deferred_fold(fa, oracle, monkeypatch, R, split, base):
    """fused steps of several workgroups back to back with a ballot per cell (FPX_F_TRUSTED): each step's fold rides in or
    behind the next launch; Phase1a's arrive while a fold is pending and decide by the launch's bound (k_p1a_fast) or,
    with FPX_P1A_SPLIT=1, by the three launches.  The script's last step is read back with its fold still pending: flushed
    alone.  max_voted, promised and the ballots are in the snapshot compared with the oracle and the unlifted run.
    Which Phase1a path ran shows in the fates of the six steps' folds: k_p1a_fast leaves a pending fold alone, the split
    path launches it first.  Steps 1, 2 and 4 are followed by a Phase1a, steps 3 and 5 by the next step, step 6 by the
    readback.  Without FPX_P1A_SPLIT only the Phase1a with a watermark above the earlier ones (q + 1, behind step 4: the
    split path by itself) and the readback flush a fold: 2 flushed, 4 ride with the next vote launch; with it 4 and 2"""
    monkeypatch.delenv("FPX_NO_DEFER_FINALIZE", raising=False)
    if split:
        monkeypatch.setenv("FPX_P1A_SPLIT", "1")
    else:
        monkeypatch.delenv("FPX_P1A_SPLIT", raising=False)
    kw = dict(num_slots=8192, num_replicas=R, f=R // 2, ballot_mode=1, tally_ways=8)
    gpu = run_lifted(fa, oracle, kw, RC.phase1a_script(R), base, flags=fa.FPX_F_TRUSTED, play=play_on_device)
    G = RC.lanes(R)
    census = gpu.vote_launch_census()
    count = lambda form: sum(cells(gpu, G=G, fused=1, form=form).values())
    riding = "fold_carried" if G in (1, 64) else "fold_behind"
    assert count(riding) == (2 if split else 4) and count("fold_flushed") == (4 if split else 2), census
    assert count("fin") == (count(riding) if G in (1, 64) else 0) and count("grid") + count("fin") == 6, census
    gpu.close()


# ---------------------------------------------------------------------------------------------------------------------
# tally keys
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ways", [1, 8])
@pytest.mark.parametrize("R,base", [(5, "top"), (200, "top"), (5, "29")])
def test_tally_keys(fa, oracle, R, ways, base):
    """several live rounds of one slot up to MAX_ROUND, a Done key there, fpx_proxy_forget and the same (slot, round)
    unknown afterwards; with one way per slot the rounds follow each other, each forgotten before the next"""
    kw = dict(num_slots=1024, num_replicas=R, f=R // 2, tally_ways=ways)
    script = RC.tally_script(R, ways)
    gpu = run_lifted(fa, oracle, kw, script, base)
    vmap, b = W.ValueMap(), W.lift_bases(script)[base]
    out = W.run_script(oracle.System(oracle.make_config(**kw)), W.lift_script(script, b, vmap))
    assert [o[1] for o in out if o[0] == "phase2b"][-2] == UNKNOWN
    assert all(o[1] == 0 for o in out if o[0] == "open")
    # K2 has no census; the K1 launches of the script are pinned to their template
    census, G = gpu.vote_launch_census(), RC.lanes(R)
    launches = lambda mode: sum(cells(gpu, G=G, mode=mode, ps=0, fused=0, form=f).get((G, mode, 0, 0, f), 0) for f in ("solo", "grid"))
    assert {k[:4] for k in census["cells"]} == {(G, 1, 0, 0), (G, 0, 0, 0)}, census
    assert launches(1) == 5 and launches(0) == 1, census         # five Phase2a batches with target masks, one dense
    gpu.close()


def fold_rows(acc, slot, rnd):
    """per-acceptor Phase2b's as one row per (slot, round) in order of first appearance (include/fpx.h, the contract of
    fpx_proxy_phase2b_msgs): (index of the first message, slot, round, 4 words)"""
    rows, at = [], {}
    for i, (a, s, r) in enumerate(zip(acc, slot, rnd)):
        key = (int(s), int(r))
        if key not in at:
            at[key] = len(rows)
            rows.append([i, key[0], key[1], np.zeros(4, np.uint64)])
        rows[at[key]][3][a >> 6] |= np.uint64(1 << (a & 63))
    return rows


@pytest.mark.parametrize("form", ["host", "dev"])
def test_per_message_phase2bs_at_the_top_rounds(fa, oracle, form):
    """fpx_proxy_phase2b_msgs for rounds MAX_ROUND - 1 and MAX_ROUND of the same slots in mixed order, with duplicates:
    = the rows of the burst handed to the oracle's handlePhase2b, each outcome at its row's first message; and the lift
    of what a second context answers at rounds 0 and 1"""
    import torch

    S, R, n_slots = 512, 9, 40
    kw = dict(num_slots=S, num_replicas=R, f=4, tally_ways=8)
    rng = np.random.default_rng(3)
    vmap, b = W.ValueMap(), W.MAX_ROUND - 1
    slots = (np.arange(n_slots) * 5 + 1).astype(np.int32)
    acc, slot, rnd = (x.ravel() for x in np.meshgrid(np.arange(R), slots, np.arange(2), indexing="ij"))
    keep = rng.random(len(acc)) < 0.7                      # some rows stay below the quorum of 5
    order = rng.permutation(np.concatenate([np.nonzero(keep)[0], np.nonzero(keep)[0][::7]]))     # duplicates too
    acc, slot, rnd = acc[order].astype(np.int32), slot[order].astype(np.int32), rnd[order].astype(np.int32)
    results = {}
    for name, base in (("lifted", b), ("plain", 0)):
        lift = (lambda v: vmap(v)) if base else W.identity_values
        gpu, ref = fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))
        for be in (gpu, ref):
            for r in (0, 1):
                st, new = be.proxy_open(slots, RC.whole(n_slots, r + base), lift(W.steady_values(slots) + r))
                assert st == 0 and new.all()
        rr = (rnd + base).astype(np.int32)
        if form == "host":
            got = gpu.proxy_phase2b_msgs(acc, slot, rr)
        else:
            dev = torch.device("cuda:0")
            gpu.set_stream(torch.cuda.current_stream().cuda_stream)
            d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            ch = torch.zeros(len(acc), dtype=torch.uint8, device=dev)
            cr, cv = (torch.full((len(acc),), -7, dtype=torch.int32, device=dev) for _ in range(2))
            gpu.proxy_phase2b_msgs_dev(d(acc), d(slot), d(rr), newly_chosen=ch, chosen_round=cr, chosen_value=cv)
            got = (gpu.sync(), ch.cpu().numpy(), cr.cpu().numpy(), cv.cpu().numpy())
        rows = fold_rows(acc, slot, rr)
        st, ch, cr, cv = ref.proxy_phase2b(np.array([x[1] for x in rows], np.int32), np.array([x[2] for x in rows], np.int32),
                                           np.stack([x[3] for x in rows]))
        want = [np.zeros(len(acc), np.uint8), np.full(len(acc), -1, np.int32), np.full(len(acc), -1, np.int32)]
        first = np.array([x[0] for x in rows])
        want[0][first], want[1][first], want[2][first] = ch, cr, cv
        assert got[0] == st == 0 and 0 < ch.sum() < len(rows)
        for x, y in zip(got[1:], want):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
        W.assert_same_state(gpu, ref, tally_slots=slots)
        results[name] = (got, {int(s): gpu.read_tally(int(s)) for s in slots})
        assert not gpu.vote_launch_census()["cells"]          # (K2 alone: no vote launch, and K2 has no census)
        gpu.close()
    (lo, lt), (po, pt) = results["lifted"], results["plain"]
    np.testing.assert_array_equal(lo[1], po[1])
    np.testing.assert_array_equal(lo[2], W.lift_rounds(po[2], b))
    np.testing.assert_array_equal(lo[3], W.lift_values(po[3], po[1] == 1, vmap))
    assert lt == {s: W.lift_tally(t, b, vmap) for s, t in pt.items()}
    assert max(r for t in lt.values() for r, _, _, _ in t) == W.MAX_ROUND


# ---------------------------------------------------------------------------------------------------------------------
# Mencius noop ranges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,base", [("leader-group-major", "top"), ("slot-major", "top"), ("leader-group-major", "29"),
                                         ("slot-major", "24")])
def test_noop_ranges(fa, oracle, monkeypatch, layout, base):
    """the range shapes dense, with target masks and after a competing Phase1a, fused and in the three unfused calls (the
    proxy leader's range tally among them); a length-one range next to the single-slot key of the same (slot, round) in
    both orders; garbage collection (a rehash) of a table holding such entries, and 900 ranges after it (four launches
    in place of the chain)"""
    monkeypatch.delenv("FPX_SLOT_MAJOR", raising=False)
    g = RC.range_geometry()
    S, script = RC.range_script()
    kw = dict(num_slots=S, num_replicas=g["R"], num_groups=g["A"], num_leader_groups=g["L"], f=g["f"], tally_ways=8)
    flags = fa.FPX_F_SLOT_MAJOR_ROWS if layout == "slot-major" else 0
    gpu = run_lifted(fa, oracle, kw, script, base, flags=flags, keep_noop=True)
    census = gpu.range_launch_census()
    fill = "fill_lg" if layout == "leader-group-major" else "fill_sweep"
    for form in ("chain", "steps", fill, "open_only", "acceptors_only", "tally_only", "rehash"):
        assert census[form] > 0, (form, census)
    assert census["rehash"] == 2 and census["band"] == 0, census
    gpu.close()


def test_band_at_the_top_round(fa, oracle, monkeypatch):
    """fpx_mencius_band_fused_dev with independent halves in round MAX_ROUND: 1024 commands and 256 ranges, the range chain
    as the vote kernel's first workgroup (k_phase2_band); against the oracle running the halves one after the other, and
    against the same step in round 0"""
    import torch

    monkeypatch.delenv("FPX_SLOT_MAJOR", raising=False)
    monkeypatch.delenv("FPX_BAND_SERIAL", raising=False)
    L, rows, R, n_ranges = 64, 64, 3, 256
    S = L * rows
    kw = dict(num_slots=S, num_replicas=R, num_groups=1, num_leader_groups=L, f=1, tally_ways=4)
    vmap = W.ValueMap(keep_noop=True)
    slot, start, end = RC.RB.band_halves(L, rows, n_ranges)
    tm = RC.RB.target_masks(n_ranges, 1, R, 1)
    got = {}
    for base in (W.MAX_ROUND, 0):
        lift = vmap if base else W.identity_values
        gpu, ref = fa.Context(fa.make_config(flags=fa.FPX_F_TRUSTED, **kw)), oracle.System(oracle.make_config(**kw))
        gpu.set_stream(torch.cuda.current_stream().cuda_stream)
        rr, rnd, val = RC.whole(len(slot), base), RC.whole(n_ranges, base), lift(W.steady_values(slot))
        st, cmd, rng_ = W.band_on_device(fa, gpu, ("fused", slot, rr, val, None), ("ranges", start, end, rnd, tm), True)
        b1, b2 = ref.phase2_fused(slot, rr, val, None), ref.noop_ranges_fused(start, end, rnd, tm)
        assert st == b1[0] == b2[0] == 0 and b1[1].all() and 0 < b2[5].sum() < n_ranges
        for x, y in zip(cmd, b1[1:]):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(rng_, b2[1:]):
            np.testing.assert_array_equal(x, np.asarray(y).reshape(x.shape))
        W.assert_same_state(gpu, ref, tally_slots=slot[::37])
        np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
        for key in zip(start[::11].tolist(), end[::11].tolist(), rnd[::11].tolist()):
            a, b = gpu.read_range_tally(*key), ref.read_range_tally(*key)
            assert a[0] == b[0]
            np.testing.assert_array_equal(a[1], b[1])
        assert gpu.band_merged_steps() == 1 and gpu.range_launch_census()["band"] == 1
        assert cells(gpu, G=1, mode=0, ps=0, fused=1, form="band"), gpu.vote_launch_census()
        got[base] = (cmd, rng_, W.snapshot(gpu))
        gpu.close()
    (cmd, rng_, snap), (pcmd, prng, psnap) = got[W.MAX_ROUND], got[0]
    want = W.lift_outputs([("fused", 0) + tuple(pcmd), ("ranges", 0) + tuple(prng)], W.MAX_ROUND, vmap)
    W.assert_same_outputs([("fused", 0) + tuple(cmd), ("ranges", 0) + tuple(rng_)], want)
    W.assert_same_snapshot(snap, W.lift_snapshot(psnap, W.MAX_ROUND, vmap))


# ---------------------------------------------------------------------------------------------------------------------
# recovery and the read path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,base", [(5, "top"), (200, "top"), (17, "24"), (200, "29")])
def test_recovery_scan_and_replica_log(fa, oracle, R, base):
    """fpx_leader_phase1b_scan over votes up to MAX_ROUND: best round and value per slot, negative values and -1 with a
    real vote (the round says there is one); Phase1b.info of single acceptors; the replica's log fed with negative values"""
    kw = dict(num_slots=2048, num_replicas=R, f=(R - 1) // 2, tally_ways=8)
    gpu = run_lifted(fa, oracle, kw, RC.recovery_script(R), base)
    # the scan and the log kernels have no census; the four K3 launches that cast the votes are pinned to their template
    census, G = gpu.vote_launch_census(), RC.lanes(R)
    assert all(k[:4] == (G, 1, 0, 1) for k in census["cells"]), census
    assert sum(cells(gpu, form="solo").values()) + sum(cells(gpu, form="grid").values()) == 4 and cells(gpu, form="grid"), census
    gpu.close()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_recovery_from_phase1b_messages(fa, oracle, form):
    """fpx_leader_phase1b_msgs(_dev) in round MAX_ROUND over Phase1b messages whose records carry vote rounds up to
    MAX_ROUND and negative values (what the oracle's acceptors report after the lifted votes), a message of round
    MAX_ROUND - 1 among them (ignored): best round and value per slot equal to the plain model of Leader.handlePhase1b
    (tests/leader_phase1b_model.py), and to the lift of the same burst in small rounds"""
    import torch

    from tests import leader_phase1b_model as M

    R, f, wm = 5, 2, 37
    kw = dict(num_slots=2048, num_replicas=R, f=f, tally_ways=8)
    votes = [op for op in RC.recovery_script(R) if op[0] in ("phase1a", "fused")]
    vmap, b = W.ValueMap(), W.lift_bases(votes)["top"]
    geo = M.Geometry(num_groups=1, num_leader_groups=1, f=f, total=R)
    got = {}
    for base, script in ((b, W.lift_script(votes, b, vmap)), (0, votes)):
        ref = oracle.System(oracle.make_config(**kw))
        W.run_script(ref, script)
        leader_round = W.script_rounds(script)[-1]
        info = lambda a: [(int(x), int(y), int(z)) for x, y, z in zip(*ref.acceptor_phase1b_info(0, a, wm))]
        msgs = [M.Msg(round=leader_round - 1, group=0, acceptor=0, info=info(0))] + \
            [M.Msg(round=leader_round, group=0, acceptor=a, info=info(a)) for a in (4, 1, 3)]
        want = M.handle_burst(geo, leader_round, wm, msgs)
        assert want.status == 0 and want.complete == 1 and want.decided_at == 3
        gpu = fa.Context(fa.make_config(**kw))
        arrays = M.flatten(msgs)
        if form == "host":
            st, res = gpu.leader_phase1b_msgs(leader_round, wm, **arrays)
        else:
            dev = torch.device("cuda:0")
            gpu.set_stream(torch.cuda.current_stream().cuda_stream)
            d = {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
            result = torch.full((fa._lib.FPX_P1B_RESULT_WORDS,), -1, dtype=torch.int64, device=dev)
            outs = [torch.full((want.count,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
            held = torch.zeros((1, 4), dtype=torch.int64, device=dev)
            gpu.leader_phase1b_msgs_dev(leader_round, wm, result=result, cap=want.count, out_slot=outs[0], safe_round=outs[1],
                                        safe_value=outs[2], held_bits=held, **d)
            st = gpu.sync()
            res = gpu._p1b_result(result.cpu().numpy(), *[o.cpu().numpy() for o in outs], held.cpu().numpy().view(np.uint64))
        assert st == 0 and (res["complete"], res["decided_at"], res["count"], res["max_slot"], res["next_slot"]) == \
            (1, want.decided_at, want.count, want.max_slot, want.next_slot)
        np.testing.assert_array_equal(res["out_slot"], want.out_slot)
        np.testing.assert_array_equal(res["safe_round"], want.safe_round)
        np.testing.assert_array_equal(res["safe_value"], want.safe_value)
        got[base] = res
        assert not gpu.vote_launch_census()["cells"]          # (the recovery kernels have no census)
        gpu.close()
    top, low = got[b], got[0]
    assert top["safe_round"].max() == W.MAX_ROUND and (top["safe_value"][top["safe_round"] >= 0] < -1).any()
    np.testing.assert_array_equal(top["safe_round"], W.lift_rounds(low["safe_round"], b))
    np.testing.assert_array_equal(top["safe_value"], W.lift_values(low["safe_value"], low["safe_round"] >= 0, vmap))


# ---------------------------------------------------------------------------------------------------------------------
# sharded: the replica-sharded step of two ranks (tests/rccl_double), its max of Nack rounds and its summed tallies
# ---------------------------------------------------------------------------------------------------------------------
def _rank_at_the_top(rank, world, so, conn, ballot_mode):
    try:
        import os
        import sys

        os.environ["FPX_RCCL_LIB"] = so          # before libfpx binds its collectives (once per process)
        from tests.test_gpu_sharding_world2 import ROOT
        sys.path.insert(0, ROOT)
        import torch
        import frankenpaxos_amd as fa
        from frankenpaxos_amd import sharding
        from oracle import pyoracle

        pyoracle.build()
        S, R = 4096, 256
        script = RC.sharded_script(S, R)          # (tests/test_round_range_cpu.py: the oracle commutes with its lift)
        vmap, b = W.ValueMap(), W.lift_bases(script)["top"]
        base, nloc = sharding.replica_shard(R, world, rank)
        mine = W.bits_from_bool(((np.arange(R) >= base) & (np.arange(R) < base + nloc))[None, :])[0]
        dev = torch.device("cuda:0")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        if rank == 0:
            uids = (fa.comm_unique_id(), fa.comm_unique_id())      # a communicator per run
            conn.send(uids)
        else:
            uids = conn.recv()
        per = S // world
        lo, hi = rank * per, (rank + 1) * per
        runs = []
        for k, ops in enumerate((W.lift_script(script, b, vmap), script)):
            whole = pyoracle.System(pyoracle.make_config(num_slots=S, num_replicas=R, f=127, ballot_mode=ballot_mode, tally_ways=8))
            want = W.run_script(whole, ops)
            gpu = fa.Context(fa.make_config(num_slots=S, num_replicas=nloc, f=127, ballot_mode=ballot_mode,
                                            replica_base=base, replicas_total=R, tally_ways=8))
            gpu.set_stream(torch.cuda.current_stream().cuda_stream)
            gpu.comm_create(uids[k], rank, world)
            got = []
            for op, w in zip(ops, want):
                if op[0] == "phase1a":
                    st, pb, nb = gpu.acceptor_phase1a(*op[1:])
                    assert st == w[1] == 0
                    np.testing.assert_array_equal(pb, w[2] & mine)           # my acceptors' bits of the group's answer
                    np.testing.assert_array_equal(nb, w[3] & mine)
                    got.append((pb, nb))
                    continue
                _, slot, rr, val, tgt, _ = op
                ch = torch.zeros(per, dtype=torch.uint8, device=dev)
                cr, cv = (torch.zeros(per, dtype=torch.int32, device=dev) for _ in range(2))
                nr = torch.zeros(S, dtype=torch.int32, device=dev)
                gpu.phase2_replica_sharded_dev(t(slot), t(rr), t(val), t(tgt.view(np.int64)), ch, cr, cv, nr)
                assert gpu.sync() == 0
                out = tuple(x.cpu().numpy() for x in (ch, cr, cv, nr))
                np.testing.assert_array_equal(out[0], w[8][lo:hi])          # my slots, tallied over ALL acceptors' votes
                np.testing.assert_array_equal(out[1], w[9][lo:hi])
                np.testing.assert_array_equal(out[2], w[10][lo:hi])
                np.testing.assert_array_equal(out[3], w[6])                 # the largest Nack round over BOTH ranks
                got.append(out)
            top = W.script_rounds(ops)[-1]
            assert (got[2][3] == top).any() and 0 < int(want[2][8].sum()) < S         # round top - 1: Nacks that carry top
            assert (got[3][1][got[3][0] == 1] == top).all() and got[3][0].any()       # round top: Chosen there
            # my acceptors' state == the matching columns of the unsharded group; my tallies == the group's, for my slots
            snap, ws = W.snapshot(gpu), W.snapshot(whole)
            for key in snap:
                np.testing.assert_array_equal(snap[key], ws[key][:, base:base + nloc], err_msg=key)
            assert snap["vote_round"].max() == top == (W.MAX_ROUND if k == 0 else 4)
            tallies = {int(s): gpu.read_tally(int(s)) for s in range(lo, hi, 97)}
            assert tallies == {s: whole.read_tally(s) for s in tallies}
            runs.append((got, snap, tallies))
            if k == 0:
                # refusals: the same bad batch on every rank.  The validation pass raises the abort flag on the device and
                # every rank still enqueues both collectives (fpx_api.hip, fpx_phase2_replica_sharded_dev: they do not
                # depend on the flag), so no rank waits for another; open and tally then apply nothing
                before = gpu.state_digest()
                slot, val = ops[3][1], ops[3][3]
                outs = (torch.zeros(per, dtype=torch.uint8, device=dev), torch.zeros(per, dtype=torch.int32, device=dev),
                        torch.zeros(per, dtype=torch.int32, device=dev), torch.zeros(S, dtype=torch.int32, device=dev))
                for bad in BAD_ROUNDS:
                    for at in (0, S // 2, S - 1):
                        rr = np.full(S, W.MAX_ROUND, np.int32)
                        rr[at] = bad
                        gpu.phase2_replica_sharded_dev(t(slot), t(rr), t(val), None, *outs)
                        assert gpu.sync() == EINVAL, (bad, at)
                        assert gpu.error_detail() == (at, int(slot[at]), bad)
                        np.testing.assert_array_equal(gpu.state_digest(), before)
            gpu.comm_destroy()
            gpu.set_stream(None)
            gpu.close()
        # the metamorphic half: the lifted run == the lift of the run in rounds 0 .. 4
        (got, snap, tallies), (pgot, psnap, ptallies) = runs
        for x, y in zip(got[:2], pgot[:2]):
            np.testing.assert_array_equal(x[0], y[0])
            np.testing.assert_array_equal(x[1], y[1])
        for x, y in zip(got[2:], pgot[2:]):
            np.testing.assert_array_equal(x[0], y[0])
            np.testing.assert_array_equal(x[1], W.lift_rounds(y[1], b))
            np.testing.assert_array_equal(x[2], W.lift_values(y[2], y[0] == 1, vmap))
            np.testing.assert_array_equal(x[3], W.lift_rounds(y[3], b))
        W.assert_same_snapshot(snap, W.lift_snapshot(psnap, b, vmap))
        assert tallies == {s: W.lift_tally(tl, b, vmap) for s, tl in ptallies.items()}
        conn.send("ok")
    except BaseException as e:  # noqa: BLE001 -- the parent reports
        import traceback
        conn.send("rank %d: %s\n%s" % (rank, e, traceback.format_exc()))


@pytest.mark.parametrize("ballot_mode", [0, 1])
def test_replica_sharded_step_at_the_top_rounds(ballot_mode):
    """two ranks (two processes, the RCCL double of tests/test_gpu_sharding_world2.py) play RC.sharded_script lifted to
    MAX_ROUND: a step in MAX_ROUND - 1 that acceptors of both ranks Nack with MAX_ROUND, then one in MAX_ROUND; Chosen
    records, the all-reduced Nack rounds, my columns of the state and my slots' tallies equal to the unsharded oracle
    group, and to the lift of the same ranks' run of the unlifted script on a second context and communicator; then a
    batch with one round outside the range, first, in the middle and last: FPX_EINVAL on every rank, nothing applied"""
    import multiprocessing as mp

    from tests.test_gpu_sharding_world2 import build_double

    so, world = build_double(), 2
    ctx = mp.get_context("spawn")
    pipes = [ctx.Pipe() for _ in range(world)]
    procs = [ctx.Process(target=_rank_at_the_top, args=(r, world, so, pipes[r][1], ballot_mode)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        assert pipes[0][0].poll(400), "rank 0 never produced the communicator ids"
        uids = pipes[0][0].recv()
        assert isinstance(uids, tuple), uids
        pipes[1][0].send(uids)
        for r in range(world):
            assert pipes[r][0].poll(600), "rank %d did not finish" % r
            msg = pipes[r][0].recv()
            assert msg == "ok", msg
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.terminate()


# ---------------------------------------------------------------------------------------------------------------------
# refusals: a batch that is valid but for one message's round
# ---------------------------------------------------------------------------------------------------------------------
def refusal_batch(n, at, bad):
    slot = (np.arange(n) * 3 + 2).astype(np.int32)
    rnd = RC.whole(n, W.MAX_ROUND)
    rnd[at] = bad
    return slot, rnd, W.steady_values(slot)


def warmed(fa, flags=0, **extra):
    """a context with state to lose: promised rounds, votes, tallies (some at MAX_ROUND)"""
    kw = dict(dict(num_slots=4096, num_replicas=9, f=4, tally_ways=8), **extra)
    gpu = fa.Context(fa.make_config(flags=flags, **kw))
    slot = np.arange(0, 4096, 2, dtype=np.int32)
    for g in range(gpu.ngroups):
        assert gpu.acceptor_phase1a(g, W.MAX_ROUND - 1)[0] == 0
    few = W.bits_from_bool(np.arange(9)[None, :].repeat(len(slot), 0) < 3)
    assert gpu.phase2_fused(slot, RC.whole(len(slot), W.MAX_ROUND - 1), W.steady_values(slot), few)[0] == 0
    return gpu


POSITIONS = {"first": 0, "middle": 300, "last": 599}


@pytest.mark.parametrize("bad", BAD_ROUNDS)
@pytest.mark.parametrize("where", sorted(POSITIONS))
def test_host_entry_points_refuse_a_round_outside_the_range(fa, where, bad):
    """fpx_phase2_fused, fpx_acceptor_phase2a, fpx_proxy_open, fpx_proxy_phase2b, fpx_proxy_phase2b_msgs: FPX_EINVAL,
    fpx_error_detail names the message, nothing applied (the digest stays).  The batch fails the min / max shortcut in
    front of the host's per-message loop and is then found by the loop; every valid batch of this file passes the
    shortcut"""
    n, at = 600, POSITIONS[where]
    gpu = warmed(fa)
    before = gpu.state_digest()
    slot, rnd, val = refusal_batch(n, at, bad)
    all_bits = W.bits_from_bool(np.ones((n, 9), bool))
    calls = {"fused": lambda: gpu.phase2_fused(slot, rnd, val),
             "phase2a": lambda: gpu.acceptor_phase2a(slot, rnd, val),
             "open": lambda: gpu.proxy_open(slot, rnd, val),
             "phase2b": lambda: gpu.proxy_phase2b(slot, rnd, all_bits),
             "phase2b_msgs": lambda: gpu.proxy_phase2b_msgs(np.zeros(n, np.int32), slot, rnd)}
    for name, call in calls.items():
        assert call()[0] == EINVAL, name
        assert gpu.error_detail() == (at, int(slot[at]), bad), name
        np.testing.assert_array_equal(gpu.state_digest(), before, err_msg=name)
    gpu.close()


@pytest.mark.parametrize("bad", BAD_ROUNDS)
@pytest.mark.parametrize("where", sorted(POSITIONS))
def test_device_entry_points_refuse_a_round_outside_the_range(fa, where, bad):
    """the _dev forms on a context that validates its batches: FPX_EINVAL from fpx_sync, nothing applied"""
    import torch

    n, at = 600, POSITIONS[where]
    gpu = warmed(fa)
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    before = gpu.state_digest()
    dev = torch.device("cuda:0")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    slot, rnd, val = refusal_batch(n, at, bad)
    ds, dr, dv = d(slot), d(rnd), d(val)
    bits = d(W.bits_from_bool(np.ones((n, 9), bool)).view(np.int64))
    acc = torch.zeros(n, dtype=torch.int32, device=dev)
    calls = {"fused": lambda: gpu.phase2_fused_dev(ds, dr, dv),
             "phase2a": lambda: gpu.acceptor_phase2a_dev(ds, dr, dv),
             "open": lambda: gpu.proxy_open_dev(ds, dr, dv),
             "phase2b": lambda: gpu.proxy_phase2b_dev(ds, dr, bits),
             "phase2b_msgs": lambda: gpu.proxy_phase2b_msgs_dev(acc, ds, dr)}
    for name, call in calls.items():
        call()
        assert gpu.sync() == EINVAL, name
        assert gpu.error_detail() == (at, int(slot[at]), bad), name
        np.testing.assert_array_equal(gpu.state_digest(), before, err_msg=name)
    gpu.close()


@pytest.mark.parametrize("bad", BAD_ROUNDS)
def test_submit_refuses_a_round_outside_the_range(fa, bad):
    """fpx_phase2_fused_submit / _wait on page-locked arrays: FPX_EINVAL from wait, nothing applied"""
    import ctypes as C

    n = 600
    gpu = warmed(fa)
    before = gpu.state_digest()
    L = fa.lib()
    for at in POSITIONS.values():
        slot, rnd, val = refusal_batch(n, at, bad)
        pins = {k: fa.PinnedArray((n,), dt) for k, dt in (("slot", np.int32), ("rnd", np.int32), ("val", np.int32), ("ch", np.uint8),
                                                           ("cr", np.int32), ("cv", np.int32), ("nr", np.int32))}
        pins["slot"].array[:], pins["rnd"].array[:], pins["val"].array[:] = slot, rnd, val
        p = lambda a: a.ctypes.data
        ticket = C.c_int32(-1)
        st = L.fpx_phase2_fused_submit(gpu._h, n, p(pins["slot"].array), p(pins["rnd"].array), p(pins["val"].array), None,
                                       p(pins["ch"].array), p(pins["cr"].array), p(pins["cv"].array), p(pins["nr"].array),
                                       C.byref(ticket))
        if st == 0:
            st = L.fpx_phase2_fused_wait(gpu._h, ticket.value)
        assert st == EINVAL
        assert gpu.error_detail() == (at, int(slot[at]), bad)
        np.testing.assert_array_equal(gpu.state_digest(), before)
        for a in pins.values():
            a.free()
    gpu.close()


@pytest.mark.parametrize("bad", BAD_ROUNDS)
def test_range_and_scalar_entry_points_refuse_a_round_outside_the_range(fa, bad):
    """the noop-range entry points (the fused one also as _dev) and the per-message tally of a Mencius proxy leader (host
    and _dev) with a bad round first, in the middle and last; and the scalar round of fpx_acceptor_phase1a, _dev,
    fpx_acceptor_phase1 and fpx_leader_phase1b_msgs, which is refused at once with nothing enqueued (include/fpx.h
    defines no fpx_error_detail for that)"""
    import torch

    dev = torch.device("cuda:0")
    gpu = warmed(fa, num_leader_groups=4)
    before = gpu.state_digest()
    n = 60
    start = (np.arange(n) * 64 + np.arange(n) % 4).astype(np.int32)
    end = (start + 9).astype(np.int32)
    for at in (0, n // 2, n - 1):
        rnd = RC.whole(n, W.MAX_ROUND)
        rnd[at] = bad
        for name, call in (("fused", lambda: gpu.noop_ranges_fused(start, end, rnd)),
                           ("acceptors", lambda: gpu.acceptor_phase2a_noop_ranges(start, end, rnd)),
                           ("open", lambda: gpu.proxy_open_noop_ranges(start, end, rnd)),
                           ("tally", lambda: gpu.proxy_phase2b_noop_ranges(start, end, rnd, np.zeros((n, 1, 4), np.uint64)))):
            assert call()[0] == EINVAL, name
            assert gpu.error_detail() == (at, int(start[at]), bad), name
            np.testing.assert_array_equal(gpu.state_digest(), before, err_msg=name)
        # the fused ranges as _dev, and the per-message tally of a Mencius proxy leader (the ranges' first slots as
        # Phase2b's of acceptor 0) in both forms
        gpu.set_stream(torch.cuda.current_stream().cuda_stream)
        ds, de, dr = (torch.from_numpy(a).to(dev) for a in (start, end, rnd))
        acc = torch.zeros(n, dtype=torch.int32, device=dev)
        for name, call in (("fused_dev", lambda: gpu.noop_ranges_fused_dev(ds, de, dr)),
                           ("msgs_dev", lambda: gpu.mencius_proxy_phase2b_msgs_dev(acc, ds, dr))):
            call()
            assert gpu.sync() == EINVAL, name
            assert gpu.error_detail() == (at, int(start[at]), bad), name
            np.testing.assert_array_equal(gpu.state_digest(), before, err_msg=name)
        gpu.set_stream(None)
        assert gpu.mencius_proxy_phase2b_msgs(np.zeros(n, np.int32), start, rnd)[0] == EINVAL
        assert gpu.error_detail() == (at, int(start[at]), bad)
        np.testing.assert_array_equal(gpu.state_digest(), before)
    # the scalar round of Phase1a in its three forms
    assert gpu.acceptor_phase1a(0, bad)[0] == EINVAL
    with pytest.raises(fa.FpxError) as err:
        gpu.acceptor_phase1(bad)
    assert err.value.status == EINVAL
    with pytest.raises(fa.FpxError) as err:
        gpu.acceptor_phase1a_dev(0, bad)
    assert err.value.status == EINVAL
    # the scalar round of the recovery from Phase1b messages
    one = np.zeros(1, np.int32)
    st, res = gpu.leader_phase1b_msgs(bad, 0, one + bad, one, np.zeros(2, np.int64), one[:0], one[:0], one[:0], cap=4)
    assert st == EINVAL
    np.testing.assert_array_equal(gpu.state_digest(), before)
    gpu.close()


@pytest.mark.parametrize("bad", BAD_ROUNDS)
def test_band_refuses_a_round_outside_the_range(fa, bad):
    """fpx_mencius_band_fused_dev on a context that validates its batches: 600 commands of leader groups 0 and 1 and 60
    ranges of leader groups 2 and 3 (independent halves), the bad round in either half, first, in the middle and last.
    The step is fpx_phase2_fused_dev followed by fpx_noop_ranges_fused_dev "with exactly their outputs and errors"
    (include/fpx.h): a bad command refuses the step before anything is applied; a bad range refuses the ranges, behind
    commands that were valid and have been applied -- the state is then that of a context which got the commands alone"""
    gpu, twin = warmed(fa, num_leader_groups=4), warmed(fa, num_leader_groups=4)
    before = gpu.state_digest()
    np.testing.assert_array_equal(twin.state_digest(), before)
    j = np.arange(600)
    slot = (4 * j + j % 2).astype(np.int32)
    k = np.arange(60)
    start = (64 * k + 2 + k % 2).astype(np.int32)
    end = (start + 9).astype(np.int32)
    tm = RC.RB.target_masks(60, 1, 9, 4)
    val = W.steady_values(slot)
    for at in (0, 300, 599):
        rr = RC.whole(600, W.MAX_ROUND)
        rr[at] = bad
        st, _, _ = W.band_on_device(fa, gpu, ("fused", slot, rr, val, None), ("ranges", start, end, RC.whole(60, W.MAX_ROUND), tm), True)
        assert st == EINVAL, at
        assert gpu.error_detail() == (at, int(slot[at]), bad), at
        np.testing.assert_array_equal(gpu.state_digest(), before, err_msg="commands %d" % at)
    assert twin.phase2_fused(slot, RC.whole(600, W.MAX_ROUND), val)[0] == 0
    commands_alone = twin.state_digest()
    assert (commands_alone != before).any()
    for at in (0, 30, 59):            # (from the second time on the commands are known and change nothing)
        rnd = RC.whole(60, W.MAX_ROUND)
        rnd[at] = bad
        st, cmd, rng_ = W.band_on_device(fa, gpu, ("fused", slot, RC.whole(600, W.MAX_ROUND), val, None), ("ranges", start, end, rnd, tm), True)
        assert st == EINVAL, at
        assert gpu.error_detail() == (at, int(start[at]), bad), at
        np.testing.assert_array_equal(gpu.state_digest(), commands_alone, err_msg="ranges %d" % at)
        assert not rng_[3].any() and not rng_[4].any() and not rng_[0].any()         # no range opened, chosen or voted
        assert gpu.read_range_tally(int(start[0]), int(end[0]), W.MAX_ROUND)[0] == 0
    gpu.close(), twin.close()


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("bad", BAD_ROUNDS)
def test_phase1b_messages_refuse_a_vote_round_outside_the_range(fa, form, bad):
    """fpx_leader_phase1b_msgs(_dev): five acceptors' messages complete the quorum (f = 4 of 9), a sixth follows; one
    record's vote_round is bad, in the first, a middle or the last message the result uses: FPX_EINVAL, fpx_error_detail
    names the message (the lowest offending index is all it defines), nothing is applied"""
    import torch

    from tests import leader_phase1b_model as M

    gpu = warmed(fa)
    before = gpu.state_digest()
    dev = torch.device("cuda:0")
    for at in (0, 2, 4):
        msgs = [M.Msg(round=W.MAX_ROUND, group=0, acceptor=a, info=[(s, W.MAX_ROUND - a, 7 * s) for s in (1, 2, 3)]) for a in range(6)]
        msgs[at].info[1] = (2, bad, 14)
        want = M.handle_burst(M.Geometry(num_groups=1, num_leader_groups=1, f=4, total=9), W.MAX_ROUND, 0, msgs)
        assert want.status == EINVAL and want.err_index == at
        arrays = M.flatten(msgs)
        if form == "host":
            st, res = gpu.leader_phase1b_msgs(W.MAX_ROUND, 0, cap=8, **arrays)
        else:
            gpu.set_stream(torch.cuda.current_stream().cuda_stream)
            d = {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
            result = torch.full((fa._lib.FPX_P1B_RESULT_WORDS,), -1, dtype=torch.int64, device=dev)
            outs = [torch.full((8,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
            gpu.leader_phase1b_msgs_dev(W.MAX_ROUND, 0, result=result, cap=8, out_slot=outs[0], safe_round=outs[1],
                                        safe_value=outs[2], **d)
            st = gpu.sync()
            assert all((o.cpu().numpy() == -7).all() for o in outs)          # nothing written
            gpu.set_stream(None)
        assert st == EINVAL, at
        assert gpu.error_detail()[0] == at
        np.testing.assert_array_equal(gpu.state_digest(), before)
    gpu.close()
