"""The vote kernel's launch forms at every lanes-per-slot width, against the CPU oracle bit for bit -- and, through the
context's census of its vote launches (include/fpx.h, fpx_vote_launch_census), proof that each case ran the form it
is about.

Below G = 64 a chunk is 64 messages, so a batch of at most 512 messages is one workgroup that finalises itself
(`solo`); the per-workgroup maxima rows, their two halves and the fold over them only run in bigger launches.  The
cells (G, mode, ps, fused, form) this file reaches, by width:
  G = 2, 4, 8, 16, 32   mode 0 / 1 / 2 (dense, target masks, FPX_F_SCATTERED_TARGETS) x ps 0 / 1 / 2 x fused 0 / 1 x
                        form solo / grid (k_phase2 has no k_phase2_fin form at these widths), the grid also capped at
                        max_grid; with ps 1 / 2 fused, the fold left pending and launched behind the next vote launch;
                        at G <= 8, mode 0 / ps 0 / fused 1 also as the Mencius band (k_phase2_band)
  G = 1, 64 (controls)  as above plus form fin (k_phase2_fin, the fold of the launch before in the grid)
test_matrix_cells_cover_every_width checks that the case list below reaches every one of the solo / grid cells.
"""
import itertools

import numpy as np
import pytest

from tests import workloads as W

pytestmark = pytest.mark.gpu

WIDTHS = {2: (5, 8), 4: (9, 16), 8: (17, 32), 16: (33, 64), 32: (65, 128)}
DELIVERY = {"dense": 0, "masks": 1, "scattered": 2}


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()  # raises if libfpx.so is missing: no fallback
    return frankenpaxos_amd


def lanes(R):
    G = 1
    while 4 * G < R:
        G *= 2
    return G


def cells(ctx, **want):
    """the census cells of ctx that match every given coordinate (G, mode, ps, fused, form)"""
    keys = ("G", "mode", "ps", "fused", "form")
    return {k: v for k, v in ctx.vote_launch_census()["cells"].items()
            if all(k[keys.index(name)] == val for name, val in want.items())}


shaped = W.shaped   # (shared with tests/round_range_cases.py)


def steady_ops(kind, lo, n, R, rng, delivery):
    """a batch of fresh slots [lo, lo + n) in round 0 with no Phase1a before it: with a ballot per cell no lazy promise is
    outstanding yet (ps 1)"""
    slot = np.arange(lo, lo + n, dtype=np.int32)
    rr = np.zeros(n, np.int32)
    tgt = None if delivery == "dense" else W.bits_from_bool(W.random_subsets(rng, n, R, max(1, R // 2), R))
    if kind == "fused":
        return [("fused", slot, rr, W.steady_values(slot), tgt)]
    return [("k1k2", slot, rr, W.steady_values(slot), tgt, rng.random(n) < 0.1)]


def run_case(fa, oracle, R, ballot_mode, delivery, fused, per, epochs, seed, num_groups=1, solo_every=2):
    solo_n = 32 if lanes(R) == 64 else 400     # (at G = 64 a small batch takes chunks of 4 messages)
    S_adv = per * epochs
    S = S_adv + 4096
    flags = fa.FPX_F_SCATTERED_TARGETS if delivery == "scattered" else 0
    kw = dict(num_slots=S, num_replicas=R, num_groups=num_groups, quorum_kind=1, ballot_mode=ballot_mode, tally_ways=8)
    gpu, ref = fa.Context(fa.make_config(flags=flags, **kw)), oracle.System(oracle.make_config(**kw))
    rng = np.random.default_rng(seed)
    kind = "fused" if fused else "k1k2"
    script = steady_ops(kind, S_adv, 3000, R, rng, delivery) + steady_ops(kind, S_adv + 3000, solo_n, R, rng, delivery)
    script += shaped(W.adversarial_script(S_adv, R, R // 2 + 1, seed, epochs=epochs, fused=fused, ngroups=num_groups),
                     delivery, solo_every, solo_n)
    W.assert_same_outputs(W.run_script(gpu, script), W.run_script(ref, script))
    W.assert_same_state(gpu, ref, tally_slots=range(0, S, max(1, S // 97)))
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    return gpu


def matrix():
    """pairwise over each width: both ballot modes x the three deliveries x fused / unfused, R alternating between the
    width's two edges; every case runs solo and multi-workgroup launches"""
    out = []
    for G, edges in WIDTHS.items():
        for k, (bm, dl, fu) in enumerate(itertools.product((0, 1), DELIVERY, (True, False))):
            out.append((edges[k % 2], bm, dl, fu))
    return out


def test_matrix_cells_cover_every_width():
    """(runs without a GPU under -m gpu too: it checks the case list) every (G, mode, ps, fused) of G = 2 ... 32 is
    the target of some case; ps 1 and 2 both come from a ballot-per-cell case (steady batches first, then Phase1a's)"""
    have = set()
    for R, bm, dl, fu in matrix():
        for ps in ((0,) if bm == 0 else (1, 2)):
            have.add((lanes(R), DELIVERY[dl], ps, int(fu)))
    want = set(itertools.product(WIDTHS, range(3), range(3), range(2)))
    assert want <= have, sorted(want - have)


@pytest.mark.parametrize("R,ballot_mode,delivery,fused", matrix())
def test_widths_by_forms(fa, oracle, R, ballot_mode, delivery, fused):
    """R at both edges of G = 2 ... 32: the adversarial stream (leader changes, Nacks, re-proposals, Phase1a's with partial
    targets) in batches of ~3000 messages (12 workgroups) and cut into solo launches, against the oracle; the census
    shows both forms ran in every cell the case targets"""
    G, mode = lanes(R), DELIVERY[delivery]
    gpu = run_case(fa, oracle, R, ballot_mode, delivery, fused, per=3000, epochs=6, seed=R * 8 + ballot_mode * 4 + mode)
    for ps in ((0,) if ballot_mode == 0 else (1, 2)):
        for form in ("solo", "grid"):
            assert cells(gpu, G=G, mode=mode, ps=ps, fused=int(fused), form=form), (ps, form, gpu.vote_launch_census())
    assert not cells(gpu, form="fin") and not cells(gpu, G=64) and not cells(gpu, mode=3)
    grid = sum(cells(gpu, G=G, form="grid").values())
    folds = sum(cells(gpu, G=G, form="fold_now").values()) + sum(cells(gpu, G=G, form="fold_behind").values()) + \
        sum(cells(gpu, G=G, form="fold_flushed").values())
    assert folds == grid     # every grid launch's fold ran, by itself (no context has been read with one pending)
    gpu.close()


@pytest.mark.parametrize("R,ballot_mode,fused", [(5, 0, True), (16, 1, False), (17, 0, False), (33, 1, True), (65, 0, True)])
def test_capped_grid(fa, oracle, R, ballot_mode, fused):
    """num_groups x R close to 8192 lowers max_grid (fpx_create), so that batches of 130 k - 300 k messages need more
    workgroups than the grid has: every wavefront walks several chunks, of several acceptor groups"""
    per = 131072 if lanes(R) <= 4 else 300000
    gpu = run_case(fa, oracle, R, ballot_mode, "masks", fused, per=per, epochs=2, seed=R, num_groups=8192 // R, solo_every=0)
    census = gpu.vote_launch_census()
    assert census["capped"] > 0, census
    assert census["th_lds"] > 0 if ballot_mode == 0 else census["th_lds"] == 0, census
    assert cells(gpu, G=lanes(R), mode=1, fused=int(fused), form="grid"), census
    gpu.close()


@pytest.mark.parametrize("R,ballot_mode,delivery", [(3, 1, "masks"), (4, 0, "dense"), (200, 1, "dense"), (129, 0, "scattered")])
def test_controls_at_one_and_sixty_four_lanes(fa, oracle, R, ballot_mode, delivery):
    """the two widths with a k_phase2_fin form (the fold of the launch before in the grid: the device-resident steps of
    test_the_fold_launched_behind_the_next_vote_launch_is_not_observable reach it), through the same matrix"""
    G, mode = lanes(R), DELIVERY[delivery]
    gpu = run_case(fa, oracle, R, ballot_mode, delivery, True, per=3000, epochs=6, seed=R)
    for form in ("solo", "grid"):
        assert cells(gpu, G=G, mode=mode, fused=1, form=form), (form, gpu.vote_launch_census())
    gpu.close()


# ---------------------------------------------------------------------------------------------------------------------
# the fold left pending at G = 2 ... 32: launched by itself behind the NEXT vote launch (enqueue_phase2), which uses the
# other half of the maxima rows; k_p1a_fast reads the pending launch's bound
# ---------------------------------------------------------------------------------------------------------------------
def deferred_script(S, R, seed):
    """the adversarial stream (Phase1a's ahead of the current round, with partial targets) with two more Phase1a's after
    every third step: a stale one (round 0, once the rounds moved on: Nacked) and a repeat of the current round with a
    watermark above 0, which passes the lazy promises made at watermark 0 (k_p1a_decide / k_p1a_sweep); plus three
    dense steps back to back at the end and one on the lowest slots behind them"""
    subsets = W.fast_subsets if R & (R - 1) == 0 else None
    base = W.adversarial_script(S - 12288, R, R // 2 + 1, seed, epochs=8, fused=True, subsets=subsets)
    out, k, rnd = [], 0, 0
    for op in base:
        out.append(op)
        if op[0] != "fused":
            continue
        rnd = int(op[2][-1])
        k += 1
        if k % 3 == 1:
            out.append(("phase1a", 0, 0, 0, None))
            out.append(("phase1a", 0, rnd, int(op[1][-1]) // 2 + 1, None))
    for j in range(3):
        slot = np.arange(S - 12288 + 4096 * j, S - 12288 + 4096 * (j + 1), dtype=np.int32)
        out.append(("fused", slot, np.full(len(slot), rnd, np.int32), W.steady_values(slot), None))
    # then the lowest slots again in the round after: this launch's maxima rows are below the pending fold's (a fold that
    # read this launch's rows in place of its own would lower maxVotedSlot)
    slot = np.arange(0, 4096, dtype=np.int32)
    out.append(("phase1a", 0, rnd + 2, 0, None))
    out.append(("fused", slot, np.full(len(slot), rnd + 2, np.int32), W.steady_values(slot), None))
    return out


@pytest.mark.parametrize("R", [3, 5, 16, 17, 64, 65, 128, 200])
def test_the_fold_launched_behind_the_next_vote_launch_is_not_observable(fa, oracle, monkeypatch, R):
    """device-resident fused steps with a ballot per cell (FPX_F_TRUSTED), more than one workgroup each, back to back,
    with Phase1a's between them while a fold is pending and read-backs between steps: at G = 2 ... 32 each step's fold
    is launched by itself behind the next step's vote launch (the two use different halves of the maxima rows; at G = 1
    and 64 with target masks too, dense steps carry it in their grid) -- every output, the acceptors' scalars and the
    digest equal those of a context that folds at once (FPX_NO_DEFER_FINALIZE=1) and the oracle's"""
    import torch

    S = 45056
    kw = dict(num_slots=S, num_replicas=R, f=R // 2, ballot_mode=1, tally_ways=8)
    script = deferred_script(S, R, 11 + R)
    dev = torch.device("cuda:0")
    d = lambda a, view=None: torch.from_numpy(np.ascontiguousarray(a) if view is None else np.ascontiguousarray(a).view(view)).to(dev)

    def run(ctx):
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        seen, outs = [], []
        for k, op in enumerate(script):
            if op[0] == "phase1a":
                _, g_, rnd, wm, tgt = op
                pb, nb = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
                ctx.acceptor_phase1a_dev(g_, rnd, wm, None if tgt is None else d(tgt, np.int64), pb, nb)
                outs.append(("phase1a", pb, nb))
            else:
                _, slot, rr, val, tgt = op
                n = len(slot)
                o = [torch.zeros(n, dtype=torch.uint8, device=dev)] + [torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
                ctx.phase2_fused_dev(d(slot), d(rr), d(val), None if tgt is None else d(tgt, np.int64), *o)
                outs.append(("fused",) + tuple(o))
                if k % 5 == 3:
                    seen.append(ctx.read_acceptor(0, R - 1)[:2])          # (promised, maxVotedSlot) between two steps
        assert ctx.sync() == 0
        return seen, [(o[0],) + tuple(t.cpu().numpy() for t in o[1:]) for o in outs]

    monkeypatch.delenv("FPX_NO_DEFER_FINALIZE", raising=False)
    a = fa.Context(fa.make_config(flags=fa.FPX_F_TRUSTED, **kw))
    seen_a, out_a = run(a)
    monkeypatch.setenv("FPX_NO_DEFER_FINALIZE", "1")
    b = fa.Context(fa.make_config(flags=fa.FPX_F_TRUSTED, **kw))
    seen_b, out_b = run(b)
    assert seen_a == seen_b
    G = lanes(R)
    behind = sum(cells(a, G=G, fused=1, form="fold_behind").values())
    assert behind >= 3, a.vote_launch_census()          # folds ran behind a later vote launch ...
    if G in (1, 64):
        assert cells(a, G=G, fused=1, form="fin") and cells(a, G=G, fused=1, form="fold_carried")
    else:
        assert not cells(a, form="fin") and not cells(a, form="fold_carried")
    assert not cells(b, form="fold_behind") and not cells(b, form="fin")
    assert cells(b, G=G, fused=1, form="fold_now")  # ... and at once on the context that does not defer
    ref = oracle.System(oracle.make_config(**kw))
    want = W.run_script(ref, script)
    assert len(want) == len(out_a) == len(out_b)
    for x, y, w in zip(out_a, out_b, want):
        if x[0] == "phase1a":
            assert w[1] == 0
            for u, v, r in zip(x[1:], y[1:], w[2:]):
                np.testing.assert_array_equal(u.view(np.uint64), np.asarray(r, np.uint64))
                np.testing.assert_array_equal(v.view(np.uint64), np.asarray(r, np.uint64))
        else:
            st, ch, cr, cv, nr = w[1:]
            assert st == 0
            chosen = np.asarray(ch).astype(bool)
            for o in (x, y):
                np.testing.assert_array_equal(o[1], ch)
                np.testing.assert_array_equal(o[2][chosen], np.asarray(cr)[chosen])
                np.testing.assert_array_equal(o[3][chosen], np.asarray(cv)[chosen])
                np.testing.assert_array_equal(o[4], nr)
    np.testing.assert_array_equal(a.state_digest(), b.state_digest())
    np.testing.assert_array_equal(a.state_digest(), ref.state_digest())
    for r in (0, R // 2, R - 1):
        assert a.read_acceptor(0, r)[:2] == b.read_acceptor(0, r)[:2] == ref.read_acceptor(0, r)[:2]
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------------
# slot-ordered batches on leader-group-major rows, walked by column (k_phase2, COLS) at G = 4 and 8
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,R", [(8, 12), (12, 16), (6, 17), (16, 32)])
def test_column_walk_at_four_and_eight_lanes(fa, oracle, row_layout, L, R):
    """period P a multiple of 4 and not (P = L, or L / 2 with every other leader group silent), lengths with a plain
    tail behind the tiles, grids of 8 / 16 workgroups and of 12 / 13; the same batches on a second context as UNALIGNED
    device views (t[1:] of a longer tensor: no column quads) -- every output, the whole state and the digest equal to
    the oracle's"""
    import torch

    S = L * 4096
    kw = dict(num_slots=S, num_replicas=R, num_groups=1, num_leader_groups=L, f=(R - 1) // 2, tally_ways=8)
    dev = torch.device("cuda:0")
    ref = oracle.System(oracle.make_config(**kw))
    ali, una = fa.Context(fa.make_config(**kw)), fa.Context(fa.make_config(**kw))
    for x in (ali, una):
        x.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(L * 7 + R)
    rounds = rng.integers(0, 3, L)

    def put(a, dtype, aligned):
        """a as a device tensor: fresh (aligned), or t[1:] of a tensor one element longer (4 / 1 bytes off for int32 /
        uint8: no column quads)"""
        t = torch.zeros(len(a) + 1, *a.shape[1:], dtype=dtype, device=dev)
        t[1:] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t[1:] if not aligned else t[1:].clone()

    def fused_dev(ctx, slots, rr, val, tm, aligned):
        m = len(slots)
        o = [put(np.zeros(m, np.uint8), torch.uint8, aligned)] + [put(np.full(m, -7, np.int32), torch.int32, aligned) for _ in range(3)]
        if not aligned:
            assert o[0].data_ptr() % 4 and o[1].data_ptr() % 16
        before = ctx.vote_launch_census()["sc_lds"]
        ctx.phase2_fused_dev(put(slots, torch.int32, aligned), put(rr, torch.int32, aligned), put(val, torch.int32, aligned),
                             None if tm is None else put(tm.view(np.int64), torch.int64, aligned), *o)
        assert ctx.sync() == 0
        return ctx.vote_launch_census()["sc_lds"] - before, [t.cpu().numpy() for t in o]

    lo = 0
    for step, n in enumerate([2048, 4096 + 37, 3000, 3333, 2048 + 64 * 3 + 5, 4096]):
        slots = np.arange(lo, lo + n, dtype=np.int32)
        lo += n - n // 3                             # the next batch re-proposes a third of this one
        if step % 3 == 2:                            # every other leader group is silent: the period halves
            slots = slots[(slots % L) % 2 == 0]
        if step == 4:
            rounds = rounds + 1
        rr = rounds[slots % L].astype(np.int32)
        val = (slots * 11 + step).astype(np.int32)
        tm = None if step % 2 == 0 else W.bits_from_bool(W.random_subsets(rng, len(slots), R, 1, R))
        if step == 3:
            script = [("k1k2", slots, rr, val, tm, rng.random(len(slots)) < 0.1)]
            want = W.run_script(ref, script)
            for x in (ali, una):
                W.assert_same_outputs(W.run_script(x, script), want)
            continue
        st, ch, cr, cv, nr = ref.phase2_fused(slots, rr, val, tm)
        assert st == 0
        chosen = np.asarray(ch).astype(bool)
        for x, aligned in ((ali, True), (una, False)):
            quads, o = fused_dev(x, slots, rr, val, tm, aligned)
            # the column quads' LDS: aligned arrays on leader-group-major rows, and only those
            assert quads == (1 if aligned and row_layout == "leader-group-major" else 0), (step, aligned)
            np.testing.assert_array_equal(o[0], ch)
            np.testing.assert_array_equal(o[1][chosen], np.asarray(cr)[chosen])
            np.testing.assert_array_equal(o[2][chosen], np.asarray(cv)[chosen])
            np.testing.assert_array_equal(o[3], nr)
    G = lanes(R)
    for x in (ali, una):
        assert cells(x, G=G, fused=1, form="grid") and cells(x, G=G, fused=0, form="grid"), x.vote_launch_census()
        W.assert_same_state(x, ref, tally_slots=range(0, S, max(1, S // 200)))
        np.testing.assert_array_equal(x.state_digest(), ref.state_digest())
    ali.close(), una.close()


# ---------------------------------------------------------------------------------------------------------------------
# the Mencius band in two launches (k_phase2_band) at G = 2, 4, 8
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [5, 8, 16, 17, 32])
def test_band_form_at_two_four_and_eight_lanes(fa, oracle, R):
    """fpx_mencius_band_fused_dev with commands (dense, more than one workgroup of them) and noop ranges, on
    leader-group-major rows: every step the range chain as the vote kernel's first workgroup -- every output of both
    halves, the digest and the acceptors' scalars equal to the oracle running the halves one after the other"""
    import torch

    from tests.test_gpu_fullsize import _band_on_device, mencius_stream

    L, epochs = 8, 8
    S = L * epochs * 1024
    kw = dict(num_slots=S, num_replicas=R, num_groups=1, num_leader_groups=L, f=(R - 1) // 2, tally_ways=4)
    with pytest.MonkeyPatch.context() as m:
        m.delenv("FPX_SLOT_MAJOR", raising=False)
        m.delenv("FPX_BAND_SERIAL", raising=False)
        gpu = fa.Context(fa.make_config(flags=fa.FPX_F_TRUSTED, **kw))
        ref = oracle.System(oracle.make_config(**kw))
        gpu.set_stream(torch.cuda.current_stream().cuda_stream)
        pending, steps = None, 0
        for op in mencius_stream(S, L, R, epochs=epochs, seed=R):
            if op[0] == "phase1a":
                a, b = gpu.acceptor_phase1a(*op[1:]), ref.acceptor_phase1a(*op[1:])
                assert a[0] == b[0] == 0
                np.testing.assert_array_equal(a[1], b[1])
                np.testing.assert_array_equal(a[2], b[2])
            elif op[0] == "fused":
                pending = op[:4] + (None,)
                assert len(op[1]) > 512
            else:
                st, cmd, rng_ = _band_on_device(fa, gpu, pending, op, independent=True)
                assert st == 0
                b1, b2 = ref.phase2_fused(*pending[1:]), ref.noop_ranges_fused(*op[1:])
                assert b1[0] == b2[0] == 0
                chosen = b1[1].astype(bool)
                np.testing.assert_array_equal(cmd[0], b1[1])
                np.testing.assert_array_equal(cmd[1][chosen], b1[2][chosen])
                np.testing.assert_array_equal(cmd[2][chosen], b1[3][chosen])
                np.testing.assert_array_equal(cmd[3], b1[4])
                for x, y in zip(rng_, b2[1:]):
                    np.testing.assert_array_equal(x, np.asarray(y).reshape(x.shape))
                steps += 1
    assert steps == epochs
    assert gpu.band_merged_steps() == epochs
    assert cells(gpu, G=lanes(R), mode=0, ps=0, fused=1, form="band") == {(lanes(R), 0, 0, 1, "band"): epochs}
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    pg, mg = gpu.read_scalars()
    pr, mr = ref.read_scalars()
    np.testing.assert_array_equal(pg, pr)
    np.testing.assert_array_equal(mg, mr)
    gpu.close()
