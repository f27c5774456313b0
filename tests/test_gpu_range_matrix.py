"""The Mencius noop-range kernels (fpx_ranges.hpp) in every launch form and range shape, against the CPU oracle bit for
bit -- and, through the context's census of its range launches (include/fpx.h, fpx_range_launch_census), proof that each
case ran the forms it is about, with exact counts, and no other.

Batches come from tests/range_batches.py (checked on the CPU by tests/test_range_batches_cpu.py).  The forms:
  chain / steps / band         who walks open -> resolve -> acceptors -> tally (k_ranges_chain, four launches, or the first
                               workgroup of k_phase2_band)
  fill_lg / fill_sweep / fill_range   k_ranges_fill_lg, k_ranges_fill_rows, k_ranges_fill
  open_only / acceptors_only / tally_only   the unfused entry points
  rehash                       fpx_proxy_forget
tests/test_range_batches_cpu.py checks, without a GPU, that the case list below reaches every form and fill branch.
"""
import itertools
import os

import numpy as np
import pytest

from tests import range_batches as RB
from tests import workloads as W

pytestmark = pytest.mark.gpu

ROWS = 144                      # rows per leader group: what span_straddlers needs at L = 2
# (L, A, R, f); the last three fill the (Q, A) combinations the first seven leave open
GEOMS = [(4, 1, 3, 1), (5, 1, 4, 1), (3, 2, 5, 2), (7, 3, 8, 3), (2, 1, 9, 4), (3, 1, 32, 15), (2, 4, 100, 49),
         (3, 2, 3, 1), (4, 1, 8, 3), (2, 2, 12, 5)]
INTERLEAVED = [(4, 1, 3, 1), (4, 1, 4, 1)]
SHAPES = ("residue", "overlap", "aligned", "straddle")
FORMS = ("chain", "steps", "band", "fill_lg", "fill_sweep", "fill_range", "tally_only", "open_only", "acceptors_only", "rehash")
# the chain's admission: n <= 2048, 5 n + 16 n A <= 36000 words of LDS, n A R <= 8192 (include/fpx.h)
CHAIN_CASES = [(1024, 1, 3, "chain"), (1025, 1, 3, "chain"), (1714, 1, 3, "chain"), (1715, 1, 3, "steps"), (2048, 1, 3, "steps"),
               (2049, 1, 3, "steps"), (972, 2, 4, "chain"), (973, 2, 4, "steps"), (1024, 1, 8, "chain"), (1025, 1, 8, "steps"),
               (400, 1, 3, "chain")]
BAND_CASES = [(256, "band"), (257, "band"), (309, "band"), (310, "chain")]


@pytest.fixture(scope="module")
def fa():
    import frankenpaxos_amd

    frankenpaxos_amd.lib()  # raises if libfpx.so is missing: no fallback
    return frankenpaxos_amd


def chain_admits(n, A, R):
    return n <= 2048 and 5 * n + 16 * n * A <= 36000 and n * A * R <= 8192


def fill_form(row_layout, S, L, R, n, flags=0):
    if row_layout == "leader-group-major" and S % L == 0 and R <= 32 and L > 1 and not flags & 4:
        return "fill_lg"
    return "fill_sweep" if n <= 1024 and L <= 2048 else "fill_range"


def ambient_layout():
    """the layout of a context made outside the row_layout fixture"""
    return "slot-major" if os.environ.get("FPX_SLOT_MAJOR") else "leader-group-major"


def shape_batches(S, L, rounds):
    return {"residue": RB.residue_batch(S, L, rounds), "overlap": RB.overlap_batch(S, L, rounds)[:3],
            "aligned": RB.aligned_runs(L, ROWS, rounds), "straddle": RB.span_straddlers(L, rounds)}


def same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for k, (x, y) in enumerate(zip(a[1:], b[1:])):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg="output %d" % k)


def expect_census(gpu, **want):
    got = gpu.range_launch_census()
    assert tuple(got) == FORMS
    assert got == dict({k: 0 for k in FORMS}, **want), got


def same_everything(gpu, ref, keys):
    """the whole acceptor state, the digest, and the tally of every distinct key"""
    W.assert_same_state(gpu, ref)
    np.testing.assert_array_equal(gpu.state_digest(), ref.state_digest())
    for s, e, r in sorted(set(keys)):
        a, b = gpu.read_range_tally(s, e, r), ref.read_range_tally(s, e, r)
        assert a[0] == b[0], (s, e, r)
        np.testing.assert_array_equal(a[1], b[1])


def keys_of(start, end, rnd):
    return [(int(s), int(e), int(r)) for s, e, r in zip(start, end, rnd)]


def voted_cells(S, L, A, R, base, start, end, rnd, vb, new):
    """vote_round [S, R] after fused calls on a fresh context, worked out from the calls' outputs alone: the acceptors
    with a vote bit, in the owned slots of the ranges this call opened; every other cell is -1"""
    vr = np.full((S, R), -1, np.int32)
    for i in np.nonzero(new)[0]:
        for s in range(int(start[i]), int(end[i]), L):
            bits = W.bool_from_bits(vb[i, (s // L) % A][None, :], 256)[0][base:base + R]
            vr[s, bits] = rnd[i]
    return vr


def run_shapes(fa, oracle, geom, S, flags, fill, filler=0):
    """every shape, on one context: dense, then in higher rounds with target masks that leave acceptor groups below
    quorum, then after a competing leader's Phase1a on a few acceptors (Nacks, partial rows)"""
    L, A, R, f = geom
    kw = dict(num_slots=S, num_replicas=R, num_groups=A, num_leader_groups=L, f=f, tally_ways=8)
    gpu, ref = fa.Context(fa.make_config(flags=flags, **kw)), oracle.System(oracle.make_config(**kw))
    keys, want = [], {k: 0 for k in FORMS}
    rng = np.random.default_rng(L * 100 + R)
    first = True
    for lap, delivery in enumerate(("dense", "masks", "nacks")):
        rounds = [lg % 3 + 10 * lap for lg in range(L)]
        if delivery == "nacks":
            for g in range(0, L * A, 2):
                t = W.bits_from_bool(W.random_subsets(rng, 1, R, 1, max(1, R // 2)))[0]
                same(gpu.acceptor_phase1a(g, 25, 0, t), ref.acceptor_phase1a(g, 25, 0, t))
        for name, (start, end, rnd) in shape_batches(S, L, rounds).items():
            if filler:
                more = RB.many_ranges(S, L, filler - len(start), rounds, first_row=ROWS)
                start, end, rnd = (np.concatenate([x, y]) for x, y in zip((start, end, rnd), more))
                assert 1025 <= len(start) <= 1100
            n = len(start)
            tm = RB.target_masks(n, A, R, f) if delivery == "masks" else None
            a, b = gpu.noop_ranges_fused(start, end, rnd, tm), ref.noop_ranges_fused(start, end, rnd, tm)
            same(a, b)
            assert a[0] == 0 and a[4].sum() > 0
            if delivery == "nacks":
                assert (a[3] == 25).any() and a[2].any()
            want["chain" if chain_admits(n, A, R) else "steps"] += 1
            want[fill] += 1
            keys += keys_of(start, end, rnd)
            if filler:               # more ranges than the table holds at once: compare, then collect the garbage
                same_everything(gpu, ref, keys[::9])
                gpu.proxy_forget(0, S)
                ref.proxy_forget(0, S)
                keys, want["rehash"] = keys[:5], want["rehash"] + 1
            if first:
                # by name: every cell read_state shows but those of the voters in the ranges' own slots is still -1 (the
                # rows of other leader groups, the rows next to a range's first and last, acceptors outside the vote
                # bits); read_state shows the R cells of a row, not the padding behind them
                vr, vv, _ = gpu.read_state()
                model = voted_cells(S, L, A, R, 0, start, end, rnd, a[1], a[4])
                np.testing.assert_array_equal(vr, model)
                assert (vv == -1).all() and (vr[model == -1] == -1).all()
                first = False
    same_everything(gpu, ref, keys)
    expect_census(gpu, **want)
    gpu.close()


def shape_cases():
    """(name of the test, geometry, fill forms it targets)"""
    out = []
    for geom in GEOMS:
        lg = "fill_lg" if geom[2] <= 32 else "fill_sweep"
        out.append(("fixture", geom, (lg, "fill_sweep")))
        out.append(("flag", geom, ("fill_sweep",)))
        out.append(("many", geom, ("fill_range",)))
        out.append(("ragged", geom, ("fill_sweep",)))
    return out


@pytest.mark.parametrize("geom", GEOMS)
def test_shapes_under_both_row_layouts(fa, oracle, row_layout, geom):
    L, A, R, f = geom
    run_shapes(fa, oracle, geom, L * ROWS, 0, fill_form(row_layout, L * ROWS, L, R, 100))


@pytest.mark.parametrize("geom", INTERLEAVED)
def test_shapes_with_interleaved_vote_arrays(fa, oracle, row_layout, monkeypatch, geom):
    """FPX_INTERLEAVE=1: vote round and vote value of a slot share one 32-byte sector (VS = 8)"""
    monkeypatch.setenv("FPX_INTERLEAVE", "1")
    L, A, R, f = geom
    run_shapes(fa, oracle, geom, L * ROWS, 0, fill_form(row_layout, L * ROWS, L, R, 100))


@pytest.mark.parametrize("geom", GEOMS)
def test_shapes_on_slot_major_rows_by_flag(fa, oracle, geom):
    run_shapes(fa, oracle, geom, geom[0] * ROWS, fa.FPX_F_SLOT_MAJOR_ROWS, "fill_sweep")


@pytest.mark.parametrize("geom", GEOMS)
def test_shapes_among_more_than_1024_ranges(fa, oracle, geom):
    """slot-ordered rows and 1025 ... 1100 ranges: k_ranges_fill, range by range"""
    L = geom[0]
    run_shapes(fa, oracle, geom, L * (ROWS + 512), fa.FPX_F_SLOT_MAJOR_ROWS, "fill_range", filler=1025 + 7 * L)


@pytest.mark.parametrize("geom", GEOMS)
def test_shapes_in_a_window_that_is_no_whole_number_of_rows(fa, oracle, row_layout, geom):
    """S % L != 0: the rows are slot-ordered whatever the layout asked for"""
    run_shapes(fa, oracle, geom, geom[0] * ROWS + 1, 0, "fill_sweep")


# ---------------------------------------------------------------------------------------------------------------------
# the chain's passes and its three admission limits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,A,R,form", CHAIN_CASES)
def test_chain_passes_and_admission_limits(fa, oracle, row_layout, n, A, R, form):
    """one fused call of n distinct ranges on 128 leader groups, some of them promised to a competing leader first: a
    second pass of the 1024 threads over the ranges (n > 1024) and over the acceptors (n A R > 1024), and both sides of
    n <= 2048, of the LDS words and of n A R <= 8192"""
    L, rows = 128, 72
    S = L * rows
    kw = dict(num_slots=S, num_replicas=R, num_groups=A, num_leader_groups=L, f=(R - 1) // 2, tally_ways=8)
    gpu, ref = fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))
    for lg in range(0, L, 5):
        t = W.bits_from_bool(np.arange(R)[None, :] >= 1)[0]      # all but acceptor 0: its lone vote is no quorum
        same(gpu.acceptor_phase1a(lg * A, 5, 0, t), ref.acceptor_phase1a(lg * A, 5, 0, t))
    rounds = [3 if lg % 2 else 7 for lg in range(L)]
    start, end, rnd = RB.many_ranges(S, L, n, rounds)
    assert chain_admits(n, A, R) == (form == "chain") and (n > 1024 or n * A * R > 1024)
    a, b = gpu.noop_ranges_fused(start, end, rnd), ref.noop_ranges_fused(start, end, rnd)
    same(a, b)
    assert a[0] == 0 and a[4].all() and (a[3] == 5).any() and 0 < a[5].sum() < n
    same_everything(gpu, ref, keys_of(start, end, rnd)[::37] + keys_of(start, end, rnd)[-3:])
    expect_census(gpu, **{form: 1, fill_form(row_layout, S, L, R, n): 1})
    gpu.close()


# ---------------------------------------------------------------------------------------------------------------------
# the band: the chain as the first workgroup of k_phase2_band (256 threads)
# ---------------------------------------------------------------------------------------------------------------------
band_halves = RB.band_halves


@pytest.mark.parametrize("n_ranges,form", BAND_CASES)
def test_band_chain_passes(fa, oracle, n_ranges, form):
    """fpx_mencius_band_fused_dev with independent halves: 1024 commands (16 chunks) and 256 / 257 / 309 ranges -- the 256
    threads of the band's chain make a second pass from 257 on -- and 310, whose chain no longer fits the vote kernel's
    LDS: the halves run side by side and the census shows k_ranges_chain instead"""
    import torch

    from tests.test_gpu_fullsize import _band_on_device

    L, rows, R = 64, 64, 3
    S = L * rows
    kw = dict(num_slots=S, num_replicas=R, num_groups=1, num_leader_groups=L, f=1, tally_ways=4)
    with pytest.MonkeyPatch.context() as m:
        m.delenv("FPX_SLOT_MAJOR", raising=False)
        m.delenv("FPX_BAND_SERIAL", raising=False)
        gpu = fa.Context(fa.make_config(flags=fa.FPX_F_TRUSTED, **kw))
        ref = oracle.System(oracle.make_config(**kw))
        gpu.set_stream(torch.cuda.current_stream().cuda_stream)
        slot, start, end = band_halves(L, rows, n_ranges)
        rr, rnd = np.zeros(len(slot), np.int32), np.zeros(n_ranges, np.int32)
        assert len(slot) > 512 and RB.distinct_keys(start, end, rnd)
        tm = RB.target_masks(n_ranges, 1, R, 1)
        st, cmd, rng_ = _band_on_device(fa, gpu, ("fused", slot, rr, W.steady_values(slot), None), ("ranges", start, end, rnd, tm), True)
        assert st == 0
        b1, b2 = ref.phase2_fused(slot, rr, W.steady_values(slot), None), ref.noop_ranges_fused(start, end, rnd, tm)
        assert b1[0] == b2[0] == 0 and b1[1].all() and 0 < b2[5].sum() < n_ranges
        np.testing.assert_array_equal(cmd[0], b1[1])
        np.testing.assert_array_equal(cmd[1], b1[2])
        np.testing.assert_array_equal(cmd[2], b1[3])
        np.testing.assert_array_equal(cmd[3], b1[4])
        for x, y in zip(rng_, b2[1:]):
            np.testing.assert_array_equal(x, np.asarray(y).reshape(x.shape))
        same_everything(gpu, ref, keys_of(start, end, rnd)[::11])
    if form == "band":
        assert gpu.band_merged_steps() == 1
        expect_census(gpu, band=1)
    else:
        assert gpu.band_merged_steps() == 0
        expect_census(gpu, chain=1, fill_lg=1)
    gpu.close()


# ---------------------------------------------------------------------------------------------------------------------
# the same key twice in one batch of a device entry point (no host driver cuts the batch)
# ---------------------------------------------------------------------------------------------------------------------
def fused_dev(gpu, start, end, rnd, tm):
    import torch
    dev = torch.device("cuda:0")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n, A = len(start), gpu.cfg.num_groups
    vb, nb = (torch.zeros((n, A, 4), dtype=torch.int64, device=dev) for _ in range(2))
    nr = torch.full((n,), -1, dtype=torch.int32, device=dev)
    new, ch = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
    gpu.noop_ranges_fused_dev(d(start), d(end), d(rnd), None if tm is None else d(tm.view(np.int64)), vb, nb, nr, new, ch)
    st = gpu.sync()
    h = lambda t: t.cpu().numpy()
    return st, h(vb).view(np.uint64), h(nb).view(np.uint64), h(nr), h(new), h(ch)


def widen(start, end, Lh, L):
    """the ranges of a window of Lh leader groups as ranges of the same rows and leader groups among L"""
    f = lambda s: (s // Lh) * L + s % Lh
    return f(start).astype(np.int32), np.where(end > start, f(end - 1) + 1, f(start)).astype(np.int32)


@pytest.mark.parametrize("entry", ["ranges", "band"])
def test_duplicate_keys_at_the_device_entry_points(fa, oracle, row_layout, monkeypatch, entry):
    """overlap_batch with its duplicates (the lowest copy first, the other last; two neighbours) in ONE device batch, one
    of the duplicated keys opened by an earlier call: per index is_new, chosen and the losers' empty votes as the oracle's
    fused form gives them for the same arrays"""
    import torch

    from tests.test_gpu_fullsize import _band_on_device

    monkeypatch.delenv("FPX_BAND_SERIAL", raising=False)
    Lh, L, R = 4, 64, 3               # the ranges in leader groups 0 ... 3, the band's commands in 32 ... 63
    S = L * ROWS
    start, end, rnd, dups = RB.overlap_batch(Lh * ROWS, Lh)
    start, end = widen(start, end, Lh, L)
    assert (start % L < Lh).all() and RB.overlaps(start, end, L).any()
    kw = dict(num_slots=S, num_replicas=R, num_groups=1, num_leader_groups=L, f=1, tally_ways=4)
    flags = fa.FPX_F_TRUSTED if entry == "band" else 0
    gpu, ref = fa.Context(fa.make_config(flags=flags, **kw)), oracle.System(oracle.make_config(**kw))
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    mid = dups[0][0]
    one = (start[mid:mid + 1], end[mid:mid + 1], rnd[mid:mid + 1])
    same(gpu.noop_ranges_fused(*one), ref.noop_ranges_fused(*one))
    tm = RB.target_masks(len(start), 1, R, 1)
    want = ref.noop_ranges_fused(start, end, rnd, tm)
    if entry == "ranges":
        got = fused_dev(gpu, start, end, rnd, tm)
        same(got, want)
    else:
        slot = (np.arange(32)[:, None] * L + 32 + np.arange(32)[None, :]).reshape(-1).astype(np.int32)   # 1024 commands
        rr = np.zeros(len(slot), np.int32)
        st, cmd, got = _band_on_device(fa, gpu, ("fused", slot, rr, W.steady_values(slot), None), ("ranges", start, end, rnd, tm), True)
        assert st == 0
        same((st,) + tuple(got), want)
        b1 = ref.phase2_fused(slot, rr, W.steady_values(slot), None)
        np.testing.assert_array_equal(cmd[0], b1[1])
    new = np.asarray(want[4])
    for first, later in dups:
        assert new[later] == 0 and not np.asarray(want[1])[later].any() and want[5][later] == 0
    assert new[0] == 1 and new[mid] == 0 and new.sum() == len(start) - 3
    same_everything(gpu, ref, keys_of(start, end, rnd))
    lg_major = row_layout == "leader-group-major"
    if entry == "band" and lg_major:
        assert gpu.band_merged_steps() == 1, gpu.range_launch_census()
        expect_census(gpu, chain=1, band=1, fill_lg=1)
    else:
        expect_census(gpu, chain=2, **{"fill_lg" if lg_major else "fill_sweep": 2})
    gpu.close()


# ---------------------------------------------------------------------------------------------------------------------
# ranges on a replica shard: vote bits at replica_base + r
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 60, 124, 188])
def test_shard(fa, oracle, row_layout, base):
    """8 of base + 12 replicas from bit `base` on (60: the bits straddle a 64-bit word): fused and unfused, then late
    Phase2bNoopRanges that carry bits outside the membership (masked off), complete a quorum with another shard's
    acceptor, or name a key nobody opened"""
    L, A, R, f = 3, 2, 8, 3
    S, total = L * ROWS, base + 12
    kw = dict(num_slots=S, num_replicas=R, num_groups=A, num_leader_groups=L, f=f, tally_ways=8, replica_base=base,
              replicas_total=total)
    gpu, ref = fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))
    start, end, rnd = RB.residue_batch(S, L, [1, 0, 2])
    n = len(start)
    tm = RB.target_masks(n, A, R, f, base=base)
    a, b = gpu.noop_ranges_fused(start, end, rnd, tm), ref.noop_ranges_fused(start, end, rnd, tm)
    same(a, b)
    assert a[0] == 0 and a[4].all() and 0 < a[5].sum() < n
    members = W.bool_from_bits(a[1].reshape(-1, 4), 256)
    assert members[:, base:base + R].any() and not members[:, :base].any() and not members[:, base + R:].any()
    if base == 60:
        assert (a[1][:, :, 0] >> np.uint64(60)).any() and a[1][:, :, 1].any()
    np.testing.assert_array_equal(gpu.read_state()[0], voted_cells(S, L, A, R, base, start, end, rnd, a[1], a[4]))
    pending = np.nonzero(a[5] == 0)[0]
    ps, pe, pr = start[pending], end[pending], rnd[pending]
    outside = np.zeros((len(pending), A, 4), np.uint64)
    outside[:, :, total >> 6] = np.uint64((2 ** 64 - 1) ^ ((1 << (total & 63)) - 1))       # every bit from `total` up
    same(gpu.proxy_phase2b_noop_ranges(ps, pe, pr, outside), ref.proxy_phase2b_noop_ranges(ps, pe, pr, outside))
    same_everything(gpu, ref, keys_of(ps, pe, pr))
    late = outside.copy()
    late[:, :, (base + 9) >> 6] |= np.uint64(1 << ((base + 9) & 63))                          # an acceptor of another shard
    x, y = gpu.proxy_phase2b_noop_ranges(ps, pe, pr, late), ref.proxy_phase2b_noop_ranges(ps, pe, pr, late)
    same(x, y)
    assert x[0] == 0 and x[1].all()
    # the unfused entry points, in the next round
    rnd2 = rnd + 3
    same(gpu.proxy_open_noop_ranges(start, end, rnd2), ref.proxy_open_noop_ranges(start, end, rnd2))
    u, v = gpu.acceptor_phase2a_noop_ranges(start, end, rnd2, tm), ref.acceptor_phase2a_noop_ranges(start, end, rnd2, tm)
    same(u, v)
    same(gpu.proxy_phase2b_noop_ranges(start, end, rnd2, u[1]), ref.proxy_phase2b_noop_ranges(start, end, rnd2, u[1]))
    x = gpu.proxy_phase2b_noop_ranges(start[:1], end[:1], rnd2[:1] + 50, u[1][:1])
    same(x, ref.proxy_phase2b_noop_ranges(start[:1], end[:1], rnd2[:1] + 50, u[1][:1]))
    assert x[0] == fa.FPX_EFATAL_UNKNOWN_SLOTROUND
    same_everything(gpu, ref, keys_of(start, end, rnd) + keys_of(start, end, rnd2))
    fill = fill_form(row_layout, S, L, R, n)
    expect_census(gpu, chain=1, open_only=1, acceptors_only=1, tally_only=4, **{fill: 2})
    gpu.close()


# ---------------------------------------------------------------------------------------------------------------------
# the range table: probing, capacity, garbage collection
# ---------------------------------------------------------------------------------------------------------------------
TABLE_KW = dict(num_slots=4 * 400, num_replicas=3, num_groups=1, num_leader_groups=4, f=1, tally_ways=8)


def test_table_probing_wraps_from_the_last_bucket_to_the_first(fa, oracle):
    gpu, ref = fa.Context(fa.make_config(**TABLE_KW)), oracle.System(oracle.make_config(**TABLE_KW))
    S = TABLE_KW["num_slots"]
    picked = []
    for s, width in itertools.product(range(S - 64), (6, 11, 17, 23, 30, 38, 47, 57)):
        cap, home, at = gpu.read_range_position(s, s + width, 0)
        assert cap == 4096 and at == -1 and 0 <= home < cap
        if home >= cap - 4:
            picked.append((s, s + width, home))
        if len(picked) == 5:         # five keys for the last four buckets: one of them must wrap
            break
    assert len(picked) == 5, "no candidate keys near the last bucket"
    start, end = (np.array(x, np.int32) for x in zip(*[(p[0], p[1]) for p in picked]))
    rnd = np.zeros(5, np.int32)
    same(gpu.noop_ranges_fused(start, end, rnd), ref.noop_ranges_fused(start, end, rnd))
    where = [gpu.read_range_position(int(s), int(e), 0) for s, e in zip(start, end)]
    assert [w[1] for w in where] == [p[2] for p in picked]
    assert len({w[2] for w in where}) == 5 and all(w[2] >= 0 for w in where)
    assert any(w[2] < w[1] for w in where), where        # an entry below its home bucket: it wrapped
    same_everything(gpu, ref, keys_of(start, end, rnd))
    expect_census(gpu, chain=1, **{fill_form(ambient_layout(), S, 4, 3, 5): 1})
    gpu.close()


def test_table_keeps_the_same_range_of_three_rounds_apart(fa, oracle, row_layout):
    gpu, ref = fa.Context(fa.make_config(**TABLE_KW)), oracle.System(oracle.make_config(**TABLE_KW))
    s, e = 41, 97
    one = np.zeros((1, 1, 4), np.uint64)
    for r in range(3):               # open in rounds 0, 1, 2 with one acceptor each: all Pending
        one[0, 0, 0] = np.uint64(1 << r)
        same(gpu.noop_ranges_fused([s], [e], [r], one), ref.noop_ranges_fused([s], [e], [r], one))
    where = [gpu.read_range_position(s, e, r) for r in range(3)]
    assert len({w[1] for w in where}) == 1 and len({w[2] for w in where}) == 3       # one home bucket, three entries
    assert gpu.read_range_position(s, e, 3)[2] == -1
    for r in (1, 0, 2):              # a second vote for each, separately
        one[0, 0, 0] = np.uint64(1 << ((r + 1) % 3))
        for k in range(3):
            a, b = gpu.read_range_tally(s, e, k), ref.read_range_tally(s, e, k)
            assert a[0] == b[0]
            np.testing.assert_array_equal(a[1], b[1])
        x = gpu.proxy_phase2b_noop_ranges([s], [e], [r], one)
        same(x, ref.proxy_phase2b_noop_ranges([s], [e], [r], one))
        assert x[1][0] == 1
    same_everything(gpu, ref, [(s, e, r) for r in range(4)])
    fill = fill_form(row_layout, TABLE_KW["num_slots"], 4, 3, 1)
    expect_census(gpu, chain=3, tally_only=3, **{fill: 3})
    gpu.close()


@pytest.mark.parametrize("R,form", [(3, "chain"), (9, "steps")])
def test_table_capacity_edge(fa, oracle, R, form):
    """cap / 2 = 2048 live entries: 1024 + 1023 ranges fit (the second batch on the chain's count_hint alone), one more
    fits, the next is FPX_ECAPACITY with nothing changed -- the batches through k_ranges_chain (R = 3), or as launches
    of their own with the live counter (R = 9: n A R > 8192)"""
    kw = dict(TABLE_KW, num_replicas=R, f=(R - 1) // 2)
    gpu, ref = fa.Context(fa.make_config(**kw)), oracle.System(oracle.make_config(**kw))
    start, end, rnd = RB.many_ranges(kw["num_slots"], 4, 3100)
    assert gpu.read_range_position(0, 1, 0)[0] == 4096
    cuts = [0, 1024, 2047, 2048]
    for lo, hi in zip(cuts, cuts[1:]):
        assert chain_admits(hi - lo, 1, R) == (form == "chain" or hi - lo == 1)
        a = gpu.noop_ranges_fused(start[lo:hi], end[lo:hi], rnd[lo:hi])
        same(a, ref.noop_ranges_fused(start[lo:hi], end[lo:hi], rnd[lo:hi]))
        assert a[0] == 0 and a[4].all()
    digest = gpu.state_digest()
    hi = 2049 if form == "chain" else 3100
    a = gpu.noop_ranges_fused(start[2048:hi], end[2048:hi], rnd[2048:hi])
    assert a[0] == fa.FPX_ECAPACITY and not a[4].any() and not a[5].any() and not a[1].any()
    assert chain_admits(hi - 2048, 1, R) == (form == "chain")
    # a key that is there is still found, and nothing else changed
    same(gpu.noop_ranges_fused(start[:3], end[:3], rnd[:3]), ref.noop_ranges_fused(start[:3], end[:3], rnd[:3]))
    np.testing.assert_array_equal(gpu.state_digest(), digest)
    same_everything(gpu, ref, keys_of(start, end, rnd)[2040:2052])
    fill = fill_form(ambient_layout(), kw["num_slots"], 4, R, 1)
    if form == "chain":
        expect_census(gpu, chain=5, **{fill: 5})
    else:
        assert fill == "fill_lg" or fill_form(ambient_layout(), kw["num_slots"], 4, R, 1052) == "fill_range"
        expect_census(gpu, steps=3, chain=2, **({fill: 5} if fill == "fill_lg" else {"fill_sweep": 4, "fill_range": 1}))
    gpu.close()


def test_table_rehash_window_edges(fa, oracle, row_layout):
    """fpx_proxy_forget(first, count) drops exactly the tallies with start >= first and end <= first + count: Pending
    entries (one vote) and Done ones on either side of both edges; the survivors keep state and votes"""
    gpu, ref = fa.Context(fa.make_config(**TABLE_KW)), oracle.System(oracle.make_config(**TABLE_KW))
    first, count = 400, 200
    # (start, end, Pending?, survives?)
    cases = [(400, 450, 1, 0), (400, 460, 0, 0), (399, 450, 1, 1), (399, 460, 0, 1),
             (410, 600, 1, 0), (420, 600, 0, 0), (410, 601, 1, 1), (420, 601, 0, 1)]
    start, end = (np.array([c[k] for c in cases], np.int32) for k in (0, 1))
    rnd = np.zeros(len(cases), np.int32)
    tm = np.zeros((len(cases), 1, 4), np.uint64)
    tm[:, 0, 0] = [1 if c[2] else 7 for c in cases]
    a = gpu.noop_ranges_fused(start, end, rnd, tm)
    same(a, ref.noop_ranges_fused(start, end, rnd, tm))
    assert a[5].tolist() == [0 if c[2] else 1 for c in cases]
    gpu.proxy_forget(first, count)
    ref.proxy_forget(first, count)
    for c in cases:
        state, bits = gpu.read_range_tally(c[0], c[1], 0)
        assert state == (0 if not c[3] else 1 if c[2] else 2), c
        assert int(bits[0, 0]) == (1 if c[2] and c[3] else 0), c
    same_everything(gpu, ref, keys_of(start, end, rnd))
    expect_census(gpu, chain=1, rehash=1, **{fill_form(row_layout, TABLE_KW["num_slots"], 4, 3, 8): 1})
    gpu.close()
