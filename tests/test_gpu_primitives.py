"""The workgroup primitives of frankenpaxos_amd/csrc/fpx_scan.hpp and the radix sort of fpx_burst_sort.hpp on the GPU, each
on its own through the launchers of tests/primitives_harness.hip and compared exactly with the references of
tests/primitives.py: every instantiation the library uses, at the smallest shapes and the values at which it can still be
wrong -- sums that wrap or exceed 32 bits, maxima whose words disagree, step edges and tails of the array scan, every
pass count of the sort and a device-side length far below the grid.  profiles/primitive_tests.md lists eight mutations of
the two headers and the tests here that fail under each."""
import ctypes

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

from tests import primitives as P

pytestmark = pytest.mark.gpu

BLOCKS = 3   # workgroups per launch, each on its own data: nothing may depend on a global id
TORCH = {"int": torch.int32, "u32": torch.int32, "i64": torch.int64, "ll": torch.int64}
TYPE_MAX = {"int": (1 << 31) - 1, "i64": (1 << 63) - 1, "ll": (1 << 63) - 1}
OUT_WORD = {"int": 0x3C3C3C3C, "u32": 0x3C3C3C3C, "i64": 0x3C3C3C3C3C3C3C3C, "ll": 0x3C3C3C3C3C3C3C3C}   # "never written"


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(x, t):
    a = x.cpu().numpy()
    return a.view(np.uint32) if t == "u32" else a


def filled(n, t, word=None):
    return torch.full((n,), OUT_WORD[t] if word is None else word, dtype=TORCH[t], device="cuda")


def ptr(x):
    return ctypes.c_void_p(x.data_ptr() if x is not None else None)


def call(name, *args):
    rc = getattr(P.lib(), name)(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), *args)
    assert rc == 0, "%s returned %d" % (name, rc)


def guards_of(t, blocks):
    return filled(blocks * 2 * P.lib().pt_guard_words(), t, 0)


def assert_guards(g, t):
    assert_array_equal(host(g, t), np.full(g.numel(), P.GUARD_WORD[t], P.NP[t]), err_msg="a guard word beside the LDS scratch changed")


def named(fn):
    return sorted(n for n, row in P.LAUNCHERS.items() if row["fn"] == fn)


def value_sets(op, t, blocks, threads, rng):
    """[blocks, threads] arrays to scan or reduce: for a sum one random set; for a maximum a random set with runs of -1, all
    -1, and the one largest value at every place of peak_places(), in another place in every workgroup"""
    n = blocks * threads
    if op == "sum":
        yield "random", P.gen_sum(t, n, rng).reshape(blocks, threads)
        return
    yield "runs of -1", P.gen_max(t, n, rng).reshape(blocks, threads)
    yield "all -1", np.full((blocks, threads), -1, P.NP[t])
    places = P.peak_places(threads)
    for i, _ in enumerate(places):
        v = P.gen_max(t, n, rng, minus_runs=i % 2 == 0).reshape(blocks, threads)
        for b in range(blocks):
            v[b] = P.with_peak(v[b], places[(i + b) % len(places)])
        yield "peak at %s" % [places[(i + b) % len(places)] for b in range(blocks)], v


def carries(op, t, v, rng):
    """non-identity carries for the rows of v: sums that wrap or exceed 32 bits; maxima above the row's own, inside it, below"""
    if op == "sum":
        return P.gen_sum(t, v.shape[0], rng)
    c = [int(v[b].max()) + 1 if b % 3 == 0 else int(np.median(v[b])) if b % 3 == 1 else 5 for b in range(v.shape[0])]
    return np.array(c, P.NP[t])


# ------------------------------------------------------------------------------------------------------ wavefront, workgroup
@pytest.mark.parametrize("name", named("wave_incl_scan") + named("wave_reduce"))
def test_wavefront_function(name):
    row = P.LAUNCHERS[name]
    op, t, threads = row["op"], row["type"], row["threads"]
    ref = P.ref_wave_incl_scan if row["fn"] == "wave_incl_scan" else P.ref_wave_reduce
    for what, v in value_sets(op, t, BLOCKS, threads, np.random.default_rng(11)):
        d_v, out = dev(v), filled(v.size, t)
        call(name, ptr(d_v), ptr(out), BLOCKS)
        assert_array_equal(host(out, t), ref(op, t, v), err_msg=what)


@pytest.mark.parametrize("name", named("block_excl_scan"))
def test_block_excl_scan(name):
    row = P.LAUNCHERS[name]
    op, t, threads = row["op"], row["type"], row["threads"]
    rng = np.random.default_rng(12)
    for what, v in value_sets(op, t, BLOCKS, threads, rng):
        for carry in (carries(op, t, v, rng), np.full(BLOCKS, P.identity(op), P.NP[t])):
            d_v, d_carry, out, total, g = dev(v), dev(carry), filled(v.size, t), filled(v.size, t), guards_of(t, BLOCKS)
            call(name, ptr(d_v), ptr(d_carry), ptr(out), ptr(total), ptr(g), BLOCKS)
            want, want_total = P.ref_block_excl_scan(op, t, v, carry)
            assert_array_equal(host(out, t).reshape(BLOCKS, threads), want, err_msg=what)
            if row["total"]:     # in every thread
                assert_array_equal(host(total, t).reshape(BLOCKS, threads), np.repeat(want_total[:, None], threads, axis=1), err_msg=what)
            else:                # the wrapper's own word, untouched
                assert_array_equal(host(total, t), np.full(v.size, P.GUARD_WORD[t], P.NP[t]), err_msg=what)
            assert_guards(g, t)


@pytest.mark.parametrize("name", named("block_reduce"))
def test_block_reduce(name):
    row = P.LAUNCHERS[name]
    op, t, threads = row["op"], row["type"], row["threads"]
    for what, v in value_sets(op, t, BLOCKS, threads, np.random.default_rng(13)):
        d_v, out, g = dev(v), filled(v.size, t), guards_of(t, BLOCKS)
        call(name, ptr(d_v), ptr(out), ptr(g), BLOCKS)
        assert_array_equal(host(out, t).reshape(BLOCKS, threads), P.ref_block_reduce(op, t, v), err_msg=what)
        assert_guards(g, t)


@pytest.mark.parametrize("kind", P.FLAG_KINDS)
def test_block_rank(kind):
    flags = P.gen_flags(kind, BLOCKS, np.random.default_rng(14))
    d_flags, out, total, g = dev(flags), filled(flags.size, "int"), filled(flags.size, "int"), guards_of("int", BLOCKS)
    call("pt_block_rank_256", ptr(d_flags), ptr(out), ptr(total), ptr(g), BLOCKS)
    want, want_total = P.ref_block_rank(flags)   # (an unflagged thread gets the rank it would have had: the same formula)
    assert_array_equal(host(out, "int").reshape(BLOCKS, 256), want)
    assert_array_equal(host(total, "int").reshape(BLOCKS, 256), np.repeat(want_total[:, None], 256, axis=1))
    assert_guards(g, "int")


# ---------------------------------------------------------------------------------------------------------- scan_array_excl
def array_lens(threads, per):
    s = threads * per
    lens = [0, 1, 63, 64, 65, s - 1, s, s + 1, 2 * s, 3 * s + 57]
    if per == 8:
        lens += [7, 8, 9, s - 7]    # tails inside a thread's eight elements
    return lens


def array_rows(op, t, lens, s, rng, rep, start):
    """one array per length.  Sums: random.  Maxima: rep 0 random with runs of -1; rep 1 all -1; from rep 2 on the one largest
    value at a place of peak_places() -- either side of a step among them -- that moves with the row and with rep"""
    rows = []
    for i, n in enumerate(lens):
        if op == "sum":
            rows.append(P.gen_sum(t, n, rng, headroom=start))
        elif rep == 1:
            rows.append(np.full(n, -1, P.NP[t]))
        else:
            v = P.gen_max(t, n, rng)
            places = P.peak_places(n, s)
            rows.append(P.with_peak(v, places[(i + rep) % len(places)]) if rep >= 2 and n else v)
    return rows


@pytest.mark.parametrize("name", named("scan_array_excl"))
def test_scan_array_excl(name):
    row = P.LAUNCHERS[name]
    op, t, threads, per = row["op"], row["type"], row["threads"], row["per"]
    lens = array_lens(threads, per)
    cap, pad, nblk = max(lens), P.lib().pt_array_pad(), len(lens)
    assert nblk <= P.lib().pt_array_blocks()
    # what lies behind an array: for a maximum the type's largest value, so a read past the end cannot hide below the result
    behind = OUT_WORD[t] if op == "sum" else TYPE_MAX[t]
    rng, failed = np.random.default_rng(15), []
    for rep in range(1 if op == "sum" else 6):
        sum_start = {"u32": 0xFFFF0000, "int": 1 << 20}.get(t)
        rows = array_rows(op, t, lens, threads * per, rng, rep, sum_start if row["start"] else 0)
        if not row["start"]:
            starts = [None] * nblk
        elif op == "sum":
            starts = [sum_start] * nblk
        else:   # above the array's own maximum and below it (the tile scan of k_cl_tilescan), in turn
            starts = [(int(v.max()) + 1 if v.size else 7) if (i + rep) % 2 == 0 else 3 for i, v in enumerate(rows)]
        a = np.full((nblk, cap + pad), behind, P.NP[t])
        for i, v in enumerate(rows):
            a[i, :v.size] = v
        d_a, out, g = dev(a), filled(nblk * threads, t), guards_of(t, nblk)
        c_lens = (ctypes.c_longlong * nblk)(*lens)
        if row["start"]:
            call(name, ptr(d_a), ctypes.c_longlong(cap), c_lens, (ctypes.c_longlong * nblk)(*starts), nblk, ptr(out), ptr(g))
        else:
            call(name, ptr(d_a), ctypes.c_longlong(cap), c_lens, nblk, ptr(out), ptr(g))
        got, ret = host(d_a, t).reshape(nblk, cap + pad), host(out, t).reshape(nblk, threads)
        for i, v in enumerate(rows):     # every wrong array is named, not the first alone
            want, want_all = P.ref_scan_array_excl(op, t, v, starts[i])
            if v.size == 0:
                assert want_all == P.wrap([P.identity(op) if starts[i] is None else starts[i]], t)[0]
            wrong = [label for label, x, y in (("the array", got[i, :v.size], want),
                                               ("words beyond len", got[i, v.size:], np.full(cap + pad - v.size, behind, P.NP[t])),
                                               ("the value returned", ret[i], np.full(threads, want_all, P.NP[t]))) if not np.array_equal(x, y)]
            if wrong:
                failed.append("len %d, start %s, rep %d: %s" % (v.size, starts[i], rep, " and ".join(wrong)))
        assert_guards(g, t)
    assert not failed, "%d arrays: %s" % (len(failed), "; ".join(failed))


# ------------------------------------------------------------------------------------------------------------------ the sort
SORT_WORD = 0x3C3C3C3C


def run_sort(keys, max_key, tiles, with_last):
    """sorts the pairs (keys[j], j) in a scratch of `tiles` tiles filled with SORT_WORD; returns r and the arrays afterwards"""
    lib, m = P.lib(), len(keys)
    nbytes = lib.pt_sort_scratch_bytes(tiles)
    at = (ctypes.c_longlong * 5)()
    assert lib.pt_sort_scratch_offsets(tiles, at) == 0 and nbytes % 4 == 0
    words = np.full(nbytes // 4, SORT_WORD, np.int32)
    words[at[1] // 4:at[1] // 4 + m] = keys
    words[at[3] // 4:at[3] // 4 + m] = np.arange(m, dtype=np.int32)
    scratch, d_len = dev(words), filled(1, "int")
    last = filled(tiles * P.TILE, "int", SORT_WORD) if with_last else None
    r = ctypes.c_int(-1)
    call("pt_burst_sort", ptr(scratch), ctypes.c_longlong(nbytes), ptr(d_len), m, ctypes.c_longlong(max_key), tiles, ptr(last),
         ctypes.byref(r))
    assert int(d_len.item()) == m
    words = host(scratch, "int")
    cut = lambda j, n: words[at[j] // 4:at[j] // 4 + n]
    return r.value, dict(hist=cut(0, P.RADIX * tiles), key=[cut(1, tiles * P.TILE), cut(2, tiles * P.TILE)],
                         val=[cut(3, tiles * P.TILE), cut(4, tiles * P.TILE)], last=host(last, "int") if with_last else None)


def check_sort(keys, max_key, tiles, with_last, what):
    m = len(keys)
    r, got = run_sort(keys, max_key, tiles, with_last)
    assert r == P.sort_passes(max_key) & 1, what
    order = P.ref_sort_order(keys)
    assert_array_equal(got["key"][r][:m], keys[order], err_msg=what + ": keys")
    assert_array_equal((got["last"] if with_last else got["val"][r])[:m], order, err_msg=what + ": values (stable order)")
    # nothing at or beyond the length is written, in either buffer
    for label, a in [("key[0]", got["key"][0]), ("key[1]", got["key"][1]), ("val[0]", got["val"][0]), ("val[1]", got["val"][1])] + (
            [("val_last", got["last"])] if with_last else []):
        assert_array_equal(a[m:], np.full(a.size - m, SORT_WORD, np.int32), err_msg=what + ": %s beyond len" % label)
    used = P.RADIX * ((m + P.TILE - 1) // P.TILE)
    assert_array_equal(got["hist"][used:], np.full(got["hist"].size - used, SORT_WORD, np.int32), err_msg=what + ": hist beyond the tiles of len")


def check_sorts(cases):
    """check_sort() over (keys, max_key, tiles, with_last, what) cases; every failing case is named, not the first alone"""
    failed, first = [], None
    for case in cases:
        try:
            check_sort(*case)
        except AssertionError as e:
            failed.append(case[4])
            first = first or str(e)
    assert not failed, "%d of %d cases: %s.  The first: %s" % (len(failed), len(cases), "; ".join(failed), first)


@pytest.mark.parametrize("kind", P.KEY_KINDS)
@pytest.mark.parametrize("with_last", [False, True], ids=["val_r", "val_last"])
@pytest.mark.parametrize("m", [0, 1, 16, 255, 256, 257, 1000, 513 * 256 + 57])
def test_sort_is_the_stable_argsort(m, with_last, kind):
    """every pass count at every number of pairs.  16 pairs are the most that one pass sorts with all keys distinct; 513 * 256
    + 57 pairs are 514 tiles, 8 224 digit counts: the count scan's second step (8 192 counts a step)"""
    rng = np.random.default_rng(16)
    tiles = max(1, (m + P.TILE - 1) // P.TILE)
    cases = []
    for max_key in P.MAX_KEYS:
        keys = P.gen_keys(kind, m, max_key, rng)
        if keys is not None:    # (no permutation of more keys than there are values)
            cases.append((keys, max_key, tiles, with_last, "max_key %d (%d passes)" % (max_key, P.sort_passes(max_key))))
    assert cases
    check_sorts(cases)


@pytest.mark.parametrize("with_last", [False, True], ids=["val_r", "val_last"])
@pytest.mark.parametrize("tiles", [8, 514])
def test_sort_with_a_device_side_length_below_the_grid(tiles, with_last):
    rng = np.random.default_rng(17)
    check_sorts([(P.gen_keys("few_distinct", m, max_key, rng), max_key, tiles, with_last, "len %d, max_key %d (%d passes)" % (m, max_key, P.sort_passes(max_key)))
                 for m in (0, 1, 300, tiles * P.TILE) for max_key in (255, 256)])     # both result buffers


# ------------------------------------------------------------------------------------------------- the LDS-reuse contract
def rounds_of(t, threads, rng, op):
    """[rounds][2 calls][BLOCKS][threads], a workgroup's values generated on their own (an int sum is bounded per workgroup)"""
    rows = P.lib().pt_rounds() * 2 * BLOCKS
    v = np.stack([P.gen_sum(t, threads, rng) if op == "sum" else P.gen_max(t, threads, rng) for _ in range(rows)])
    return v.reshape(P.lib().pt_rounds(), 2, BLOCKS, threads)


@pytest.mark.parametrize("name", named("reduce_twice"))
def test_block_reduce_twice_in_a_row_on_the_same_words(name):
    row = P.LAUNCHERS[name]
    op, t, threads = row["op"], row["type"], row["threads"]
    v = rounds_of(t, threads, np.random.default_rng(18), op)
    d_v, out, g = dev(v), filled(v.size, t), guards_of(t, BLOCKS)
    call(name, ptr(d_v), ptr(out), ptr(g), BLOCKS)
    want = P.ref_block_reduce(op, t, v.reshape(-1, threads)).reshape(v.shape)
    got = host(out, t).reshape(v.shape)
    for r in range(v.shape[0]):
        assert_array_equal(got[r], want[r], err_msg="round %d" % r)
    assert_guards(g, t)


def test_block_excl_scan_twice_on_the_same_words_with_the_callers_barrier():
    name, t, threads = "pt_scan_twice_same_words_sum_u32_256", "u32", 256
    v = rounds_of(t, threads, np.random.default_rng(19), "sum")
    d_v, out, total, g = dev(v), filled(v.size, t), filled(v.size, t), guards_of(t, BLOCKS)
    call(name, ptr(d_v), ptr(out), ptr(total), ptr(g), BLOCKS)
    got, got_total = host(out, t).reshape(v.shape), host(total, t).reshape(v.shape)
    for r in range(v.shape[0]):
        first, first_total = P.ref_block_excl_scan("sum", t, v[r, 0], np.zeros(BLOCKS, np.uint32))
        second, second_total = P.ref_block_excl_scan("sum", t, v[r, 1], first_total)     # the first call's total is the carry
        assert_array_equal(got[r, 0], first, err_msg="round %d, first call" % r)
        assert_array_equal(got[r, 1], second, err_msg="round %d, second call" % r)
        assert_array_equal(got_total[r, 0], np.repeat(first_total[:, None], threads, axis=1), err_msg="round %d, first total" % r)
        assert_array_equal(got_total[r, 1], np.repeat(second_total[:, None], threads, axis=1), err_msg="round %d, second total" % r)
    assert_guards(g, t)


def test_block_excl_scan_twice_on_other_words_without_a_barrier():
    name, t, threads = "pt_scan_twice_other_words_sum_u32_512", "u32", 512
    v = rounds_of(t, threads, np.random.default_rng(20), "sum")
    d_v, out, g = dev(v), filled(v.size, t), guards_of(t, BLOCKS)
    call(name, ptr(d_v), ptr(out), ptr(g), BLOCKS)
    got = host(out, t).reshape(v.shape)
    for r in range(v.shape[0]):
        for j in range(2):
            want, _ = P.ref_block_excl_scan("sum", t, v[r, j], np.zeros(BLOCKS, np.uint32))
            assert_array_equal(got[r, j], want, err_msg="round %d, call %d" % (r, j))
    assert_guards(g, t)
