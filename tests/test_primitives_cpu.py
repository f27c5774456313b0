"""The direct tests of the workgroup primitives, the part that needs no GPU: the harness tests/primitives_harness.hip
cross-compiles for gfx950 without a warning, every launcher of the table in tests/primitives.py resolves and no other is
exported, the launchers refuse arguments that are off without launching, the references and generators are right on
hand-written cases, the table's call-site counts still hold, and ScanMax on an unsigned type does not compile."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import primitives as P


def test_harness_builds_for_gfx950_without_warnings():
    flags = P.hipflags()
    assert "-Wall" in flags and "--offload-arch=gfx950" in flags and [f for f in flags if f.startswith("--offload-arch")] == ["--offload-arch=gfx950"]
    so = P.build()
    assert so == P.SO_PATH and os.path.exists(so) and not P.stale()
    with open(P.LOG_PATH) as f:
        log = f.read()
    assert "warning" not in log and "error" not in log, log


def test_every_launcher_of_the_table_resolves():
    lib = P.lib()
    missing = [name for name in P.LAUNCHERS if not hasattr(lib, name)]
    assert not missing, missing


def test_no_launcher_outside_the_table():
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm on this machine")
    out = subprocess.run([nm, "-D", "--defined-only", P.build()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("pt_")}
    assert exported == set(P.LAUNCHERS)


def test_every_call_site_of_the_library_has_its_launcher():
    """USES of tests/primitives.py lists every call site with the type read there; a new call site fails the count"""
    assert P.count_call_sites() == P.expected_call_sites()
    for name, needle, launcher, _ in P.USES:
        row = P.LAUNCHERS[launcher]
        assert needle.rstrip("<(") == row["fn"], (name, needle, launcher)


def test_launchers_refuse_arguments_that_are_off_without_launching():
    """every buffer is a null pointer here: the ranges are looked at first (-1), the pointers after them (-2), and nothing is
    launched either way"""
    lib = P.lib()
    p = None
    assert lib.pt_wave_reduce_sum_int_64(None, p, p, 0) == -1
    assert lib.pt_block_excl_scan_sum_u32_256(None, p, p, p, p, p, 0) == -1
    assert lib.pt_block_reduce_max_int_256(None, p, p, p, -3) == -1
    assert lib.pt_block_rank_256(None, p, p, p, p, 0) == -1
    assert lib.pt_reduce_twice_sum_u32_256(None, p, p, p, 0) == -1
    lens = (ctypes.c_longlong * 2)(5, 101)
    assert lib.pt_scan_array_excl_sum_u32_256_1(None, p, ctypes.c_longlong(100), lens, 2, p, p) == -1           # len > capacity
    assert lib.pt_scan_array_excl_sum_u32_256_1(None, p, ctypes.c_longlong(100), (ctypes.c_longlong * 1)(-1), 1, p, p) == -1
    assert lib.pt_scan_array_excl_sum_u32_256_1(None, p, ctypes.c_longlong(100), lens, 0, p, p) == -1           # no workgroup
    assert lib.pt_scan_array_excl_sum_u32_256_1(None, p, ctypes.c_longlong(100), lens, lib.pt_array_blocks() + 1, p, p) == -1
    assert lib.pt_scan_array_excl_max_int_256_1_start(None, p, ctypes.c_longlong(100), (ctypes.c_longlong * 1)(5), None, 1, p, p) == -1
    sort = lambda nbytes, m, max_key, tiles: lib.pt_burst_sort(None, p, ctypes.c_longlong(nbytes), p, m, ctypes.c_longlong(max_key), tiles,
                                                               None, None)
    enough = lib.pt_sort_scratch_bytes(2)
    assert sort(enough, 10, 15, 0) == -1            # tiles >= 1
    assert sort(enough, 10, -1, 2) == -1            # max_key >= 0
    assert sort(enough, 513, 15, 2) == -1           # len <= tiles * 256
    assert sort(enough, -1, 15, 2) == -1
    assert sort(enough - 4, 10, 15, 2) == -1        # the scratch holds the layout
    assert sort(enough, 10, 15, 2) == -2            # every range in order: only the pointers are missing
    assert lib.pt_sort_scratch_bytes(0) == -1


def test_sort_scratch_is_the_librarys_layout():
    """hist, two key and two value buffers, each on a multiple of the carver's 256 bytes, in lay_sort()'s order, inside the size"""
    lib = P.lib()
    for tiles in (1, 8, 514):
        at = (ctypes.c_longlong * 5)()
        assert lib.pt_sort_scratch_offsets(tiles, at) == 0
        sizes = [4 * P.RADIX * tiles] + [4 * P.TILE * tiles] * 4
        want, end = [], 0
        for size in sizes:
            end = (end + 255) // 256 * 256
            want.append(end)
            end += size
        assert list(at) == want and lib.pt_sort_scratch_bytes(tiles) == end


def test_pass_counts_of_the_sort_tests_cover_both_result_buffers():
    assert [P.sort_passes(k) for k in P.MAX_KEYS] == [1, 1, 1, 2, 2, 3, 4, 8]


def test_scan_max_on_an_unsigned_type_does_not_compile(tmp_path):
    src = tmp_path / "unsigned_max.hip"
    for body in ("fpx::ScanMax::identity<uint32_t>()", "fpx::wave_reduce<fpx::ScanMax>(*p)"):
        src.write_text('#include "fpx_scan.hpp"\n__global__ void k(uint32_t* p) { *p = %s; }\n' % body)
        run = subprocess.run([P.HIPCC] + P.hipflags() + ["-I" + P.CSRC, "-fsyntax-only", str(src)], capture_output=True, text=True)
        assert run.returncode != 0 and "ScanMax scans signed integers" in run.stderr, run.stderr[-2000:]
    src.write_text('#include "fpx_scan.hpp"\n__global__ void k(int* p) { *p = fpx::wave_reduce<fpx::ScanMax>(*p); }\n')
    run = subprocess.run([P.HIPCC] + P.hipflags() + ["-I" + P.CSRC, "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]


# ------------------------------------------------------------------------------------------- references, by hand
def test_sum_references_by_hand():
    big = 0xFFFFFFFF
    out, all_ = P.ref_scan_array_excl("sum", "u32", np.array([big, 2, big, 5], np.uint32))
    assert_array_equal(out, np.array([0, big, 1, 0], np.uint32))       # wraps at the second element and again at the third
    assert all_ == 5 and out.dtype == np.uint32
    out, all_ = P.ref_scan_array_excl("sum", "u32", np.array([1, 2], np.uint32), start=big)
    assert_array_equal(out, np.array([big, 0], np.uint32))
    assert all_ == 2
    out, all_ = P.ref_scan_array_excl("sum", "i64", np.array([1 << 40, 3, 1 << 41], np.int64), start=7)
    assert_array_equal(out, np.array([7, (1 << 40) + 7, (1 << 40) + 10], np.int64))
    assert all_ == (1 << 40) + (1 << 41) + 10
    out, all_ = P.ref_scan_array_excl("sum", "int", np.zeros(0, np.int32), start=9)
    assert out.size == 0 and all_ == 9
    with pytest.raises(AssertionError):
        P.ref_scan_array_excl("sum", "int", np.array([1 << 30, 1 << 30, 1], np.int32))


def test_max_references_by_hand():
    v = np.array([-1, -1, 4, -1, -1, 9, 2], np.int32)                  # a run of -1 first: "nothing yet" until the 4
    out, all_ = P.ref_scan_array_excl("max", "int", v)
    assert_array_equal(out, np.array([-1, -1, -1, 4, 4, 4, 9], np.int32))
    assert all_ == 9
    out, all_ = P.ref_scan_array_excl("max", "int", v, start=5)
    assert_array_equal(out, np.array([5, 5, 5, 5, 5, 5, 9], np.int32))
    assert all_ == 9
    assert P.ref_scan_array_excl("max", "int", np.full(3, -1, np.int32))[1] == -1
    assert P.ref_scan_array_excl("max", "int", np.zeros(0, np.int32), start=3)[1] == 3
    low_heavy, high_heavy = (1 << 32) | 0xFFFFFFF0, (5 << 32) | 1      # the low words say the opposite of the values
    out, all_ = P.ref_scan_array_excl("max", "ll", np.array([low_heavy, high_heavy, low_heavy], np.int64))
    assert_array_equal(out, np.array([-1, low_heavy, high_heavy], np.int64))
    assert all_ == high_heavy


def test_wavefront_and_workgroup_references_by_hand():
    v = np.arange(128, dtype=np.int32)
    scan = P.ref_wave_incl_scan("sum", "int", v)
    assert scan[0] == 0 and scan[63] == 63 * 64 // 2 and scan[64] == 64 and scan[127] == sum(range(64, 128))   # begins anew per wavefront
    assert_array_equal(P.ref_wave_reduce("max", "int", v), np.repeat([63, 127], 64))
    out, total = P.ref_block_excl_scan("sum", "u32", np.array([[1, 2, 3], [4, 5, 6]], np.uint32), np.array([0xFFFFFFFF, 10], np.uint32))
    assert_array_equal(out, np.array([[0xFFFFFFFF, 0, 2], [10, 14, 19]], np.uint32))
    assert_array_equal(total, np.array([6, 15], np.uint32))            # without the carry
    out, total = P.ref_block_excl_scan("max", "int", np.array([[3, -1, 8]], np.int32), np.array([5], np.int32))
    assert_array_equal(out, np.array([[5, 5, 5]], np.int32))
    assert_array_equal(total, np.array([8], np.int32))
    assert_array_equal(P.ref_block_reduce("max", "int", np.array([[3, -1, 8], [-1, -1, -1]], np.int32)), np.array([[8, 8, 8], [-1, -1, -1]], np.int32))


def test_rank_and_sort_references_by_hand():
    flags = np.zeros((1, 256), np.uint8)
    flags[0, [1, 2, 255]] = 1
    rank, total = P.ref_block_rank(flags)
    assert list(rank[0, [0, 1, 2, 3, 255]]) == [0, 0, 1, 2, 2] and list(total) == [3]
    assert_array_equal(P.ref_sort_order(np.array([2, 1, 2, 0, 1], np.int32)), np.array([3, 1, 4, 0, 2], np.int32))   # ties in input order


# --------------------------------------------------------------------------------------------------- the generators
def test_generator_conditions():
    rng = np.random.default_rng(1)
    v = P.gen_sum("u32", 4096, rng)
    assert v.dtype == np.uint32 and v.max() == 0xFFFFFFFF and (np.cumsum(v.astype(np.int64))[63::64] >= 1 << 32).all()
    for n, headroom in ((1, 0), (768, 0), (3 * 1024 + 57, 1 << 20), (3 * 8192 + 57, 1 << 20)):
        v = P.gen_sum("int", n, rng, headroom=headroom)
        assert v.dtype == np.int32 and v.min() >= 1 << 16 and int(v.astype(np.int64).sum()) + headroom < 1 << 31
    v = P.gen_sum("i64", 3072, rng)
    assert v.dtype == np.int64 and v.min() >= 1 << 40
    carries_ = np.cumsum(v.reshape(-1, 64), axis=1)
    assert (carries_ > 1 << 32).all() and (carries_[:, -1] > 1 << 32).all()     # every carry, every wavefront total
    for t in ("i64", "ll"):
        v = P.gen_max(t, 4096, rng)
        live = v[v >= 0].astype(np.int64)
        hi, lo = live >> 32, live & 0xFFFFFFFF
        assert (v == -1).any() and v.min() == -1
        # the values' order by low word is the reverse of their order: both kinds are there
        assert ((hi < 4) & (lo >= 1 << 31)).any() and ((hi >= 4) & (lo < 16)).any() and (((hi < 4) & (lo >= 1 << 31)) | ((hi >= 4) & (lo < 16))).all()
        assert live[np.argmax(lo)] < live.max()
    v = P.gen_max("int", 4096, rng)
    assert v.dtype == np.int32 and v.min() == -1 and v.max() <= (1 << 31) - 4
    run = np.flatnonzero(v == -1)
    assert (np.diff(run) == 1).any()                                   # runs, not single entries
    w = P.with_peak(v, 1000)
    assert int(np.argmax(w)) == 1000 and (w == w.max()).sum() == 1 and v[1000] != w[1000]
    assert {0, 63, 64, 255, 256, 1023} <= set(P.peak_places(1024, 256)) and P.peak_places(1) == [0]


def test_flag_and_key_generators():
    rng = np.random.default_rng(2)
    counts = {kind: P.gen_flags(kind, 2, rng).sum(axis=1).tolist() for kind in P.FLAG_KINDS}
    assert counts["none"] == [0, 0] and counts["all"] == [256, 256] and counts["alternating"] == [128, 128]
    assert counts["only_thread_255"] == [1, 1] and counts["only_thread_0"] == [1, 1] and counts["lane_63_of_each_wavefront"] == [4, 4]
    assert P.gen_flags("only_thread_255", 1, rng)[0, 255] == 1 and list(np.flatnonzero(P.gen_flags("lane_63_of_each_wavefront", 1, rng)[0])) == [63, 127, 191, 255]
    for max_key in P.MAX_KEYS:
        for m in (0, 1, 257, 1000):
            for kind in P.KEY_KINDS:
                k = P.gen_keys(kind, m, max_key, rng)
                if k is None:
                    assert kind == "permutation" and m > max_key + 1
                    continue
                assert k.dtype == np.int32 and k.size == m and (m == 0 or (k.min() >= 0 and k.max() <= max_key))
                if kind == "permutation":
                    assert np.unique(k).size == m
                if kind == "few_distinct":
                    assert np.unique(k).size <= 5
                if kind == "descending" and m > 1:
                    assert (np.diff(k) <= 0).all() and k[0] == max_key
