"""What the direct tests of the workgroup primitives share (frankenpaxos_amd/csrc/fpx_scan.hpp, fpx_burst_sort.hpp): the
build of the test-only harness tests/primitives_harness.hip into tests/_build/libfpx_primitives.so, the table of its
launchers, exact integer references of every primitive, and seeded generators of the values at which scans and radix
sorts go wrong.  tests/test_primitives_cpu.py checks this module without a GPU; tests/test_gpu_primitives.py compares
the kernels with the references.

Everything is integer and every comparison is exact.  Types are named as in the launchers: int, u32 (uint32_t),
i64 (int64_t), ll (long long)."""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frankenpaxos_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "primitives_harness.hip")
BUILD = os.path.join(ROOT, "tests", "_build")
SO_PATH = os.path.join(BUILD, "libfpx_primitives.so")
LOG_PATH = os.path.join(BUILD, "libfpx_primitives.log")     # what the compiler printed when SO_PATH was built
HEADERS = ("fpx_scan.hpp", "fpx_burst_sort.hpp", "fpx_scratch.hpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

NP = {"int": np.int32, "u32": np.uint32, "i64": np.int64, "ll": np.int64}
GUARD_WORD = {"int": 0x5A5A5A5A, "u32": 0x5A5A5A5A, "i64": 0x5A5A5A5A5A5A5A5A, "ll": 0x5A5A5A5A5A5A5A5A}
TILE = 256          # pairs per sort tile
RADIX = 16          # digit values per pass
RADIX_BITS = 4
MAX_KEYS = (0, 1, 15, 16, 255, 256, 4097, (1 << 31) - 1)    # of the sort tests: 1, 1, 1, 2, 2, 3, 4 and 8 passes


# ---------------------------------------------------------------------------------------------------------- the build
def hipflags():
    """the HIPFLAGS of csrc/Makefile, for gfx950"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        m = re.search(r"^HIPFLAGS \?= (.*)$", f.read(), re.M)
    return m.group(1).replace("$(ARCH)", "gfx950").split()


def build_command(out):
    return [HIPCC] + hipflags() + ["-shared", "-I" + CSRC, "-o", out, SOURCE]


def stale():
    if not os.path.exists(SO_PATH):
        return True
    built = os.path.getmtime(SO_PATH)
    return any(os.path.getmtime(p) > built for p in [SOURCE] + [os.path.join(CSRC, h) for h in HEADERS])


def build():
    """tests/_build/libfpx_primitives.so, rebuilt when it is missing or older than the harness or one of HEADERS; FPX_PRIMITIVES_LIB
    names another build of it (profiles/primitive_tests.md), taken as it is"""
    other = os.environ.get("FPX_PRIMITIVES_LIB")
    if other:
        return other
    if stale():
        os.makedirs(BUILD, exist_ok=True)
        tmp = SO_PATH + ".%d.tmp" % os.getpid()
        run = subprocess.run(build_command(tmp), capture_output=True, text=True)
        if run.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (SOURCE, run.stderr[-8000:]))
        with open(LOG_PATH, "w") as f:
            f.write(run.stdout + run.stderr)
        os.replace(tmp, SO_PATH)
    return SO_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.pt_sort_scratch_bytes.restype = ctypes.c_longlong
    return _lib


# ------------------------------------------------------------------------------------------------- the launcher table
def _wave():
    rows = {}
    for fn in ("wave_incl_scan", "wave_reduce"):
        for op, t in (("sum", "int"), ("sum", "u32"), ("sum", "i64"), ("sum", "ll"), ("max", "int"), ("max", "i64"), ("max", "ll")):
            for threads in (64, 256):
                rows["pt_%s_%s_%s_%d" % (fn, op, t, threads)] = dict(fn=fn, op=op, type=t, threads=threads)
    return rows


def _array():
    rows = {}
    for op, t, threads, per in (("sum", "u32", 256, 1), ("sum", "int", 1024, 1), ("sum", "int", 1024, 8), ("max", "int", 256, 1),
                                ("max", "int", 1024, 1), ("max", "ll", 1024, 1)):
        for start in (False, True):
            name = "pt_scan_array_excl_%s_%s_%d_%d%s" % (op, t, threads, per, "_start" if start else "")
            rows[name] = dict(fn="scan_array_excl", op=op, type=t, threads=threads, per=per, start=start)
    return rows


# every launcher of the harness: name -> what it instantiates
LAUNCHERS = dict(_wave())
LAUNCHERS.update({
    "pt_block_excl_scan_sum_u32_256": dict(fn="block_excl_scan", op="sum", type="u32", threads=256, total=False),
    "pt_block_excl_scan_sum_u32_256_total": dict(fn="block_excl_scan", op="sum", type="u32", threads=256, total=True),
    "pt_block_excl_scan_sum_u32_512": dict(fn="block_excl_scan", op="sum", type="u32", threads=512, total=False),
    "pt_block_excl_scan_sum_i64_1024_total": dict(fn="block_excl_scan", op="sum", type="i64", threads=1024, total=True),
    "pt_block_excl_scan_max_int_256": dict(fn="block_excl_scan", op="max", type="int", threads=256, total=False),
    "pt_block_excl_scan_max_ll_256": dict(fn="block_excl_scan", op="max", type="ll", threads=256, total=False),
    "pt_block_reduce_sum_u32_256": dict(fn="block_reduce", op="sum", type="u32", threads=256),
    "pt_block_reduce_sum_int_256": dict(fn="block_reduce", op="sum", type="int", threads=256),
    "pt_block_reduce_max_int_256": dict(fn="block_reduce", op="max", type="int", threads=256),
    "pt_block_reduce_max_ll_256": dict(fn="block_reduce", op="max", type="ll", threads=256),
    "pt_block_reduce_max_int_1024": dict(fn="block_reduce", op="max", type="int", threads=1024),
    "pt_block_reduce_max_i64_1024": dict(fn="block_reduce", op="max", type="i64", threads=1024),     # (no caller)
    "pt_block_rank_256": dict(fn="block_rank", threads=256),
    "pt_reduce_twice_sum_u32_256": dict(fn="reduce_twice", op="sum", type="u32", threads=256),
    "pt_reduce_twice_sum_int_256": dict(fn="reduce_twice", op="sum", type="int", threads=256),          # k_mk_total
    "pt_reduce_twice_max_ll_256": dict(fn="reduce_twice", op="max", type="ll", threads=256),
    "pt_scan_twice_same_words_sum_u32_256": dict(fn="scan_twice_same_words", op="sum", type="u32", threads=256),
    "pt_scan_twice_other_words_sum_u32_512": dict(fn="scan_twice_other_words", op="sum", type="u32", threads=512),
    "pt_burst_sort": dict(fn="burst_sort"),
    "pt_sort_scratch_bytes": dict(fn="helper"),
    "pt_sort_scratch_offsets": dict(fn="helper"),
    "pt_rounds": dict(fn="helper"),
    "pt_guard_words": dict(fn="helper"),
    "pt_array_pad": dict(fn="helper"),
    "pt_array_blocks": dict(fn="helper"),
})
LAUNCHERS.update(_array())

# Every call site of a primitive in frankenpaxos_amd/csrc, with the value type READ AT THE CALL SITE (the template
# arguments do not name it), and the launcher that runs the same instantiation: (file, text searched for, launcher, how
# many such calls the file has).  A wavefront function does not depend on the workgroup's size, so its launchers of 64 and
# of 256 threads both stand for a call.  tests/test_primitives_cpu.py counts the texts in every file again: whoever adds a
# call site comes here, reads its type, and either finds its launcher or writes one with its test.
USES = [
    ("fpx_phase1b_msgs.hpp", "wave_incl_scan<", "pt_wave_incl_scan_sum_int_256", 1),          # int wi
    ("fpx_phase1b_msgs.hpp", "wave_incl_scan<", "pt_wave_incl_scan_sum_i64_256", 1),          # int64_t ui
    ("fpx_epaxos_mk.hpp", "wave_reduce<", "pt_wave_reduce_sum_int_256", 2),                   # int u, not_one
    ("fpx_epx_leader.hpp", "block_excl_scan<", "pt_block_excl_scan_sum_u32_256", 1),
    ("fpx_epaxos_mk.hpp", "block_excl_scan<", "pt_block_excl_scan_sum_u32_256", 1),
    ("fpx_phase1_info.hpp", "block_excl_scan<", "pt_block_excl_scan_sum_i64_1024_total", 1),
    ("fpx_acceptor_inbox.hpp", "block_excl_scan<", "pt_block_excl_scan_max_ll_256", 2),
    ("fpx_mencius_acceptor_inbox.hpp", "block_excl_scan<", "pt_block_excl_scan_max_ll_256", 2),
    ("fpx_epaxos.hip", "block_excl_scan<", "pt_block_excl_scan_sum_u32_512", 2),              # 64 * RS_SW threads
    ("fpx_epaxos.hip", "block_excl_scan<", "pt_block_excl_scan_sum_u32_256", 1),
    ("fpx_replica_inbox.hpp", "block_excl_scan<", "pt_block_excl_scan_max_int_256", 1),
    ("fpx_depgraph_dev.hpp", "block_excl_scan<", "pt_block_excl_scan_sum_u32_256_total", 1),
    ("fpx_epx_leader.hpp", "block_reduce<", "pt_block_reduce_sum_u32_256", 1),
    ("fpx_phase1b_msgs.hpp", "block_reduce<", "pt_block_reduce_max_int_1024", 1),             # int ms
    ("fpx_epaxos_mk.hpp", "block_reduce<", "pt_block_reduce_sum_int_256", 3),                 # int u, not_one; int s
    ("fpx_acceptor_inbox.hpp", "block_reduce<", "pt_block_reduce_max_ll_256", 1),
    ("fpx_epaxos.hip", "block_reduce<", "pt_block_reduce_max_int_256", 1),
    ("fpx_replica_inbox.hpp", "block_reduce<", "pt_block_reduce_max_int_256", 1),
    ("fpx_depgraph_dev.hpp", "block_reduce<", "pt_block_reduce_sum_u32_256", 3),
    ("fpx_epx_leader.hpp", "scan_array_excl<", "pt_scan_array_excl_sum_u32_256_1", 1),
    ("fpx_replica_msgs.hpp", "scan_array_excl<", "pt_scan_array_excl_sum_int_1024_1", 1),
    ("fpx_epaxos_mk.hpp", "scan_array_excl<", "pt_scan_array_excl_sum_u32_256_1", 1),
    ("fpx_tally_msgs.hpp", "scan_array_excl<", "pt_scan_array_excl_sum_int_1024_1", 1),
    ("fpx_acceptor_inbox.hpp", "scan_array_excl<", "pt_scan_array_excl_max_ll_1024_1", 1),    # AI_SCAN_THREADS
    ("fpx_mencius_acceptor_inbox.hpp", "scan_array_excl<", "pt_scan_array_excl_sum_int_1024_1", 1),
    ("fpx_epaxos.hip", "scan_array_excl<", "pt_scan_array_excl_max_int_256_1_start", 1),
    ("fpx_replica_inbox.hpp", "scan_array_excl<", "pt_scan_array_excl_max_int_1024_1", 1),    # RI_SCAN_THREADS
    ("fpx_burst_sort.hpp", "scan_array_excl<", "pt_scan_array_excl_sum_int_1024_8", 1),       # Len = long long
    ("fpx_replica_msgs.hpp", "block_rank(", "pt_block_rank_256", 2),
    ("fpx_mencius_msgs.hpp", "block_rank(", "pt_block_rank_256", 1),
    ("fpx_tally_msgs.hpp", "block_rank(", "pt_block_rank_256", 2),
    ("fpx_replica_inbox.hpp", "block_rank(", "pt_block_rank_256", 3),
    ("fpx_api.hip", "burst_sort(", "pt_burst_sort", 3),
]
# the same texts where they are no call from outside: the definitions, the primitives' calls of each other, a comment
NOT_USES = {
    ("fpx_scan.hpp", "wave_incl_scan<"): 1, ("fpx_scan.hpp", "wave_reduce<"): 1, ("fpx_scan.hpp", "block_excl_scan<"): 1,
    ("fpx_scan.hpp", "block_rank("): 1, ("fpx_burst_sort.hpp", "burst_sort("): 2,
}


def expected_call_sites():
    want = dict(NOT_USES)
    for name, needle, _, count in USES:
        want[(name, needle)] = want.get((name, needle), 0) + count
    return want


def count_call_sites():
    """{(file, text): occurrences} over every source file of csrc, for the texts USES searches for"""
    needles = sorted({needle for _, needle, _, _ in USES})
    got = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".inc", ".cpp", ".h")):
            with open(os.path.join(CSRC, name)) as f:
                text = f.read()
            for needle in needles:
                if text.count(needle):
                    got[(name, needle)] = text.count(needle)
    return got


# ------------------------------------------------------------------------------------------------------ the references
def wrap(a, t):
    """exact int64 results as the kernel's type holds them: a uint32_t sum wraps, nothing else may"""
    a = np.asarray(a, dtype=np.int64)
    if t == "u32":
        return (a % (1 << 32)).astype(np.uint32)
    if t == "int":
        assert a.size == 0 or (a.min() >= -(1 << 31) and a.max() < (1 << 31)), "a signed sum overflowed: the generator's fault"
    return a.astype(NP[t])


def identity(op):
    return 0 if op == "sum" else -1


def incl_scan(op, v, axis=-1):
    """exact inclusive scan along `axis`, int64"""
    v = np.asarray(v).astype(np.int64)
    return np.cumsum(v, axis=axis, dtype=np.int64) if op == "sum" else np.maximum.accumulate(v, axis=axis)


def excl_scan(op, v, first):
    """exact exclusive scan of the rows of v[rows, n] that begins with first[rows]: (scan, op over `first` and the whole row)"""
    v = np.asarray(v).astype(np.int64)
    first = np.asarray(first, dtype=np.int64).reshape(-1, 1)
    inc = incl_scan(op, np.concatenate([first, v], axis=1))
    return inc[:, :-1], inc[:, -1]


def ref_wave_incl_scan(op, t, v):
    return wrap(incl_scan(op, np.asarray(v).reshape(-1, 64)).reshape(-1), t)


def ref_wave_reduce(op, t, v):
    inc = incl_scan(op, np.asarray(v).reshape(-1, 64))
    return wrap(np.repeat(inc[:, -1], 64), t)


def ref_block_excl_scan(op, t, v, carry):
    """v[blocks, threads], carry[blocks] -> (every thread's return value, the block's total WITHOUT the carry)"""
    v = np.asarray(v)
    out, _ = excl_scan(op, v, carry)
    total = incl_scan(op, v)[:, -1]
    return wrap(out, t), wrap(total, t)


def ref_block_reduce(op, t, v):
    v = np.asarray(v)
    return wrap(np.repeat(incl_scan(op, v)[:, -1:], v.shape[1], axis=1), t)


def ref_scan_array_excl(op, t, a, start=None):
    """(a's exclusive scan beginning with `start`, op over `start` and all of a)"""
    out, all_ = excl_scan(op, np.asarray(a).reshape(1, -1), [identity(op) if start is None else start])
    return wrap(out[0], t), wrap(all_, t)[0]


def ref_block_rank(flags):
    """flags[blocks, 256] -> (rank among the block's flagged threads, in every thread; the block's count)"""
    f = (np.asarray(flags) != 0).astype(np.int64)
    inc = np.cumsum(f, axis=1)
    return (inc - f).astype(np.int32), inc[:, -1].astype(np.int32)


def ref_sort_order(keys):
    return np.argsort(np.asarray(keys), kind="stable").astype(np.int32)


def sort_passes(max_key):
    """how many passes burst_sort runs for keys 0 .. max_key: one per RADIX_BITS bits of max_key, and never none"""
    return max(1, (int(max_key).bit_length() + RADIX_BITS - 1) // RADIX_BITS)


# ------------------------------------------------------------------------------------------------------ the generators
def gen_sum(t, n, rng, headroom=0):
    """n summands of type t.  u32: up to 2^32 - 1 (with both ends present), so the sum wraps every few elements.  int: each at
    least 2^16, the total with `headroom` below 2^31 (signed overflow is undefined and not the kernel's fault).  i64, ll:
    around 2^40, so every carry and wavefront total exceeds 2^32"""
    if t == "u32":
        v = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        if n:
            v[rng.integers(0, n, size=max(1, n // 16))] = 0xFFFFFFFF
        return v
    if t == "int":
        if n == 0:
            return np.zeros(0, np.int32)
        spare = ((1 << 31) - 1 - int(headroom) - n * (1 << 16)) // n
        assert spare >= 1, "no int sum of %d elements of 2^16 stays below 2^31" % n
        return ((1 << 16) + rng.integers(0, min(spare, 1 << 20), size=n)).astype(np.int32)
    return ((1 << 40) + rng.integers(0, 1 << 36, size=n)).astype(np.int64)


def gen_max(t, n, rng, minus_runs=True):
    """n values >= -1 to take maxima of.  int: up to 2^31 - 3.  i64, ll: high and low words disagree -- half the values have a
    small high word under a low word with its top bit set, the other half a large high word over a small low word -- so a
    comparison or a shuffle of the low words alone gives another answer.  minus_runs: runs of -1, "nothing yet", among them.
    The largest value generated is at least 2 below the type's largest, which leaves with_peak() room"""
    if t == "int":
        v = rng.integers(0, (1 << 31) - 3, size=n).astype(np.int64)
    else:
        low_heavy = (rng.integers(0, 4, size=n) << 32) | rng.integers(1 << 31, 1 << 32, size=n)
        high_heavy = (rng.integers(4, 1 << 30, size=n) << 32) | rng.integers(0, 16, size=n)
        v = np.where(rng.integers(0, 2, size=n) == 1, low_heavy, high_heavy).astype(np.int64)
    if minus_runs and n:
        for _ in range(max(1, n // 96)):
            at = int(rng.integers(0, n))
            v[at:at + int(rng.integers(1, 70))] = -1
    return v.astype(NP[t])


def with_peak(v, at):
    """a copy of v whose one largest value sits at index `at` (of the flattened array)"""
    v = np.array(v)
    flat = v.reshape(-1)
    flat[at] = int(flat.max()) + 1
    return v


def peak_places(n, threads=None):
    """where a maximum must be tried in n elements: element 0, the last, lane 63 and lane 0 of a wavefront, either side of
    every step of `threads` elements"""
    places = {0, n - 1, 63, 64, 127, 128, n // 2}
    if threads:
        for s in range(threads, n, threads):
            places |= {s - 1, s}
    return sorted(p for p in places if 0 <= p < n)


FLAG_KINDS = ("none", "all", "alternating", "only_thread_255", "only_thread_0", "lane_63_of_each_wavefront", "random")


def gen_flags(kind, blocks, rng):
    f = np.zeros((blocks, 256), np.uint8)
    if kind == "all":
        f[:] = 1
    elif kind == "alternating":
        f[:, 1::2] = 1
    elif kind == "only_thread_255":
        f[:, 255] = 1
    elif kind == "only_thread_0":
        f[:, 0] = 1
    elif kind == "lane_63_of_each_wavefront":
        f[:, 63::64] = 1
    elif kind == "random":
        f[:] = rng.integers(0, 2, size=f.shape)
    else:
        assert kind == "none", kind
    return f


KEY_KINDS = ("all_equal", "two_values", "permutation", "few_distinct", "descending")


def gen_keys(kind, m, max_key, rng):
    """m keys in 0 .. max_key, or None where the kind cannot be had (a permutation of m keys needs m <= max_key + 1).
    few_distinct: at most 5 values spread over every digit of max_key, so each tile and each wavefront holds many equal keys
    and only a stable sort keeps their input order"""
    if kind == "all_equal":
        k = np.full(m, max_key, np.int64)
    elif kind == "two_values":
        k = np.where(rng.integers(0, 2, size=m) == 1, max_key, max_key // 3)
    elif kind == "permutation":
        if m > max_key + 1:
            return None
        if max_key + 1 <= 4 * max(m, 1):
            k = rng.permutation(max_key + 1)[:m]
        else:   # distinct keys from a range too large to permute: distinct offsets on a stride
            k = rng.permutation(m) * (max_key // max(m, 1)) + rng.integers(0, max(1, max_key // max(m, 1)), size=m)
    elif kind == "few_distinct":
        values = np.unique(np.array([0, max_key, max_key // 2, max_key // 3, (max_key * 5) // 7], np.int64))
        k = values[rng.integers(0, len(values), size=m)]
    else:
        assert kind == "descending", kind
        k = np.linspace(max_key, 0, num=m).astype(np.int64) if m else np.zeros(0, np.int64)
    k = np.asarray(k, dtype=np.int64)
    assert k.size == 0 or (k.min() >= 0 and k.max() <= max_key)
    return k.astype(np.int32)
