"""What the direct test of the second form's record shares (frankenpaxos_amd/csrc/fpx_epaxos_rec.hpp): the build of the
test-only harness tests/epaxos_record_harness.hip into tests/_build/libfpx_epaxos_record.so, the way tests/primitives.py
builds its own, and the records to try."""
import ctypes
import itertools
import os
import subprocess

import numpy as np

from tests import primitives as P

SOURCE = os.path.join(P.ROOT, "tests", "epaxos_record_harness.hip")
SO_PATH = os.path.join(P.BUILD, "libfpx_epaxos_record.so")
HEADER = os.path.join(P.CSRC, "fpx_epaxos_rec.hpp")


def build():
    """tests/_build/libfpx_epaxos_record.so, rebuilt when it is missing or older than the harness or the header;
    FPX_EPAXOS_RECORD_LIB names another build of it (profiles/epaxos_tick_path_tests.md), taken as it is"""
    other = os.environ.get("FPX_EPAXOS_RECORD_LIB")
    if other:
        return other
    if not os.path.exists(SO_PATH) or any(os.path.getmtime(p) > os.path.getmtime(SO_PATH) for p in (SOURCE, HEADER)):
        os.makedirs(P.BUILD, exist_ok=True)
        tmp = SO_PATH + ".%d.tmp" % os.getpid()
        run = subprocess.run([P.HIPCC] + P.hipflags() + ["-shared", "-I" + P.CSRC, "-o", tmp, SOURCE], capture_output=True, text=True)
        if run.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (SOURCE, run.stderr[-8000:]))
        os.replace(tmp, SO_PATH)
    return SO_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.er_round_trip.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 12
    return _lib


INDICES = (0, 1, (1 << 20) - 1, 1 << 20, (1 << 21) - 1)
RANKS = (0, 1, 2047, 2048, (1 << 20) - 1, 1 << 20, (1 << 21) - 2)
NUMBERS = (0, (1 << 31) - 1)


def headers(n):
    """every legal (leader, resp_mask, seen_mask): resp_mask is n - 2 of the non-leaders, seen_mask contains it and excludes
    the leader (so it is resp_mask, or all the non-leaders)"""
    full = (1 << n) - 1
    out = []
    for L in range(n):
        for q in range(n):
            if q != L:
                resp = full & ~(1 << L) & ~(1 << q)
                out += [(L, resp, resp), (L, resp, resp | (1 << q))]
    return out


def records(n):
    """the columns of the records to try, as int32 arrays: every header with both is_set values under a walk through the
    index, number and rank values; every rank value in every rank position against two settings of the other ranks (all
    zero, all 2^21 - 2); every index value"""
    rows = []
    hs = headers(n)
    walk = itertools.cycle(itertools.product(INDICES, NUMBERS))
    for j, ((L, resp, seen), is_set) in enumerate(itertools.product(hs, (0, 1))):
        i, x = next(walk)
        rows.append((i, x, L, is_set, resp, seen) + tuple(RANKS[(j + q) % len(RANKS)] for q in range(n)))
    for j, (q, v, rest) in enumerate(itertools.product(range(n), RANKS, (0, (1 << 21) - 2))):
        L, resp, seen = hs[j % len(hs)]
        rk = [rest] * n
        rk[q] = v
        rows.append((INDICES[j % len(INDICES)], NUMBERS[j % 2], L, j & 1, resp, seen) + tuple(rk))
    for j, (i, x) in enumerate(itertools.product(INDICES, NUMBERS)):
        L, resp, seen = hs[(3 * j) % len(hs)]
        rows.append((i, x, L, j & 1, resp, seen) + tuple(RANKS[(2 * j + q) % len(RANKS)] for q in range(n)))
    rng = np.random.default_rng(n)
    for j in range(3000):   # and a few thousand mixed ones, every field an edge value or a random one
        L, resp, seen = hs[int(rng.integers(len(hs)))]
        edge = lambda vals, hi: int(vals[int(rng.integers(len(vals)))]) if rng.random() < 0.5 else int(rng.integers(0, hi))
        rows.append((edge(INDICES, 1 << 21), edge(NUMBERS, 1 << 31), L, int(rng.integers(2)), resp, seen)
                    + tuple(edge(RANKS, (1 << 21) - 1) for _ in range(n)))
    cols = np.array(rows, dtype=np.int64).T
    return [np.ascontiguousarray(c, np.int32) for c in cols[:6]], np.ascontiguousarray(cols[6:], np.int32)
