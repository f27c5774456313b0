"""csrc/fpx_wire_emit.hpp -- the one emitter source of the wire adapter, compiled for the host encoders (g++) and the
device encoders (hipcc).  Here it is compiled by g++ ALONE into a small harness (tests/wire_emit_test.cpp), as
tests/test_fastdiv.py does for fpx_fastdiv.hpp: every layout's *_len equals the bytes its *_emit writes on a few million
field values that include every varint boundary and negative values (ten bytes), and the harness's bytes equal the host
encoders' of libfpx.so.  Also the C ABI of the device encoders and of the bytes-to-bytes tick as far as it can be checked
without a GPU: the names are exported, and bad arguments are refused before a device is touched."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "build")

EDGES = [0, 127, 128, 16383, 16384, 2 ** 21 - 1, 2 ** 21, 2 ** 28 - 1, 2 ** 28, 2 ** 31 - 1, -1, -2 ** 31]
NEW = ["fpx_wire_encode_replica_chosen_dev", "fpx_wire_encode_phase2b_batch_dev", "fpx_wire_encode_leader_nack_dev",
       "fpx_wire_phase2_tick"]


@pytest.fixture(scope="module")
def harness():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libwire_emit_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "wire_emit_test.cpp"), "-o", so])
    H = C.CDLL(so)
    H.check_lens.restype = C.c_int64
    H.check_lens.argtypes = [C.c_int64, C.c_uint64]
    for name in ("emit_chosen", "emit_phase2a", "emit_phase2b", "emit_nack", "emit_ints"):
        getattr(H, name).restype = C.c_int64
    H.emit_chosen.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
    H.emit_phase2a.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
    H.emit_phase2b.argtypes = [C.c_void_p] + [C.c_int32] * 5
    H.emit_nack.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    H.emit_ints.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p]
    return H


@pytest.fixture(scope="module")
def L():
    from frankenpaxos_amd import wire

    return wire._L()


def test_len_equals_the_bytes_emit_writes(harness):
    assert harness.check_lens(3_000_000, 12345) == 0


def test_the_header_has_no_hip_in_it():
    src = open(os.path.join(ROOT, "frankenpaxos_amd", "csrc", "fpx_wire_emit.hpp")).read()
    for word in ("__global__", "__device__", "__shared__", "hip/", "threadIdx", "__builtin_amdgcn"):
        assert word not in src, word


def _host(fn, *args):
    out = np.full(70100, 0xEE, np.uint8)
    n = fn(out.ctypes.data, len(out), *args)
    assert n > 0
    return out[:n].tobytes()


def _mine(fn, *args):
    out = np.full(70100, 0xEE, np.uint8)
    n = fn(out.ctypes.data, *args)
    assert n > 0 and out[n] == 0xEE
    return out[:n].tobytes()


def test_harness_bytes_equal_the_host_encoders(harness, L):
    rng = np.random.default_rng(5)
    value = rng.integers(0, 256, 70000, dtype=np.uint8)
    vp = value.ctypes.data
    for slot, round_ in itertools.product(EDGES, EDGES):
        for vl, noop in ((0, 0), (1, 0), (127, 0), (128, 0), (300, 0), (20000, 0), (5, 1), (-3, 0)):
            assert _mine(harness.emit_chosen, slot, vp, vl, noop) == _host(L.fpx_wire_encode_replica_chosen, slot, vp, vl, noop)
            assert _mine(harness.emit_chosen, slot, vp, vl, noop) == \
                _host(L.fpx_wire_mencius_encode_replica_chosen, slot, vp, vl, noop)
        for vl, noop in ((0, 0), (128, 0), (20000, 0), (9, 1)):
            assert _mine(harness.emit_phase2a, 1, slot, round_, vp, vl, noop) == \
                _host(L.fpx_wire_encode_proxy_leader_phase2a, slot, round_, vp, vl, noop)
            assert _mine(harness.emit_phase2a, 2, slot, round_, vp, vl, noop) == \
                _host(L.fpx_wire_encode_acceptor_phase2a, slot, round_, vp, vl, noop)
        for g, a in ((0, 0), (127, 128), (128, 127), (255, 255), (-1, 3)):
            assert _mine(harness.emit_phase2b, 0, g, a, slot, round_) == \
                _host(L.fpx_wire_encode_proxy_leader_phase2b, g, a, slot, round_)
            assert _mine(harness.emit_phase2b, 1, g, a, slot, round_) == \
                _host(L.fpx_wire_mencius_encode_proxy_leader_phase2b, a, slot, round_)
        v = np.array([slot, round_], np.int32)
        assert _mine(harness.emit_ints, 1, 2, v.ctypes.data) == _host(L.fpx_wire_encode_acceptor_phase1a, slot, round_)
        assert _mine(harness.emit_ints, 2, 2, v.ctypes.data) == \
            _host(L.fpx_wire_mencius_encode_replica_chosen_noop_range, slot, round_)
    for r in EDGES:
        assert _mine(harness.emit_nack, 0, r) == _host(L.fpx_wire_encode_leader_nack, r)
        assert _mine(harness.emit_nack, 1, r) == _host(L.fpx_wire_mencius_encode_leader_nack, r)


def test_library_exports_the_new_names():
    import frankenpaxos_amd

    lib = C.CDLL(frankenpaxos_amd._lib.SO_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "fpx_wire.h")).read()
    for name in NEW:
        assert name + "(" in hdr, name


def test_bad_arguments_are_refused_without_a_gpu(L):
    """a NULL context or n < 0 is FPX_EINVAL before anything touches a device (there is none on this side of the suite)"""
    EINVAL = 1
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    fake = C.c_void_p(p)  # never dereferenced: n < 0 is refused first
    for ctx, n in ((None, 4), (fake, -1)):
        assert L.fpx_wire_encode_replica_chosen_dev(ctx, n, None, p, None, p, 8, p, p, p, 8, p, p) == EINVAL
        assert L.fpx_wire_encode_phase2b_batch_dev(ctx, 0, n, p, p, p, None, 0, p, 8, p, 4, p) == EINVAL
        assert L.fpx_wire_encode_leader_nack_dev(ctx, 0, n, p, p, 8, p, 4, p) == EINVAL
        cnt, need, bad = C.c_int64(), C.c_int64(), C.c_int32()
        assert L.fpx_wire_phase2_tick(ctx, p, 8, p, n, p, 8, p, C.byref(cnt), None, C.byref(need), C.byref(bad)) == EINVAL
