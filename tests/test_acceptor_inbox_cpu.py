"""fpx_acceptor_inbox without a GPU: the two models of tests/acceptor_inbox_model.py agree on every stream of
tests/acceptor_inbox_streams.py, the named streams reach every branch the call has, a burst cut anywhere equals the whole
burst, and the symbol exists in every layer: libfpx.so, ctypes, include/fpx.h, the JNI shim, the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

from frankenpaxos_amd import wire
from tests import acceptor_inbox_model as M
from tests import acceptor_inbox_streams as AS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [nm for nm, _, _ in AS.NAMED]
ALL = NAMES + [nm for nm, _, _ in AS.SMALL]


def both(b):
    return M.Sequential(b.R, b.groups, b.S), M.Arrays(b.R, b.groups, b.S)


def run_same(models, b, what):
    outs = [m.run(b) for m in models]
    assert outs[0][:2] == outs[1][:2], what
    if outs[0][0] == 0:
        np.testing.assert_array_equal(outs[0][2], outs[1][2], err_msg="%s reply_kind" % (what,))
        np.testing.assert_array_equal(outs[0][3], outs[1][3], err_msg="%s reply_value" % (what,))
    M.assert_same_state(models[0], models[1], what)
    return outs[0]


@pytest.mark.parametrize("name", ALL)
def test_the_two_models_agree(name):
    b = AS.named(name)
    models = both(b)
    assert run_same(models, b, name)[0] == 0
    assert run_same(models, AS.follow_up(name), name + " follow-up")[0] == 0


@pytest.mark.parametrize("name", NAMES)
def test_the_streams_are_not_vacuous(name):
    b = AS.named(name)
    seq = M.Sequential(b.R, b.groups, b.S)
    st, _, rk, rv = M.Arrays(b.R, b.groups, b.S).run(b)
    assert st == 0
    c = M.conditions(b, seq, rk, rv)
    for what, count in c.items():
        assert count >= 1, (name, what, c)
    assert (b.kind == wire.OTHER).sum() >= 1
    # the follow-up meets the state the stream left: Nacks that only the earlier burst explains
    models = both(b)
    run_same(models, b, name)
    f = AS.follow_up(name)
    st, _, rk, rv = models[0].run(f)
    fresh = M.Sequential(b.R, b.groups, b.S).run(f)
    assert st == 0 and ((rk != fresh[2]) | (rv != fresh[3])).sum() >= 1


def test_by_hand():
    """three acceptors, every branch once, expectations spelled out"""
    P2A, P1A, MSR, BMSR, OTHER = M.P2A, M.P1A, M.MSR, M.BMSR, M.OTHER
    msgs = [  # kind, acceptor, slot, round, value
        (P2A, 0, 5, 2, 50),    # 0  votes: round 2
        (MSR, 0, 99, -7, 0),   # 1  5
        (P2A, 0, 3, 1, 51),    # 2  Nack(2)
        (P2A, 0, 5, 2, 52),    # 3  an equal round again with another value: votes, the cell keeps 52
        (P1A, 0, 0, 4, 0),     # 4  promises 4
        (P2A, 0, 9, 3, 53),    # 5  Nack(4): the Phase1a before it
        (BMSR, 0, 0, 0, 0),    # 6  5
        (P2A, 0, 9, 4, 54),    # 7  votes
        (P1A, 0, 0, 3, 0),     # 8  Nack(4)
        (OTHER, -1, -1, -1, -1),  # 9
        (MSR, 1, 0, 0, 0),     # 10 -1: acceptor 1 saw nothing
        (P1A, 2, 0, 0, 0),     # 11 promises 0 (round -1 before)
        (MSR, 0, 0, 0, 0),     # 12 9
    ]
    k, a, s, r, v = (np.array([m[j] for m in msgs], np.int32) for j in range(5))
    b = AS.Burst(3, 1, 16, 0, k, np.zeros(len(msgs), np.int32), a, s, r, v)
    want_kind = [M.PHASE2B, MSR, M.NACK, M.PHASE2B, M.PHASE1B, M.NACK, MSR, M.PHASE2B, M.NACK, 0, MSR, M.PHASE1B, MSR]
    want_value = [2, 5, 2, 2, 4, 4, 5, 4, 4, -1, -1, 0, 9]
    for model in both(b):
        st, bad, rk, rv = model.run(b)
        assert (st, bad) == (0, -1) and rk.tolist() == want_kind and rv.tolist() == want_value
        pr, mv = model.scalars()
        assert pr.tolist() == [[4, -1, 0]] and mv.tolist() == [[9, -1, -1]]
        vr, vv = model.cells()
        assert (vr[5, 0], vv[5, 0], vr[9, 0], vv[9, 0], vr[3, 0]) == (2, 52, 4, 54, -1) and (vr[:, 1:] == -1).all()


@pytest.mark.parametrize("name", ["n3000", "groups3", "grid2x2"])
def test_the_models_refuse_a_bad_burst_alike(name):
    b = AS.named(name)
    for what, c, at in AS.spoiled(b):
        models = both(b)
        got = run_same(models, c, what)
        assert got[:2] == (M.EINVAL, at), what
        M.assert_same_state(models[0], M.Sequential(b.R, b.groups, b.S), what)     # nothing applied


@pytest.mark.parametrize("name", NAMES)
def test_a_burst_cut_anywhere_equals_the_whole(name):
    b = AS.named(name)
    n = len(b)
    whole = M.Arrays(b.R, b.groups, b.S)
    _, _, rk, rv = whole.run(b)
    for k in (range(n + 1) if n < 1000 else list(range(0, n + 1, 97)) + [n - 1]):
        two = M.Arrays(b.R, b.groups, b.S) if k % 2 else M.Sequential(b.R, b.groups, b.S)
        h, t = two.run(b.cut(0, k)), two.run(b.cut(k, n))
        np.testing.assert_array_equal(np.r_[h[2], t[2]], rk)
        np.testing.assert_array_equal(np.r_[h[3], t[3]], rv)
        M.assert_same_state(two, whole, (name, k))


# ---- bindings -------------------------------------------------------------------------------------------------------
def test_libfpx_exports_both_symbols_and_the_prototypes_match():
    import frankenpaxos_amd as fa
    from frankenpaxos_amd import _lib

    L = fa.lib()
    for name in ("fpx_acceptor_inbox", "fpx_acceptor_inbox_dev"):
        assert hasattr(L, name) and len(_lib.SIGNATURES[name][1]) == 11
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    assert " T fpx_acceptor_inbox\n" in nm and " T fpx_acceptor_inbox_dev\n" in nm
    header = open(os.path.join(ROOT, "include", "fpx.h")).read()
    assert "int32_t fpx_acceptor_inbox_dev(fpx_ctx* ctx, int32_t n," in header
    assert "int32_t fpx_acceptor_inbox(fpx_ctx* ctx, int32_t n," in header
    assert "fpx_acceptor_phase1b_info_all[_dev] for the promisers" in header and "Acceptor.scala:122-254" in header
    assert hasattr(fa.Context, "acceptor_inbox") and hasattr(fa.Context, "acceptor_inbox_dev")
    # refused before anything touches a device
    assert L.fpx_acceptor_inbox(None, 0, *[None] * 6, 0, None, None) == 1
    assert L.fpx_acceptor_inbox_dev(None, 0, *[None] * 6, 0, None, None) == 1


def test_the_scala_native_matches_the_c_function():
    """name and arity (tests/test_jni_shim.py holds this for every native; here for the new one by name)"""
    import re

    scala = open(os.path.join(ROOT, "frankenpaxos_amd", "jni", "Native.scala")).read()
    shim = open(os.path.join(ROOT, "frankenpaxos_amd", "jni", "fpx_jni.c")).read()
    m = re.search(r"@native def acceptorInbox\(([^)]*)\): Int", scala)
    assert m, "Native.acceptorInbox is not declared"
    c = re.search(r"Java_frankenpaxos_gpu_Native_acceptorInbox\(([^)]*)\)", shim, re.S)
    assert c, "the shim has no acceptorInbox"
    assert len(m.group(1).split(",")) + 2 == len(c.group(1).split(","))       # + JNIEnv*, jclass


def test_the_cxx_mirror_compiles_with_the_new_method(tmp_path):
    src = tmp_path / "m.cpp"
    src.write_text('#include "frankenpaxos_amd/host/fpx.hpp"\n'
                   'int main() { auto p = &frankenpaxos::multipaxos::Phase2Engine::acceptorsHandleInbox; (void)p; return 0; }\n')
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
