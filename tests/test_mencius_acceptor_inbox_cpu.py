"""fpx_mencius_acceptor_inbox without a GPU: the two models of tests/mencius_acceptor_inbox_model.py agree on every stream
of tests/mencius_acceptor_inbox_streams.py, the named streams reach every branch the call has, a burst cut anywhere
equals the whole burst, and the symbol exists in every layer: libfpx.so, ctypes, include/fpx.h, the JNI shim, the C++
mirror."""
import os
import re
import subprocess

import numpy as np
import pytest

from frankenpaxos_amd import wire
from tests import mencius_acceptor_inbox_model as M
from tests import mencius_acceptor_inbox_streams as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [nm for nm, _, _ in MS.NAMED]
ALL = NAMES + [nm for nm, _, _ in MS.SMALL]
P2A, NR, P1A, OTHER = M.P2A, M.NR, M.P1A, M.OTHER


def both(b):
    return M.Sequential(b.L, b.A, b.R, b.S), M.Arrays(b.L, b.A, b.R, b.S)


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
    b = MS.named(name)
    models = both(b)
    assert run_same(models, b, name)[0] == 0
    assert run_same(models, MS.follow_up(name), name + " follow-up")[0] == 0


@pytest.mark.parametrize("name", NAMES)
def test_the_streams_are_not_vacuous(name):
    b = MS.named(name)
    assert len(b) >= 255
    st, _, rk, rv = M.Arrays(b.L, b.A, b.R, b.S).run(b)
    assert st == 0
    c = M.conditions(b, rk, rv)
    for what, count in c.items():
        if b.A == 1 and what in ("range_owning_nothing", "start_of_another_group"):
            assert count == 0
        else:
            assert count >= 1, (name, what, c)
    assert (b.kind == OTHER).sum() >= 1 and (b.kind == P1A).sum() >= 1
    # the follow-up meets the state the stream left: Nacks that only the earlier burst explains
    models = both(b)
    run_same(models, b, name)
    f = MS.follow_up(name)
    st, _, rk, rv = models[0].run(f)
    fresh = M.Sequential(b.L, b.A, b.R, b.S).run(f)
    assert st == 0 and ((rk != fresh[2]) | (rv != fresh[3])).sum() >= 1


def test_the_chunked_stream_has_300_accepted_ranges_at_one_acceptor():
    b = MS.named("many_ranges")
    _, _, rk, rv = M.Arrays(b.L, b.A, b.R, b.S).run(b)
    assert M.conditions(b, rk, rv)["most_accepted_ranges_at_one_acceptor"] >= 300


def test_the_named_streams_cover_the_shapes():
    kws = [kw for _, _, kw in MS.NAMED]
    bs = [MS.named(nm) for nm in NAMES]
    assert {255, 256, 257, 3000} <= {len(b) for b in bs}
    assert {b.L for b in bs} == {1, 2, 3} and {b.A for b in bs} == {1, 2, 3} and {3, 4, 65} <= {b.R for b in bs}
    assert any(b.flags & 4 for b in bs) and any(kw.get("one") for kw in kws)
    assert all(b.S % b.L == 0 and 100 <= b.S <= 1000 for b in bs)
    assert [len(MS.named(nm)) for nm, _, _ in MS.SMALL] == [0, 1]


def test_by_hand():
    """L = 2, A = 2: the acceptor (leader group 1, acceptor group 0, index 0) owns slots 1, 5, 9, 13, ...; expectations
    spelled out"""
    msgs = [  # kind, group, acceptor, slot, slot_end, round, value
        (P2A, 2, 0, 5, -1, 2, 50),    # 0  votes: round 2
        (NR, 2, 0, 1, 11, 2, 0),      # 1  rows 0 .. 4 -> slots 1, 5, 9 are Noop in round 2 (5 overwritten in an equal round)
        (P2A, 2, 0, 9, -1, 2, 51),    # 2  votes: 9 keeps 51
        (NR, 2, 0, 3, 8, 1, 0),       # 3  Nack(2)
        (NR, 2, 0, 3, 4, 3, 0),       # 4  starts in acceptor group 1's row and owns nothing: votes, round 3
        (P2A, 2, 0, 1, -1, 2, 52),    # 5  Nack(3): the range before it
        (NR, 2, 0, 7, 7, 3, 0),       # 6  empty: votes
        (P1A, 2, 0, 0, 0, 5, 0),      # 7  promises 5
        (NR, 2, 0, 1, 2, 4, 0),       # 8  Nack(5): the Phase1a before it
        (NR, 2, 0, 9, 15, 5, 0),      # 9  slots 9, 13 are Noop in round 5
        (OTHER, -1, -1, -1, -1, -1, -1),  # 10
        (NR, 3, 1, 3, 16, 0, 0),      # 11 (leader group 1, acceptor group 1, index 1): slots 3, 7, 11, 15 in round 0
    ]
    cols = [np.array([m[j] for m in msgs], np.int32) for j in range(7)]
    b = MS.Burst(2, 2, 3, 16, 0, *cols)
    want_kind = [M.PHASE2B, M.PHASE2B_NR, M.PHASE2B, M.NACK, M.PHASE2B_NR, M.NACK, M.PHASE2B_NR, M.PHASE1B, M.NACK,
                 M.PHASE2B_NR, 0, M.PHASE2B_NR]
    want_value = [2, 2, 2, 2, 3, 3, 3, 5, 5, 5, -1, 0]
    for model in both(b):
        st, bad, rk, rv = model.run(b)
        assert (st, bad) == (0, -1) and rk.tolist() == want_kind and rv.tolist() == want_value
        pr, mv = model.scalars()
        assert pr.tolist() == [[-1] * 3, [-1] * 3, [5, -1, -1], [-1, 0, -1]]
        assert mv.tolist() == [[-1] * 3, [-1] * 3, [13, -1, -1], [-1, 15, -1]]
        vr, vv = model.cells()
        assert [(int(vr[s, 0]), int(vv[s, 0])) for s in (1, 5, 9, 13)] == [(2, -1), (2, -1), (5, -1), (5, -1)]
        assert [int(vr[s, 1]) for s in (3, 7, 11, 15)] == [0] * 4 and (vr[:, 2] == -1).all()
        assert (vr[0::2] == -1).all()


@pytest.mark.parametrize("name", ["n3000", "L3_A3", "L1_A1"])
def test_the_models_refuse_a_bad_burst_alike(name):
    b = MS.named(name)
    for what, c, at in MS.spoiled(b):
        models = both(b)
        got = run_same(models, c, what)
        assert got[:2] == (M.EINVAL, at), what
        M.assert_same_state(models[0], M.Sequential(b.L, b.A, b.R, b.S), what)     # nothing applied
    assert len(MS.spoiled(b)) == 7 + (b.L * b.A > 1) + (b.L > 1)


@pytest.mark.parametrize("name", NAMES)
def test_a_burst_cut_anywhere_equals_the_whole(name):
    b = MS.named(name)
    n = len(b)
    whole = M.Arrays(b.L, b.A, b.R, b.S)
    _, _, rk, rv = whole.run(b)
    for k in (range(0, n + 1, 5) if n < 1000 else list(range(0, n + 1, 487)) + [n - 1]):
        two = M.Arrays(b.L, b.A, b.R, b.S)
        h, t = two.run(b.cut(0, k)), two.run(b.cut(k, n))
        np.testing.assert_array_equal(np.r_[h[2], t[2]], rk)
        np.testing.assert_array_equal(np.r_[h[3], t[3]], rv)
        M.assert_same_state(two, whole, (name, k))


# ---- bindings -------------------------------------------------------------------------------------------------------
def test_libfpx_exports_both_symbols_and_the_prototypes_match():
    import frankenpaxos_amd as fa
    from frankenpaxos_amd import _lib

    L = fa.lib()
    for name in ("fpx_mencius_acceptor_inbox", "fpx_mencius_acceptor_inbox_dev"):
        assert hasattr(L, name) and len(_lib.SIGNATURES[name][1]) == 11
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    assert " T fpx_mencius_acceptor_inbox\n" in nm and " T fpx_mencius_acceptor_inbox_dev\n" in nm
    header = open(os.path.join(ROOT, "include", "fpx.h")).read()
    for form in ("_dev", ""):
        m = re.search(r"int32_t fpx_mencius_acceptor_inbox%s\(([^)]*)\);" % form, header)
        assert m and len(m.group(1).split(",")) == 11
    assert "Acceptor.scala:142-291" in header
    assert hasattr(fa.Context, "mencius_acceptor_inbox") and hasattr(fa.Context, "mencius_acceptor_inbox_dev")
    # refused before anything touches a device
    assert L.fpx_mencius_acceptor_inbox(None, 0, *[None] * 7, None, None) == 1
    assert L.fpx_mencius_acceptor_inbox_dev(None, 0, *[None] * 7, None, None) == 1


def test_the_scala_native_matches_the_c_function():
    """name and arity; the natives of every protocol are declared in object Native (Native.scala), and
    MenciusNative.scala's engine calls this one"""
    jni = os.path.join(ROOT, "frankenpaxos_amd", "jni")
    scala = open(os.path.join(jni, "Native.scala")).read()
    shim = open(os.path.join(jni, "fpx_jni.c")).read()
    m = re.search(r"@native def menciusAcceptorInbox\(([^)]*)\): Int", scala)
    assert m, "Native.menciusAcceptorInbox is not declared"
    c = re.search(r"Java_frankenpaxos_gpu_Native_menciusAcceptorInbox\(([^)]*)\)", shim, re.S)
    assert c, "the shim has no menciusAcceptorInbox"
    assert len(m.group(1).split(",")) + 2 == len(c.group(1).split(","))       # + JNIEnv*, jclass
    assert "Native.menciusAcceptorInbox(" in open(os.path.join(jni, "MenciusNative.scala")).read()


def test_the_cxx_mirror_compiles_with_the_new_method(tmp_path):
    src = tmp_path / "m.cpp"
    src.write_text('#include "frankenpaxos_amd/host/fpx.hpp"\n'
                   'int main() { auto p = &frankenpaxos::mencius::NoopRangeEngine::acceptorsHandleInbox; (void)p; return 0; }\n')
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
