"""fpx_proxy_phase2b_msgs / _dev and fpx_wire_phase2b_tick without a GPU: the symbols are exported, declared and bound;
the argument checks that need no device; and the streams tests/test_gpu_phase2b_msgs.py runs are not vacuous."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import phase2b_streams as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fpx_proxy_phase2b_msgs", "fpx_proxy_phase2b_msgs_dev", "fpx_wire_phase2b_tick")
EINVAL = 1


def test_the_three_symbols_are_exported_declared_and_bound():
    import frankenpaxos_amd as fa
    from frankenpaxos_amd import _lib, wire

    L = fa.lib()
    headers = open(os.path.join(ROOT, "include", "fpx.h")).read() + open(os.path.join(ROOT, "include", "fpx_wire.h")).read()
    for name in NAMES:
        assert getattr(L, name) is not None
        assert re.search(r"int32_t " + name + r"\(", headers), name
    assert "fpx_proxy_phase2b_msgs" in _lib.SIGNATURES and "fpx_proxy_phase2b_msgs_dev" in _lib.SIGNATURES
    assert wire._L().fpx_wire_phase2b_tick.argtypes is not None
    for method in ("proxy_phase2b_msgs", "proxy_phase2b_msgs_dev", "wire_phase2b_tick"):
        assert callable(getattr(fa.Context, method))
    jni = os.path.join(ROOT, "frankenpaxos_amd", "jni")
    assert "def proxyPhase2bMsgs(" in open(os.path.join(jni, "Native.scala")).read()
    assert "Java_frankenpaxos_gpu_Native_proxyPhase2bMsgs(" in open(os.path.join(jni, "fpx_jni.c")).read()
    assert "proxyLeaderHandlePhase2bMsgs" in open(os.path.join(ROOT, "frankenpaxos_amd", "host", "fpx.hpp")).read()


def test_null_context_and_negative_n_are_einval_without_a_device():
    import frankenpaxos_amd as fa
    from frankenpaxos_amd import wire

    L = fa.lib()
    a = np.zeros(4, np.int32)
    p = a.ctypes.data
    for fn in (L.fpx_proxy_phase2b_msgs, L.fpx_proxy_phase2b_msgs_dev):
        assert fn(None, 4, None, None, p, p, p, 0, None, None, None) == EINVAL
        assert fn(None, -1, None, None, p, p, p, 0, None, None, None) == EINVAL
        assert fn(None, 0, None, None, None, None, None, 0, None, None, None) == EINVAL
    cnt, bad = C.c_int32(7), C.c_int32(7)
    tick = wire._L().fpx_wire_phase2b_tick
    assert tick(None, p, 8, p, 1, 0, p, p, p, 4, C.byref(cnt), C.byref(bad)) == EINVAL
    assert tick(None, p, 8, p, -1, 0, p, p, p, 4, C.byref(cnt), C.byref(bad)) == EINVAL


@pytest.mark.parametrize("shape", sorted(PS.SHAPES))
@pytest.mark.parametrize("layout", PS.LAYOUTS)
def test_the_streams_are_not_vacuous(shape, layout):
    """a condition on the INPUTS, judged by the oracle alone: of the opened entries at least a quarter end Chosen and at
    least a tenth end Pending, and some votes arrive after Done"""
    from oracle import pyoracle

    pyoracle.build()
    st = PS.Stream(shape, 20000, layout, seed=7)
    assert st.n == 20000
    ref, chosen, states = PS.oracle_run(pyoracle, st)
    opened = len(states)
    done = sum(1 for v in states.values() if v == 2)
    assert done == len(chosen) and len({(s, r) for _, s, r, _ in chosen}) == len(chosen)
    assert 4 * done >= opened, (done, opened)
    assert 10 * (opened - done) >= opened, (opened - done, opened)
    if shape == "ways4":  # two rounds of one slot are both live
        assert len({s for s, r in states}) < opened
    # votes after Done: a chosen entry's later messages
    when = {(s, r): i for i, s, r, _ in chosen}
    late = sum(1 for i, (s, r) in enumerate(zip(st.slot.tolist(), st.round.tolist())) if when.get((s, r), st.n) < i)
    assert late > 0
