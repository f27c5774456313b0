"""fpx_replica_chosen_msgs / _dev without a GPU: the symbols are exported, declared and bound; the argument checks that
need no device; the dictionary restatement of tests/replica_streams.py against the oracle, message by message; and the
streams tests/test_gpu_replica_msgs.py runs are not vacuous."""
import os
import re

import numpy as np
import pytest

from tests import replica_streams as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fpx_replica_chosen_msgs", "fpx_replica_chosen_msgs_dev")
EINVAL = 1


def test_the_two_symbols_are_exported_declared_and_bound():
    import frankenpaxos_amd as fa
    from frankenpaxos_amd import _lib

    L = fa.lib()
    header = open(os.path.join(ROOT, "include", "fpx.h")).read()
    for name in NAMES:
        assert getattr(L, name) is not None
        assert re.search(r"int32_t " + name + r"\(", header), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["fpx_replica_chosen_msgs"][1]) == 9 and len(_lib.SIGNATURES["fpx_replica_chosen_msgs_dev"][1]) == 7
    for method in ("replica_chosen_msgs", "replica_chosen_msgs_dev"):
        assert callable(getattr(fa.Context, method))
    jni = os.path.join(ROOT, "frankenpaxos_amd", "jni")
    assert "def replicaChosenMsgs(" in open(os.path.join(jni, "Native.scala")).read()
    assert "Java_frankenpaxos_gpu_Native_replicaChosenMsgs(" in open(os.path.join(jni, "fpx_jni.c")).read()
    assert "replicaHandleChosenMsgs" in open(os.path.join(ROOT, "frankenpaxos_amd", "host", "fpx.hpp")).read()
    assert "fpx_replica_msgs.hpp" in open(os.path.join(ROOT, "frankenpaxos_amd", "csrc", "Makefile")).read()


def test_the_kinds_are_those_of_the_wire_header():
    from frankenpaxos_amd import wire

    assert (RS.CHOSEN, RS.CHOSEN_NOOP_RANGE, RS.PHASE2B) == (wire.CHOSEN, wire.CHOSEN_NOOP_RANGE, wire.PHASE2B)
    header = open(os.path.join(ROOT, "include", "fpx_wire.h")).read()
    assert re.search(r"FPX_WIRE_CHOSEN = %d," % RS.CHOSEN, header)
    assert re.search(r"FPX_WIRE_CHOSEN_NOOP_RANGE = %d," % RS.CHOSEN_NOOP_RANGE, header)


def test_null_context_and_negative_n_are_einval_without_a_device():
    import frankenpaxos_amd as fa

    L = fa.lib()
    p = np.zeros(4, np.int32).ctypes.data
    assert L.fpx_replica_chosen_msgs_dev(None, 4, p, p, p, p, None) == EINVAL
    assert L.fpx_replica_chosen_msgs_dev(None, -1, p, p, p, p, None) == EINVAL
    assert L.fpx_replica_chosen_msgs_dev(None, 0, None, None, None, None, None) == EINVAL
    assert L.fpx_replica_chosen_msgs(None, 4, p, p, p, p, None, None, None) == EINVAL
    assert L.fpx_replica_chosen_msgs(None, -1, p, p, p, p, None, None, None) == EINVAL
    assert L.fpx_replica_chosen_msgs(None, 0, None, None, None, None, None, None, None) == EINVAL


def test_the_restatement_on_the_pinned_corners():
    """by hand: the lower index puts a slot, a range is cut by an earlier message only, the watermark lags"""
    C, R = RS.C, RS.R
    r = RS.Replica(4)
    r.handle(RS.burst_of([C(20, 200)]))
    r.handle(RS.burst_of([C(49, 490), R(0, 40), R(41, 61), R(2, 18), C(10, 100), C(49, 491)]))
    want = {20: 200, 49: 490, 0: -1, 4: -1, 8: -1, 12: -1, 16: -1, 41: -1, 45: -1, 2: -1, 6: -1, 10: -1, 14: -1}
    assert r.log == want and (r.executed_watermark, r.num_chosen) == (1, 13)
    r = RS.Replica(4)
    r.handle(RS.burst_of([C(0, 1), C(1, 2), C(2, 3), C(11, 9)]))
    r.handle(RS.burst_of([R(3, 15)]))
    assert (r.executed_watermark, r.num_chosen, r.prefix()) == (3, 6, 4)
    r.handle(RS.burst_of([C(1, 99), C(3, 98)]))
    assert r.executed_watermark == 3
    r.handle(RS.burst_of([R(9, 9)]))
    assert r.executed_watermark == 4


@pytest.mark.parametrize("seed", RS.SEEDS)
@pytest.mark.parametrize("L,S", RS.SHAPES)
def test_the_restatement_equals_the_oracle_and_the_streams_are_not_vacuous(L, S, seed):
    """message by message on the committed seeds; and the conditions on the INPUTS of the GPU test, judged by the
    oracle's run alone"""
    from oracle import pyoracle

    pyoracle.build()
    ref = pyoracle.System(pyoracle.make_config(num_slots=S, num_replicas=3, num_leader_groups=L, f=1))
    model = RS.Replica(L)
    bursts = RS.stream(L, S, seed)
    assert len(bursts) == RS.BURSTS and all(0 < len(b[0]) <= 4096 for b in bursts)
    total = dict(truncated=0, full=0, redundant=0, own=0, lag=0)
    for burst in bursts:
        assert 0.05 < 1.0 - burst[4].mean() < 0.15
        for msg in zip(*burst):
            model.handle_one(*msg)
        scalars, (vals, pres), stats = RS.oracle_burst(ref, burst, S, L)
        assert scalars == (model.executed_watermark, model.num_chosen)
        mv, mp = model.arrays(S)
        np.testing.assert_array_equal(vals, mv)
        np.testing.assert_array_equal(pres, mp)
        for k in total:
            total[k] += stats[k]
    RS.assert_not_vacuous(total, scalars)
