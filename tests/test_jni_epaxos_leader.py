"""The leader natives of the JNI shim (epxCreateWithLeaderState, epxLead, epxLeaderReplies) on the mock JVM of
tests/test_jni_shim.py: the Scala declarations and the C functions agree, the actor calls them, short arrays are refused
before native code touches them; on the GPU one lead and one burst through the natives equal the Python binding's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import epaxos_leader_model as M
from tests import epaxos_leader_streams as S
from tests.test_jni_shim import JNI, jvm  # noqa: F401  (the mock-JVM fixture)

NATIVES = ("epxCreateWithLeaderState", "epxLead", "epxLeaderReplies")


def test_the_scala_natives_and_the_c_functions_agree():
    scala = open(os.path.join(JNI, "Native.scala")).read()
    shim = open(os.path.join(JNI, "fpx_jni.c")).read()
    for name in NATIVES:
        d = re.search(r"@native def " + name + r"\(([^)]*)\)", scala, flags=re.S)
        c = re.search(r"Java_frankenpaxos_gpu_Native_" + name + r"\(\s*JNIEnv\* env, jclass cls,?([^)]*)\)", shim, flags=re.S)
        assert d and c, name
        count = lambda t: len([p for p in t.split(",") if p.strip()])
        assert count(d.group(1)) == count(c.group(1)), name
    assert len(re.search(r"@native def epxLeaderReplies\(([^)]*)\)", scala, flags=re.S).group(1).split(",")) == 17


def test_the_actor_leads_through_the_natives_only_when_asked_to():
    actor = open(os.path.join(JNI, "EPaxosNative.scala")).read()
    assert "remotePeers: Boolean = false" in actor and "leaderState: Boolean = false" in actor
    assert actor.count("Native.epxLeaderReplies(") == 1 and actor.count("Native.epxLead(") == 1     # ONE call per burst
    assert "Native.epxCreateWithLeaderState(" in actor
    # the replies are enqueued, not dropped, and a fired defaultToSlowPath timer becomes a kind-3 event
    for kind, msg in ((0, "PreAcceptOk"), (1, "AcceptOk"), (2, "Nack")):
        assert re.search(r"case Request\.%s\(r\) if remotePeers\s*=>\s*enqueue\(leaderInbox, LeaderEvent\(%d," % (msg, kind), actor)
    assert "enqueue(leaderInbox, LeaderEvent(3, instance" in actor
    assert "thriftyOtherReplicas(config.fastQuorumSize - 1)" in actor and "thriftyOtherReplicas(config.slowQuorumSize - 1)" in actor


def test_argument_checks_without_a_device(jvm):  # noqa: F811
    i32 = lambda k: jvm.arr(np.zeros(k, np.int32))
    i8 = lambda k: jvm.arr(np.zeros(k, np.int8))
    n = 4
    # no context behind handle 0: refused, whatever the arrays are; a negative batch and n < 3 likewise
    assert jvm.call("epxLead", C.c_int32, 0, n, 5, i32(n), i32(n), i32(n), i32(n), i32(n), i8(n), i32(n), i8(n), None, None) == 1
    assert jvm.call("epxLead", C.c_int32, 0, -1, 5, *[None] * 10) == 1
    assert jvm.call("epxLeaderReplies", C.c_int32, 0, n, 5, *[i32(n)] * 8, i32(5 * n), i32(n), None, None, None, None) == 1
    assert jvm.call("epxLeaderReplies", C.c_int32, 0, n, 2, *[None] * 14) == 1
    assert jvm.call("epxCreateWithLeaderState", C.c_int64, 4, 4, 0, 8) == -1         # n = 4 is no EPaxos configuration


@pytest.mark.gpu
def test_one_lead_and_one_burst_through_the_natives(jvm):  # noqa: F811
    from frankenpaxos_amd.epaxos import EPaxos

    n, NI = 5, 64
    ops = S.make_stream(3, n)
    leads, burst = ops[0][1], next(op for op in ops if op[0] == "replies")[1]
    between = ops[1:ops.index(("replies", burst))]
    h = jvm.call("epxCreateWithLeaderState", C.c_int64, n, 4, 0, NI)
    assert h > 0
    assert jvm.call("epxCreateWithLeaderState", C.c_int64, n, 4, 0, 0) == -1         # the flag needs a command log
    ref = EPaxos(n, 4, num_instances=NI, leader_state=True)
    i32 = lambda a: jvm.arr(np.asarray(a, np.int32))
    i8 = lambda a: jvm.arr(np.asarray(a, np.int8))
    m = len(leads)
    cols = [np.asarray(c, np.int32) for c in zip(*leads)]
    deps, dend = jvm.arr(np.zeros(m * n, np.int32)), jvm.arr(np.zeros(m, np.int32))
    args = [i32(cols[0]), i32(cols[1]), i32(cols[2]), i32(cols[3]), i32(cols[4]), i8(cols[5]), i32(cols[6]), i8(cols[7])]
    # every array is length-checked before native code touches it
    assert jvm.call("epxLead", C.c_int32, h, m, n, *args[:7], i8(cols[7][:-1]), deps, dend) == 1
    assert jvm.call("epxLead", C.c_int32, h, m, n, *args, jvm.arr(np.zeros(m * n - 1, np.int32)), dend) == 1
    assert jvm.call("epxLead", C.c_int32, h, m, 3, *args, deps, dend) == 1            # the handle is the authority on n
    assert jvm.call("epxLead", C.c_int32, h, m, n, *args, deps, dend) == 0
    st, wd, we = ref.lead(*cols[:5], cols[5].astype(np.uint8), cols[6], cols[7].astype(np.uint8))
    assert st == 0
    np.testing.assert_array_equal(jvm.read(deps, np.int32, m * n).reshape(m, n), wd)
    np.testing.assert_array_equal(jvm.read(dend, np.int32, m), we)
    for op in between:                                                               # instances taken from their leaders
        S.run_gpu_op(ref, op)
        one = lambda v: i32([v])
        if op[0] == "preaccept":
            _, inst, ballot, key, is_set, tid, w, end, target = op
            assert jvm.call("epxHandlePreaccept", C.c_int32, h, 1, n, one(inst[0]), one(inst[1]), one(ballot[0]), one(ballot[1]),
                            one(key), i8([is_set]), one(tid), i32(w), one(end), i8([1 << target]), None, None, None, None) == 0
        elif op[0] == "accept":
            _, inst, ballot, tid, target, key, is_set = op
            assert jvm.call("epxAccept", C.c_int32, h, 1, one(inst[0]), one(inst[1]), one(ballot[0]), one(ballot[1]), one(tid),
                            one(key), i8([is_set]), i8([1 << target]), None, None) == 0
        elif op[0] == "prepare":
            _, inst, ballot, target = op
            assert jvm.call("epxPrepare", C.c_int32, h, 1, n, one(inst[0]), one(inst[1]), one(ballot[0]), one(ballot[1]),
                            i8([1 << target]), None, None, None) == 0
        else:
            _, inst, tid, w, end, target, key, is_set = op
            assert jvm.call("epxHandleCommit", C.c_int32, h, 1, n, one(inst[0]), one(inst[1]), one(tid), one(key), i8([is_set]),
                            i32(w), one(end), i8([1 << target])) == 0
    a = S.burst_arrays(n, burst)
    k = len(burst)
    outcome, triple = jvm.arr(np.full(k, -9, np.int32)), jvm.arr(np.full(3 * k, -9, np.int32))
    odeps, decided = jvm.arr(np.full(k * n, -9, np.int32)), jvm.arr(np.full(k + 1, -9, np.int32))
    ins = [i32(x) for x in a[:8]] + [i32(a[8].reshape(-1)), i32(a[9])]
    assert jvm.call("epxLeaderReplies", C.c_int32, h, k, n, *ins[:8], i32(a[8].reshape(-1)[:-1]), ins[9], outcome, triple, odeps,
                    decided) == 1
    assert jvm.call("epxLeaderReplies", C.c_int32, h, k, n, *ins, outcome, triple, odeps, jvm.arr(np.zeros(k, np.int32))) == 1
    assert (jvm.read(outcome, np.int32, k) == -9).all()
    st = jvm.call("epxLeaderReplies", C.c_int32, h, k, n, *ins, outcome, triple, odeps, decided)
    want = ref.leader_replies(*a)
    assert st == want[0] and st in (0, M.EFATAL)
    np.testing.assert_array_equal(jvm.read(outcome, np.int32, k), want[1])
    t = jvm.read(triple, np.int32, 3 * k)
    np.testing.assert_array_equal(t[:k], want[2])
    np.testing.assert_array_equal(t[k:2 * k], want[4])
    np.testing.assert_array_equal(t[2 * k:], want[5])
    np.testing.assert_array_equal(jvm.read(odeps, np.int32, k * n).reshape(k, n), want[3])
    d = jvm.read(decided, np.int32, k + 1)
    assert d[0] == len(want[6]) and d[1:1 + d[0]].tolist() == want[6].tolist()
    assert set(want[1].tolist()) >= {0, 1, 3, 4}                                    # the burst decides on both paths
    # an empty burst
    assert jvm.call("epxLeaderReplies", C.c_int32, h, 0, n, *[None] * 13, decided) == 0
    assert int(jvm.read(decided, np.int32, 1)[0]) == 0
    assert jvm.call("epxDestroy", C.c_int32, h) == 0
    ref.close()
