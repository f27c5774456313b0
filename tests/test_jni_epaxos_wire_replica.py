"""The natives of the key table and of a replica's tick from wire bytes (epxKeysEnable, epxKeysIntern, epxWireReplicaTick) on
the mock JVM of tests/test_jni_shim.py: the Scala declarations and the C functions agree, short buffers are refused before
native code touches them; on the GPU the natives give what the ctypes calls give on another context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import epaxos_cmd_cases as CC
from tests.test_jni_epaxos_wire import direct
from tests.test_jni_shim import JNI, jvm  # noqa: F401  (the mock-JVM fixture)


def test_the_scala_natives_and_the_c_functions_agree():
    scala = open(os.path.join(JNI, "Native.scala")).read()
    shim = open(os.path.join(JNI, "fpx_jni.c")).read()
    count = lambda t: len([p for p in t.split(",") if p.strip()])
    for name, args, call in (("epxKeysEnable", 2, "fpx_epx_keys_enable("), ("epxKeysIntern", 7, "fpx_epx_keys_intern("),
                             ("epxWireReplicaTick", 14, "fpx_wire_epx_replica_tick(")):
        d = re.search(r"@native def %s\(([^)]*)\)" % name, scala, flags=re.S)
        c = re.search(r"Java_frankenpaxos_gpu_Native_%s\(\s*JNIEnv\* env, jclass cls,?([^)]*)\)\s*\{(.*?)\n\}" % name, shim, flags=re.S)
        assert d and c, name
        assert count(d.group(1)) == count(c.group(1)) == args, name
        assert call in c.group(2), name
    actor = open(os.path.join(JNI, "EPaxosNative.scala")).read()
    # the engine's keyOf asks the device on a miss and caches the answer; the actor itself receives parsed messages
    assert "deviceKeys: Boolean = false" in actor and actor.count("Native.epxKeysIntern(") == 1
    assert re.search(r"if \(deviceKeys\) keyIds\.getOrElseUpdate\(k, deviceKeyOf\(k\)\)", actor)
    assert "Native.epxWireReplicaTick(" not in actor and "def isReplicaTickFrame" in actor


def test_argument_checks_without_a_device(jvm):  # noqa: F811
    m = 4
    i32 = lambda k: jvm.arr(np.zeros(k, np.int32))
    bufs = [direct(jvm, 16), C.c_int64(16), direct(jvm, 8 * (m + 1)), direct(jvm, 4 * m)]
    outs = [i32(m), i32(4 * m), i32(5 * m), i32(2)]
    call = lambda *a: jvm.call("epxWireReplicaTick", C.c_int32, C.c_int64(0), *a)
    assert call(m, 5, *bufs, 0, None, 8, *outs) == 1               # no context behind handle 0
    assert call(-1, 5, *bufs, 0, None, 8, *outs) == 1 and call(m, 2, *bufs, 0, None, 8, *outs) == 1
    intern = lambda *a: jvm.call("epxKeysIntern", C.c_int32, C.c_int64(0), *a)
    assert intern(1, jvm.arr(np.zeros(2, np.int8)), C.c_int64(2), jvm.arr(np.zeros(1, np.int64)), i32(1), i32(1)) == 1
    assert jvm.call("epxKeysEnable", C.c_int32, C.c_int64(0), C.c_int64(64)) == 1


@pytest.mark.gpu
def test_the_natives_give_what_the_ctypes_calls_give(jvm):  # noqa: F811
    from frankenpaxos_amd import wire
    from tests.test_gpu_epaxos_wire_replica_tick import NI, NK, ctx, frame, state, wire_burst

    n, m = 5, 200
    ref = ctx(n)
    h = jvm.call("epxCreateWithLog", C.c_int64, n, NK, 0, NI)
    assert h > 0
    H = C.c_int64(h)
    assert jvm.call("epxKeysEnable", C.c_int32, H, C.c_int64(1 << 12)) == 0
    assert jvm.call("epxKeysEnable", C.c_int32, H, C.c_int64(1 << 12)) == 1           # once per context
    # ---- epxKeysIntern
    d = CC.KeyDict()
    for batch in ([b"k2", b"k0", b"k2"], [b"k0", b"k3"]):
        buf, off, ln = ref.pack_keys(batch)
        st, want = ref.keys_intern(batch)
        assert st == 0 and want.tolist() == d.intern(batch)
        ids = jvm.arr(np.full(len(batch), -9, np.int32))
        args = [jvm.arr(buf.view(np.int8)), C.c_int64(len(buf)), jvm.arr(off), jvm.arr(ln)]
        # every array is length-checked before native code touches it
        assert jvm.call("epxKeysIntern", C.c_int32, H, len(batch), *args, jvm.arr(np.zeros(len(batch) - 1, np.int32))) == 1
        assert jvm.call("epxKeysIntern", C.c_int32, H, len(batch), args[0], C.c_int64(len(buf) + 1), *args[2:], ids) == 1
        assert (jvm.read(ids, np.int32, len(batch)) == -9).all()
        assert jvm.call("epxKeysIntern", C.c_int32, H, len(batch), *args, ids) == 0
        assert jvm.read(ids, np.int32, len(batch)).tolist() == want.tolist()
    # a fifth key: the table of NK = 4 is full once k1 is in; nothing applied, the ids stay
    batch = [b"k1", b"one too many"]
    buf, off, ln = ref.pack_keys(batch)
    ids = jvm.arr(np.full(2, -9, np.int32))
    assert jvm.call("epxKeysIntern", C.c_int32, H, 2, jvm.arr(buf.view(np.int8)), C.c_int64(len(buf)), jvm.arr(off), jvm.arr(ln), ids) == 5
    assert (jvm.read(ids, np.int32, 2) == -9).all()
    assert jvm.call("epxKeysIntern", C.c_int32, H, 0, None, C.c_int64(0), None, None, None) == 0
    # ---- epxWireReplicaTick
    msgs = wire_burst(91, n, m)
    frames = [frame(wire, x) for x in msgs]
    to = np.asarray([x[1] for x in msgs], np.int32)
    triple = np.asarray([x[8] for x in msgs], np.int32)
    want = ref.wire_replica_tick(frames, to, max_pairs=5 * m, triple_id=triple)
    assert want[0] == 0
    buf, off = wire.pack(frames)
    in_len = int(off[-1])
    din, doff, dto = direct(jvm, in_len, buf[:in_len]), direct(jvm, 8 * (m + 1), off), direct(jvm, 4 * m, to)
    new_outs = lambda: [jvm.arr(np.full(m, -9, np.int32)), jvm.arr(np.full(4 * m, -9, np.int32)),
                        jvm.arr(np.full(m * n, -9, np.int32)), jvm.arr(np.full(2, -9, np.int32))]
    got = new_outs()
    call = lambda *x: jvm.call("epxWireReplicaTick", C.c_int32, H, *x)
    tid = jvm.arr(triple)
    assert call(m, n, din, C.c_int64(in_len + 1), doff, dto, 0, tid, 5 * m, *got) == 1
    assert call(m, n, din, C.c_int64(in_len), direct(jvm, 8 * m), dto, 0, tid, 5 * m, *got) == 1
    assert call(m, n, din, C.c_int64(in_len), doff, direct(jvm, 4 * m - 1), 0, tid, 5 * m, *got) == 1
    assert call(m, n, din, C.c_int64(in_len), doff, dto, 0, jvm.arr(triple[:-1]), 5 * m, *got) == 1
    assert call(m, n, din, C.c_int64(in_len), doff, dto, 0, tid, 5 * m, got[0], jvm.arr(np.zeros(4 * m - 1, np.int32)), *got[2:]) == 1
    assert call(m, 3, din, C.c_int64(in_len), doff, dto, 0, tid, 5 * m, *got) == 1
    assert (jvm.read(got[0], np.int32, m) == -9).all()
    # a refused tick: the index comes back, the outputs stay
    cut = off.copy()
    cut[-1] -= 1
    assert call(m, n, din, C.c_int64(in_len - 1), direct(jvm, 8 * (m + 1), cut), dto, 0, tid, 5 * m, *got) == 1
    assert int(jvm.read(got[3], np.int32, 2)[0]) == m - 1 and (jvm.read(got[0], np.int32, m) == -9).all()
    assert call(m, n, din, C.c_int64(in_len), doff, dto, 0, tid, 5 * m, *got) == 0
    assert jvm.read(got[3], np.int32, 2).tolist() == [want[7], want[8]]
    np.testing.assert_array_equal(jvm.read(got[0], np.int32, m), want[1])
    r = jvm.read(got[1], np.int32, 4 * m).reshape(4, m)
    for g, w in zip(r, (want[2], want[3], want[5], want[6])):
        np.testing.assert_array_equal(g, w)
    np.testing.assert_array_equal(jvm.read(got[2], np.int32, m * n).reshape(m, n), want[4])
    assert len(set(jvm.read(got[0], np.int32, m).tolist())) >= 5
    # the same device state: through the handle's own readback natives that is the ctypes context's business; the key table
    # is read back through the library on the native's handle
    from frankenpaxos_amd.epaxos import EPaxos
    peer = EPaxos.__new__(EPaxos)
    peer.L, peer.n, peer.num_keys, peer._h = ref.L, n, NK, C.c_void_p(h)
    assert state(peer, msgs) == state(ref, msgs) and peer.keys_read() == ref.keys_read()
    peer._h = None
    # an empty tick
    assert call(0, n, None, C.c_int64(0), None, None, 0, None, 0, None, None, None, got[3]) == 0
    assert jvm.read(got[3], np.int32, 2).tolist() == [-1, 0]
    assert jvm.call("epxDestroy", C.c_int32, H) == 0
    ref.close()
