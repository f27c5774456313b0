"""The native of a replica's tick from wire bytes to wire bytes (epxWireReplicaTickBytes) on the mock JVM of
tests/test_jni_shim.py: the Scala declaration and the C function agree, short buffers are refused before native code touches
them; on the GPU the native gives what the ctypes call gives on another context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_jni_epaxos_wire import direct
from tests.test_jni_shim import JNI, jvm  # noqa: F401  (the mock-JVM fixture)


def test_the_scala_native_and_the_c_function_agree():
    scala = open(os.path.join(JNI, "Native.scala")).read()
    shim = open(os.path.join(JNI, "fpx_jni.c")).read()
    count = lambda t: len([p for p in t.split(",") if p.strip()])
    d = re.search(r"@native def epxWireReplicaTickBytes\(([^)]*)\)", scala, flags=re.S)
    c = re.search(r"Java_frankenpaxos_gpu_Native_epxWireReplicaTickBytes\(\s*JNIEnv\* env, jclass cls,?([^)]*)\)\s*\{(.*?)\n\}", shim,
                  flags=re.S)
    assert d and c
    assert count(d.group(1)) == count(c.group(1)) == 18
    assert "fpx_wire_epx_replica_tick_bytes(" in c.group(2)
    # the published worst case is the one the header defines
    hdr = open(os.path.join(os.path.dirname(JNI), "..", "include", "fpx_wire.h")).read()
    assert "#define FPX_WIRE_EPX_REPLY_MAX 472\n" in hdr and "472 * m" in scala
    actor = open(os.path.join(JNI, "EPaxosNative.scala")).read()
    # with the device's key table the actor's peer burst goes bytes to bytes and only the deferred replies are built
    assert actor.count("Native.epxWireReplicaTickBytes(") == 1 and "if (engine.hasDeviceKeys) wireTickBytes(" in actor
    assert "transport.send(this, e.src, encoded(i))" in actor


def test_argument_checks_without_a_device(jvm):  # noqa: F811
    m = 4
    i32 = lambda k: jvm.arr(np.zeros(k, np.int32))
    ins = [direct(jvm, 16), C.c_int64(16), direct(jvm, 8 * (m + 1)), direct(jvm, 4 * m)]
    outs = [direct(jvm, 64), C.c_int64(64), direct(jvm, 8 * (m + 1)), direct(jvm, m), i32(m), i32(4 * m), i32(5 * m),
            jvm.arr(np.zeros(6, np.int64))]
    call = lambda *a: jvm.call("epxWireReplicaTickBytes", C.c_int32, C.c_int64(0), *a)
    assert call(m, 5, *ins, 0, None, 8, *outs) == 1                # no context behind handle 0
    assert call(-1, 5, *ins, 0, None, 8, *outs) == 1 and call(m, 2, *ins, 0, None, 8, *outs) == 1


@pytest.mark.gpu
def test_the_native_gives_what_the_ctypes_call_gives(jvm):  # noqa: F811
    from frankenpaxos_amd import wire
    from tests.test_gpu_epaxos_wire_replica_tick import NI, NK, ctx, frame, state, wire_burst

    n, m = 5, 200
    ref = ctx(n)
    h = jvm.call("epxCreateWithLog", C.c_int64, n, NK, 0, NI)
    assert h > 0
    H = C.c_int64(h)
    assert jvm.call("epxKeysEnable", C.c_int32, H, C.c_int64(1 << 12)) == 0
    msgs = wire_burst(93, n, m)
    frames = [frame(wire, x) for x in msgs]
    to = np.asarray([x[1] for x in msgs], np.int32)
    triple = np.asarray([x[8] for x in msgs], np.int32)
    want = ref.wire_replica_tick_bytes(frames, to, max_pairs=5 * m, triple_id=triple)
    assert want["status_code"] == 0 and want["totals"][0] > m // 2 and want["totals"][2] > 0
    need = int(want["totals"][1])
    buf, off = wire.pack(frames)
    in_len = int(off[-1])
    din, doff, dto = direct(jvm, in_len, buf[:in_len]), direct(jvm, 8 * (m + 1), off), direct(jvm, 4 * m, to)
    cap = m * wire.EPX_REPLY_MAX
    fill = lambda k, v, t: direct(jvm, k * np.dtype(t).itemsize, np.full(k, v, t))
    dout, dooff, dkind = fill(cap, 0xEE, np.uint8), fill(m + 1, -9, np.int64), fill(m, 9, np.uint8)
    new_outs = lambda: [jvm.arr(np.full(m, -9, np.int32)), jvm.arr(np.full(4 * m, -9, np.int32)),
                        jvm.arr(np.full(m * n, -9, np.int32)), jvm.arr(np.full(6, -9, np.int64))]
    got = new_outs()
    tid = jvm.arr(triple)
    call = lambda *x: jvm.call("epxWireReplicaTickBytes", C.c_int32, H, *x)
    ok = (m, n, din, C.c_int64(in_len), doff, dto, 0, tid, 5 * m, dout, C.c_int64(cap), dooff, dkind)
    # every buffer is length-checked before native code touches it
    assert call(*ok[:9], dout, C.c_int64(cap + 1), dooff, dkind, *got) == 1
    assert call(*ok[:11], direct(jvm, 8 * m), dkind, *got) == 1
    assert call(*ok[:12], direct(jvm, m - 1), *got) == 1
    assert call(*ok[:3], C.c_int64(in_len + 1), *ok[4:], *got) == 1
    assert call(*ok, got[0], jvm.arr(np.zeros(4 * m - 1, np.int32)), *got[2:]) == 1
    assert call(*ok, *got[:3], jvm.arr(np.zeros(5, np.int64))) == 1
    assert call(m, 3, *ok[2:], *got) == 1
    raw = lambda b, t, k: jvm.read(b, t, k)                      # (a mock direct buffer's bytes)
    assert (jvm.read(got[0], np.int32, m) == -9).all() and (raw(dkind, np.uint8, m) == 9).all()
    # a refused tick: the index comes back, the outputs stay
    cut = off.copy()
    cut[-1] -= 1
    assert call(*ok[:3], C.c_int64(in_len - 1), direct(jvm, 8 * (m + 1), cut), *ok[5:], *got) == 1
    assert jvm.read(got[3], np.int64, 6).tolist() == [m - 1, 0, 0, 0, 0, -1]
    assert (jvm.read(got[0], np.int32, m) == -9).all() and (raw(dkind, np.uint8, m) == 9).all() and (raw(dout, np.uint8, cap) == 0xEE).all()
    # the tick
    assert call(*ok, *got) == 0
    assert jvm.read(got[3], np.int64, 6).tolist() == [-1, want["num_pairs"]] + want["totals"].tolist()
    np.testing.assert_array_equal(jvm.read(got[0], np.int32, m), want["outcome"])
    r = jvm.read(got[1], np.int32, 4 * m).reshape(4, m)
    for g, k in zip(r, ("out_ballot", "out_status", "out_values_end", "out_triple")):
        np.testing.assert_array_equal(g, want[k])
    np.testing.assert_array_equal(jvm.read(got[2], np.int32, m * n).reshape(m, n), want["out_deps"])
    np.testing.assert_array_equal(raw(dooff, np.int64, m + 1), want["out_offsets"])
    np.testing.assert_array_equal(raw(dkind, np.uint8, m), want["reply_kind"])
    o = raw(dout, np.uint8, cap)
    assert o[:need].tobytes() == want["out"][:need].tobytes() and (o[need:] == 0xEE).all()
    from frankenpaxos_amd.epaxos import EPaxos
    peer = EPaxos.__new__(EPaxos)
    peer.L, peer.n, peer.num_keys, peer._h = ref.L, n, NK, C.c_void_p(h)
    assert state(peer, msgs) == state(ref, msgs) and peer.keys_read() == ref.keys_read()
    peer._h = None
    # an empty tick needs no input buffer
    res = jvm.arr(np.full(6, -9, np.int64))
    assert call(0, n, None, C.c_int64(0), None, None, 0, None, 0, None, C.c_int64(0), dooff, None, None, None, None, res) == 0
    assert jvm.read(res, np.int64, 6).tolist() == [-1, 0, 0, 0, 0, -1] and raw(dooff, np.int64, 1)[0] == 0
    assert jvm.call("epxDestroy", C.c_int32, H) == 0
    ref.close()
