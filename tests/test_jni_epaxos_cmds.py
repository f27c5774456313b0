"""The natives of the command store (epxCmdsEnable, epxCmdsPut, epxCmdsStats) on the mock JVM of tests/test_jni_shim.py: the
Scala declarations and the C functions agree, short arrays are refused before native code touches them; on the GPU the store
behind the natives is the store behind the ctypes calls, and the bytes tick native then encodes the replies with a command."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_jni_epaxos_wire import direct
from tests.test_jni_shim import JNI, jvm  # noqa: F401  (the mock-JVM fixture)


def test_the_scala_natives_and_the_c_functions_agree():
    scala = open(os.path.join(JNI, "Native.scala")).read()
    shim = open(os.path.join(JNI, "fpx_jni.c")).read()
    count = lambda t: len([p for p in t.split(",") if p.strip()])
    for name, args, calls in (("epxCmdsEnable", 3, "fpx_epx_cmds_enable("), ("epxCmdsPut", 8, "fpx_epx_cmds_put("),
                              ("epxCmdsStats", 2, "fpx_epx_cmds_stats(")):
        d = re.search(r"@native def %s\(([^)]*)\)" % name, scala, flags=re.S)
        c = re.search(r"Java_frankenpaxos_gpu_Native_%s\(\s*JNIEnv\* env, jclass cls,?([^)]*)\)\s*\{(.*?)\n\}" % name, shim, flags=re.S)
        assert d and c, name
        assert count(d.group(1)) == count(c.group(1)) == args and calls in c.group(2)
    # the engine: the store needs the key table, every triple reaches the store before a bytes tick, and the tick's output is
    # sized for replies that carry a command (FPX_WIRE_EPX_CMD_REPLY_MAX(c) <= 503 + c)
    actor = open(os.path.join(JNI, "EPaxosNative.scala")).read()
    assert "logger.check(!deviceCommands || deviceKeys)" in actor and actor.count("Native.epxCmdsEnable(") == 1
    assert actor.count("Native.epxCmdsPut(") == 1 and "engine.putNewTriples(inTick = carried)" in actor
    assert "(503L + math.min(engine.maxCommandBytes, 65536)) * k" in actor and "Int.MaxValue - 8L" in actor
    assert "if (st == 5 && result(3) > outCap) return Array.fill[Array[Byte]](k)(null)" in actor
    from frankenpaxos_amd import wire

    assert all(wire.epx_cmd_reply_max(c) <= 503 + c for c in (0, 1, 127, 128, 16383, 16384, 1 << 16))
    # flushPeerInbox has no new branch: it sends encoded(i) wherever the device wrote the reply
    assert actor.count("transport.send(this, e.src, encoded(i))") == 1


def test_argument_checks_without_a_device(jvm):  # noqa: F811
    i64, i32 = lambda k: jvm.arr(np.zeros(k, np.int64)), lambda k: jvm.arr(np.zeros(k, np.int32))
    b = jvm.arr(np.zeros(8, np.uint8))
    assert jvm.call("epxCmdsEnable", C.c_int32, C.c_int64(0), 4, C.c_int64(64)) == 1     # no context behind handle 0
    assert jvm.call("epxCmdsPut", C.c_int32, C.c_int64(0), 2, b, C.c_int64(8), i64(2), i32(2), i32(2), i64(4)) == 1
    assert jvm.call("epxCmdsStats", C.c_int32, C.c_int64(0), i64(4)) == 1


@pytest.mark.gpu
def test_the_natives_give_what_the_ctypes_calls_give(jvm):  # noqa: F811
    from frankenpaxos_amd import wire
    from tests.test_gpu_epaxos_wire_replica_tick import NI, NK, command_of, ctx, frame
    from tests import epaxos_inbox_model as IM

    n = 3
    ref = ctx(n)
    ref.cmds_enable(64, 4096)
    h = jvm.call("epxCreateWithLog", C.c_int64, n, NK, 0, NI)
    assert h > 0
    H = C.c_int64(h)
    assert jvm.call("epxKeysEnable", C.c_int32, H, C.c_int64(1 << 12)) == 0
    assert jvm.call("epxCmdsEnable", C.c_int32, H, 64, C.c_int64(4096)) == 0
    assert jvm.call("epxCmdsEnable", C.c_int32, H, 64, C.c_int64(4096)) == 1              # a second call
    cmds = [b"first", b"", b"the third command", b"never stored", b"x" * 300, b"late"]
    ids = np.array([5, 6, 7, 5, 64, -1], np.int32)
    buf = np.frombuffer(b"".join(cmds), np.uint8)
    ln = np.array([len(c) for c in cmds], np.int32)
    off = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.int64)
    res = jvm.arr(np.full(4, -9, np.int64))
    put = lambda o, r, count=len(cmds): jvm.call("epxCmdsPut", C.c_int32, H, count, jvm.arr(buf), C.c_int64(len(buf)), o,
                                                 jvm.arr(ln), jvm.arr(ids), r)
    # every array is length-checked before native code touches it
    assert put(jvm.arr(off[:-1]), res) == 1 and put(jvm.arr(off), jvm.arr(np.zeros(3, np.int64))) == 1
    assert jvm.call("epxCmdsPut", C.c_int32, H, len(cmds), jvm.arr(buf), C.c_int64(len(buf) + 1), jvm.arr(off), jvm.arr(ln),
                    jvm.arr(ids), res) == 1
    assert jvm.read(res, np.int64, 4).tolist() == [-9] * 4
    # a span outside the bytes: refused with its index
    bad = off.copy()
    bad[2] = len(buf) - 3
    assert put(jvm.arr(bad), res) == 1 and jvm.read(res, np.int64, 4).tolist() == [-1, 2, 0, 0]
    # the put: three new ids, the second record of id 5 loses, id 64 is skipped, id -1 is not considered
    assert put(jvm.arr(off), res) == 0
    st, want = ref.cmds_put(cmds, ids)
    assert st == 0 and jvm.read(res, np.int64, 4).tolist() == list(want) == [3, 22, 1, 0]
    stats = jvm.arr(np.full(4, -9, np.int64))
    assert jvm.call("epxCmdsStats", C.c_int32, H, stats) == 0
    assert tuple(jvm.read(stats, np.int64, 4).tolist()) == ref.cmds_stats() == (3, 22, 1, 0)
    assert jvm.call("epxCmdsStats", C.c_int32, H, jvm.arr(np.zeros(3, np.int64))) == 1
    assert put(jvm.arr(off), None, count=0) == 0                                          # an empty burst, no result asked for
    from frankenpaxos_amd.epaxos import EPaxos
    peer = EPaxos.__new__(EPaxos)
    peer.L, peer.n, peer.num_keys, peer._h = ref.L, n, NK, C.c_void_p(h)
    assert [peer.cmds_read(t) for t in range(64)] == [ref.cmds_read(t) for t in range(64)]
    assert peer.cmds_read(5) == b"first" and peer.cmds_read(6) == b"" and peer.cmds_read(8) is None
    # the bytes tick native on this context: a Commit learnt and asked for comes back as a Commit with its bytes
    z = [0] * n
    msgs = [(IM.IN_COMMIT, 0, 1, 2, 0, 1, (1, 2), 1, 9, z, 0), (IM.IN_PREPARE, 0, 1, 2, 9, 2, (), 0, -1, z, 0)]
    frames = [frame(wire, x) for x in msgs]
    m = len(msgs)
    fb, fo = wire.pack(frames)
    in_len = int(fo[-1])
    cap = m * wire.epx_cmd_reply_max(len(command_of(msgs[0])))
    fill = lambda k, v, t: direct(jvm, k * np.dtype(t).itemsize, np.full(k, v, t))
    dout, dooff, dkind = fill(cap, 0xEE, np.uint8), fill(m + 1, -9, np.int64), fill(m, 9, np.uint8)
    result = jvm.arr(np.full(6, -9, np.int64))
    assert jvm.call("epxWireReplicaTickBytes", C.c_int32, H, m, n, direct(jvm, in_len, fb[:in_len]), C.c_int64(in_len),
                    direct(jvm, 8 * (m + 1), fo), direct(jvm, 4 * m, np.zeros(m, np.int32)), 0,
                    jvm.arr(np.array([9, -1], np.int32)), 8, dout, C.c_int64(cap), dooff, dkind, None, None, None, result) == 0
    want = ref.wire_replica_tick_bytes(frames, [0, 0], max_pairs=8, triple_id=[9, -1], out_cap=cap)
    assert want["status_code"] == 0 and want["reply_kind"].tolist() == [0, 1] and want["totals"][2] == 0
    need = int(want["totals"][1])
    assert jvm.read(result, np.int64, 6).tolist()[2:] == want["totals"].tolist()
    assert jvm.read(dkind, np.uint8, m).tolist() == [0, 1]
    assert jvm.read(dout, np.uint8, cap)[:need].tobytes() == want["out"][:need].tobytes()
    assert command_of(msgs[0]) in want["replies"][1] and peer.cmds_read(9) == command_of(msgs[0])
    peer._h = None
    assert jvm.call("epxDestroy", C.c_int32, H) == 0
    ref.close()
