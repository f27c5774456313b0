"""fpx_epx_replica_inbox without a GPU: the model the GPU tests compare with (tests/epaxos_inbox_model.py) against the set
model's own Accept phase, a census of what the generated bursts exercise (so that the GPU comparison cannot be vacuous), the
call's scratch layout in a stand-alone program under the sanitizers, and the JNI native's declaration and argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from oracle import epaxos_sets as ES
from tests import epaxos_inbox_model as IM
from tests import epaxos_inbox_streams as S
from tests.test_jni_shim import JNI, jvm  # noqa: F401  (the mock-JVM fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bursts tests/test_gpu_epaxos_inbox.py holds against the model: (seed, n, m)
MODEL_BURSTS = [(11, 3, 400), (12, 5, 400), (13, 7, 400)]


def at_replica(model, t, inst, num_keys):
    rep = model.replicas[t]
    e = rep.cmd_log.get(inst)
    entry = None if e is None else (e.kind, e.ballot, e.vote_ballot, e.triple_id, e.deps)
    return entry, rep.largest_ballot, [list(r) for r in rep.gets], [list(r) for r in rep.sets]


def clone(model):
    """a copy that shares nothing mutable with `model` (dependency sets are frozen)"""
    out = IM.InboxModel(model.n, model.num_keys, model.num_instances)
    for src, dst in zip(model.replicas, out.replicas):
        dst.cmd_log = {k: ES.Entry(e.kind, e.ballot, e.vote_ballot, e.triple_id, e.deps) for k, e in src.cmd_log.items()}
        dst.largest_ballot = src.largest_ballot
        dst.gets, dst.sets = [list(r) for r in src.gets], [list(r) for r in src.sets]
    return out


def test_handle_accept_is_the_target_branch_of_the_accept_phase():
    n, num_keys = 5, 4
    base = IM.InboxModel(n, num_keys)
    seen, legal = {}, 0
    for msg in S.make_burst(5, n, 1500, num_keys=num_keys):
        kind, to, L, x, bo, br, key, is_set, tid, w, end = msg
        if kind == IM.IN_ACCEPT and br != to:
            whole, alone = clone(base), clone(base)
            # the whole phase: the proposer's own step, then handleAccept at `to`; at n = 5 two AcceptOks are no quorum
            fatal, replies, committed = ES.EPaxos.accept(whole, (L, x), (bo, br), tid, [to], key, bool(is_set))
            if not fatal:                                     # (the proposer's own step is legal)
                legal += 1
                assert not committed
                r = alone.handle_accept((L, x), (bo, br), tid, None, to, key, bool(is_set))
                want = replies[to]
                assert {"commit": "commit", "nack": "nack", "again": "ok", "ok": "ok"}[r[0]] == want[0]
                if r[0] == "nack":
                    assert r[1] == want[1]
                assert at_replica(alone, to, (L, x), num_keys) == at_replica(whole, to, (L, x), num_keys)
                seen[r[0]] = seen.get(r[0], 0) + 1
        base.deliver(msg)
    assert legal >= 100, legal
    assert all(seen.get(k, 0) >= 3 for k in ("commit", "nack", "again", "ok")), seen


def test_census_of_the_generated_bursts():
    for seed, n, m in MODEL_BURSTS:
        c = S.census(n, 4, S.make_burst(seed, n, m))
        missing = IM.REACHABLE - set(c["pairs"])
        assert not missing, (n, [(k, IM.OUTCOME_NAMES[o]) for k, o in missing], c["pairs"])
        assert set(c["pairs"]) <= IM.REACHABLE, c["pairs"]
        assert c["longest_run"] >= 3, c["longest_run"]
        assert c["multi_to"] >= 1, c["multi_to"]
        assert c["conflict_from"][IM.IN_ACCEPT] >= 1 and c["conflict_from"][IM.IN_COMMIT] >= 1, c["conflict_from"]
        for o in (IM.RI_PRE_ACCEPT_OK_AGAIN, IM.RI_COMMIT_BACK, IM.RI_PREPARE_OK):
            assert c["deps_from_burst"].get(o, 0) >= 1, (n, IM.OUTCOME_NAMES[o], c["deps_from_burst"])
        assert c["nack_raised"] >= 1, c["nack_raised"]
    # the shaped bursts: one cell 200 messages long with every kind on it; one key under every message
    c = S.census(5, 4, S.long_run(5, 200))
    assert c["longest_run"] == 200 and len({k for k, _ in c["pairs"]}) == 4 and len(c["pairs"]) >= 10, c
    hot = S.make_burst(3, 5, 1025, hot_key=0, hot_to=2)
    assert len(hot) == 1025 and {x[6] for x in hot} == {0} and {x[1] for x in hot} == {2}
    c = S.census(5, 4, hot)
    puts = sum(c["pairs"].get(p, 0) for p in ((IM.IN_PRE_ACCEPT, IM.RI_PRE_ACCEPT_OK), (IM.IN_ACCEPT, IM.RI_ACCEPT_OK),
                                              (IM.IN_COMMIT, IM.RI_LEARNT)))
    assert puts > 4 * 64, c["pairs"]                  # the (replica 2, key 0) segment of the scan: more than four chunks


def test_every_generated_message_is_valid_and_the_checks_refuse():
    n = 5
    model = IM.InboxModel(n, 4, 64)
    burst = S.make_burst(12, n, 400)
    assert all(model.valid(x) for x in burst)
    good = (IM.IN_PRE_ACCEPT, 1, 2, 5, 1, 1, 0, 1, 7, [0, 0, 5, 0, 0], 7)
    assert model.valid(good)
    for field, value in ((0, 4), (1, n), (2, -1), (3, 64), (4, 1 << 27), (5, n), (6, 4), (6, -2), (9, [0, -1, 5, 0, 0]),
                         (9, [0, 0, 4, 0, 0]), (10, 6)):
        bad = list(good)
        bad[field] = value
        assert not model.valid(tuple(bad)), (field, value)
    assert model.valid((IM.IN_COMMIT, 0, 2, 5, -7, 99, 0, 0, 7, [-1, 0, 0, 0, 0], 0))      # no ballot on a Commit
    assert model.valid((IM.IN_PREPARE, 0, 2, 5, 0, 0, 99, 0, 7, [0] * n, 0))               # no key on a Prepare
    assert not model.valid((IM.IN_COMMIT, 0, 2, 5, 0, 0, 0, 0, 7, [0, 0, 6, 0, 0], 7))     # explicit ids over a cover


def test_the_scratch_layout_is_aligned_disjoint_and_inside_its_size(tmp_path):
    exe = str(tmp_path / "epx_inbox_scratch")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                            exe, os.path.join(ROOT, "tests", "epx_inbox_scratch_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "all layouts ok" and not [ln for ln in lines if ln.startswith("FAIL")]
    assert sum(ln.startswith("ok ") for ln in lines) == 7 * 3          # seven sizes at three replica counts
    assert "arrays=7" in lines[0]


def test_the_binding_the_header_and_the_natives_agree():
    from frankenpaxos_amd import _lib, epaxos as E

    hdr = open(os.path.join(ROOT, "include", "fpx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("fpx_epx_replica_inbox", "fpx_epx_replica_inbox_dev"):
        decl = re.search(r"\b" + name + r"\(([^)]*)\)", code, flags=re.S).group(1)
        assert len(decl.split(",")) == 19 == len(_lib.SIGNATURES[name][1]), name
    for k, name in enumerate(("PRE_ACCEPT", "ACCEPT", "COMMIT", "PREPARE")):
        assert re.search(r"FPX_EPX_IN_%s = %d\b" % (name, k), code) and getattr(E, "IN_" + name) == k
    for o, name in enumerate(IM.OUTCOME_NAMES):
        assert re.search(r"FPX_EPX_RI_%s = %d\b" % (name, o), code), name
        assert getattr(E, "RI_" + name) == o == getattr(IM, "RI_" + name)
    assert "#define FPX_EPX_INBOX_MAX (1 << 24)" in hdr and E.INBOX_MAX == 1 << 24 >= 1 << 20
    scala = open(os.path.join(JNI, "Native.scala")).read()
    shim = open(os.path.join(JNI, "fpx_jni.c")).read()
    d = re.search(r"@native def epxReplicaInbox\(([^)]*)\)", scala, flags=re.S)
    c = re.search(r"Java_frankenpaxos_gpu_Native_epxReplicaInbox\(\s*JNIEnv\* env, jclass cls,?([^)]*)\)", shim, flags=re.S)
    assert d and c
    count = lambda t: len([p for p in t.split(",") if p.strip()])
    assert count(d.group(1)) == count(c.group(1)) == 17


def test_native_argument_checks_without_a_device(jvm):  # noqa: F811
    i32 = lambda k: jvm.arr(np.zeros(k, np.int32))
    i8 = lambda k: jvm.arr(np.zeros(k, np.int8))
    n, m = 5, 4
    full = lambda: [i32(m)] * 7 + [i8(m), i32(m), i32(n * m), i32(m), i32(m), i32(4 * m), i32(n * m)]
    # no context behind handle 0: refused, whatever the arrays are; a negative batch and n < 3 likewise
    assert jvm.call("epxReplicaInbox", C.c_int32, 0, m, n, *full()) == 1
    assert jvm.call("epxReplicaInbox", C.c_int32, 0, -1, n, *[None] * 14) == 1
    assert jvm.call("epxReplicaInbox", C.c_int32, 0, m, 2, *[None] * 14) == 1
    # every array one short, and every input missing: refused, and the mock JVM (which aborts on any access outside an
    # array) was never asked for a region that is not there.  On a live handle: tests/test_gpu_epaxos_inbox.py
    short = [i32(m - 1)] * 7 + [i8(m - 1), i32(m - 1), i32(n * m - 1), i32(m - 1), i32(m - 1), i32(4 * m - 1), i32(n * m - 1)]
    for j in range(14):
        args = full()
        args[j] = short[j]
        assert jvm.call("epxReplicaInbox", C.c_int32, 0, m, n, *args) == 1
        if j < 10:
            args[j] = None
            assert jvm.call("epxReplicaInbox", C.c_int32, 0, m, n, *args) == 1


def test_the_actor_sends_a_burst_through_one_native_call_only_when_asked_to():
    actor = open(os.path.join(JNI, "EPaxosNative.scala")).read()
    assert "inboxBurst: Boolean = false" in actor
    assert actor.count("Native.epxReplicaInbox(") == 1                                       # ONE call per flush
    for kind, msg in ((0, "PreAccept"), (1, "Accept"), (2, "Commit"), (3, "Prepare")):
        assert re.search(r"case Request\.%s\(r\) if inboxBurst\s*=>\s*enqueue\(peerInbox, PeerEvent\(%d," % (msg, kind), actor), msg
