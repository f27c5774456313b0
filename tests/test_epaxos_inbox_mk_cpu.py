"""fpx_epx_replica_inbox_mk without a GPU: the key-list model the GPU tests compare with (tests/epaxos_inbox_mk_model.py)
against the single-key InboxModel on one-key lists, a census of what the generated bursts exercise (so that the GPU comparison
cannot pass on bursts that never need the merge over a command's keys), two bursts worked by hand, the call's scratch layout
in a stand-alone program under the sanitizers, and the declarations of the new entry points through every layer."""
import os
import re
import subprocess

from tests import epaxos_inbox_model as IM
from tests import epaxos_inbox_mk_model as MM
from tests import epaxos_inbox_mk_streams as MS
from tests import epaxos_inbox_streams as S
from tests.test_epaxos_inbox_cpu import MODEL_BURSTS as SINGLE_KEY_BURSTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JNI = os.path.join(ROOT, "frankenpaxos_amd", "jni")
NK, NI = 4, 64
# the bursts tests/test_gpu_epaxos_inbox_mk.py holds against the model: (seed, n, m)
MODEL_BURSTS = [(111 + j, n, m) for j, (n, m) in enumerate((n, m) for n in (3, 5, 7) for m in (65, 1025))]


def replica_state(model):
    out = []
    for rep in model.replicas:
        log = {k: (e.kind, e.ballot, e.vote_ballot, e.triple_id, e.deps) for k, e in rep.cmd_log.items()}
        out.append((log, rep.largest_ballot, [list(r) for r in rep.gets], [list(r) for r in rep.sets]))
    return out


def test_one_key_lists_are_the_single_key_model():
    for seed, n, m in SINGLE_KEY_BURSTS + [(5, 5, 1500)]:
        single = S.make_burst(seed, n, m, num_keys=NK)
        lists = [x[:6] + ((x[6],) if x[6] >= 0 else (),) + x[7:] for x in single]     # a Noop is the empty list
        assert MS.single_key_form(lists) == single
        a, b = IM.InboxModel(n, NK, NI), MM.InboxMkModel(n, NK, NI)
        (st_a, rows_a), (st_b, rows_b) = a.inbox(single), b.inbox(lists)
        assert st_a == st_b == IM.OK
        for i, (x, y) in enumerate(zip(rows_a, rows_b)):
            assert x == y, (seed, i, single[i], x, y)
        assert replica_state(a) == replica_state(b), seed


def test_census_of_the_generated_bursts():
    """conditions on the INPUTS of the GPU test: every reachable (kind, outcome), at least 5 % of the processed PreAccepts
    with a conflict only the merge over the command's keys finds, repeated keys, empty lists, the longest list"""
    processed = cross = 0
    for seed, n, m in MODEL_BURSTS:
        msgs = MS.make_burst(seed, n, m, num_keys=NK, num_instances=NI)
        assert len(msgs) == m
        c = MS.census(n, NK, msgs)
        assert set(c["pairs"]) <= IM.REACHABLE, c["pairs"]
        if m >= 1000:
            missing = IM.REACHABLE - set(c["pairs"])
            assert not missing, (n, [(k, IM.OUTCOME_NAMES[o]) for k, o in missing], c["pairs"])
            assert 20 * c["cross_key"] >= c["processed"] > 0, (seed, c["cross_key"], c["processed"])
            assert c["empty"] >= 1 and c["max_keys"] == 5
        assert c["repeated"] >= 1, seed
        processed, cross = processed + c["processed"], cross + c["cross_key"]
    assert 20 * cross >= processed, (cross, processed)
    # ... and over the small bursts alone
    small = [MS.census(n, NK, MS.make_burst(seed, n, m)) for seed, n, m in MODEL_BURSTS if m < 1000]
    assert 20 * sum(c["cross_key"] for c in small) >= sum(c["processed"] for c in small) > 0
    seen = set().union(*(set(MS.census(n, NK, MS.make_burst(seed, n, m))["pairs"]) for seed, n, m in MODEL_BURSTS))
    assert seen == IM.REACHABLE


def test_the_generated_messages_are_valid_and_the_list_rules_refuse():
    n = 5
    model = MM.InboxMkModel(n, NK, NI)
    burst = MS.make_burst(112, n, 400)
    assert all(model.valid(x) for x in burst)
    good = (IM.IN_PRE_ACCEPT, 1, 2, 5, 1, 1, (0, 3, 0), 1, 7, [0, 0, 5, 0, 0], 7)
    assert model.valid(good)
    for keys in ((NK,), (0, -1), (1, 2, NK + 3)):
        assert not model.valid(good[:6] + (keys,) + good[7:]), keys
    for field, value in ((0, 4), (1, n), (2, -1), (3, NI), (4, 1 << 27), (5, n), (9, [0, -1, 5, 0, 0]), (10, 6)):
        bad = list(good)
        bad[field] = value
        assert not model.valid(tuple(bad)), (field, value)
    assert model.valid(good[:6] + ((),) + good[7:])                                   # no keys: as a Noop
    off, keys = MS.csr(burst)
    assert off[0] == 0 and off[-1] == len(keys) == sum(len(x[6]) for x in burst) and (off[1:] >= off[:-1]).all()
    for pairs in (0, 1023, 1024, 1025):
        assert sum(len(x[6]) for x in MS.with_pairs(burst, pairs)) == pairs


# ---- two bursts worked by hand, n = 3, at replica 0; keys a, b, c, d = 0, 1, 2, 3 -------------------------------------------
def _hand(second_keys):
    z = [0, 0, 0]
    return [(IM.IN_PRE_ACCEPT, 0, 1, 4, 0, 1, (0, 1), 1, 7, z, 0),          # a set on {a, b}: instance (1, 4)
            (IM.IN_PRE_ACCEPT, 0, 2, 6, 0, 2, second_keys, 0, 8, z, 0)]     # a get: instance (2, 6)


def test_a_get_depends_on_a_set_through_the_one_key_they_share():
    model = MM.InboxMkModel(3, NK, NI)
    st, rows = model.inbox(_hand((1, 2)))
    assert st == IM.OK
    assert rows[0] == (IM.RI_PRE_ACCEPT_OK, -1, -1, frozenset(), 7)
    # through b alone: the set is the top of b's set row in column 1, and a top-one index answers the prefix below it
    assert rows[1] == (IM.RI_PRE_ACCEPT_OK, -1, -1, frozenset({(1, 0), (1, 1), (1, 2), (1, 3), (1, 4)}), 8)
    rep = model.replicas[0]
    assert rep.sets == [[0, 5, 0], [0, 5, 0], [0, 0, 0], [0, 0, 0]]                  # the set under a and under b
    assert rep.gets == [[0, 0, 0], [0, 0, 7], [0, 0, 7], [0, 0, 0]]                  # the get under b and under c
    assert all(r.sets == [[0] * 3] * 4 and r.gets == [[0] * 3] * 4 for r in model.replicas[1:])
    assert MS.census(3, NK, _hand((1, 2)))["cross_key"] == 0                          # b is the FIRST key of the get's list
    assert MS.census(3, NK, _hand((2, 1)))["cross_key"] == 1                          # ... and here it is not


def test_a_get_on_other_keys_has_no_dependency():
    model = MM.InboxMkModel(3, NK, NI)
    st, rows = model.inbox(_hand((2, 3)))
    assert st == IM.OK
    assert rows == [(IM.RI_PRE_ACCEPT_OK, -1, -1, frozenset(), 7), (IM.RI_PRE_ACCEPT_OK, -1, -1, frozenset(), 8)]
    rep = model.replicas[0]
    assert rep.sets == [[0, 5, 0], [0, 5, 0], [0, 0, 0], [0, 0, 0]]
    assert rep.gets == [[0, 0, 0], [0, 0, 0], [0, 0, 7], [0, 0, 7]]


def test_the_scratch_layout_is_aligned_disjoint_and_inside_its_size(tmp_path):
    exe = str(tmp_path / "epx_inbox_mk_scratch")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                            exe, os.path.join(ROOT, "tests", "epx_inbox_mk_scratch_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "all layouts ok" and not [ln for ln in lines if ln.startswith("FAIL")]
    assert sum(ln.startswith("ok ") for ln in lines) == 6 * 4 * 3        # m x P x n
    assert "arrays=9" in lines[0]


def test_the_binding_the_header_and_the_natives_agree():
    from frankenpaxos_amd import _lib, epaxos as E

    hdr = open(os.path.join(ROOT, "include", "fpx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, args in (("fpx_epx_replica_inbox_mk", 20), ("fpx_epx_replica_inbox_mk_dev", 21), ("fpx_epx_lead_mk", 13),
                       ("fpx_epx_lead_accept_mk", 13)):
        decl = re.search(r"\b" + name + r"\(([^)]*)\)", code, flags=re.S).group(1)
        assert len(decl.split(",")) == args == len(_lib.SIGNATURES[name][1]), name
    assert "#define FPX_EPX_KEY_LIST (-2)" in hdr and E.KEY_LIST == -2
    assert MM.MAX_PAIRS == 1 << 23 and "#define FPX_EPX_MK_MAX_PAIRS (1 << 23)" in hdr
    scala = open(os.path.join(JNI, "Native.scala")).read()
    shim = open(os.path.join(JNI, "fpx_jni.c")).read()
    names = lambda text: [p.split(":")[0].split()[-1].strip("* ") for p in text.split(",") if p.strip()]
    for name, call in (("epxReplicaInboxMk", "fpx_epx_replica_inbox_mk"), ("epxLeadMk", "fpx_epx_lead_mk"),
                       ("epxLeadAcceptMk", "fpx_epx_lead_accept_mk")):
        d = re.search(r"@native def %s\(([^)]*)\)" % name, scala, flags=re.S)
        c = re.search(r"Java_frankenpaxos_gpu_Native_%s\(\s*JNIEnv\* env, jclass cls,?([^)]*)\)\s*\{(.*?)\n\}" % name, shim, flags=re.S)
        assert d and c, name
        assert names(d.group(1)) == ["handle" if x == "h" else x for x in names(c.group(1))], name
        assert call + "(" in c.group(2), name


def test_the_actor_has_no_single_key_limit_left_among_remote_peers():
    actor = open(os.path.join(JNI, "EPaxosNative.scala")).read()
    assert "multi-key lead is not built" not in actor and "Limits: single-key" not in actor
    assert "single-key commands and Noops only" not in actor
    for native in ("epxReplicaInbox", "epxLead", "epxLeadAccept"):                  # one call of each form per flush
        assert actor.count("Native.%s(" % native) == 1 and actor.count("Native.%sMk(" % native) == 1, native
        assert re.search(r"if \(engine\.singleKeys\(\w+\)\)\s*Native\.%s\(" % native, actor), native
