"""fpx_leader_phase1b_msgs without a GPU: the model of tests/leader_phase1b_model.py against the existing oracle's
Phase-1 scan and against the hand-written cases, the streams' promises, the bindings, the JNI native's argument checks
on the mock JNIEnv, and the host half of the entry point under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import phase1b_streams as PS
from tests import workloads as W
from tests.leader_phase1b_model import Geometry, Msg, flatten, handle_burst
from tests.test_jni_shim import jvm  # noqa: F401  (the mock JVM fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def group_of(s, L, A):
    return (s % L) * A + (s // L) % A


def vote(ref, S, R, L, A, seed):
    rng = np.random.default_rng(seed)
    for rnd in (0, 1, 3):
        slot = np.sort(rng.permutation(S)[: S // 2]).astype(np.int32)
        tgt = W.bits_from_bool(W.random_subsets(rng, len(slot), R, 1, R))
        rr = np.full(len(slot), rnd, np.int32)
        ref.proxy_open(slot, rr, W.steady_values(slot) + rnd)
        assert ref.acceptor_phase2a(slot, rr, W.steady_values(slot) + rnd, tgt)[0] == 0


@pytest.mark.parametrize("A,L", [(1, 1), (3, 1), (2, 4)])
def test_model_equals_the_oracles_scan(oracle, A, L):
    S, R, f, wm = 512, 5, 2, 37
    ref = oracle.System(oracle.make_config(num_slots=S, num_replicas=R, num_groups=A, num_leader_groups=L, f=f, tally_ways=8))
    vote(ref, S, R, L, A, 10 * A + L)
    rng = np.random.default_rng(A + L)
    quorum = W.random_subsets(rng, A * L, R, f + 1, f + 1)   # exactly f + 1: the handler stops there
    st, mx, sr, sv = ref.leader_phase1b_scan(wm, W.bits_from_bool(quorum), S)
    assert st == 0 and mx > wm and (sr >= 0).any() and (sr < 0).any()
    geo = Geometry(num_groups=A, num_leader_groups=L, f=f, total=R)
    tops = []
    for lg in range(L):
        msgs = []
        for ag in range(A):
            for a in np.flatnonzero(quorum[lg * A + ag]):
                sl, vr, vv = ref.acceptor_phase1b_info(lg * A + ag, int(a), wm)
                msgs.append(Msg(7, ag, int(a), list(zip(sl.tolist(), vr.tolist(), vv.tolist()))))
        order = rng.permutation(len(msgs))
        got = handle_burst(geo, 7, wm, [msgs[i] for i in order], leader_group=lg)
        assert got.status == 0 and got.complete == 1
        tops.append(got.max_slot)
        idx = np.array(got.out_slot) - wm
        assert (np.array(got.out_slot) % L == lg).all() and len(idx) == len(range(W.next_classic_round(L, lg, wm - 1), got.max_slot + 1, L))
        np.testing.assert_array_equal(got.safe_round, sr[idx])
        np.testing.assert_array_equal(got.safe_value, sv[idx])
    assert max(tops) == mx


@pytest.mark.parametrize("name", sorted(PS.hand_cases()))
def test_hand_written_cases(name):
    cfg, geo, kw, msgs, exp = PS.hand_cases()[name]
    got = handle_burst(geo, msgs=msgs, **kw)
    for k, v in exp.items():
        assert getattr(got, k) == v, (k, getattr(got, k), v)


@pytest.mark.parametrize("name", sorted(PS.einval_cases()))
def test_einval_cases(name):
    cfg, geo, kw, msgs, index, off_bad = PS.einval_cases()[name]
    got = handle_burst(geo, msgs=msgs, offsets_bad_at=off_bad, **kw)
    assert (got.status, got.err_index, got.complete) == (1, index, None)
    if off_bad is not None:
        off = PS.break_offsets(flatten(msgs), name)["offsets"]
        assert off[0] != 0 or (np.diff(off) < 0).argmax() == off_bad


def test_the_literal_grid_rule_and_all_rows_differ():
    c = PS.hand_cases()
    assert c["i_grid_literal"][4]["safe_value"] != c["i_grid_all_rows"][4]["safe_value"]


def test_streams_keep_their_promises():
    for shape in PS.SHAPES:
        runs = set()
        for seed in PS.SEEDS:
            s = PS.Stream(shape, seed)      # (asserts its own promises)
            runs |= s.used_runs
            assert flatten(s.msgs)["offsets"][-1] == sum(len(m.info) for m in s.msgs)
        if PS.SHAPES[shape]["flavour"] == "edges":
            assert runs >= set(PS.EDGE_RUNS), (shape, runs)
    assert PS.SHAPES["r130"]["cfg"]["f"] + 1 > 64               # the held bits cross a 64-bit word


# ---- bindings ------------------------------------------------------------------------------------------------------
def test_abi_and_python_prototypes():
    import frankenpaxos_amd as fa
    from frankenpaxos_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "fpx.h")).read()
    for name in ("fpx_leader_phase1b_msgs", "fpx_leader_phase1b_msgs_dev"):
        decl = re.search(r"int32_t %s\((.*?)\);" % name, hdr, re.S).group(1)
        nargs = len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(","))
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs == 22
        assert getattr(fa.lib(), name) is not None
    assert (_lib.FPX_P1B_GRID_ALL_ROWS, _lib.FPX_P1B_RESULT_WORDS) == (1, 8)
    for word, at in (("COMPLETE", 0), ("DECIDED_AT", 1), ("COUNT", 2), ("MAX_SLOT", 3), ("NEXT_SLOT", 4), ("WRITTEN", 5)):
        assert re.search(r"FPX_P1B_%s = %d," % (word, at), hdr) and getattr(_lib, "FPX_P1B_" + word) == at
    assert hasattr(fa.Context, "leader_phase1b_msgs") and hasattr(fa.Context, "leader_phase1b_msgs_dev")
    for f, needle in (("frankenpaxos_amd/host/fpx.hpp", "leaderHandlePhase1bMsgs"), ("frankenpaxos_amd/jni/Native.scala", "leaderPhase1bMsgs"),
                      ("frankenpaxos_amd/jni/Native.scala", "class GpuLeaderRecovery"),
                      ("frankenpaxos_amd/jni/MenciusNative.scala", "class GpuMenciusLeaderRecovery")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)


def test_the_jni_native_checks_its_arrays_before_native_code_runs(jvm):  # noqa: F811
    a = flatten(PS.hand_cases()["a_basic"][3])
    names = ("kind", "msg_round", "group_index", "acceptor_index", "offsets", "info_slot", "info_vote_round", "info_value_id")
    outs = [jvm.arr(np.zeros(5, np.int32)) for _ in range(3)]
    result = jvm.arr(np.zeros(8, np.int64))
    scalars = jvm.arr(np.array([4, 1, 0, -1, 0, 0], np.int32))

    def call(short=None, scalars=scalars, result=result, n=3, cap=5, outs=outs):
        ins = [jvm.arr(a[k][:-1] if k == short else a[k]) for k in names]
        return jvm.call("leaderPhase1bMsgs", C.c_int32, 0, scalars, n, *ins, cap, *outs, result, None)   # handle 0

    for short in ("msg_round", "acceptor_index", "offsets", "kind", "group_index"):
        assert call(short) == 1
    assert call(scalars=jvm.arr(np.zeros(5, np.int32))) == 1 and call(result=jvm.arr(np.zeros(7, np.int64))) == 1
    assert call(n=-1) == 1 and call(cap=-1) == 1 and call(outs=[outs[0], outs[1], jvm.arr(np.zeros(4, np.int32))]) == 1
    assert call() == 1                                           # no context behind the handle


def test_the_cxx_mirror_compiles_with_the_new_method(tmp_path):
    src = tmp_path / "m.cpp"
    src.write_text('#include "frankenpaxos_amd/host/fpx.hpp"\nint main() { return 0; }\n')
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_host_half_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "leader_phase1b_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                            os.path.join(ROOT, "tests", "leader_phase1b_host_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "host half ok" in run.stdout, run.stdout + run.stderr
