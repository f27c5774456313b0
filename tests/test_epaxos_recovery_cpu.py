"""Originating recovery without a GPU: the model the GPU tests compare with (tests/epaxos_recovery_model.py) against the set
model's independent restatement of handlePrepareOk (oracle/epaxos_sets.py), the census of the generator's streams, hand-worked
cases with their reference lines, and the surface: header, binding, model codes, exported symbols, refusals that need no
device, the C++ mirror, the JNI shim."""
import collections
import ctypes as C
import os
import random
import re
import subprocess

import pytest

from oracle import epaxos_sets as ES
from tests import epaxos_leader_model as M
from tests import epaxos_leader_streams as LS
from tests import epaxos_recovery_model as R
from tests import epaxos_recovery_streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fpx_epx_recover", "fpx_epx_recovery_replies", "fpx_epx_recovery_replies_dev", "fpx_epx_lead_accept",
               "fpx_epx_read_recovery_state")


# ---- the decision against oracle/epaxos_sets.py::EPaxos.handle_prepare_oks ---------------------------------------------------
def _random_case(seed, n):
    """entries of one instance at the replicas of ONE model, a recovery at `me`, the Prepare at f peers: (model, instance,
    me, ballot, the peers' PrepareOks as the set model's handlePrepare answers them)"""
    rng = random.Random(seed)
    model = R.RecoveryModel(n, 4, 16)
    inst = (rng.randrange(n), rng.randrange(4))
    other = ((inst[0] + 1) % n, 0)                                  # (a prefix of another leader's column)
    for r in range(n):
        what = rng.choice(("none", "pre", "pre", "pre_deps", "pre_high", "accepted", "no_command"))
        if what == "pre":
            model.peer_preaccept(inst, (0, inst[0]), 1, True, 50, set(), [r])
        elif what == "pre_deps":                                       # another triple: one more dependency
            model.peer_preaccept(inst, (0, inst[0]), 1, True, 50, {other}, [r])
        elif what == "pre_high":
            model.peer_preaccept(inst, (1, (r + 1) % n), 1, True, 51, set(), [r])
        elif what == "accepted":
            model.replicas[r].cmd_log[inst] = ES.Entry(ES.ACCEPTED, (2, 0), (2, 0), 52, frozenset({other}))
            model.replicas[r].largest_ballot = max(model.replicas[r].largest_ballot, (2, 0))
        elif what == "no_command":
            model.peer_prepare(inst, (1, (r + 1) % n), [r])
    me = rng.randrange(n)
    for rep in model.replicas:                                         # (so that the recovery's ballot is above every entry's)
        model.replicas[me].largest_ballot = max(model.replicas[me].largest_ballot, rep.largest_ballot)
    peers = [r for r in range(n) if r != me]
    rng.shuffle(peers)
    return model, inst, me, peers[:model.f]


@pytest.mark.parametrize("as_intended", [False, True])
@pytest.mark.parametrize("n", [3, 5, 7])
def test_the_decision_equals_the_set_models_handle_prepare_oks(n, as_intended):
    seen = collections.Counter()
    for seed in range(120):
        model, inst, me, peers = _random_case(seed, n)
        st, out = model.recover([(inst[0], inst[1], me)])
        assert st == R.OK and out[0][0] == R.RV_PREPARING
        ballot = (out[0][1], me)
        own = model.leader_states[me][inst].responses[me]
        responses = {me: (own.status, own.vote_ballot, own.triple_id, own.deps)}
        msgs = []
        for q in peers:
            rep = ES.EPaxos.prepare(model, inst, ballot, [q])[q]       # the set model's handlePrepare
            assert rep[0] == "ok"
            deps = model.replicas[q].cmd_log[inst].deps if rep[1] != ES.NONE else None
            responses[q] = (rep[1], rep[2], rep[3], deps)
            w, end = LS.encode_deps(n, inst, deps) if deps is not None else ([0] * n, 0)
            msgs.append((me, inst[0], inst[1], ballot[0], ballot[1], q, rep[1], rep[2][0], rep[2][1], rep[3], 0, w, end))
        want = ES.EPaxos.handle_prepare_oks(model, inst, ballot, me, responses, as_intended)
        st, rows, decided = model.prepare_oks(msgs, as_intended)
        assert st == R.OK and decided == [len(msgs) - 1] and all(r[0] == R.RC_WAITING for r in rows[:-1])
        outcome, src, tid = rows[-1][:3]
        got = {R.RC_ACCEPT: ("accept", src, tid), R.RC_PRE_ACCEPT: ("preaccept", src, tid), R.RC_PRE_ACCEPT_NOOP: ("noop",)}[outcome]
        assert got == want, (seed, responses)
        seen[want[0]] += 1
        # and one response short, both wait
        assert ES.EPaxos.handle_prepare_oks(model, inst, ballot, me, {me: responses[me]}, as_intended) == ("wait",) or model.f == 0
    assert seen["preaccept"] and seen["noop"] and (seen["accept"] or not as_intended), seen


# ---- the census: a condition on the generator --------------------------------------------------------------------------------
@pytest.mark.parametrize("as_intended", [False, True])
@pytest.mark.parametrize("n", [3, 5, 7])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_stream_reaches_every_branch_and_every_outcome(seed, n, as_intended):
    ops, census = S.make_stream(seed, n, as_intended)
    missing = [k for k in S.CENSUS_COMMON + S.CENSUS_DECISIONS[as_intended] if not census[k]]
    assert not missing, missing
    # the outcome codes themselves, from a model of its own
    model, rv, rc, nack = R.RecoveryModel(n, 4, 64), collections.Counter(), collections.Counter(), collections.Counter()
    fatal_status = collections.Counter()
    for op in ops:
        res = S.run_op(model, op)
        if op[0] == "recover":
            rv.update(r[0] for r in res[1])
            fatal_status[("recover", res[0])] += 1
        elif op[0] == "prepare_oks":
            rc.update(r[0] for r in res[1])
            fatal_status[("prepare_oks", res[0])] += 1
            assert res[2] == [i for i, r in enumerate(res[1]) if r[0] in (R.RC_ACCEPT, R.RC_PRE_ACCEPT, R.RC_PRE_ACCEPT_NOOP)]
        elif op[0] == "replies":
            nack.update(r[0] for r in res[1])
    assert set(rv) == {R.RV_PREPARING, R.RV_COMMITTED, R.RV_FATAL}
    want = {R.RC_IGNORED, R.RC_WAITING, R.RC_PRE_ACCEPT, R.RC_PRE_ACCEPT_NOOP, R.RC_FATAL} | ({R.RC_ACCEPT} if as_intended else set())
    assert set(rc) == want, rc
    assert nack[M.NACK_RECOVER] and nack[M.NACK_IGNORED] and nack[M.SLOW_COMMIT]
    assert fatal_status[("recover", R.EFATAL)] and fatal_status[("prepare_oks", R.EFATAL)]
    assert model.census == census


def test_the_burst_generator_decides_and_repeats():
    for m in (257, 4097):
        rec, burst = S.random_burst(m, 7, m)
        model = R.RecoveryModel(7, 4, 64)
        S.run_op(model, rec)
        st, rows, decided = S.run_op(model, ("prepare_oks", burst, True))
        assert st == R.OK and len(rows) == m and decided
        assert model.census["ok_replaced"] and model.census["ok_stale"] and model.census["ok_not_preparing"]


# ---- hand-worked cases ------------------------------------------------------------------------------------------------------
def _ok(q, status=0, vote=(-1, -1), tid=-1, w=None, end=0, to=0, inst=(1, 2), ballot=(1, 0), seq=0, n=5):
    return (to, inst[0], inst[1], ballot[0], ballot[1], q, status, vote[0], vote[1], tid, seq, list(w or [0] * n), end)


def test_recover_takes_the_next_ordering_and_answers_its_own_prepare():
    m = R.RecoveryModel(5, 2, 16)
    m.peer_preaccept((1, 2), (0, 1), 0, True, 9, set(), [0])           # replica 0 pre-accepted (1, 2) in the default ballot
    assert m.replicas[0].largest_ballot == (0, 1)
    st, out = m.recover([(1, 2, 0), (3, 0, 0), (3, 1, 2)])             # :972-975: Ballot(largestBallot.ordering + 1, index)
    assert st == R.OK and out == [(R.RV_PREPARING, 1, 2, 1, 9), (R.RV_PREPARING, 2, 0, -1, -1), (R.RV_PREPARING, 1, 0, -1, -1)]
    assert m.replicas[0].largest_ballot == (2, 0) and m.replicas[2].largest_ballot == (1, 2)
    e = m.replicas[0].cmd_log[(1, 2)]
    assert (e.kind, e.ballot, e.vote_ballot) == (ES.PRE_ACCEPTED, (1, 0), (0, 1))       # :1711-1743 only `ballot` moves
    e = m.replicas[0].cmd_log[(3, 0)]
    assert (e.kind, e.ballot, e.vote_ballot) == (ES.NO_COMMAND, (2, 0), ES.NULL_BALLOT)   # :1654-1669
    assert isinstance(m.leader_states[0][(1, 2)], R.Preparing) and m.leader_states[0][(1, 2)].ballot == (1, 0)


def test_a_committed_instance_is_not_recovered_but_the_ballot_is_spent():
    m = R.RecoveryModel(5, 2, 16)
    m.peer_commit((1, 2), 9, set(), [0], 0, True)
    assert m.recover([(1, 2, 0)]) == (R.OK, [(R.RV_COMMITTED, 1, -1, -1, -1)])
    assert (1, 2) not in m.leader_states[0] and m.replicas[0].largest_ballot == (1, 0)


def test_the_two_tests_as_written_and_as_intended():
    for as_intended, want in [(False, R.RC_PRE_ACCEPT_NOOP), (True, R.RC_ACCEPT)]:
        m = R.RecoveryModel(5, 2, 16)
        m.recover([(1, 2, 0)])
        # the Accepted response is the only one of the highest voteBallot (:1806-1808); :1813 as written never matches
        st, rows, dec = m.prepare_oks([_ok(1, 2, (0, 1), 9), _ok(2, 3, (1, 4), 8, [0, 1, 0, 0, 0], seq=3)], as_intended)
        assert [r[0] for r in rows] == [R.RC_WAITING, want] and dec == [1]
        if as_intended:
            assert rows[1][1:5] == (2, 8, 8, 3) and rows[1][5] == frozenset({(1, 0)})
    for as_intended, want in [(False, R.RC_PRE_ACCEPT), (True, R.RC_ACCEPT)]:
        m = R.RecoveryModel(5, 2, 16)
        m.recover([(1, 2, 0)])
        # f = 2 matching PreAccepted triples of Ballot(0, leader) from others; :1836 as written reads the Prepare's ballot
        st, rows, dec = m.prepare_oks([_ok(3, 2, (0, 1), 9), _ok(4, 2, (0, 1), 9)], as_intended)
        assert rows[1][0] == want and rows[1][1] == 3 and rows[1][2] == 9
        assert (1, 2) not in m.leader_states[0]                       # a decision clears the state
    m = R.RecoveryModel(5, 2, 16)
    m.recover([(1, 2, 0)])                                            # differing dependencies: no candidate (:1845-1851)
    st, rows, dec = m.prepare_oks([_ok(3, 2, (0, 1), 9), _ok(4, 2, (0, 1), 9, [1, 0, 0, 0, 0])], True)
    assert rows[1][:3] == (R.RC_PRE_ACCEPT, 3, 9)


def test_matching_on_the_own_column_is_set_equality():
    m = R.RecoveryModel(5, 2, 16)                                      # instance (1, 2): a cover of 2 and of 3 are one set (:582)
    m.recover([(1, 2, 0)])
    st, rows, dec = m.prepare_oks([_ok(3, 2, (0, 1), 9, [0, 2, 0, 0, 0]), _ok(4, 2, (0, 1), 9, [0, 3, 0, 0, 0])], True)
    assert rows[1][0] == R.RC_ACCEPT and LS.encode_deps(5, (1, 2), rows[1][5]) == ([0, 2, 0, 0, 0], 0)


def test_stale_too_large_replaced_and_late_prepare_oks():
    m = R.RecoveryModel(5, 2, 16)
    m.recover([(1, 2, 0)])
    msgs = [_ok(1, ballot=(0, 0)), _ok(1, ballot=(1, 1)), _ok(1, 3, (2, 2), 7), _ok(1), _ok(0), _ok(2), _ok(3)]
    st, rows, dec = m.prepare_oks(msgs, True)
    assert st == R.EFATAL                                             # logger.checkLt :1792
    assert [r[0] for r in rows] == [R.RC_IGNORED, R.RC_FATAL, R.RC_WAITING, R.RC_WAITING, R.RC_WAITING, R.RC_PRE_ACCEPT_NOOP,
                                    R.RC_IGNORED] and dec == [5]       # the Accepted answer of replica 1 was replaced (:1796)


def test_a_nack_a_higher_prepare_and_a_commit_while_preparing():
    z = [0] * 5
    m = R.RecoveryModel(5, 2, 16)
    m.recover([(1, 2, 0)])
    nack = lambda b: (M.NACK, 0, 1, 2, b[0], b[1], 3, 0, z, 0)
    st, out, dec = m.replies([nack((1, 0)), nack((2, 3)), (M.PRE_ACCEPT_OK, 0, 1, 2, 1, 0, 3, 0, z, 0),
                              (M.SLOW_PATH_TIMER, 0, 1, 2, 0, 0, 0, 0, z, 0)])
    assert [o[0] for o in out] == [M.NACK_IGNORED, M.NACK_RECOVER, M.IGNORED, M.FATAL]      # :1609-1617; :1296-1315; :1024-1028
    assert m.replicas[0].largest_ballot == (2, 3)
    m.peer_prepare((1, 2), (3, 1), [0])                               # :1645-1648
    assert (1, 2) not in m.leader_states[0] and m.replicas[0].cmd_log[(1, 2)].ballot == (3, 1)    # the rule the device tests
    assert m.prepare_oks([_ok(1), _ok(2)])[1][1][0] == R.RC_IGNORED
    st, out = m.recover([(1, 2, 0)])                                  # and again, above everything seen
    assert out[0][:2] == (R.RV_PREPARING, 4)
    m.peer_commit((1, 2), 9, set(), [0], 0, True)                     # :831
    assert m.prepare_oks([_ok(1, ballot=(4, 0)), _ok(2, ballot=(4, 0))])[1][1][0] == R.RC_IGNORED


def test_lead_accept_dies_where_the_reference_dies_and_checks_its_arguments():
    z = [0] * 5
    m = R.RecoveryModel(5, 2, 16)
    assert m.lead_accept([(1, 2, 0, 3, 0, 1, 9, 1, [0, 0, 0, 2, 0], 0)]) == R.OK
    e, st = m.replicas[0].cmd_log[(1, 2)], m.leader_states[0][(1, 2)]
    assert (e.kind, e.ballot, e.vote_ballot, e.triple_id) == (ES.ACCEPTED, (3, 0), (3, 0), 9) and e.deps == {(3, 0), (3, 1)}
    assert isinstance(st, M.Accepting) and st.responses == {0} and st.triple == (1, e.deps)
    assert m.replicas[0].sets[0][1] == 3 and m.replicas[0].largest_ballot == (0, 0)          # :763; largestBallot untouched
    assert m.lead_accept([(1, 2, 0, 2, 0, 1, 9, 0, z, 0), (1, 3, 0, 2, 0, 1, 9, 0, z, 0)]) == R.EFATAL     # checkLe :749-757
    assert m.replicas[0].cmd_log[(1, 3)].kind == ES.ACCEPTED                                  # the rest is applied
    m.peer_commit((2, 0), 5, set(), [0], 0, True)
    assert m.lead_accept([(2, 0, 0, 9, 0, 1, 5, 0, z, 0)]) == R.EFATAL                        # :740-744
    for bad in [(5, 0, 0, 0, 0, 1, 1, 0, z, 0), (0, 16, 0, 0, 0, 1, 1, 0, z, 0), (0, 2, 5, 0, 0, 1, 1, 0, z, 0),
                (0, 2, 0, 0, 2, 1, 1, 0, z, 0), (0, 2, 0, 0, 0, 1, 1, 0, [0, -1, 0, 0, 0], 0), (0, 2, 0, 0, 0, 1, 1, 0, z, 3)]:
        assert m.lead_accept([(0, 3, 0, 0, 0, 1, 1, 0, z, 0), bad]) == R.EINVAL
        assert (0, 3) not in m.replicas[0].cmd_log


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_the_header_the_binding_and_the_model_name_the_same_codes_and_the_flag():
    h = open(os.path.join(ROOT, "include", "fpx.h")).read()
    from frankenpaxos_amd import _lib, epaxos as E

    assert "#define FPX_EPX_F_RECOVERY 2u" in h
    assert E.FPX_EPX_F_RECOVERY == _lib.FPX_EPX_F_RECOVERY == R.F_RECOVERY == 2 and R.F_LEADER_STATE == E.FPX_EPX_F_LEADER_STATE
    assert "enum { FPX_EPX_RV_PREPARING = 0, FPX_EPX_RV_COMMITTED = 1, FPX_EPX_RV_FATAL = 2 };" in h
    for name, value in [("PREPARING", 0), ("COMMITTED", 1), ("FATAL", 2)]:
        assert getattr(E, "RV_" + name) == getattr(R, "RV_" + name) == getattr(_lib, "FPX_EPX_RV_" + name) == value
    for name, value in [("IGNORED", 0), ("WAITING", 1), ("ACCEPT", 2), ("PRE_ACCEPT", 3), ("PRE_ACCEPT_NOOP", 4), ("FATAL", 5)]:
        assert re.search(r"FPX_EPX_RC_%s = %d\b" % (name, value), h), name
        assert getattr(E, "RC_" + name) == getattr(R, "RC_" + name) == getattr(_lib, "FPX_EPX_RC_" + name) == value
    assert (R.NOT_SEEN, R.PRE_ACCEPTED, R.ACCEPTED) == (ES.NONE, ES.PRE_ACCEPTED, ES.ACCEPTED)
    kernels = open(os.path.join(ROOT, "frankenpaxos_amd", "csrc", "fpx_epx_leader.hpp")).read()
    assert "LS_PREPARING = 3" in kernels


def test_the_library_exports_the_new_symbols():
    from frankenpaxos_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported and name in _lib.SIGNATURES, name
    dg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpx_depgraph.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(fpx_depgraph_[a-z0-9_]+)\s*\(", dg))) == 9


def test_refusals_that_come_before_a_device_is_touched():
    from frankenpaxos_amd import _lib
    from frankenpaxos_amd.epaxos import FpxEpxConfig

    L = _lib.lib()
    a = (C.c_int32 * 8)()
    p = C.cast(a, C.c_void_p)
    assert L.fpx_epx_recover(None, 1, p, p, p, None, None, None, None, None) == R.EINVAL
    assert L.fpx_epx_recover(None, 0, None, None, None, None, None, None, None, None) == R.EINVAL
    assert L.fpx_epx_recovery_replies(None, 1, *[p] * 13, 0, *[None] * 9) == R.EINVAL
    assert L.fpx_epx_recovery_replies_dev(None, 1, *[p] * 13, 1, *[None] * 9) == R.EINVAL
    assert L.fpx_epx_lead_accept(None, 1, *[p] * 10) == R.EINVAL
    assert L.fpx_epx_read_recovery_state(None, 0, 0, 0, p) == R.EINVAL
    # the flag alone, without FPX_EPX_F_LEADER_STATE, is refused whether or not there is a device
    h = C.c_void_p()
    cfg = FpxEpxConfig(5, 4, 0, R.F_RECOVERY, 64)
    assert L.fpx_epx_create(C.byref(cfg), C.byref(h)) == R.EINVAL and not h.value
    cfg = FpxEpxConfig(5, 4, 0, R.F_RECOVERY | R.F_LEADER_STATE, 0)           # leader state needs a command log
    assert L.fpx_epx_create(C.byref(cfg), C.byref(h)) == R.EINVAL and not h.value


def test_the_cxx_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "m.cpp"
    src.write_text('#include "frankenpaxos_amd/host/fpx.hpp"\n'
                   'using namespace frankenpaxos::epaxos;\n'
                   'int main() { using E = PreAcceptEngine; auto p = &E::recover; auto q = &E::leadAccept;\n'
                   '  std::vector<RecoveryReply> (E::*r)(const std::vector<PrepareOkInbound>&, bool, std::vector<int>*) = '
                   '&E::handlePrepareOks;\n'
                   '  (void)p; (void)q; (void)r;\n'
                   '  return (int)RecoveryOutcome::AcceptPhase - 2 + (int)RecoverOutcome::Committed - 1; }\n')
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", ROOT, "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_natives_and_the_shim_take_the_same_arguments():
    scala = open(os.path.join(ROOT, "frankenpaxos_amd", "jni", "Native.scala")).read()
    shim = open(os.path.join(ROOT, "frankenpaxos_amd", "jni", "fpx_jni.c")).read()
    for name, library_call in [("epxCreateWithRecovery", "fpx_epx_create"), ("epxRecover", "fpx_epx_recover"),
                               ("epxRecoveryReplies", "fpx_epx_recovery_replies"), ("epxLeadAccept", "fpx_epx_lead_accept")]:
        d = re.search(r"@native def %s\(([^)]*)\)" % name, scala, flags=re.S)
        c = re.search(r"Java_frankenpaxos_gpu_Native_%s\(\s*JNIEnv\* env, jclass cls,?([^)]*)\)\s*\{(.*?)\n\}" % name, shim, flags=re.S)
        assert d and c, name
        names = lambda text: [p.split(":")[0].split()[-1].strip("* ") for p in text.split(",") if p.strip()]
        assert names(d.group(1)) == ["handle" if x == "h" else x for x in names(c.group(1))], name
        assert library_call + "(" in c.group(2), name
