"""The leader half of EPaxos on the CPU: the reference-shaped model (tests/epaxos_leader_model.py: dict leaderStates, sets of
instances, eager drops) against the stand-alone array-shaped C++ restatement (tests/epaxos_leader_host_main.cpp, built with
-fsanitize=address,undefined and run as its own program) on the generator's streams, plus hand-worked cases with their
reference lines.  No GPU; nothing of the library is loaded under a sanitizer."""
import collections
import os
import subprocess

import pytest

from tests import epaxos_leader_model as M
from tests import epaxos_leader_streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("epx_leader") / "epaxos_leader_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                            exe, os.path.join(ROOT, "tests", "epaxos_leader_host_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def _enc(b):
    return -1 if b == (-1, -1) else b[0] * 8 + b[1]


def host_play(exe, n, num_keys, num_instances, ops):
    """the stream through the C++ program: (results per op in run_op's form, state in model_state's form).  Acceptor-side
    ops reach the program as the state a LeaderModel shows after them (the acceptor half is not what it restates)."""
    side = M.LeaderModel(n, num_keys, num_instances)
    lines = ["CFG %d %d %d" % (n, num_keys, num_instances)]
    for op in ops:
        if op[0] == "lead":
            lines.append("LEAD %d" % len(op[1]))
            lines += [" ".join(str(int(v)) for v in msg) for msg in op[1]]
            side.lead(op[1])
        elif op[0] == "replies":
            lines.append("REPLIES %d" % len(op[1]))
            for (kind, to, L, x, bo, br, q, seq, w, end) in op[1]:
                lines.append(" ".join(str(int(v)) for v in [kind, to, L, x, bo, br, q, seq, end] + list(w)))
            side.replies(op[1])
        else:
            S.run_op(side, op)
            inst = op[1]
            for r in range(n):                           # (an Accept also moves its proposer, and a commit every replica)
                e = side.replicas[r].cmd_log.get(inst)
                if e is not None:
                    w, end = ([0] * n, 0) if e.deps is None else S.encode_deps(n, inst, e.deps)
                    lines.append("ENTRY %d %d %d %d %d %d %d %d %d %s" % (r, inst[0], inst[1], e.kind, _enc(e.ballot),
                                                                           _enc(e.vote_ballot), e.triple_id,
                                                                           0 if e.deps is None else 1, end, " ".join(map(str, w))))
                for k in range(num_keys):
                    lines.append("SETINDEX %d %d %s %s" % (r, k, " ".join(map(str, side.replicas[r].gets[k])),
                                                           " ".join(map(str, side.replicas[r].sets[k]))))
                lines.append("LARGEST %d %d" % (r, _enc(side.replicas[r].largest_ballot)))
    cells, keys = S.touched(ops)
    for (r, inst) in cells:
        lines.append("READ %d %d %d" % (r, inst[0], inst[1]))
    for r in range(n):
        lines.append("LARGESTQ %d" % r)
        for k in keys:
            lines.append("INDEX %d %d" % (r, k))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    out = iter(run.stdout.splitlines())
    results = []
    for op in ops:
        if op[0] == "lead":
            st = int(next(out).split()[1])
            if st == M.EINVAL:
                results.append((st, None))
                continue
            rows = []
            for _ in op[1]:
                v = [int(t) for t in next(out).split()]
                rows.append((v[:n], v[n]))
            results.append((st, rows))
        elif op[0] == "replies":
            _, st, nd = next(out).split()
            if int(st) == M.EINVAL:
                results.append((int(st), None, None))
                continue
            rows = []
            for _ in op[1]:
                v = [int(t) for t in next(out).split()]
                rows.append((v[0], v[1], v[4:4 + n], v[2], v[3]))
            dec = [int(t) for t in next(out).split()]
            assert len(dec) == int(nd)
            results.append((int(st), rows, dec))
        else:
            results.append(None)
    state, largest, index = {}, [], {}
    for (r, inst) in cells:
        left, right = next(out)[2:].split("|")
        c = [int(t) for t in left.split()]
        kind, ballot, vote, tid, dend = c[:5]
        deps = None if (kind == 0 or c[5] == -1) else (c[5:5 + n], dend)
        parts = right.split("/")
        hd = [int(t) for t in parts[0].split()]
        rows = {}
        for p in parts[1:]:
            v = [int(t) for t in p.split()]
            rows[v[0]] = tuple(v[1:])
        phase, lb, avoid, ltid, key, is_set, mask = hd
        if phase == 0:
            ls = (0,)
        elif phase == 1:
            ls = (1, lb, avoid, ltid, key, is_set, rows)
        else:
            ls = (2, lb, ltid, key, is_set, sorted(rows), rows[r])
        state[(r, inst)] = ((kind, ballot, vote, tid) if kind else (0, -1, -1, -1), deps, ls)
    for r in range(n):
        largest.append(int(next(out).split()[1]))
        for k in keys:
            v = [int(t) for t in next(out).split()[1:]]
            index[(r, k)] = (v[:n], v[n:])
    return results, (state, largest, index)


def histogram(ops, results):
    h = collections.Counter()
    for op, res in zip(ops, results):
        if op[0] == "lead":
            h["lead_status_%d" % res[0]] += 1
        elif op[0] == "replies":
            h["replies_status_%d" % res[0]] += 1
            for row in res[1]:
                h[row[0]] += 1
    return h


@pytest.mark.parametrize("n", [3, 5, 7])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_two_models_agree_on_the_generators_streams(host_exe, n, seed):
    ops = S.make_stream(seed, n)
    model = M.LeaderModel(n, 4, 64)
    want = S.run_model(model, ops)
    got, got_state = host_play(host_exe, n, 4, 64, ops)
    assert got == want
    assert got_state == S.model_state(model, ops)


@pytest.mark.parametrize("n", [3, 5, 7])
def test_the_streams_reach_every_outcome_and_both_fatal_sources(n):
    """the parity condition: a generator change that stops reaching a branch fails here"""
    h = collections.Counter()
    for seed in (1, 2, 3):
        ops = S.make_stream(seed, n)
        h += histogram(ops, S.run_model(M.LeaderModel(n, 4, 64), ops))
    want = set(range(9)) - ({M.START_SLOW_PATH_TIMER} if n == 3 else set())   # n = 3: slow == fast, no timer ever
    assert want <= {k for k in h if isinstance(k, int)}, h
    assert h["lead_status_%d" % M.EFATAL] > 0 and h["replies_status_%d" % M.EFATAL] > 0, h
    assert h["lead_status_0"] > 0 and h["replies_status_0"] + h["replies_status_%d" % M.EFATAL] > 0


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------
def _led(n, avoid=0, key=0, number=0):
    m = M.LeaderModel(n, 2, 16)
    st, deps = m.lead([(0, number, 0, 0, key, 1, 77, avoid)])
    assert st == M.OK and deps == [frozenset()]
    return m


def _ok(q, w, end=0, seq=0, n=5, to=0, number=0, ballot=(0, 0)):
    return (M.PRE_ACCEPT_OK, to, 0, number, ballot[0], ballot[1], q, seq, list(w), end)


def _outcomes(m, msgs):
    st, out, dec = m.replies(msgs)
    return st, [o[0] for o in out], dec


def test_n3_the_first_peer_answer_decides_fast():
    # Config.scala:8-9: n = 3 has slowQuorumSize = fastQuorumSize = 2; handlePreAcceptOk :1353-1356 never starts the timer
    m = _led(3)
    st, out, dec = m.replies([_ok(1, [0, 0, 0], n=3), _ok(2, [0, 0, 0], n=3)])
    assert st == M.OK and [o[0] for o in out] == [M.FAST_COMMIT, M.IGNORED] and dec == [0]
    assert m.replicas[0].cmd_log[(0, 0)].kind == 4 and (0, 0) not in m.leader_states[0]


def test_n5_timer_at_the_second_answer_fast_iff_all_three_agree():
    z = [0] * 5
    m = _led(5)                                                     # :1345, :1353-1364, :1376-1410
    assert _outcomes(m, [_ok(1, z), _ok(2, z), _ok(3, z)]) == (M.OK, [M.WAITING, M.START_SLOW_PATH_TIMER, M.FAST_COMMIT], [2])
    m = _led(5)                                                     # :1411-1415 -> preAcceptingSlowPath :796-813
    st, out, dec = m.replies([_ok(1, z), _ok(2, [0, 3, 0, 0, 0]), _ok(3, [0, 0, 2, 0, 0])])
    assert [o[0] for o in out] == [M.WAITING, M.START_SLOW_PATH_TIMER, M.ACCEPT]
    assert out[2][2] == frozenset({(1, 0), (1, 1), (1, 2), (2, 0), (2, 1)})
    e = m.replicas[0].cmd_log[(0, 0)]
    assert (e.kind, e.ballot, e.vote_ballot, e.deps) == (3, (0, 0), (0, 0), out[2][2])      # transitionToAcceptPhase :760-762


def test_n7_timer_at_the_third_waiting_at_the_fourth_decision_at_the_fifth():
    z = [0] * 7
    m = _led(7)
    got = _outcomes(m, [_ok(q, z, n=7) for q in (1, 2, 3, 4, 5)])
    assert got == (M.OK, [M.WAITING, M.WAITING, M.START_SLOW_PATH_TIMER, M.WAITING, M.FAST_COMMIT], [4])


def test_a_later_answer_of_one_sender_replaces_the_earlier_one():
    z = [0] * 5
    m = _led(5)                                                     # responses(replicaIndex) = preAcceptOk :1340
    assert _outcomes(m, [_ok(1, [0, 4, 0, 0, 0]), _ok(1, z), _ok(2, z), _ok(3, z)])[1] == [M.WAITING, M.WAITING,
                                                                                       M.START_SLOW_PATH_TIMER, M.FAST_COMMIT]
    m = _led(5)
    assert _outcomes(m, [_ok(1, z), _ok(1, [0, 4, 0, 0, 0]), _ok(2, z), _ok(3, z)])[1][-1] == M.ACCEPT


def test_answers_that_differ_only_in_sequence_number_do_not_agree():
    z = [0] * 5
    m = _led(5)                                                     # popularItems compares (sequenceNumber, dependencies) :1382-1396
    st, out, dec = m.replies([_ok(1, z, seq=2), _ok(2, z), _ok(3, z)])
    assert out[2][0] == M.ACCEPT and out[2][1] == 2 and out[2][2] == frozenset()   # the max of the sequence numbers :803


def test_own_column_covers_x_and_x_plus_1_are_the_same_set():
    # instance (0, 4): {0..3} and {0..4} \ {(0, 4)} are one set (dependencies.subtractOne :582)
    m = M.LeaderModel(5, 2, 16)
    m.lead([(0, 4, 0, 0, 0, 1, 9, 0)])
    st, out, dec = m.replies([_ok(1, [4, 0, 0, 0, 0], number=4), _ok(2, [5, 0, 0, 0, 0], number=4), _ok(3, [4, 0, 0, 0, 0], number=4)])
    assert out[2][0] == M.FAST_COMMIT and S.encode_deps(5, (0, 4), out[2][2]) == ([4, 0, 0, 0, 0], 0)


def test_the_leaders_own_index_replaces_its_own_response():
    z = [0] * 5
    m = _led(5)
    st, out, dec = m.replies([_ok(0, [0, 0, 0, 0, 6]), _ok(1, z), _ok(2, z), _ok(3, [0, 1, 0, 0, 0])])
    assert [o[0] for o in out] == [M.WAITING, M.WAITING, M.START_SLOW_PATH_TIMER, M.ACCEPT]
    assert (4, 5) in out[3][2] and (1, 0) in out[3][2]                # the union takes ALL responses, the own one included :805-807


def test_avoid_fast_path_decides_at_the_slow_quorum():
    z = [0] * 5
    m = _led(5, avoid=1)                                            # :1369-1372
    assert _outcomes(m, [_ok(1, z), _ok(2, z), _ok(3, z)]) == (M.OK, [M.WAITING, M.ACCEPT, M.IGNORED], [1])


def test_timer_before_and_after_the_decision():
    z = [0] * 5
    tm = (M.SLOW_PATH_TIMER, 0, 0, 0, 0, 0, 0, 0, z, 0)
    m = _led(5)                                                     # :1023-1031; after it the state is Accepting: logger.fatal
    st, out, dec = m.replies([_ok(1, z), _ok(2, z), tm, tm, (M.ACCEPT_OK, 0, 0, 0, 0, 0, 1, 0, z, 0), (M.ACCEPT_OK, 0, 0, 0, 0, 0, 2, 0, z, 0)])
    assert st == M.EFATAL
    assert [o[0] for o in out] == [M.WAITING, M.START_SLOW_PATH_TIMER, M.ACCEPT, M.FATAL, M.WAITING, M.SLOW_COMMIT] and dec == [2, 5]


def test_accept_ok_before_and_after_the_answer_that_opens_the_accept_phase():
    z = [0] * 5
    aok = lambda q: (M.ACCEPT_OK, 0, 0, 0, 0, 0, q, 0, z, 0)
    m = _led(5, avoid=1)                                            # :1525-1529 pre-accepting: ignored; :1554-1563
    assert _outcomes(m, [aok(1), _ok(1, z), aok(2), _ok(2, z), aok(1), aok(2), aok(3)])[1] == [
        M.IGNORED, M.WAITING, M.IGNORED, M.ACCEPT, M.WAITING, M.SLOW_COMMIT, M.IGNORED]


def test_stale_and_too_large_ballots():
    z = [0] * 5
    m = M.LeaderModel(5, 2, 16)
    m.lead([(0, 0, 2, 3, 0, 1, 5, 0)])                              # replica 2 leads (0, 0) in ballot (3, 2)
    st, out, dec = m.replies([_ok(1, z, to=2, ballot=(2, 2)), _ok(1, z, to=2, ballot=(3, 3)), _ok(1, z, to=2, ballot=(3, 2))])
    assert st == M.EFATAL and [o[0] for o in out] == [M.IGNORED, M.FATAL, M.WAITING]     # :1325-1335


def test_nacks_of_all_three_kinds_raise_largest_ballot():
    z = [0] * 5
    nack = lambda x, b: (M.NACK, 0, 0, x, b[0], b[1], 1, 0, z, 0)
    m = _led(5)                                                     # :1578 always; :1581-1587 not led; :1589-1597; :1623-1629
    assert _outcomes(m, [nack(9, (4, 1)), nack(0, (0, 0)), nack(0, (2, 3))])[1] == [M.NACK_IGNORED, M.NACK_IGNORED, M.NACK_RECOVER]
    assert m.replicas[0].largest_ballot == (4, 1)


@pytest.mark.parametrize("how", ["preaccept", "accept", "prepare", "commit"])
def test_an_instance_taken_away_makes_the_replies_outcome_0(how):
    z = [0] * 5
    m = _led(5)
    if how == "preaccept":
        m.peer_preaccept((0, 0), (1, 3), 0, True, 5, set(), [0])    # :1239-1242
    elif how == "accept":
        m.peer_accept((0, 0), (1, 3), 5, [0], 0, True)              # :1480-1483
    elif how == "prepare":
        m.peer_prepare((0, 0), (1, 3), [0])                         # :1645-1648
    else:
        m.peer_commit((0, 0), 77, set(), [0], 0, True)              # :831
    assert (0, 0) not in m.leader_states[0]
    e = m.replicas[0].cmd_log[(0, 0)]
    assert e.kind == 4 or e.ballot != (0, 0) or e.vote_ballot != (0, 0)      # the rule the device tests instead (include/fpx.h)
    assert _outcomes(m, [_ok(1, z), _ok(2, z), _ok(3, z)]) == (M.OK, [M.IGNORED] * 3, [])


def test_lead_dies_where_the_reference_dies_and_checks_its_arguments():
    m = _led(5)
    m.peer_commit((0, 0), 77, set(), [0], 0, True)
    assert m.lead([(0, 0, 0, 1, 0, 1, 78, 0), (0, 1, 0, 0, 0, 1, 79, 0)]) == (M.EFATAL, [None, frozenset({(0, 0)})])   # :663-667
    m.peer_prepare((1, 0), (2, 3), [0])
    assert m.lead([(1, 0, 0, 1, 0, 1, 80, 0)])[0] == M.EFATAL       # checkLe(noCommand.ballot, ballot) :672-673
    for bad in [(5, 0, 0, 0, 0, 1, 1, 0), (0, 16, 0, 0, 0, 1, 1, 0), (0, 2, 5, 0, 0, 1, 1, 0), (0, 2, 0, 0, 2, 1, 1, 0)]:
        assert m.lead([(0, 3, 0, 0, 0, 1, 1, 0), bad]) == (M.EINVAL, None)
        assert (0, 3) not in m.replicas[0].cmd_log


def test_the_cxx_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "m.cpp"
    src.write_text('#include "frankenpaxos_amd/host/fpx.hpp"\n'
                   'int main() { using E = frankenpaxos::epaxos::PreAcceptEngine; auto p = &E::lead; auto q = &E::handleReplies;\n'
                   '  (void)p; (void)q; return (int)frankenpaxos::epaxos::LeaderOutcome::CommitFastPath - 3; }\n')
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", ROOT, "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_header_the_binding_and_the_models_name_the_same_codes():
    h = open(os.path.join(ROOT, "include", "fpx.h")).read()
    from frankenpaxos_amd import epaxos as E

    for name, value in [("IGNORED", 0), ("WAITING", 1), ("START_SLOW_PATH_TIMER", 2), ("FAST_COMMIT", 3), ("ACCEPT", 4),
                        ("SLOW_COMMIT", 5), ("NACK_RECOVER", 6), ("NACK_IGNORED", 7), ("FATAL", 8)]:
        assert "FPX_EPX_%s = %d," % (name, value) in h or "FPX_EPX_%s = %d " % (name, value) in h, name
        assert getattr(E, name) == getattr(M, name) == value
    assert "#define FPX_EPX_F_LEADER_STATE 1u" in h and E.FPX_EPX_F_LEADER_STATE == 1
