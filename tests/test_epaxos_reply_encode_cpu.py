"""A replica tick's replies as wire bytes, without a GPU: the host batch encoder (fpx_wire_epx_encode_replica_replies, the
emitter of csrc/fpx_wire_epx_emit.hpp that the device encoder compiles too) against three references -- the yardstick
fpx_wire_epaxos_encode_replica_inbound called once per message, the writer written a second time in Python
(tests/epaxos_reply_cases.py), and a round trip through fpx_wire_epaxos_decode_replica_inbound -- and a stand-alone program
that runs the emitter header over the same kind of cases under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from tests import epaxos_reply_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPX_EINVAL, FPX_ECAPACITY = 1, 5


@pytest.fixture(scope="module")
def wire():
    import frankenpaxos_amd
    from frankenpaxos_amd import wire as w

    if not os.path.exists(frankenpaxos_amd._lib.SO_PATH):
        frankenpaxos_amd.build()
    return w


def assert_encodes(wire, n, records):
    want, kinds, offsets, totals = RC.expected(n, records)
    got = wire.epx_encode_replica_replies(n, **RC.arrays(n, records))
    assert got["status_code"] == 0
    assert np.array_equal(got["totals"], totals) and np.array_equal(got["reply_kind"], kinds)
    assert np.array_equal(got["out_offsets"], offsets)
    for i, (g, w) in enumerate(zip(got["replies"], want)):
        assert g == w, (i, records[i])
    return got


@pytest.mark.parametrize("n", [3, 5, 7])
def test_batch_encoder_equals_the_python_writer_and_the_yardstick(wire, n):
    records = RC.case_records(n)
    got = assert_encodes(wire, n, records)
    kinds = set()
    for i, r in enumerate(records):
        assert got["replies"][i] == RC.yardstick_reply(wire, n, r), (i, r)
        kinds.add((r[5], int(got["reply_kind"][i])))
    # every outcome is there, and both fates of the three that can be deferred
    assert {o for o, _ in kinds} == set(range(9))
    assert {(1, 1), (1, 2), (2, 1), (2, 2), (6, 1), (6, 2), (8, 2), (0, 0), (5, 0)} <= kinds


@pytest.mark.parametrize("n", [3, 5, 7])
def test_replies_decode_back_to_their_fields(wire, n):
    records = [r for r in RC.case_records(n) if RC.plan(n, r) == RC.ENCODED]
    got = assert_encodes(wire, n, records)
    d = wire.epaxos_decode_replica_inbound(got["replies"], max_replicas=n)
    assert d["status_code"] == 0
    for i, r in enumerate(records):
        to, leader, number, bo, br, outcome, ob, status, deps, end = r
        kind = {1: wire.EPX_PRE_ACCEPT_OK, 2: wire.EPX_PRE_ACCEPT_OK, 3: wire.EPX_ACCEPT_OK, 4: wire.EPX_ACCEPT_OK,
                6: wire.EPX_PREPARE_OK, 7: wire.EPX_NACK}[outcome]
        assert d["kind"][i] == kind and (d["instance_leader"][i], d["instance_number"][i]) == (leader, number), (i, r)
        ballot = (ob >> 3, ob & 7) if outcome == 7 else (bo, br)
        assert (d["ballot_ordering"][i], d["ballot_replica"][i]) == ballot, (i, r)
        if outcome != 7:
            assert d["replica_index"][i] == to
        lo, hi = int(d["values_off"][i]), int(d["values_off"][i + 1])
        if outcome in (1, 2):
            assert d["sequence_number"][i] == 0 and d["deps_num_replicas"][i] == n
            assert tuple(d["deps_watermark"][i][:n]) == deps
            assert list(d["values_id"][lo:hi]) == RC.own_ids(r) and set(d["values_leader"][lo:hi]) <= {leader}
        else:
            assert d["deps_num_replicas"][i] == -1 and lo == hi
        if outcome == 6:
            assert d["status"][i] == 0 and d["is_noop"][i] == -1
            assert (d["vote_ballot_ordering"][i], d["vote_ballot_replica"][i]) == ((-1, -1) if ob < 0 else (ob >> 3, ob & 7))


def test_the_closed_form_length_is_the_emitted_length_on_every_run_of_ids(wire):
    """id runs of every count up to the cap that begin on either side of a varint boundary: the offsets the encoder reports
    come from the closed-form length, the bytes from the writer's loop"""
    n = 3
    records = [RC.id_run(n, 1, count, first) for edge in (128, 16384, 1 << 21, 1 << 28)
               for count in (1, 2, 31, 63, 64) for first in (edge - count, edge - count + 1, edge - 1, edge, edge + 1)]
    assert_encodes(wire, n, records)


def test_capacity_sizing_and_the_empty_batch(wire):
    n = 5
    records = RC.case_records(n)
    a = RC.arrays(n, records)
    want, kinds, offsets, totals = RC.expected(n, records)
    need = int(totals[1])
    exact = wire.epx_encode_replica_replies(n, cap=need, **a)
    assert exact["status_code"] == 0 and exact["out"].tobytes() == b"".join(want)
    for cap in (need - 1, 0):
        short = wire.epx_encode_replica_replies(n, cap=cap, **a)
        assert short["status_code"] == FPX_ECAPACITY and np.array_equal(short["totals"], totals)
        assert short["out_offsets"][0] == 0 and (short["out_offsets"][1:] == -9).all()      # nothing beyond [0]
        assert (short["reply_kind"] == 9).all() and (short["out"] == 0xEE).all()
    empty = wire.epx_encode_replica_replies(n, **RC.arrays(n, []))
    assert empty["status_code"] == 0 and list(empty["totals"]) == [0, 0, 0, -1] and list(empty["out_offsets"]) == [0]


def test_an_unknown_outcome_is_refused_with_its_index(wire):
    n = 3
    records = RC.case_records(n)[:40]
    for at, outcome in ((17, 9), (3, -1)):
        bad = list(records)
        bad[at] = bad[at][:5] + (outcome,) + bad[at][6:]
        bad[30] = bad[30][:5] + (12,) + bad[30][6:]
        got = wire.epx_encode_replica_replies(n, cap=1 << 16, **RC.arrays(n, bad))
        assert got["status_code"] == FPX_EINVAL and list(got["totals"]) == [0, 0, 0, at]
        assert got["out_offsets"][0] == 0 and (got["out_offsets"][1:] == -9).all() and (got["reply_kind"] == 9).all()
        assert (got["out"] == 0xEE).all()


def test_reply_max_is_the_longest_reply_there_is(wire):
    n = 7
    want, _, _, _ = RC.expected(n, RC.case_records(n))
    assert max(len(b) for b in want) == wire.EPX_REPLY_MAX == len(RC.py_reply(n, RC.worst_case(n))[1])
    hdr = open(os.path.join(ROOT, "include", "fpx_wire.h")).read()
    assert "#define FPX_WIRE_EPX_REPLY_MAX %d\n" % wire.EPX_REPLY_MAX in hdr


def test_the_emitter_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "epx_reply_emit")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                            exe, os.path.join(ROOT, "tests", "epx_reply_emit_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "all ok" and not [ln for ln in lines if ln.startswith("FAIL")]
    counts = dict(kv.split("=") for ln in lines if ln.startswith("ok replies") for kv in ln.split()[2:])
    # every reply was reached, and both fates of a record
    assert all(int(counts[k]) > 100 for k in ("pre_accept_ok", "accept_ok", "nack", "prepare_ok", "deferred", "none"))
    assert sum(ln.startswith("ok layout") for ln in lines) == 8 * 3
