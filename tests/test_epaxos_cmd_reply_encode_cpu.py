"""The replies of a replica tick that carry a stored command -- the Commit sent back, the PrepareOk of a PreAccepted /
Accepted instance -- from the host batch encoder with a command store (fpx_wire_epx_encode_replica_replies_cmds,
csrc/fpx_wire_epx_emit.hpp): held against the yardstick fpx_wire_epaxos_encode_replica_inbound message by message, against a
writer written a second time in Python, round trip through the decoder, every fallback to deferred, the null store, the sizing
call, the length bound -- and the emitter header as a program of its own under the sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from tests import epaxos_cmd_reply_cases as CC
from tests import epaxos_reply_cases as RC
from tests.epaxos_wire_cases import varint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = 1, 5
MAX_TRIPLES = 64


@pytest.fixture(scope="module")
def wire():
    import __graft_entry__ as ge
    import frankenpaxos_amd

    if not os.path.exists(frankenpaxos_amd._lib.SO_PATH):
        ge.build()
    from frankenpaxos_amd import wire as w

    return w


@pytest.fixture(scope="module")
def store():
    return CC.case_store(MAX_TRIPLES)


def encode(wire, n, records, st, **kw):
    a = CC.arrays(n, records)
    tr = a.pop("out_triple")
    return wire.epx_encode_replica_replies_cmds(n, tr, None if st is None else st.arrays(), **kw, **a)


@pytest.mark.parametrize("n", [3, 5, 7])
def test_case_set_equals_the_yardstick_and_the_python_writer(wire, store, n):
    st, by_len, noop = store
    records = CC.case_records(n, by_len, noop, MAX_TRIPLES)
    got = encode(wire, n, records, st)
    replies, kinds, offsets, totals = CC.expected(n, records, st)
    assert got["status_code"] == 0
    assert np.array_equal(got["reply_kind"], kinds) and np.array_equal(got["out_offsets"], offsets)
    assert np.array_equal(got["totals"], totals)
    for i, r in enumerate(records):
        assert got["replies"][i] == replies[i], (i, r[:8])
        want = CC.yardstick_reply(wire, n, r, st)
        assert want is None or got["replies"][i] == want, (i, r[:8])     # (None: a command of no bytes, see there)
    # the census of the case set: every length, the Noop, the id counts, nullBallot, and every way back to deferred
    enc = [r for r, k in zip(records, kinds) if k == CC.ENCODED and (r[5] == 8 or r[7] in (2, 3))]
    assert {len(st.get(r[10])) for r in enc} >= set(CC.CMD_LENS) and any(st.get(r[10]) == CC.NOOP for r in enc)
    assert {(r[5], r[7]) for r in enc} == {(8, -1), (6, 2), (6, 3)}
    assert {len(RC.own_ids(r)) for r in enc} >= {0, 1, 64} and any(r[6] < 0 and r[5] == 6 for r in enc)
    deferred = [r for r, k in zip(records, kinds) if k == CC.DEFERRED]
    assert any(r[10] < 0 for r in deferred) and any(r[10] >= MAX_TRIPLES for r in deferred)
    assert any(0 <= r[10] < MAX_TRIPLES and st.get(r[10]) is None for r in deferred)
    assert any(r[8][0] < 0 for r in deferred) and any(len(RC.own_ids(r)) == 65 for r in deferred)
    assert any(r[5] == 6 and r[7] == 1 for r in deferred)


@pytest.mark.parametrize("n", [3, 5, 7])
def test_round_trip_and_the_command_span_equals_the_stored_bytes(wire, store, n):
    st, by_len, noop = store
    records = [r for r in CC.case_records(n, by_len, noop, MAX_TRIPLES) if CC.plan(n, r, st) == CC.ENCODED]
    records = [r for r in records if len(st.get(r[10]) or b"") >= 2]   # (the decoder wants a CommandOrNoop with its oneof)
    got = encode(wire, n, records, st)
    assert got["status_code"] == 0
    dec = wire.epaxos_decode_replica_inbound(got["replies"], max_replicas=7)
    assert dec["status_code"] == 0
    buf = dec["buf"]                       # the replies back to back: cmd_off indexes it
    assert buf.tobytes() == got["out"].tobytes()
    for i, r in enumerate(records):
        to, leader, number, bo, br, outcome, ob, status, deps, end, triple = r
        assert (dec["instance_leader"][i], dec["instance_number"][i]) == (leader, number)
        assert list(dec["deps_watermark"][i][:n]) == list(deps) and dec["deps_num_replicas"][i] == n
        lo, hi = int(dec["values_off"][i]), int(dec["values_off"][i + 1])
        assert list(dec["values_id"][lo:hi]) == RC.own_ids(r) and set(dec["values_leader"][lo:hi]) <= {leader}
        if outcome == 8 or status in (2, 3):
            want = st.get(triple)
            at = int(dec["cmd_off"][i])
            assert got["out_offsets"][i] < at <= got["out_offsets"][i + 1] - len(want)
            assert dec["cmd_len"][i] == len(want) and buf[at:at + len(want)].tobytes() == want
            assert dec["sequence_number"][i] == 0
            if outcome == 6:
                assert dec["kind"][i] == wire.EPX_PREPARE_OK and dec["status"][i] == status - 1
                assert (dec["ballot_ordering"][i], dec["ballot_replica"][i], dec["replica_index"][i]) == (bo, br, to)
                vote = (-1, -1) if ob < 0 else (ob >> 3, ob & 7)
                assert (dec["vote_ballot_ordering"][i], dec["vote_ballot_replica"][i]) == vote
            else:
                assert dec["kind"][i] == wire.EPX_COMMIT


@pytest.mark.parametrize("n", [3, 5, 7])
def test_a_null_store_is_the_existing_function(wire, store, n):
    st, by_len, noop = store
    records = CC.burst(n, 400, by_len, noop, MAX_TRIPLES, shift=n)
    a = CC.arrays(n, records)
    a.pop("out_triple")
    want = wire.epx_encode_replica_replies(n, **a)
    got = encode(wire, n, records, None)
    assert got["status_code"] == want["status_code"] == 0
    assert got["out"].tobytes() == want["out"].tobytes() and got["replies"] == want["replies"]
    for k in ("out_offsets", "reply_kind", "totals"):
        assert np.array_equal(got[k], want[k])
    # and with the store every record that carries no command keeps its bytes and its kind
    with_store = encode(wire, n, records, st)
    for i, r in enumerate(records):
        if not (r[5] == 8 or (r[5] == 6 and r[7] in (2, 3))):
            assert with_store["replies"][i] == want["replies"][i] and with_store["reply_kind"][i] == want["reply_kind"][i]


def test_mixed_bursts_equal_the_python_writer(wire, store):
    st, by_len, noop = store
    for n, m, only in ((3, 257, False), (5, 1025, False), (7, 130, True)):
        records = CC.burst(n, m, by_len, noop, MAX_TRIPLES, shift=m, only_cmds=only, big=m < 300)
        got = encode(wire, n, records, st)
        replies, kinds, offsets, totals = CC.expected(n, records, st)
        assert got["status_code"] == 0 and got["replies"] == replies
        assert np.array_equal(got["reply_kind"], kinds) and np.array_equal(got["out_offsets"], offsets)
        assert np.array_equal(got["totals"], totals)


def test_capacity_and_the_sizing_call(wire, store):
    st, by_len, noop = store
    n = 5
    records = CC.case_records(n, by_len, noop, MAX_TRIPLES)
    want = encode(wire, n, records, st)
    need = int(want["totals"][1])
    for cap in (0, need - 1):
        got = encode(wire, n, records, st, cap=cap, out=np.full(max(cap, 1), 0xEE, np.uint8))
        assert got["status_code"] == ECAPACITY and np.array_equal(got["totals"], want["totals"])
        assert got["out_offsets"][0] == 0 and (got["out_offsets"][1:] == -9).all() and (got["reply_kind"] == 9).all()
        assert (got["out"] == 0xEE).all()
    got = encode(wire, n, records, st, cap=need)
    assert got["status_code"] == 0 and got["replies"] == want["replies"]


def test_half_a_store_is_refused(wire, store):
    st, by_len, noop = store
    n = 3
    a = CC.arrays(n, CC.case_records(n, by_len, noop, MAX_TRIPLES)[:4])
    rec = wire.epx_reply_records(n, **{k: a[k] for k in wire.EPX_REPLY_RECORDS})
    off, ln, arena = st.arrays()
    out, ooff, kind, totals = np.zeros(1 << 18, np.uint8), np.zeros(5, np.int64), np.zeros(4, np.uint8), np.zeros(4, np.int64)
    fn = wire._L().fpx_wire_epx_encode_replica_replies_cmds
    p = lambda x: x.ctypes.data
    tail = [p(out), len(out), p(ooff), p(kind), p(totals)]
    for extra in ([p(a["out_triple"]), None, p(ln), p(arena), MAX_TRIPLES], [p(a["out_triple"]), p(off), None, p(arena), MAX_TRIPLES],
                  [None, p(off), p(ln), p(arena), MAX_TRIPLES], [p(a["out_triple"]), p(off), p(ln), p(arena), -1]):
        assert fn(n, 4, *[p(x) for x in rec], *extra, *tail) == EINVAL
    assert fn(n, 4, *[p(x) for x in rec], p(a["out_triple"]), p(off), p(ln), p(arena), MAX_TRIPLES, *tail) == 0


def test_length_bound_is_reached_and_never_exceeded(wire, store):
    st, by_len, noop = store
    reached = set()
    for n in (3, 5, 7):
        records = CC.case_records(n, by_len, noop, MAX_TRIPLES)
        got = encode(wire, n, records, st)
        for r, reply, kind in zip(records, got["replies"], got["reply_kind"]):
            if kind == CC.ENCODED and (r[5] == 8 or (r[5] == 6 and r[7] in (2, 3))):
                length = len(st.get(r[10]))
                assert len(reply) <= wire.epx_cmd_reply_max(length)
                if len(reply) == wire.epx_cmd_reply_max(length):
                    reached.add((n, length))
    # the bound is the worst case at n = 7, at both ends of the command lengths
    assert reached == {(7, 0), (7, CC.CMD_MAX_LEN)}
    # the closed form, field by field (include/fpx_wire.h)
    vl = lambda v: len(varint(v))
    for length in (0, 1, 127, 128, 16383, 16384, CC.CMD_MAX_LEN):
        inner = 9 + 10 + 2 + 24 + 2 + (1 + vl(length) + length) + 2 + (3 + 443)
        assert wire.epx_cmd_reply_max(length) == 1 + vl(inner) + inner


def test_emitter_under_the_sanitizers(tmp_path):
    """the emitter header as a stand-alone program: every reply into a heap buffer of exactly its planned length, the arena a
    heap block of exactly the bytes used"""
    exe = str(tmp_path / "epx_cmd_reply_emit_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                            exe, os.path.join(ROOT, "tests", "epx_cmd_reply_emit_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "all ok" and not [ln for ln in lines if ln.startswith("FAIL")]
    counts = dict(kv.split("=") for ln in lines if ln.startswith("ok replies") for kv in ln.split()[2:])
    assert all(int(counts[k]) > 100 for k in ("commit", "prepare_ok_cmd", "deferred", "short"))
