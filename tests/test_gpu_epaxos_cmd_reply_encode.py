"""The replies that carry a stored command, encoded on the device from the context's command store
(fpx_wire_epx_encode_replica_replies_cmds_dev, csrc/fpx_wire_epx_enc_dev.hpp) against the host encoder with the same store as
plain arrays (tests/test_epaxos_cmd_reply_encode_cpu.py holds that one against the yardstick): bytes, offsets, kinds and
totals -- command replies alone and mixed with short ones, at the wavefront and workgroup edges, at every alignment of the
output, in both emit forms and both copy forms; and a context without the store."""
import os

import numpy as np
import pytest

from tests import epaxos_cmd_reply_cases as CC

pytestmark = pytest.mark.gpu
ECAPACITY = 5
MAX_TRIPLES = 64


@pytest.fixture(scope="module")
def wire():
    from frankenpaxos_amd import wire as w

    return w


@pytest.fixture(scope="module")
def store():
    return CC.case_store(MAX_TRIPLES)


@pytest.fixture(scope="module", params=["span-words", "direct-words", "span-bytes"])
def ctxs(request, store):
    """one context per replica count with the case store put into it, in the emit form and the copy form the parameter
    names (FPX_EPX_ENC_DIRECT and FPX_EPX_CMDS_WORDS are read by fpx_epx_create)"""
    from frankenpaxos_amd.epaxos import EPaxos

    names = {"FPX_EPX_ENC_DIRECT": request.param.startswith("direct"), "FPX_EPX_CMDS_WORDS": request.param.endswith("words")}
    old = {k: os.environ.pop(k, None) for k in names}
    for k, on in names.items():
        if on:
            os.environ[k] = "1"
    made = {n: EPaxos(n, 4, num_instances=8) for n in (3, 5, 7)}
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    st = store[0]
    ids = [t for t in range(MAX_TRIPLES) if st.get(t) is not None]
    ids.sort(key=lambda t: int(st.off[t]))
    for e in made.values():
        e.cmds_enable(MAX_TRIPLES, len(st.arena) + 3)
        code, res = e.cmds_put([st.get(t) for t in ids], ids)
        assert code == 0 and list(res) == [len(ids), len(st.arena), 0, 0]
    yield made
    for e in made.values():
        e.close()


def assert_same(got, want, m):
    assert got["status_code"] == want["status_code"] == 0
    assert np.array_equal(got["totals"], want["totals"])
    assert np.array_equal(got["out_offsets"], want["out_offsets"]) and np.array_equal(got["reply_kind"], want["reply_kind"])
    need = int(want["totals"][1])
    assert got["out"][:need].tobytes() == want["out"][:need].tobytes()
    assert got["replies"] == want["replies"] and len(got["replies"]) == m
    before, after = got["around"]
    assert (before == 0xEE).all() and (after == 0xEE).all() and (got["out"][need:] == 0xEE).all()    # not a byte outside


def both(wire, e, n, records, st, **kw):
    a = CC.arrays(n, records)
    tr = a.pop("out_triple")
    want = wire.epx_encode_replica_replies_cmds(n, tr, st.arrays(), **a)
    return e.encode_replica_replies(out_triple=tr, **kw, **a), want


@pytest.mark.parametrize("only_cmds", [True, False])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257])
def test_device_encoder_equals_the_host_encoder(wire, ctxs, store, m, only_cmds):
    st, by_len, noop = store
    for n in (3, 5, 7):
        records = CC.burst(n, m, by_len, noop, MAX_TRIPLES, shift=m * n, only_cmds=only_cmds, big=m <= 65)
        got, want = both(wire, ctxs[n], n, records, st, base_offset=(m + n) % 16)
        assert_same(got, want, m)
        assert want["totals"][0] > 0


@pytest.mark.parametrize("base", range(16))
def test_every_alignment_of_the_output(wire, ctxs, store, base):
    st, by_len, noop = store
    n, m = 5, 150
    records = CC.burst(n, m, by_len, noop, MAX_TRIPLES, shift=base, big=base % 8 == 0)
    got, want = both(wire, ctxs[n], n, records, st, base_offset=base)
    assert_same(got, want, m)


def test_a_wavefront_of_short_replies_next_to_one_with_a_single_command_reply(wire, ctxs, store):
    st, by_len, noop = store
    n = 5
    records = CC.wave_records(n, by_len)
    kinds = [CC.plan(n, r, st) for r in records]
    carries = [r[5] == 8 or (r[5] == 6 and r[7] in (2, 3)) for r in records]
    assert not any(carries[:64]) and sum(carries[64:]) == 1 and set(kinds) == {CC.ENCODED}
    for lead in (0, 1, 64):                                   # the wavefronts as they are, and shifted across the edges
        rs = [CC.short(n, j) for j in range(lead)] + records
        got, want = both(wire, ctxs[n], n, rs, st, base_offset=3)
        assert_same(got, want, len(rs))


def test_sizing_call_one_byte_short_and_the_next_call(wire, ctxs, store):
    st, by_len, noop = store
    n, m = 3, 100
    e = ctxs[n]
    records = CC.burst(n, m, by_len, noop, MAX_TRIPLES, shift=11, big=False)
    _, want = both(wire, e, n, records, st, cap=0)
    need = int(want["totals"][1])
    for cap in (0, need - 1):
        got, _ = both(wire, e, n, records, st, cap=cap, base_offset=5)
        assert got["status_code"] == ECAPACITY and np.array_equal(got["totals"], want["totals"])
        assert got["out_offsets"][0] == 0 and (got["out_offsets"][1:] == -9).all() and (got["reply_kind"] == 9).all()
        assert (got["out"] == 0xEE).all() and all((x == 0xEE).all() for x in got["around"])
    got, _ = both(wire, e, n, records, st, cap=need, base_offset=5)
    assert_same(got, want, m)
    assert e.sync() == 0


def test_a_context_without_the_store_equals_the_existing_call(wire, store):
    from frankenpaxos_amd.epaxos import EPaxos

    st, by_len, noop = store
    n, m = 5, 300
    records = CC.burst(n, m, by_len, noop, MAX_TRIPLES, shift=9)
    a = CC.arrays(n, records)
    tr = a.pop("out_triple")
    e = EPaxos(n, 4, num_instances=8)
    try:
        want = e.encode_replica_replies(base_offset=7, **a)
        got = e.encode_replica_replies(base_offset=7, out_triple=tr, **a)
        assert_same(got, want, m)
        assert_same(got, wire.epx_encode_replica_replies(n, **a), m)
    finally:
        e.close()
