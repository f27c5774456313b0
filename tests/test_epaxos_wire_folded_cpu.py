"""The folded EPaxos decoder on the host (fpx_wire_epaxos_decode_replica_inbound_folded, include/fpx_wire.h): the sink with
fixed-size state that the device runs, compiled by g++ and run here without a GPU.  It must equal the existing host decoder
on every shared field, and its two folded words must equal a fold written independently in Python from the explicit ids
the existing decoder hands out (tests/epaxos_wire_cases.py)."""
import os

import numpy as np
import pytest

from tests import epaxos_wire_cases as W


@pytest.fixture(scope="module")
def wire():
    import frankenpaxos_amd

    if not os.path.exists(frankenpaxos_amd._lib.SO_PATH):
        frankenpaxos_amd.build()
    from frankenpaxos_amd import wire as w

    return w


def test_every_golden_epaxos_vector(wire):
    msgs = W.golden_epaxos_messages()
    assert len(msgs) >= 30
    d = W.assert_folded_equals(wire, msgs, 7)
    assert set(d["kind"].tolist()) == set(range(16, 24)) | {0}
    assert 1 in d["deps_shape"].tolist() and -1 in d["deps_shape"].tolist()
    # a row shorter than a message's sets is malformed at that message, as max_replicas is in the existing decoder
    widest = int(d["deps_num_replicas"].max())
    first = int(np.flatnonzero(d["deps_num_replicas"] == widest)[0])
    old = wire.epaxos_decode_replica_inbound(msgs, max_replicas=widest - 1)
    new = wire.epaxos_decode_replica_inbound_folded(msgs, num_replicas=widest - 1)
    assert (new["status_code"], new["bad_index"]) == (old["status_code"], old["bad_index"]) == (1, first)


@pytest.mark.parametrize("n", [3, 5, 7])
def test_generated_bursts_of_every_kind(wire, n):
    msgs = W.generated_burst(wire, 10 + n, n, 400)
    d = W.assert_folded_equals(wire, msgs, n)
    assert set(d["kind"].tolist()) == set(range(16, 24)) | {0}
    assert set(d["deps_shape"].tolist()) == {-1, 0, 1}
    pre_ok = d["kind"] == wire.EPX_PRE_ACCEPT_OK
    assert (d["deps_shape"][pre_ok] == 1).any() and (d["deps_shape"][pre_ok] == 0).any()
    assert (d["deps_values_end"][d["deps_shape"] == 1] > 0).any()


@pytest.mark.parametrize("n", [3, 5, 7])
def test_fold_edge_cases(wire, n):
    cases = W.edge_cases(n)
    msgs = [c[1] for c in cases]
    d = W.assert_folded_equals(wire, msgs, n)
    for i, (name, _, kind, shape, end) in enumerate(cases):
        assert (int(d["kind"][i]), int(d["deps_shape"][i]), int(d["deps_values_end"][i])) == (kind, shape, end), name
    # each alone as well: no state of one message reaches the next
    for name, msg, kind, shape, end in cases:
        one = wire.epaxos_decode_replica_inbound_folded([msg], num_replicas=n)
        assert (one["status_code"], int(one["kind"][0]), int(one["deps_shape"][0]), int(one["deps_values_end"][0])) == \
            (0, kind, shape, end), name
    by = {c[0]: i for i, c in enumerate(cases)}
    i = by["negative int32s"]
    assert d["sequence_number"][i] == -7 and d["deps_watermark"][i].tolist() == [10 if l == 1 else -1 - l for l in range(n)]
    i = by["dependencies twice: the last one holds"]
    assert d["deps_watermark"][i].tolist() == [10 if l == 1 else l + 2 for l in range(n)]
    i = by["instance twice: the last one holds, the fold is against it"]
    assert d["instance_number"][i] == 10
    i = by["two members: an AcceptOk after a PreAcceptOk"]
    assert d["deps_num_replicas"][i] == -1 and not d["deps_watermark"][i].any() and d["sequence_number"][i] == -1


@pytest.mark.parametrize("n", [3, 5])
def test_malformed_messages_are_refused_by_both(wire, n):
    good = W.edge_cases(n)[2][1]
    for name, msg in W.malformed_cases(n):
        for at, msgs in enumerate(([msg, good, good], [good, msg, good], [good, good, msg])):
            old = wire.epaxos_decode_replica_inbound(msgs, max_replicas=n)
            new = wire.epaxos_decode_replica_inbound_folded(msgs, num_replicas=n)
            assert (old["status_code"], old["bad_index"]) == (1, at), name
            assert (new["status_code"], new["bad_index"]) == (1, at), name
    # the row length bounds the sets whether the watermark array is asked for or not
    name, msg = W.malformed_cases(n)[-1]
    assert wire.epaxos_decode_replica_inbound_folded([msg], num_replicas=n, only_kind=True)["status_code"] == 1
    assert wire.epaxos_decode_replica_inbound_folded([msg], num_replicas=n + 1, only_kind=True)["status_code"] == 0


def test_truncation_at_every_length(wire):
    n = 5
    full = wire.epaxos_encode(wire.EPX_PRE_ACCEPT_OK, (2, 300), (1, 2), replica_index=4, sequence_number=1,
                              deps=[7, 0, 300, 129, 1 << 20], values=[(2, 302), (2, 301), (2, 303)])
    assert len(full) > 40
    well_formed = []
    for cut in range(len(full) + 1):
        old = wire.epaxos_decode_replica_inbound([full[:cut]], max_replicas=n)
        new = wire.epaxos_decode_replica_inbound_folded([full[:cut]], num_replicas=n)
        assert old["status_code"] == new["status_code"] and old["status_code"] in (0, 1), cut
        assert (new["bad_index"] == -1) == (new["status_code"] == 0)
        if new["status_code"] == 0:
            well_formed.append(cut)
            W.assert_folded_equals(wire, [full[:cut]], n)
    assert well_formed == [0, len(full)]            # (nothing at all is an empty ReplicaInbound: OTHER)
    d = wire.epaxos_decode_replica_inbound_folded([full], num_replicas=n)
    assert (int(d["deps_shape"][0]), int(d["deps_values_end"][0])) == (1, 304)


def test_offsets_are_judged_before_messages_and_every_optional_array_may_be_left_out(wire):
    n = 3
    cases = W.edge_cases(n)
    msgs = [c[1] for c in cases]
    d = wire.epaxos_decode_replica_inbound_folded(msgs, num_replicas=n, only_kind=True)
    assert d["status_code"] == 0 and d["kind"].tolist() == [c[2] for c in cases] and "deps_shape" not in d
    # a malformed message at 0 and a decreasing offset at 2: the offset wins, as in the existing decoder
    bad = W.malformed_cases(n)[0][1]
    good = msgs[1]
    off = [0, len(bad), len(bad) + len(good), len(bad), len(bad) + len(good)]
    old = wire.epaxos_decode_replica_inbound([bad, good], max_replicas=n, offsets=off)
    new = wire.epaxos_decode_replica_inbound_folded([bad, good], num_replicas=n, offsets=off)
    assert (new["status_code"], new["bad_index"]) == (old["status_code"], old["bad_index"]) == (1, 3)
    off = [0, len(bad), len(bad) + len(good) + 1]
    new = wire.epaxos_decode_replica_inbound_folded([bad, good], num_replicas=n, offsets=off)
    assert (new["status_code"], new["bad_index"]) == (1, 1)
    empty = wire.epaxos_decode_replica_inbound_folded([], num_replicas=n)
    assert empty["status_code"] == 0 and empty["bad_index"] == -1 and len(empty["kind"]) == 0
