"""A replica tick's replies encoded on the device (fpx_wire_epx_encode_replica_replies_dev, csrc/fpx_wire_epx_enc_dev.hpp)
against the host batch encoder, which tests/test_epaxos_reply_encode_cpu.py holds equal to the yardstick: bytes, offsets,
reply kinds and totals, at the wavefront and workgroup edges of the scan and of the span writer, at every alignment of the
output, in both emit forms; and the refusals, every one a return code."""
import os

import numpy as np
import pytest

from tests import epaxos_reply_cases as RC

pytestmark = pytest.mark.gpu
EINVAL, ECAPACITY = 1, 5


@pytest.fixture(scope="module")
def wire():
    from frankenpaxos_amd import wire as w

    return w


@pytest.fixture(scope="module", params=["span", "direct"])
def ctxs(request):
    """one context per replica count, in the emit form the parameter names (FPX_EPX_ENC_DIRECT is read by fpx_epx_create)"""
    from frankenpaxos_amd.epaxos import EPaxos

    old = os.environ.pop("FPX_EPX_ENC_DIRECT", None)
    if request.param == "direct":
        os.environ["FPX_EPX_ENC_DIRECT"] = "1"
    made = {n: EPaxos(n, 4, num_instances=8) for n in (3, 5, 7)}
    os.environ.pop("FPX_EPX_ENC_DIRECT", None)
    if old is not None:
        os.environ["FPX_EPX_ENC_DIRECT"] = old
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


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_device_encoder_equals_the_host_encoder(wire, ctxs, m):
    for n in (3, 5, 7):
        records = RC.burst(n, m, shift=m * n)
        a = RC.arrays(n, records)
        want = wire.epx_encode_replica_replies(n, **a)
        assert_same(ctxs[n].encode_replica_replies(base_offset=(m + n) % 16, **a), want, m)


@pytest.mark.parametrize("base", range(16))
def test_every_alignment_of_the_output(wire, ctxs, base):
    n, m = 5, 200
    records = RC.burst(n, m, shift=64 * 2 + base)           # (begins inside the wavefront that holds the one long reply)
    a = RC.arrays(n, records)
    want = wire.epx_encode_replica_replies(n, **a)
    assert_same(ctxs[n].encode_replica_replies(base_offset=base, cap=int(want["totals"][1]), **a), want, m)


def test_wavefronts_of_no_replies_of_deferred_ones_and_one_long_reply(wire, ctxs):
    n = 5
    records = RC.wave_records(n)
    kinds = [RC.plan(n, r) for r in records]
    assert set(kinds[:64]) == {RC.NONE} and set(kinds[64:128]) == {RC.DEFERRED}
    lens = [len(RC.py_reply(n, r)[1]) for r in records[128:192]]
    assert sum(x > 100 for x in lens) == 1 and max(lens) > 250 and min(lens) > 0
    for lead in (0, 1, 64):                                   # the wavefronts as they are, and shifted across the edges
        rs = RC.burst(n, lead, shift=7) + records
        a = RC.arrays(n, rs)
        assert_same(ctxs[n].encode_replica_replies(base_offset=3, **a), wire.epx_encode_replica_replies(n, **a), len(rs))
    # nothing but records without bytes
    a = RC.arrays(n, records[:128])
    got = ctxs[n].encode_replica_replies(cap=0, **a)
    assert got["status_code"] == 0 and list(got["totals"]) == [0, 0, 64, -1] and not got["out_offsets"].any()


def test_sizing_call_one_byte_short_and_the_next_call(wire, ctxs):
    n, m = 3, 300
    e = ctxs[n]
    a = RC.arrays(n, RC.burst(n, m, shift=11))
    want = wire.epx_encode_replica_replies(n, **a)
    need = int(want["totals"][1])
    for cap in (0, need - 1):
        got = e.encode_replica_replies(cap=cap, base_offset=5, **a)
        assert got["status_code"] == ECAPACITY and np.array_equal(got["totals"], want["totals"])
        assert got["out_offsets"][0] == 0 and (got["out_offsets"][1:] == -9).all() and (got["reply_kind"] == 9).all()
        assert (got["out"] == 0xEE).all() and all((x == 0xEE).all() for x in got["around"])
        # FPX_ECAPACITY is this call's alone: the context encodes the next one, and a tick of its own runs
        assert_same(e.encode_replica_replies(cap=need, base_offset=5, **a), want, m)
    assert e.sync() == 0


def test_capacity_does_not_stop_the_calls_enqueued_behind_it(wire, ctxs):
    """no sync between the refused call and the next: the per-call code stops nothing, and sync reports it once"""
    import torch

    n, m = 5, 130
    e = ctxs[n]
    a = RC.arrays(n, RC.burst(n, m, shift=3))
    want = wire.epx_encode_replica_replies(n, **a)
    need = int(want["totals"][1])
    dev = torch.device("cuda", torch.cuda.current_device())
    up = [torch.from_numpy(x.reshape(-1)).to(dev) for x in wire.epx_reply_records(n, **a)]
    mk = lambda: (torch.full((need,), 0xEE, dtype=torch.uint8, device=dev), torch.full((m + 1,), -9, dtype=torch.int64, device=dev),
                  torch.full((m,), 9, dtype=torch.uint8, device=dev), torch.full((4,), -9, dtype=torch.int64, device=dev))
    o1, o2 = mk(), mk()
    torch.cuda.synchronize()
    e.encode_replica_replies_dev(*up, o1[0], need - 1, o1[1], o1[2], o1[3])
    e.encode_replica_replies_dev(*up, o2[0], need, o2[1], o2[2], o2[3])
    assert e.sync() == ECAPACITY and e.sync() == 0
    assert (o1[0].cpu().numpy() == 0xEE).all() and o1[1].cpu().numpy().tolist() == [0] + [-9] * m
    assert o2[0].cpu().numpy().tobytes() == want["out"][:need].tobytes()
    assert np.array_equal(o2[1].cpu().numpy(), want["out_offsets"]) and np.array_equal(o2[3].cpu().numpy(), want["totals"])


def test_an_unknown_outcome_is_refused_with_its_index(wire, ctxs):
    n, m = 7, 300
    e = ctxs[n]
    records = RC.burst(n, m, shift=5)
    for at, outcome in ((261, 9), (0, -1)):
        bad = list(records)
        bad[at] = bad[at][:5] + (outcome,) + bad[at][6:]
        bad[290] = bad[290][:5] + (77,) + bad[290][6:]
        a = RC.arrays(n, bad)
        got = e.encode_replica_replies(cap=1 << 17, **a)
        want = wire.epx_encode_replica_replies(n, cap=1 << 17, **a)
        assert got["status_code"] == want["status_code"] == EINVAL
        assert list(got["totals"]) == list(want["totals"]) == [0, 0, 0, at]
        assert got["out_offsets"][0] == 0 and (got["out_offsets"][1:] == -9).all() and (got["reply_kind"] == 9).all()
        assert (got["out"] == 0xEE).all()
    a = RC.arrays(n, records)
    assert_same(e.encode_replica_replies(**a), wire.epx_encode_replica_replies(n, **a), m)     # fit for the next call


def test_arguments_are_checked_at_once(wire, ctxs):
    import torch

    from frankenpaxos_amd._lib import FpxError

    e = ctxs[3]
    dev = torch.device("cuda", torch.cuda.current_device())
    z = torch.zeros(8, dtype=torch.int32, device=dev)
    out, off = torch.zeros(64, dtype=torch.uint8, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
    kind, totals = torch.zeros(2, dtype=torch.uint8, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    rec = [z] * 10
    for args, kw in (((rec + [out, 64, off, kind, None]), {}), ((rec + [out, 64, None, kind, totals]), {}),
                     ((rec + [None, 64, off, kind, totals]), {}), ((rec + [out, -1, off, kind, totals]), {}),
                     ((rec[:5] + [None] + rec[6:] + [out, 64, off, kind, totals]), {}),
                     ((rec + [out, 64, off, kind, totals]), {"m": -1}), ((rec + [out, 64, off, kind, totals]), {"m": (1 << 24) + 1})):
        with pytest.raises(FpxError) as err:
            e.encode_replica_replies_dev(*args, m=kw.get("m", 2))
        assert err.value.status == EINVAL
    # m = 0 needs no record array
    e.encode_replica_replies_dev(*([None] * 10), None, 0, off, None, totals, m=0)
    assert e.sync() == 0 and totals.cpu().numpy().tolist() == [0, 0, 0, -1] and off.cpu().numpy()[0] == 0
