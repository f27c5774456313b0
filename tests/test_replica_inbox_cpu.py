"""fpx_replica_inbox without a GPU: the two models of tests/replica_inbox_model.py against each other and against
re-submission at every cut point, the streams' promises, the read decoder against google.protobuf's bytes
(tests/golden/wire_replica_reads.json), the bindings, and the parser under the address and undefined-behaviour
sanitizers from a stand-alone program."""
import json
import os
import subprocess

import numpy as np
import pytest

from frankenpaxos_amd import wire
from tests import replica_inbox_model as M
from tests import replica_inbox_streams as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(seed, n) for seed in RS.SEEDS for n in RS.SIZES]
COVERING = [(seed, n) for seed in RS.SEEDS for n in (255, 256, 257, 3000)]   # the sizes that promise every class


@pytest.mark.parametrize("seed,n", CASES)
def test_the_two_models_agree(seed, n):
    b = RS.make(seed, n)
    M.assert_same(M.sequential(*b.state(), *b.arrays()), M.arrays(*b.state(), *b.arrays()), (seed, n))
    M.assert_same(M.sequential(*b.state(), b.kind, b.slot, b.value), M.arrays(*b.state(), b.kind, b.slot, b.value), "no mask")


def test_the_models_agree_on_a_bad_slot_and_by_hand():
    b = RS.make(1, 64)
    live = np.flatnonzero((b.kind == wire.CHOSEN) & (b.mask != 0))
    for bad_slot in (-1, b.num_slots):
        slot = b.slot.copy()
        slot[live[5]], slot[live[9]] = bad_slot, bad_slot
        for model in (M.sequential, M.arrays):
            r = model(*b.state(), b.kind, slot, b.value, b.mask)
            assert (r.status, r.bad_index) == (M.EINVAL, live[5])
    # W0 = 2; Chosen 3, read under 2 (deferred), read under 3 (deferred, slot in the log), Chosen 2 (executes 2 and 3)
    present, values = np.zeros(16, np.uint8), np.full(16, -1, np.int32)
    present[:2], values[:2] = 1, 7
    kind = [wire.CHOSEN, wire.READ_REQUEST, wire.SEQUENTIAL_READ_REQUEST, wire.EVENTUAL_READ_REQUEST, wire.CHOSEN,
            wire.READ_REQUEST]
    for model in (M.sequential, M.arrays):
        r = model(present, values, 2, 2, kind, [3, 2, 3, 0, 2, 3], [30, 0, 0, 0, 20, 0])
        assert r.exec_count.tolist() == [-2, 3, 4, 2, -2, 4] and r.reply_slot.tolist() == [-2, 1, 2, 1, -2, 3]
        assert r.order.tolist() == [3, 1, 2, 5] and r.counts == (4, 4, 2, 4) and r.num_chosen == 4


@pytest.mark.parametrize("seed,n", COVERING)
def test_the_streams_are_not_vacuous(seed, n):
    b = RS.make(seed, n)
    r = M.sequential(*b.state(), *b.arrays())
    assert r.status == 0 and set(r.classes) == set(M.CLASSES)
    missing = [c for c in M.CLASSES if r.classes[c] < 1]
    assert not missing, (missing, r.classes)
    assert r.counts[2] < r.counts[3] < b.num_slots


def two_bursts(model, b, k):
    """burst[:k], then the still-deferred reads followed by burst[k:]: per read of the whole burst (exec_count,
    reply_slot), and the run order, in the whole burst's indices"""
    head = model(*b.state(), *(a[:k] for a in b.arrays()))
    assert head.status == 0
    (kind, slot, value, mask), idx = RS.resubmit(b, k, head.still_deferred())
    tail = model(head.present, head.values, head.w1, head.num_chosen, kind, slot, value, mask)
    exec_count, reply_slot = np.full(len(b.kind), M.NOT_A_READ, np.int32), np.full(len(b.kind), M.NOT_A_READ, np.int32)
    exec_count[:k], reply_slot[:k] = head.exec_count, head.reply_slot
    again = tail.exec_count != M.NOT_A_READ
    exec_count[idx[again]], reply_slot[idx[again]] = tail.exec_count[again], tail.reply_slot[again]
    ran = np.concatenate([head.order[:head.counts[1]], idx[tail.order[:tail.counts[1]]]])
    left = idx[tail.order[tail.counts[1]:tail.counts[0]]]
    return exec_count, reply_slot, ran, left, tail


@pytest.mark.parametrize("seed,n", [(s, n) for s in RS.SEEDS for n in (65, 257)] + [(1, 3000)])
def test_resubmission_is_exact_at_every_cut(seed, n):
    b = RS.make(seed, n)
    whole = M.sequential(*b.state(), *b.arrays())
    model, cuts = (M.sequential, range(n + 1)) if n < 1000 else (M.arrays, range(0, n + 1, 97))
    for k in cuts:
        exec_count, reply_slot, ran, left, tail = two_bursts(model, b, k)
        np.testing.assert_array_equal(exec_count, whole.exec_count, err_msg="cut %d" % k)
        np.testing.assert_array_equal(reply_slot, whole.reply_slot, err_msg="cut %d" % k)
        np.testing.assert_array_equal(ran, whole.order[:whole.counts[1]], err_msg="cut %d" % k)
        np.testing.assert_array_equal(left, whole.still_deferred(), err_msg="cut %d" % k)
        assert (tail.w1, tail.num_chosen) == (whole.w1, whole.num_chosen)
        np.testing.assert_array_equal(tail.values, whole.values)


# ---- the decoder ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "wire_replica_reads.json")))


def test_decoder_against_protobuf_vectors(golden):
    vs = golden["vectors"]
    assert {v["member"] for v in vs} == {"chosen", "read_request", "sequential_read_request", "eventual_read_request",
                                         "read_request_batch", "sequential_read_request_batch", "eventual_read_request_batch"}
    msgs = [bytes.fromhex(v["bytes"]) for v in vs]
    d = wire.decode_replica_inbound_reads(msgs)
    assert d["status"] == 0
    base = np.cumsum([0] + [len(m) for m in msgs])
    for i, v in enumerate(vs):
        got = {k: int(d[k][i]) for k in ("kind", "slot", "count", "is_noop", "value_len")}
        assert got == {k: v[k] for k in got}, (i, v["member"], got)
        off = int(d["value_off"][i])
        assert off == base[i] + v["value_off"]
        assert d["buf"][off:off + v["value_len"]].tobytes().hex() == v["value_hex"]
    # the existing decoder is unchanged: it still leaves the reads to the actor
    old = wire.decode_replica_inbound(msgs)
    assert old["status"] == 0
    assert [int(k) for k in old["kind"]] == [wire.CHOSEN if v["member"] == "chosen" else wire.OTHER for v in vs]
    same = [i for i, v in enumerate(vs) if v["member"] == "chosen"]
    for k in ("slot", "is_noop", "value_off", "value_len"):
        np.testing.assert_array_equal(old[k][same], d[k][same])


def test_decoder_on_malformed_and_foreign_input(golden):
    good = bytes.fromhex(golden["vectors"][0]["bytes"])
    assert len(golden["malformed"]) > 80
    for m in golden["malformed"]:
        d = wire.decode_replica_inbound_reads([good, bytes.fromhex(m["bytes"]), good])
        assert (d["status"], d["bad_index"]) == (1, 1), m["why"]
    d = wire.decode_replica_inbound_reads([bytes.fromhex(m["bytes"]) for m in golden["other"]])
    assert d["status"] == 0 and not d["kind"].any() and (d["slot"] == -1).all() and (d["count"] == -1).all()
    w = golden["last_member_wins"]
    d = wire.decode_replica_inbound_reads([bytes.fromhex(w["bytes"])])
    assert d["status"] == 0 and {k: int(d[k][0]) for k in w if k != "bytes"} == {k: w[k] for k in w if k != "bytes"}
    # offsets are checked before a byte is parsed, as in the other decoders
    d = wire.decode_replica_inbound_reads([good, good], offsets=[0, 10**9, len(good)])
    assert (d["status"], d["bad_index"]) == (1, 1)
    assert wire.decode_replica_inbound_reads([])["status"] == 0


# ---- bindings -------------------------------------------------------------------------------------------------------
def test_abi_and_python_prototypes():
    import frankenpaxos_amd as fa
    from frankenpaxos_amd import _lib

    L = fa.lib()
    for name, nargs in (("fpx_replica_inbox", 12), ("fpx_replica_inbox_dev", 10)):
        assert hasattr(L, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert hasattr(L, "fpx_wire_decode_replica_inbound_reads")
    header = open(os.path.join(ROOT, "include", "fpx.h")).read()
    assert "int32_t fpx_replica_inbox_dev(fpx_ctx* ctx, int32_t n," in header and "r - 1" in header
    kinds = (wire.READ_REQUEST, wire.SEQUENTIAL_READ_REQUEST, wire.EVENTUAL_READ_REQUEST, wire.READ_REQUEST_BATCH,
             wire.SEQUENTIAL_READ_REQUEST_BATCH, wire.EVENTUAL_READ_REQUEST_BATCH)
    assert kinds == (12, 13, 14, 24, 25, 26)
    wire_h = open(os.path.join(ROOT, "include", "fpx_wire.h")).read()
    for name, k in zip(("READ_REQUEST", "SEQUENTIAL_READ_REQUEST", "EVENTUAL_READ_REQUEST", "READ_REQUEST_BATCH",
                        "SEQUENTIAL_READ_REQUEST_BATCH", "EVENTUAL_READ_REQUEST_BATCH"), kinds):
        assert "FPX_WIRE_%s = %d," % (name, k) in wire_h
    # refused before anything touches a device
    assert L.fpx_replica_inbox(None, 0, *[None] * 10) == 1 and L.fpx_replica_inbox_dev(None, 0, *[None] * 8) == 1


def test_the_cxx_mirror_compiles_with_the_new_method(tmp_path):
    src = tmp_path / "m.cpp"
    src.write_text('#include "frankenpaxos_amd/host/fpx.hpp"\n'
                   'int main() { auto p = &frankenpaxos::multipaxos::Phase2Engine::replicaHandleInbox; (void)p; return 0; }\n')
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_parser_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "replica_inbox_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                            os.path.join(ROOT, "tests", "replica_inbox_host_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "replica inbox parser ok" in run.stdout, run.stdout + run.stderr
