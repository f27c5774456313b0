"""epaxos_wire_cases.py -- TEST INFRASTRUCTURE ONLY: serialised EPaxos ReplicaInbound messages for the folded decoders
(include/fpx_wire.h): a varint assembler for what wire.epaxos_encode cannot produce, the fold edge cases with what each
must fold to, seeded bursts of every kind, and the fold written a second time, in Python, from the explicit ids the
existing host decoder hands out."""
import json
import os
import random

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = ("kind", "instance_leader", "instance_number", "ballot_ordering", "ballot_replica", "replica_index",
          "sequence_number", "vote_ballot_ordering", "vote_ballot_replica", "status", "is_noop", "cmd_off", "cmd_len",
          "deps_num_replicas", "deps_watermark")
FOLD_MAX = 64


# ---- protobuf by hand ------------------------------------------------------------------------------------------------
def varint(v):
    v &= (1 << 64) - 1                      # a negative int32 travels sign-extended: ten bytes
    out = bytearray()
    while True:
        b = v & 0x7f
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def tag(field, wt):
    return varint(field << 3 | wt)


def i32(field, v):
    return tag(field, 0) + varint(v)


def ld(field, body):
    return tag(field, 2) + varint(len(body)) + body


def pair(field, a, b):
    return ld(field, i32(1, a) + i32(2, b))


def prefix_set(wm, ids=(), packed=False, wm_last=False):
    """IntPrefixSetProto { watermark = 1; repeated int32 value = 2 }"""
    vals = ld(2, b"".join(varint(x) for x in ids)) if packed else b"".join(i32(2, x) for x in ids)
    return vals + i32(1, wm) if wm_last else i32(1, wm) + vals


def deps_body(sets, num_replicas=None):
    """InstancePrefixSetProto { numReplicas = 1; repeated IntPrefixSetProto int_prefix_set = 2 }; sets: bodies"""
    return i32(1, len(sets) if num_replicas is None else num_replicas) + b"".join(ld(2, s) for s in sets)


def pre_accept_ok_body(inst, ballot, replica, seq, deps, order="ibrsd", extra=b""):
    """PreAcceptOk { instance = 1; ballot = 2; replica_index = 3; sequence_number = 4; dependencies = 5 }; order: the
    byte order of the fields (a letter twice: the field twice, deps then a list of bodies)"""
    deps = [deps] if isinstance(deps, bytes) else list(deps)
    parts = {"i": lambda: pair(1, *inst), "b": lambda: pair(2, *ballot), "r": lambda: i32(3, replica), "s": lambda: i32(4, seq),
             "d": lambda: ld(5, deps.pop(0))}
    return b"".join(parts[c]() for c in order) + extra


def pre_accept_ok(*a, **kw):
    return ld(3, pre_accept_ok_body(*a, **kw))


def accept_ok(inst, ballot, replica):
    return ld(5, pair(2, *inst) + pair(3, *ballot) + i32(7, replica))


def nack(inst, ballot):
    return ld(9, pair(1, *inst) + pair(2, *ballot))


CLIENT_REQUEST = ld(1, ld(1, b"abc"))      # member 1 of the oneof: OTHER to these decoders


# ---- the fold edge cases ---------------------------------------------------------------------------------------------
def edge_cases(n):
    """[(name, bytes, kind, deps_shape, deps_values_end)] at n replicas; the instance is (1, 10) unless the case says so"""
    L, x = 1, 10
    inst, bal = (L, x), (0, 1)

    def sets(own_ids=(), own_wm=x, foreign=None, packed=False, wm_last=False):
        out = []
        for l in range(n):
            if l == L:
                out.append(prefix_set(own_wm, own_ids, packed, wm_last))
            elif foreign and l == foreign[0]:
                out.append(prefix_set(3, foreign[1], packed))
            else:
                out.append(prefix_set(l + 2))
        return out

    def ok(own_ids=(), order="ibrsd", **kw):
        return pre_accept_ok(inst, bal, 2, 0, deps_body(sets(own_ids, **kw)), order)

    run = lambda k: list(range(x + 1, x + 1 + k))
    shuffled = run(9)
    random.Random(5).shuffle(shuffled)
    unknown = i32(15, 7) + tag(14, 1) + b"\x01" * 8 + ld(13, b"xy") + tag(12, 5) + b"\x02" * 4
    cases = [
        ("no ids", ok(), 17, 1, 0),
        ("one id", ok(run(1)), 17, 1, x + 2),
        ("two ids", ok(run(2)), 17, 1, x + 3),
        ("ids shuffled", ok(shuffled), 17, 1, x + 10),
        ("64 entries", ok(run(64)), 17, 1, x + 65),
        ("64 entries, reversed", ok(run(64)[::-1]), 17, 1, x + 65),
        ("65 entries", ok(run(65)), 17, 0, x + 66),
        ("65 entries, 64 distinct", ok(run(64) + [x + 1]), 17, 0, x + 65),
        ("a repeated id", ok([x + 1, x + 2, x + 1]), 17, 1, x + 3),
        ("a gap in the run", ok([x + 1, x + 3]), 17, 0, x + 4),
        ("the run starts late", ok([x + 2, x + 3]), 17, 0, x + 4),
        ("an id far above", ok([x + 1, x + 70]), 17, 0, x + 71),
        ("an id equal to the number", ok([x, x + 1]), 17, 0, x + 2),
        ("an id below the number", ok([x - 3]), 17, 0, x - 2),
        ("own watermark above the number", ok(run(2), own_wm=x + 1), 17, 0, x + 3),
        ("own watermark below the number", ok(run(2), own_wm=x - 1), 17, 1, x + 3),
        ("own watermark above the number, no ids", ok((), own_wm=x + 5), 17, 1, 0),
        ("an id in a foreign column", ok((), foreign=(0, [4])), 17, 0, 0),
        ("ids in the own and a foreign column", ok(run(2), foreign=(n - 1, [4, 5])), 17, 0, x + 3),
        ("packed value", ok(run(3), packed=True), 17, 1, x + 4),
        ("packed value, foreign", ok(run(1), foreign=(2, [9]), packed=True), 17, 0, x + 2),
        ("watermark after the values", ok(run(2), wm_last=True), 17, 1, x + 3),
        ("dependencies before instance", ok(run(2), order="dibrs"), 17, 1, x + 3),
        ("dependencies first, instance last", ok(run(2), order="dbrsi"), 17, 1, x + 3),
        ("dependencies twice: the last one holds",
         pre_accept_ok(inst, bal, 2, 0, [deps_body(sets([x + 1, x + 3], foreign=(0, [1]))), deps_body(sets(run(2)))], "ibdrsd"),
         17, 1, x + 3),
        ("dependencies twice: the last one is the odd one",
         pre_accept_ok(inst, bal, 2, 0, [deps_body(sets(run(2))), deps_body(sets([x + 1, x + 3]))], "dibrsd"), 17, 0, x + 4),
        ("instance twice: the last one holds, the fold is against it",
         ld(3, pair(1, L, x - 4) + pre_accept_ok_body(inst, bal, 2, 0, deps_body(sets(run(2))))), 17, 1, x + 3),
        ("two members: an AcceptOk after a PreAcceptOk", ok([x + 1, x + 3]) + accept_ok(inst, bal, 2), 19, -1, 0),
        ("two members: a PreAcceptOk after a Nack", nack(inst, (3, 0)) + ok(run(1)), 17, 1, x + 2),
        ("two members: the second PreAcceptOk has fewer ids", ok(run(5)) + ok(run(1)), 17, 1, x + 2),
        ("a ClientRequest after a PreAcceptOk: still the PreAcceptOk", ok(run(1)) + CLIENT_REQUEST, 17, 1, x + 2),
        ("negative int32s", pre_accept_ok((L, x), bal, 2, -7, deps_body([prefix_set(x if l == L else -1 - l) for l in range(n)])),
         17, 1, 0),
        ("a negative instance number", pre_accept_ok((L, -5), bal, 2, 0, deps_body(sets([-4, -3], own_wm=-6))), 17, 1, -2),
        ("unknown fields in the member", ld(3, unknown + pre_accept_ok_body(inst, bal, 2, 0, deps_body(sets(run(2)))) + unknown),
         17, 1, x + 3),
        ("unknown fields around the member", unknown.replace(i32(15, 7), i32(11, 7)) + ok(run(2)) + i32(10, 1), 17, 1, x + 3),
        ("unknown fields in the dependencies",
         pre_accept_ok(inst, bal, 2, 0, unknown + deps_body([unknown + s + unknown for s in sets(run(2))]) + unknown), 17, 1, x + 3),
        ("the instance's leader is outside the columns", pre_accept_ok((n, x), bal, 2, 0, deps_body(sets())), 17, 0, 0),
        ("the instance's leader is negative", pre_accept_ok((-1, x), bal, 2, 0, deps_body(sets())), 17, 0, 0),
        ("an AcceptOk", accept_ok(inst, bal, 0), 19, -1, 0),
        ("a Nack", nack(inst, (2, 2)), 23, -1, 0),
        ("a ClientRequest", CLIENT_REQUEST, 0, -1, 0),
        ("an empty message", b"", 0, -1, 0),
    ]
    return cases


def malformed_cases(n):
    """[(name, bytes)]: each must be refused by both host decoders and by the device decoder"""
    inst, bal = (1, 10), (0, 1)
    full = [prefix_set(l) for l in range(n)]
    good = pre_accept_ok_body(inst, bal, 2, 0, deps_body(full))
    return [
        ("numReplicas is one more than the sets", pre_accept_ok(inst, bal, 2, 0, deps_body(full, n + 1))),
        ("numReplicas is one less than the sets", pre_accept_ok(inst, bal, 2, 0, deps_body(full, n - 1))),
        ("a set without its watermark", pre_accept_ok(inst, bal, 2, 0, deps_body(full[:-1] + [i32(2, 4)]))),
        ("no numReplicas", pre_accept_ok(inst, bal, 2, 0, b"".join(ld(2, s) for s in full))),
        ("field number 0", ld(3, good + i32(0, 1))),
        ("a group wire type", ld(3, good + tag(9, 3))),
        ("no ballot", pre_accept_ok(inst, bal, 2, 0, deps_body(full), "irsd")),
        ("no dependencies", ld(3, pair(1, *inst) + pair(2, *bal) + i32(3, 2) + i32(4, 0))),
        ("an eleven-byte varint", ld(3, good + tag(3, 0) + b"\xff" * 10 + b"\x01")),
        ("a length past the end", ld(3, good)[:-3] + b"\x7f\x01\x01"),
        ("more sets than the caller's rows", pre_accept_ok(inst, bal, 2, 0, deps_body(full + [prefix_set(0)]))),
    ]


# ---- seeded bursts of every kind ---------------------------------------------------------------------------------------
def generated_burst(wire, seed, n, count):
    """count messages: the eight kinds, ClientRequest and the empty message, dependencies of n sets in every shape"""
    rng = random.Random(seed)
    out = []
    for j in range(count):
        kind = 16 + j % 10
        if kind == 24:
            out.append(CLIENT_REQUEST)
            continue
        if kind == 25:
            out.append(b"")
            continue
        L, x = rng.randrange(n), rng.randrange(0, 1 << rng.choice([3, 9, 20]))
        inst, bal = (L, x), (rng.randrange(4), rng.randrange(n))
        wm = [rng.randrange(0, 300) for _ in range(n)]
        values = []
        how = rng.randrange(8)
        if how >= 3:
            wm[L] = x
            values = [(L, x + 1 + k) for k in range(rng.randrange(1, 6))]
            rng.shuffle(values)
        if how == 5:
            values.pop(rng.randrange(len(values))) if len(values) > 2 else values.append((L, x + 40))
        if how == 6:
            values.append(((L + 1) % n, rng.randrange(400)))
        if how == 7:
            wm[L] = x + rng.choice([-1, 1])
        cmd = rng.choice([None, ld(1, bytes(rng.randrange(256) for _ in range(rng.randrange(0, 12))))])
        seq = rng.randrange(3)
        kw = dict(deps=wm, values=values)
        if kind in (16, 18):
            m = wire.epaxos_encode(kind, inst, bal, sequence_number=seq, command=cmd, **kw)
        elif kind == 17:
            m = wire.epaxos_encode(kind, inst, bal, replica_index=rng.randrange(n), sequence_number=seq, **kw)
        elif kind == 19:
            m = wire.epaxos_encode(kind, inst, bal, replica_index=rng.randrange(n))
        elif kind == 20:
            m = wire.epaxos_encode(kind, inst, sequence_number=seq, command=cmd, **kw)
        elif kind in (21, 23):
            m = wire.epaxos_encode(kind, inst, bal)
        elif rng.random() < 0.3:
            m = wire.epaxos_encode(22, inst, bal, replica_index=rng.randrange(n), vote_ballot=(-1, -1), status=0)
        else:
            m = wire.epaxos_encode(22, inst, bal, replica_index=rng.randrange(n), vote_ballot=(bal[0] // 2, bal[1]),
                                   status=rng.choice([1, 2]), sequence_number=seq, command=cmd, **kw)
        out.append(m)
    return out


def golden_epaxos_messages():
    """every serialised EPaxos message of tests/golden/wire_vectors.json"""
    vec = json.load(open(os.path.join(ROOT, "tests", "golden", "wire_vectors.json")))["vectors"]
    keys = ("pre_accept", "pre_accept_ok", "accept", "accept_ok", "commit", "prepare", "prepare_ok", "prepare_ok_bare", "nack",
            "client_request")
    return [bytes.fromhex(c[k]) for c in vec if c["msg"] == "epaxos" for k in keys]


# ---- the fold, a second time ---------------------------------------------------------------------------------------------
def py_fold(d, i):
    """(deps_values_end, deps_shape) of message i from wire.epaxos_decode_replica_inbound's outputs: the rules of
    include/fpx_wire.h spelt out on the explicit ids, with Python sets and no thought for fixed-size state"""
    nr = int(d["deps_num_replicas"][i])
    if nr < 0:
        return 0, -1
    lo, hi = int(d["values_off"][i]), int(d["values_off"][i + 1])
    ids = [(int(l), int(v)) for l, v in zip(d["values_leader"][lo:hi], d["values_id"][lo:hi])]
    L, x = int(d["instance_leader"][i]), int(d["instance_number"][i])
    own = [v for l, v in ids if l == L]
    end = max(own) + 1 if own else 0
    form = len(ids) <= FOLD_MAX and all(l == L for l, _ in ids) and 0 <= L < nr
    if form and own:
        form = int(d["deps_watermark"][i][L]) <= x and set(own) == set(range(x + 1, end))
    return end, 1 if form else 0


def assert_folded_equals(wire, msgs, n):
    """the folded host decoder against the existing one (every shared field) and against py_fold; returns the folded dict"""
    old = wire.epaxos_decode_replica_inbound(msgs, max_replicas=n)
    new = wire.epaxos_decode_replica_inbound_folded(msgs, num_replicas=n)
    assert old["status_code"] == 0 and new["status_code"] == 0, (old["bad_index"], new["bad_index"])
    assert new["bad_index"] == -1
    for k in SHARED:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
    want = [py_fold(old, i) for i in range(len(msgs))]
    assert new["deps_values_end"].tolist() == [w[0] for w in want]
    assert new["deps_shape"].tolist() == [w[1] for w in want]
    return new
