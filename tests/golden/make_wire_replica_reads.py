"""Generates tests/golden/wire_replica_reads.json: the bytes google.protobuf produces for a MultiPaxos replica's inbox WITH
its read path, from descriptors transcribed field by field from multipaxos/MultiPaxos.proto (CommandId :188-196, Command
:198-204, Chosen :292-298, ReadRequest :351-358, ReadRequestBatch :360-366, SequentialReadRequest :368-374,
SequentialReadRequestBatch :376-382, EventualReadRequest :384-389, EventualReadRequestBatch :391-396, ReplicaInbound
:563-576), what fpx_wire_decode_replica_inbound_reads must make of them, and truncated / malformed inputs with the
verdict expected.

Run where google.protobuf is importable:  python tests/golden/make_wire_replica_reads.py
The committed JSON is what tests/test_replica_inbox_cpu.py checks the decoder against (it needs no protobuf runtime)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_wire_golden import F, _file  # noqa: E402

KINDS = {"chosen": 4, "read_request": 12, "sequential_read_request": 13, "eventual_read_request": 14,
         "read_request_batch": 24, "sequential_read_request_batch": 25, "eventual_read_request_batch": 26}


def build():
    REQ, OPT, REP = F.LABEL_REQUIRED, F.LABEL_OPTIONAL, F.LABEL_REPEATED
    I32, BYT, MSG = F.TYPE_INT32, F.TYPE_BYTES, F.TYPE_MESSAGE
    i = lambda n, k: (n, k, I32, REQ, None, None)
    one = lambda n, k, t: (n, k, MSG, OPT, t, "request")
    return _file("fpx_multipaxos_reads.proto", "frankenpaxos.multipaxos", {
        "Noop": [],
        "CommandId": [("client_address", 1, BYT, REQ, None, None), i("client_pseudonym", 2), i("client_id", 3)],
        "Command": [("command_id", 1, MSG, REQ, "CommandId", None), ("command", 2, BYT, REQ, None, None)],
        "CommandBatch": [("command", 1, MSG, REP, "Command", None)],
        "CommandBatchOrNoop": [("command_batch", 1, MSG, OPT, "CommandBatch", "value"), ("noop", 2, MSG, OPT, "Noop", "value")],
        "Chosen": [i("slot", 1), ("command_batch_or_noop", 2, MSG, REQ, "CommandBatchOrNoop", None)],
        "ReadRequest": [i("slot", 1), ("command", 2, MSG, REQ, "Command", None)],
        "ReadRequestBatch": [i("slot", 1), ("command", 2, MSG, REP, "Command", None)],
        "SequentialReadRequest": [i("slot", 1), ("command", 2, MSG, REQ, "Command", None)],
        "SequentialReadRequestBatch": [i("slot", 1), ("command", 2, MSG, REP, "Command", None)],
        "EventualReadRequest": [("command", 1, MSG, REQ, "Command", None)],
        "EventualReadRequestBatch": [("command", 1, MSG, REP, "Command", None)],
        "ReplicaInbound": [one("chosen", 1, "Chosen"), one("read_request", 2, "ReadRequest"),
                           one("sequential_read_request", 3, "SequentialReadRequest"),
                           one("eventual_read_request", 4, "EventualReadRequest"),
                           one("read_request_batch", 5, "ReadRequestBatch"),
                           one("sequential_read_request_batch", 6, "SequentialReadRequestBatch"),
                           one("eventual_read_request_batch", 7, "EventualReadRequestBatch")],
    })


def fill(c, spec):
    addr, pseud, cid, payload = spec
    c.command_id.client_address, c.command_id.client_pseudonym, c.command_id.client_id, c.command = addr, pseud, cid, payload


def main():
    M = build()
    commands = [(b"\x0a\x00\x00\x01:9000", 3, 17, b"get x"), (b"", 0, 0, b""), (b"client-7", 2147483647, -5, bytes(range(200))),
                (b"c", 128, 300, b"k" * 130)]
    slots = [-1, 0, 5, 127, 128, 1 << 20, 2147483647, -2147483648]
    vectors = []

    def add(member, r, slot, inner, count, is_noop=-1):
        whole = r.SerializeToString()
        at = whole.find(inner) if inner else len(whole)
        assert at >= 0
        vectors.append({"member": member, "kind": KINDS[member], "slot": slot, "count": count, "is_noop": is_noop,
                        "value_off": at, "value_len": len(inner), "value_hex": inner.hex(), "bytes": whole.hex()})

    for j, slot in enumerate(slots):
        spec = commands[j % len(commands)]
        for member in ("read_request", "sequential_read_request"):
            r = M["ReplicaInbound"]()
            x = getattr(r, member)
            x.slot = slot
            fill(x.command, spec)
            add(member, r, slot, x.command.SerializeToString(), 1)
        for member in ("read_request_batch", "sequential_read_request_batch"):
            for k in (0, 1, 4):
                r = M["ReplicaInbound"]()
                x = getattr(r, member)
                x.slot = slot
                for q in range(k):
                    fill(x.command.add(), commands[(j + q) % len(commands)])
                add(member, r, slot, x.SerializeToString(), k)
    for j, spec in enumerate(commands):
        r = M["ReplicaInbound"]()
        fill(r.eventual_read_request.command, spec)
        add("eventual_read_request", r, -1, r.eventual_read_request.command.SerializeToString(), 1)
        r = M["ReplicaInbound"]()
        r.eventual_read_request_batch.SetInParent()
        for q in range(j):
            fill(r.eventual_read_request_batch.command.add(), commands[q])
        add("eventual_read_request_batch", r, -1, r.eventual_read_request_batch.SerializeToString(), j)
    for slot, noop in [(0, True), (9, False), (1 << 20, False)]:
        r = M["ReplicaInbound"]()
        r.chosen.slot = slot
        if noop:
            r.chosen.command_batch_or_noop.noop.SetInParent()
        else:
            fill(r.chosen.command_batch_or_noop.command_batch.command.add(), commands[0])
        add("chosen", r, slot, r.chosen.command_batch_or_noop.SerializeToString(), -1, int(noop))

    # malformed: every proper prefix of three messages that cuts a field short, and hand-made damage
    good = {}
    for v in vectors:
        if v["slot"] in (-1, 9):
            good.setdefault(v["member"], bytes.fromhex(v["bytes"]))
    bad = []
    for member in ("read_request", "read_request_batch", "eventual_read_request"):
        whole = good[member]
        for cut in range(1, len(whole)):
            bad.append({"why": "%s cut at %d" % (member, cut), "bytes": whole[:cut].hex()})
    r = M["ReplicaInbound"]()
    r.read_request.slot = 3
    fill(r.read_request.command, commands[0])
    inner = r.read_request.SerializeToString()
    no_slot = inner[2:]                                     # the slot field (tag 0x08, value 3) dropped
    bad.append({"why": "ReadRequest without slot", "bytes": (bytes([0x12, len(no_slot)]) + no_slot).hex()})
    bad.append({"why": "ReadRequest without command", "bytes": bytes([0x12, 2, 0x08, 3]).hex()})
    bad.append({"why": "EventualReadRequest without command", "bytes": bytes([0x22, 0]).hex()})
    cmd_no_id = bytes([0x12, 1, 0x41])                      # Command { command = "A" }: command_id missing
    bad.append({"why": "Command without command_id", "bytes": (bytes([0x22, len(cmd_no_id) + 2, 0x0a, len(cmd_no_id)]) + cmd_no_id).hex()})
    cid_short = bytes([0x0a, 0, 0x10, 1])                   # CommandId without client_id
    cmd = bytes([0x0a, len(cid_short)]) + cid_short + bytes([0x12, 0])
    bad.append({"why": "CommandId without client_id", "bytes": (bytes([0x3a, len(cmd) + 2, 0x0a, len(cmd)]) + cmd).hex()})
    bad.append({"why": "length past the end", "bytes": bytes([0x2a, 0x7f, 0x08, 1]).hex()})
    bad.append({"why": "varint of 11 bytes", "bytes": (bytes([0x12, 13, 0x08]) + b"\xff" * 11 + b"\x01").hex()})
    bad.append({"why": "group wire type", "bytes": bytes([0x12, 2, 0x0b, 0x0c]).hex()})
    # well-formed, but not for this path
    other = [{"why": "empty message", "bytes": ""}, {"why": "unknown member 9", "bytes": bytes([0x4a, 1, 0x00]).hex()},
             {"why": "unknown varint field", "bytes": bytes([0x78, 5]).hex()}]
    # the last member of the oneof wins (bytes concatenated: what a merging parser sees)
    last = good["chosen"] + good["read_request"]
    v = next(x for x in vectors if x["member"] == "read_request" and x["slot"] == -1)
    wins = {"bytes": last.hex(), "kind": v["kind"], "slot": v["slot"], "count": 1, "value_off": len(good["chosen"]) + v["value_off"],
            "value_len": v["value_len"]}
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wire_replica_reads.json")
    json.dump({"generator": "google.protobuf " + __import__("google.protobuf").protobuf.__version__, "vectors": vectors,
               "malformed": bad, "other": other, "last_member_wins": wins}, open(out, "w"), indent=0)
    print(len(vectors), "vectors,", len(bad), "malformed ->", out)


if __name__ == "__main__":
    main()
