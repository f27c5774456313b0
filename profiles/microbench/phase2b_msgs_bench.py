"""One tick of 2^20 slots x 2 Phase2b votes each (R = 3, f = 1), slot-major or in random order:

  new       fpx_wire_phase2b_tick end to end (copy up, device decode, claim / gather / tally, compaction, copy down)
  baseline  the same tick through the host: fpx_wire_decode_proxy_leader_inbound + fpx_wire_phase2b_rows +
            fpx_proxy_phase2b.  --lib picks the library (a build of the commit before the device tally, whose symbols
            these all are), so the new code is never its own yardstick.

Wall-clock ms per tick, median of --reps; run under `rocprofv3 --kernel-trace --stats` for the per-kernel times
(profiles/phase2b_msgs.md)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["new", "baseline"], required=True)
ap.add_argument("--order", choices=["slot_major", "random"], default="slot_major")
ap.add_argument("--lib", default=None)
ap.add_argument("--log-slots", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
if args.lib:
    os.environ["FPX_LIB"] = os.path.abspath(args.lib)

from frankenpaxos_amd._lib import FpxConfig  # noqa: E402

S, R = 1 << args.log_slots, 3
VP, I32 = C.c_void_p, C.c_int32


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def phase2b(acc, slot, rnd):  # ProxyLeaderInbound{phase2b = 2}{group_index 1, acceptor_index 2, slot 3, round 4}
    body = b"\x08\x00\x10" + varint(acc) + b"\x18" + varint(slot) + b"\x20" + varint(rnd)
    return b"\x12" + varint(len(body)) + body


rng = np.random.default_rng(1)
slots = np.repeat(np.arange(S, dtype=np.int64), 2)
accs = rng.permuted(np.tile(np.arange(R), (S, 1)), axis=1)[:, :2].reshape(-1)  # two DIFFERENT acceptors per slot
if args.order == "random":
    p = rng.permutation(len(slots))
    slots, accs = slots[p], accs[p]
msgs = [phase2b(int(a), int(s), 0) for a, s in zip(accs.tolist(), slots.tolist())]
n = len(msgs)
offsets = np.zeros(n + 1, np.int64)
np.cumsum([len(m) for m in msgs], out=offsets[1:])
raw = np.frombuffer(b"".join(msgs), np.uint8)
in_len = int(offsets[-1])

L = C.CDLL(os.environ.get("FPX_LIB") or os.path.join(ROOT, "frankenpaxos_amd", "csrc", "libfpx.so"), mode=C.RTLD_GLOBAL)
cfg = FpxConfig(S, R, 1, 1, 1, 0, 0, 0, 2, 0, 4, 0, 0, 0, 0)
h = VP()
assert L.fpx_create(C.byref(cfg), C.byref(h)) == 0
open_slot = np.arange(S, dtype=np.int32)
zeros, vals, new = np.zeros(S, np.int32), np.arange(S, dtype=np.int32), np.zeros(S, np.uint8)


def ptr(a):
    return VP(a.ctypes.data)


def reopen():
    assert L.fpx_reset(h) == 0
    assert L.fpx_proxy_open(h, I32(S), ptr(open_slot), ptr(zeros), ptr(vals), ptr(new)) == 0


def pinned(nbytes, dtype):
    p = VP()
    assert L.fpx_host_alloc(C.c_int64(max(1, nbytes)), C.byref(p)) == 0
    return np.frombuffer((C.c_char * nbytes).from_address(p.value), dtype=dtype)


times, parts, chosen = [], [], 0
if args.mode == "new":
    pin_in, pin_off = pinned(in_len, np.uint8), pinned(8 * (n + 1), np.int64)
    pin_in[:], pin_off[:] = raw, offsets
    outs = [pinned(4 * S, np.int32) for _ in range(3)]
    cnt, bad = I32(0), I32(-1)
    for rep in range(args.reps + 1):
        reopen()
        t0 = time.perf_counter()
        st = L.fpx_wire_phase2b_tick(h, ptr(pin_in), C.c_int64(in_len), ptr(pin_off), I32(n), I32(0), ptr(outs[0]),
                                     ptr(outs[1]), ptr(outs[2]), I32(S), C.byref(cnt), C.byref(bad))
        t1 = time.perf_counter()
        assert st == 0, st
        chosen = cnt.value
        if rep:
            times.append((t1 - t0) * 1e3)
else:
    f = {k: np.zeros(n, np.int32) for k in ("kind", "slot", "round", "is_noop", "value_len", "group", "acc")}
    voff = np.zeros(n, np.int64)
    rs, rr, rb = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 4), np.uint64)
    ch, cr, cv = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
    bad, m = I32(-1), I32(0)
    for rep in range(args.reps + 1):
        reopen()
        t0 = time.perf_counter()
        st = L.fpx_wire_decode_proxy_leader_inbound(ptr(raw), C.c_int64(in_len), ptr(offsets), I32(n), ptr(f["kind"]),
                                                    ptr(f["slot"]), ptr(f["round"]), ptr(f["is_noop"]), ptr(voff),
                                                    ptr(f["value_len"]), ptr(f["group"]), ptr(f["acc"]), C.byref(bad))
        t1 = time.perf_counter()
        assert st == 0
        st = L.fpx_wire_phase2b_rows(I32(n), ptr(f["kind"]), ptr(f["group"]), ptr(f["acc"]), ptr(f["slot"]), ptr(f["round"]),
                                     I32(0), C.byref(m), ptr(rs), ptr(rr), ptr(rb))
        t2 = time.perf_counter()
        assert st == 0
        st = L.fpx_proxy_phase2b(h, m, ptr(rs), ptr(rr), ptr(rb), ptr(ch), ptr(cr), ptr(cv))
        t3 = time.perf_counter()
        assert st == 0
        chosen = int(ch[:m.value].sum())
        if rep:
            times.append((t3 - t0) * 1e3)
            parts.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3])
assert chosen == S, chosen  # two votes of three acceptors, f = 1: every slot is chosen
res = dict(mode=args.mode, order=args.order, slots=S, messages=n, bytes=in_len, chosen=chosen,
           ms_median=float(np.median(times)), ms_min=float(np.min(times)), ms_all=[round(t, 3) for t in times])
if parts:
    res["ms_decode_rows_tally_median"] = [float(x) for x in np.median(np.array(parts), axis=0)]
print(json.dumps(res))
L.fpx_destroy(h)
