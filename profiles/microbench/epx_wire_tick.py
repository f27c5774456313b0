"""A leader's reply burst from wire bytes: the host parser in front of fpx_epx_leader_replies against the tick that decodes
on the device.  The numbers of profiles/epx_wire_tick.md.

    python profiles/microbench/epx_wire_tick.py                    (a), (b), (c) and the device-resident tick, one process
    python profiles/microbench/epx_wire_tick.py --mode decode      (c) alone: the run to put under rocprofv3 --kernel-trace --stats

The burst: n = 5, 2^18 led instances -- instance j is (j % 5, j / 5), led by its own leader in its default ballot, a Noop,
so no instance depends on another -- and the n - 1 = 4 PreAcceptOks of each, 2^20 serialised ReplicaInbound messages,
sender-major (all first answers, then all second, ...), in page-locked memory (fpx_host_alloc).  The fourth answer of an
instance arrives after its fast commit and is ignored.
  (a) fpx_wire_epaxos_decode_replica_inbound (one host thread) + the kind map + fpx_epx_leader_replies: the path the parent
      commit has, the yardstick
  (b) fpx_wire_epx_leader_tick: copy up, decode on the device, check, the same kernels, copy down
  (c) fpx_wire_epaxos_decode_replica_inbound_dev alone, the bytes already in HBM, every output array asked for
  (d) fpx_wire_epx_leader_tick_dev, the bytes already in HBM: what is left of (b) without the copy up
(a) and (b) are synchronous calls timed by the host clock, alternating, each on a fresh context with the instances led
(outside the timed region: a committed instance cannot be led again); (c) and (d) between two HIP events on the context's
stream, enqueue to fpx_epx_sync.  The median of --bursts after --warmup.  (a) and (b) must give the same outputs.  One JSON
line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
N = 5


def varint_len(v):
    return 1 + (v >= 128).astype(np.int64) + (v >= 16384).astype(np.int64)


def build_burst(leader, number, replica):
    """the serialised PreAcceptOk(instance (leader, number), ballot (0, leader), replica_index, sequence_number 0, n empty
    sets) of every message, back to back: (bytes, offsets).  Written with numpy -- a message differs from the next in four
    places -- and checked against the library's encoder by the caller"""
    m = len(leader)
    xl = varint_len(number)
    size = 41 + xl
    off = np.zeros(m + 1, np.int64)
    np.cumsum(size, out=off[1:])
    buf = np.zeros(int(off[-1]), np.uint8)
    deps = [0x2A, 2 + 4 * N, 0x08, N] + [0x12, 0x02, 0x08, 0x00] * N
    for k in (1, 2, 3):
        idx = np.flatnonzero(xl == k)
        if not len(idx):
            continue
        x = number[idx].astype(np.int64)
        xb = [(x >> (7 * j) & 0x7F) | (0x80 if j < k - 1 else 0) for j in range(k)]
        row = np.zeros((len(idx), 41 + k), np.uint8)
        cols = [0x1A, 39 + k, 0x0A, 3 + k, 0x08, leader[idx], 0x10] + xb + [0x12, 0x04, 0x08, 0x00, 0x10, leader[idx], 0x18,
                                                                              replica[idx], 0x20, 0x00] + deps
        assert len(cols) == 41 + k
        for c, v in enumerate(cols):
            row[:, c] = v
        buf[(off[idx][:, None] + np.arange(41 + k)[None, :]).reshape(-1)] = row.reshape(-1)
    return buf, off


class Cfg(C.Structure):
    _fields_ = [("num_replicas", C.c_int32), ("num_keys", C.c_int32), ("device", C.c_int32), ("flags", C.c_uint32),
                ("num_instances", C.c_int32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["all", "decode"], default="all")
    ap.add_argument("--instances", type=int, default=1 << 18)
    ap.add_argument("--bursts", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch  # the HIP runtime both sides share

    from frankenpaxos_amd import wire

    lib = wire._L()
    I = a.instances
    per = (I + N - 1) // N
    j = np.arange(I, dtype=np.int64)
    leader, number = (j % N).astype(np.int32), (j // N).astype(np.int32)
    m = (N - 1) * I
    to = np.tile(leader, N - 1)
    ridx = np.concatenate([(leader + 1 + k) % N for k in range(N - 1)]).astype(np.int32)
    buf, off = build_burst(to, np.tile(number, N - 1), ridx)
    for i in list(range(64)) + list(range(m - 64, m)) + [int(v) for v in np.linspace(0, m - 1, 64)]:
        want = wire.epaxos_encode(wire.EPX_PRE_ACCEPT_OK, (int(to[i]), int(number[i % I])), (0, int(to[i])),
                                  replica_index=int(ridx[i]), sequence_number=0, deps=[0] * N)
        assert buf[off[i]:off[i + 1]].tobytes() == want, i
    in_len = int(off[-1])

    def locked(arr):
        p = C.c_void_p()
        assert lib.fpx_host_alloc(max(arr.nbytes, 8), C.byref(p)) == 0
        C.memmove(p, arr.ctypes.data, arr.nbytes)
        return p

    h_buf, h_off, h_to = locked(buf), locked(off), locked(to)
    stream = torch.cuda.Stream()
    hp = lambda v: C.c_void_p(v.ctypes.data)
    dp = lambda t: C.c_void_p(t.data_ptr())
    zeros, noop, z8, tid = np.zeros(I, np.int32), np.full(I, -1, np.int32), np.zeros(I, np.uint8), np.arange(I, dtype=np.int32)

    def fresh(led=True):
        h = C.c_void_p()
        cfg = Cfg(N, 1, 0, 1, per)                       # FPX_EPX_F_LEADER_STATE
        assert lib.fpx_epx_create(C.byref(cfg), C.byref(h)) == 0
        assert lib.fpx_epx_set_stream(h, C.c_void_p(stream.cuda_stream)) == 0
        if led:
            assert lib.fpx_epx_lead(h, I, hp(leader), hp(number), hp(leader), hp(zeros), hp(noop), hp(z8), hp(tid), hp(z8), None,
                                    None) == 0
        return h

    i32 = lambda k: np.zeros(k, np.int32)
    outs = lambda: dict(outcome=i32(m), oseq=i32(m), odeps=i32(m * N), oend=i32(m), otr=i32(m), dec=i32(m), nd=i32(1))
    out_args = lambda o: [hp(o[k]) for k in ("outcome", "oseq", "odeps", "oend", "otr", "dec", "nd")]
    names = ["kind", "il", "in", "bo", "br", "ri", "seq", "vbo", "vbr", "status", "is_noop", "cmd_off", "cmd_len", "nr"]
    dec = {k: (np.zeros(m, np.int64) if k == "cmd_off" else i32(m)) for k in names}
    dec["wm"], dec["voff"] = i32(m * N), np.zeros(m + 1, np.int64)
    lut = np.full(32, -1, np.int32)
    lut[[wire.EPX_PRE_ACCEPT_OK, wire.EPX_ACCEPT_OK, wire.EPX_NACK]] = [0, 1, 2]
    t = dict(a_decode=[], a_call=[], a=[], b=[], c=[], d=[])
    res = {}
    with torch.cuda.stream(stream):
        d_buf = torch.from_numpy(buf).cuda()
        d_off = torch.from_numpy(off).cuda()
        d_to = torch.from_numpy(to).cuda()
        d_dec = [torch.zeros(m, dtype=torch.int64 if k == 11 else torch.int32, device="cuda") for k in range(14)]
        d_dec += [torch.zeros(m * N, dtype=torch.int32, device="cuda")] + [torch.zeros(m, dtype=torch.int32, device="cuda")
                                                                          for _ in range(2)]
        d_out = [torch.zeros(m * (N if k == 2 else 1), dtype=torch.int32, device="cuda") for k in range(6)]
        d_nd, d_bad = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
    stream.synchronize()

    def timed_dev(fn, h):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        assert fn() == 0
        assert lib.fpx_epx_sync(h) == 0
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for it in range(a.warmup + a.bursts):
        keep = it >= a.warmup
        if a.mode == "all":
            # (a) the host parser, then the call
            h = fresh()
            oa = outs()
            bad = C.c_int32(-1)
            t0 = time.perf_counter()
            st = lib.fpx_wire_epaxos_decode_replica_inbound(h_buf, in_len, h_off, m, N, *[hp(dec[k]) for k in names], hp(dec["wm"]),
                                                            hp(dec["voff"]), 0, None, None, C.byref(bad))
            assert st == 0 and dec["voff"][m] == 0           # (no explicit ids in this burst: every deps_values_end is 0)
            kind = lut[dec["kind"]]
            t1 = time.perf_counter()
            st = lib.fpx_epx_leader_replies(h, m, hp(kind), h_to, hp(dec["il"]), hp(dec["in"]), hp(dec["bo"]), hp(dec["br"]),
                                            hp(dec["ri"]), hp(dec["seq"]), hp(dec["wm"]), None, *out_args(oa))
            t2 = time.perf_counter()
            assert st == 0
            assert lib.fpx_epx_destroy(h) == 0
            # (b) the tick
            h = fresh()
            ob = outs()
            bad = C.c_int32(-9)
            t3 = time.perf_counter()
            st = lib.fpx_wire_epx_leader_tick(h, h_buf, in_len, h_off, m, h_to, *out_args(ob), C.byref(bad))
            t4 = time.perf_counter()
            assert st == 0 and bad.value == -1
            assert lib.fpx_epx_destroy(h) == 0
            for k in oa:
                assert (oa[k] == ob[k]).all(), k
            assert int(ob["nd"][0]) == I
            # (d) the tick with the bytes already in HBM
            h = fresh()
            ms_d = timed_dev(lambda: lib.fpx_wire_epx_leader_tick_dev(h, dp(d_buf), in_len, dp(d_off), m, dp(d_to),
                                                                      *[dp(x) for x in d_out], dp(d_nd), dp(d_bad)), h)
            assert int(d_nd.item()) == I and int(d_bad.item()) == -1
            assert lib.fpx_epx_destroy(h) == 0
            if keep:
                t["a_decode"].append((t1 - t0) * 1e3), t["a_call"].append((t2 - t1) * 1e3), t["a"].append((t2 - t0) * 1e3)
                t["b"].append((t4 - t3) * 1e3), t["d"].append(ms_d)
            oc = ob["outcome"]
            res = dict(decided=int(ob["nd"][0]), fast=int((oc == 3).sum()), ignored=int((oc == 0).sum()))
        # (c) the decode kernel alone
        h = fresh(led=False)
        ms_c = timed_dev(lambda: lib.fpx_wire_epaxos_decode_replica_inbound_dev(h, dp(d_buf), in_len, dp(d_off), m,
                                                                                *[dp(x) for x in d_dec], dp(d_bad)), h)
        assert int(d_bad.item()) == -1 and int(d_dec[16].min().item()) == 1 and int(d_dec[0].min().item()) == wire.EPX_PRE_ACCEPT_OK
        assert lib.fpx_epx_destroy(h) == 0
        if keep:
            t["c"].append(ms_c)
    out = dict(n=N, instances=I, messages=m, bytes=in_len, bytes_per_message=round(in_len / m, 2), bursts=a.bursts, **res)
    for k, v in t.items():
        if v:
            med = statistics.median(v)
            out[k] = dict(ms_median=round(med, 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3),
                          msgs_per_s=round(m / med * 1e3), bytes_per_s=round(in_len / med * 1e3))
    # what the decode kernel writes: 16 int32 and one int64 per message, and the watermark row
    out["decode_bytes_written_per_message"] = 16 * 4 + 8 + 4 * N
    print(json.dumps(out))


if __name__ == "__main__":
    main()
