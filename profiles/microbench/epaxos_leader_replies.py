"""One burst of PreAcceptOks at hosted EPaxos leaders: fpx_epx_leader_replies_dev against the parent commit's only route to
the same decisions (the all-in-one-process fpx_epx_preaccept_dev tick, which does MORE work: it also runs the acceptors'
conflict scans) and against one host thread (tests/epaxos_leader_host_main.cpp, its BENCH op).  The numbers of
profiles/epaxos_leader_replies.md.

    python profiles/microbench/epaxos_leader_replies.py --mode replies [--slow-per-mille 10]
    python profiles/microbench/epaxos_leader_replies.py --mode tick [--lib <libfpx.so of the PARENT commit>]
    <the host program built from tests/epaxos_leader_host_main.cpp>  <<< "BENCH 1048576 10"

The burst: n = 5, 2^20 instances -- instance x is (x % 5, x / 5), led by its own leader in its default ballot, a Noop, so
no instance depends on another -- and the n - 2 = 3 PreAcceptOks of each, 3 * 2^20 messages, sender-major: all first
answers, then all second, then all third, so the three messages of an instance are 2^20 messages apart.  --slow-per-mille
s: the first answer of s in 1000 instances names one more dependency than the others (the slow path: the union, the
AcceptedEntry); the rest agree and commit on the fast path.
Every burst runs on a fresh context with the instances led (outside the timed region: a committed instance cannot be led
again); timed between two HIP events on the context's stream, enqueue to fpx_epx_sync.  The median of --bursts after
--warmup.  --mode tick uses only entry points the parent has, through plain ctypes.  One JSON line.  Per-kernel times: run
--mode replies under rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
N = 5


class Cfg(C.Structure):
    _fields_ = [("num_replicas", C.c_int32), ("num_keys", C.c_int32), ("device", C.c_int32), ("flags", C.c_uint32),
                ("num_instances", C.c_int32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["replies", "tick"], required=True)
    ap.add_argument("--lib", default=os.path.join(ROOT, "frankenpaxos_amd", "csrc", "libfpx.so"))
    ap.add_argument("--instances", type=int, default=1 << 20)
    ap.add_argument("--slow-per-mille", type=int, default=0)
    ap.add_argument("--bursts", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch  # the HIP runtime both sides share

    lib = C.CDLL(a.lib, mode=C.RTLD_GLOBAL)
    I = a.instances
    per = (I + N - 1) // N
    x = np.arange(I, dtype=np.int64)
    leader, number = (x % N).astype(np.int32), (x // N).astype(np.int32)
    stream = torch.cuda.Stream()
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda v: C.c_void_p(v.ctypes.data)
    ms, extra = [], {}
    if a.mode == "replies":
        slow = (x * 7919) % 1000 < a.slow_per_mille
        m = 3 * I
        kind = np.zeros(m, np.int32)
        to = np.tile(leader, 3)
        ridx = np.concatenate([(leader + 1 + k) % N for k in range(3)]).astype(np.int32)
        deps = np.zeros((m, N), np.int32)
        deps[np.flatnonzero(slow), ((x[slow] + 1) % N).astype(np.int64)] = 1
        with torch.cuda.stream(stream):
            d = [T(kind), T(to), T(np.tile(leader, 3)), T(np.tile(number, 3)), T(np.zeros(m, np.int32)), T(to), T(ridx),
                 T(np.zeros(m, np.int32)), T(deps), T(np.zeros(m, np.int32))]
            outs = [torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(5)]
            odeps = torch.zeros((m, N), dtype=torch.int32, device="cuda")
            nd = torch.zeros(1, dtype=torch.int32, device="cuda")
        stream.synchronize()
        zeros, noop = np.zeros(I, np.int32), np.full(I, -1, np.int32)
        z8 = np.zeros(I, np.uint8)
        tid = np.arange(I, dtype=np.int32)
        for it in range(a.warmup + a.bursts):
            h = C.c_void_p()
            cfg = Cfg(N, 1, 0, 1, per)                       # FPX_EPX_F_LEADER_STATE
            assert lib.fpx_epx_create(C.byref(cfg), C.byref(h)) == 0
            assert lib.fpx_epx_set_stream(h, C.c_void_p(stream.cuda_stream)) == 0
            assert lib.fpx_epx_lead(h, I, hp(leader), hp(number), hp(leader), hp(zeros), hp(noop), hp(z8), hp(tid), hp(z8), None,
                                    None) == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert lib.fpx_epx_leader_replies_dev(h, m, *(p(t) for t in d), p(outs[0]), p(outs[1]), p(odeps), p(outs[2]),
                                                  p(outs[3]), p(outs[4]), p(nd)) == 0
            assert lib.fpx_epx_sync(h) == 0
            e1.record(stream)
            e1.synchronize()
            if it >= a.warmup:
                ms.append(e0.elapsed_time(e1))
            if it == a.warmup + a.bursts - 1:
                oc = outs[0].cpu().numpy()
                extra = dict(decided=int(nd.item()), fast=int((oc == 3).sum()), accept=int((oc == 4).sum()),
                             waiting=int((oc == 1).sum()), timer=int((oc == 2).sum()))
                assert extra["decided"] == I and extra["accept"] == int(slow.sum()) and extra["fast"] == I - int(slow.sum())
                assert extra["waiting"] == I and extra["timer"] == I
                dec = outs[4][:I].cpu().numpy()
                assert (np.diff(dec) > 0).all() and dec[0] >= 2 * I
            assert lib.fpx_epx_destroy(h) == 0
        # what the burst must move at the least: the arrays in and out, and per instance its leader state and log entry
        in_b, out_b = (9 + N) * 4, (4 + N) * 4
        state_b = 2 * 16 + 9 + 3 * (N + 2) * 4 + (1 + 3 * 4 + N * 4 + 4)
        extra["bytes_min"] = m * (in_b + out_b) + I * (state_b + 4)
        extra["messages"] = m
    else:
        m = I
        key = np.arange(I, dtype=np.int32)                    # one key per command: conflict-free
        mask = np.zeros(I, np.uint8)
        for k in range(3):
            mask |= (1 << ((leader + 1 + k) % N)).astype(np.uint8)
        rank = np.tile(np.arange(I, dtype=np.int32), N)
        with torch.cuda.stream(stream):
            d = [T(leader), T(number), T(key), T(np.ones(I, np.uint8)), T(mask), None, T(rank), T(np.arange(I, dtype=np.int32))]
            fast = torch.zeros(I, dtype=torch.uint8, device="cuda")
            deps, ldeps = (torch.zeros((I, N), dtype=torch.int32, device="cuda") for _ in range(2))
            own = torch.zeros((I, 2), dtype=torch.int32, device="cuda")
        stream.synchronize()
        for it in range(a.warmup + a.bursts):
            h = C.c_void_p()
            cfg = Cfg(N, I, 0, 0, per)
            assert lib.fpx_epx_create(C.byref(cfg), C.byref(h)) == 0
            assert lib.fpx_epx_set_stream(h, C.c_void_p(stream.cuda_stream)) == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert lib.fpx_epx_preaccept_dev(h, I, *(p(t) for t in d), p(fast), p(deps), p(ldeps), p(own)) == 0
            assert lib.fpx_epx_sync(h) == 0
            e1.record(stream)
            e1.synchronize()
            if it >= a.warmup:
                ms.append(e0.elapsed_time(e1))
            assert lib.fpx_epx_destroy(h) == 0
        extra = dict(messages=m, fast=int(fast.sum().item()))
        assert extra["fast"] == I
    print(json.dumps(dict(mode=a.mode, lib=os.path.abspath(a.lib), instances=I, slow_per_mille=a.slow_per_mille, bursts=len(ms),
                          ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), **extra)))


if __name__ == "__main__":
    main()
