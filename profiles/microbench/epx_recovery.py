"""Originating recovery at hosted EPaxos replicas: fpx_epx_recovery_replies_dev on a burst of PrepareOks, fpx_epx_recover and
fpx_epx_lead_accept on a batch of instances, and beside them fpx_epx_leader_replies_dev -- the closest burst there was: the
same sort, the same walk shape -- on a burst of PreAcceptOks over the same cells.  The numbers of profiles/epx_recovery.md.

    python profiles/microbench/epx_recovery.py --mode replies|leader_replies --log2m 16..20
    python profiles/microbench/epx_recovery.py --mode recover|lead_accept --log2m 16

The burst (seeded, n = 5, 1024 keys): m / 4 cells (at, leader, number < m / 8) of pairwise distinct instances, every message
on one of them (runs of 4 on average, interleaved), senders drawn at random.  replies: the cells are recovered first
(fpx_epx_recover, outside the timed region); statuses NotSeen : PreAccepted : Accepted = 2 : 2 : 1, a PreAccepted vote in
Ballot(0, leader), an Accepted one in (1, sender), triple ids of 2 values per cell, dependencies of a valid shape,
as_intended = 1 (the longer decision).  leader_replies: the cells are led first (fpx_epx_lead), the messages are PreAcceptOks
in the ballot led in.  Every round runs on a fresh context, created and prepared outside the timed region.  replies /
leader_replies: between two HIP events on the context's stream, enqueue to fpx_epx_sync.  recover / lead_accept (host
pointers only): the host clock around the call, copies included.  The median of --rounds after --warmup.  One JSON line.
Per-kernel times: run a mode under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
N, NUM_KEYS = 5, 1024


def make_cells(m, seed=1):
    rng = np.random.default_rng(seed)
    per = max(64, m // 8)
    cells = max(1, m // 4)
    flat = rng.choice(N * per, cells, replace=False)                  # pairwise distinct instances
    leader, number = (flat // per).astype(np.int32), (flat % per).astype(np.int32)
    at = rng.integers(0, N, cells).astype(np.int32)
    pick = rng.integers(0, cells, m)
    deps = rng.integers(0, per + 1, (m, N)).astype(np.int32)
    dend = np.zeros(m, np.int32)
    rows = np.arange(m)
    L, x = leader[pick], number[pick]
    explicit = rng.random(m) < 0.5                                    # the own-leader column: explicit ids above the instance ...
    deps[rows, L] = np.where(explicit, x, rng.integers(0, 1 << 30, m) % (x + 1))   # ... or a plain watermark
    dend[explicit] = x[explicit] + 2 + rng.integers(0, 3, int(explicit.sum()))
    return dict(rng=rng, per=per, cells=cells, leader=leader, number=number, at=at, pick=pick, deps=deps, dend=dend,
                key=rng.integers(0, NUM_KEYS, cells).astype(np.int32), is_set=rng.integers(0, 2, cells).astype(np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["replies", "leader_replies", "recover", "lead_accept"], required=True)
    ap.add_argument("--log2m", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import torch  # the HIP runtime both sides share

    from frankenpaxos_amd.epaxos import EPaxos

    m = 1 << a.log2m
    c = make_cells(m)
    rng, pick = c["rng"], c["pick"]
    ms, extra = [], {"messages": m}
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    stream = torch.cuda.Stream()
    fresh = lambda: EPaxos(N, NUM_KEYS, num_instances=c["per"], leader_state=True, recovery=True)
    if a.mode in ("recover", "lead_accept"):
        # a batch of m pairwise distinct instances, out of n * per with per = m / 4
        per = max(64, m // 4)
        flat = rng.choice(N * per, m, replace=False)
        leader, number = (flat // per).astype(np.int32), (flat % per).astype(np.int32)
        at = rng.integers(0, N, m).astype(np.int32)
        key, is_set = rng.integers(0, NUM_KEYS, m).astype(np.int32), rng.integers(0, 2, m).astype(np.uint8)
        deps = np.zeros((m, N), np.int32)
        for it in range(a.warmup + a.rounds):
            e = EPaxos(N, NUM_KEYS, num_instances=per, leader_state=True, recovery=True)
            t0 = time.perf_counter()
            if a.mode == "recover":
                st, outcome = e.recover(leader, number, at)[:2]
            else:
                st = e.lead_accept(leader, number, at, np.ones(m, np.int32), key, is_set, np.arange(m, dtype=np.int32), None, deps)
                outcome = np.zeros(1, np.int32)
            dt = (time.perf_counter() - t0) * 1e3
            assert st == 0, st
            if it >= a.warmup:
                ms.append(dt)
            e.close()
        extra["outcomes"] = {int(k): int(v) for k, v in zip(*np.unique(outcome, return_counts=True))}
    else:
        to, L, x = c["at"][pick], c["leader"][pick], c["number"][pick]
        q = rng.integers(0, N, m).astype(np.int32)
        status = rng.choice([0, 2, 3], m, p=[0.4, 0.4, 0.2]).astype(np.int32)
        vo = np.where(status == 0, -1, np.where(status == 2, 0, 1)).astype(np.int32)
        vr = np.where(status == 0, -1, np.where(status == 2, L, q)).astype(np.int32)
        tid = (pick * 2 + rng.integers(0, 2, m)).astype(np.int32)
        seq = np.zeros(m, np.int32)
        with torch.cuda.stream(stream):
            outs = [torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(7)]
            odeps = torch.zeros((m, N), dtype=torch.int32, device="cuda")
            nd = torch.zeros(1, dtype=torch.int32, device="cuda")
        for it in range(a.warmup + a.rounds):
            e = fresh()
            if a.mode == "replies":
                st, outcome, ord_ = e.recover(c["leader"], c["number"], c["at"])[:3]
                assert st == 0 and (outcome == 0).all()
                with torch.cuda.stream(stream):
                    d = [T(v) for v in (to, L, x, ord_[pick], to, q, status, vo, vr, tid, seq, c["deps"], c["dend"])]
            else:
                st = e.lead(c["leader"], c["number"], c["at"], np.zeros(c["cells"], np.int32), c["key"], c["is_set"],
                            np.arange(c["cells"], dtype=np.int32))[0]
                assert st == 0
                with torch.cuda.stream(stream):
                    d = [T(v) for v in (np.zeros(m, np.int32), to, L, x, np.zeros(m, np.int32), to, q, seq, c["deps"], c["dend"])]
            stream.synchronize()
            e.set_stream(stream.cuda_stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if a.mode == "replies":
                e.recovery_replies_dev(*d, as_intended=True, outcome=outs[0], out_source=outs[1], out_triple=outs[2],
                                       out_ballot=outs[3], out_seq=outs[4], out_deps=odeps, out_values_end=outs[5],
                                       decided_index=outs[6], num_decided=nd)
            else:
                e.leader_replies_dev(*d, outcome=outs[0], out_seq=outs[1], out_deps=odeps, out_values_end=outs[2],
                                     out_triple=outs[3], decided_index=outs[4], num_decided=nd)
            assert e.sync() == 0
            e1.record(stream)
            e1.synchronize()
            if it >= a.warmup:
                ms.append(e0.elapsed_time(e1))
            outcome = outs[0].cpu().numpy()
            extra["decided"] = int(nd.item())
            e.set_stream(None)
            e.close()
        extra["outcomes"] = {int(k): int(v) for k, v in zip(*np.unique(outcome, return_counts=True))}
    med = statistics.median(ms)
    print(json.dumps(dict(mode=a.mode, log2m=a.log2m, rounds=len(ms), ms_median=round(med, 4), ms_min=round(min(ms), 4),
                          ms_max=round(max(ms), 4), us_per_message=round(med * 1e3 / m, 4), **extra)))


if __name__ == "__main__":
    main()
