"""One burst of peer messages at hosted EPaxos replicas: fpx_epx_replica_inbox[_dev] against the parent commit's only way to
handle the same messages -- the per-kind host calls (fpx_epx_handle_preaccept, fpx_epx_handle_commit, fpx_epx_prepare) over
maximal runs of consecutive messages of one kind with pairwise distinct instances.  Accepts are left out of BOTH sides: the
parent has no handleAccept at one replica.  The numbers of profiles/epx_replica_inbox.md.

    python profiles/microbench/epx_replica_inbox.py --mode inbox   --log2m 16|20 [--form host|dev]
    python profiles/microbench/epx_replica_inbox.py --mode perkind --log2m 16|20 [--limit K]   (the first K messages only)

The burst (seeded, n = 5, 1024 keys): the shape of tests/epaxos_inbox_streams.make_burst, vectorised -- m / 4 cells
(to, leader, number < m / 8) drawn at random, every message on one of them (runs of 4 on average, interleaved), kinds
PreAccept : Commit : Prepare = 40 : 10 : 25, ballots (0..3, 0..n-1), a tenth of the commands Noops, dependencies of a valid
shape (a third of the Commits by id).  Every round runs on a fresh context (outside the timed region).  --form dev: between
two HIP events on the context's stream, enqueue to fpx_epx_sync; --form host and --mode perkind: the host clock around
calls that each end in a synchronise.  The median of --rounds after --warmup.  One JSON line.  Per-kernel times: run
--mode inbox --form dev under rocprofv3 --kernel-trace --stats."""
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
N, NUM_KEYS = 5, 1024
PRE_ACCEPT, COMMIT, PREPARE = 0, 2, 3


def make_burst(m, seed=1):
    rng = np.random.default_rng(seed)
    per = max(64, m // 8)
    cells = max(1, m // 4)
    c_to, c_leader, c_number = rng.integers(0, N, cells), rng.integers(0, N, cells), rng.integers(0, per, cells)
    c_key = np.where(rng.random(cells) < 0.1, -1, rng.integers(0, NUM_KEYS, cells))
    c_set = rng.integers(0, 2, cells)
    pick = rng.integers(0, cells, m)
    kind = rng.choice([PRE_ACCEPT, COMMIT, PREPARE], m, p=[40 / 75, 10 / 75, 25 / 75]).astype(np.int32)
    to, leader, number = (v[pick].astype(np.int32) for v in (c_to, c_leader, c_number))
    key, is_set = c_key[pick].astype(np.int32), c_set[pick].astype(np.uint8)
    bo, br = rng.integers(0, 4, m).astype(np.int32), rng.integers(0, N, m).astype(np.int32)
    deps = rng.integers(0, per + 1, (m, N)).astype(np.int32)
    dend = np.zeros(m, np.int32)
    rows = np.arange(m)
    explicit = rng.random(m) < 0.5                            # the own-leader column: explicit ids above the instance ...
    deps[rows, leader] = np.where(explicit, number, rng.integers(0, 1 << 30, m) % (number + 1))   # ... or a plain watermark
    dend[explicit] = number[explicit] + 2 + rng.integers(0, 3, int(explicit.sum()))
    by_id = (kind == COMMIT) & (rng.random(m) < 0.3)
    return dict(kind=kind, to=to, leader=leader, number=number, bo=bo, br=br, key=key, is_set=is_set,
                triple=np.arange(m, dtype=np.int32), deps=deps, dend=dend, by_id=by_id, per=per)


def runs_of(b, limit):
    """maximal runs of consecutive messages of one kind with pairwise distinct instances: (first, end) pairs"""
    out, first, seen = [], 0, set()
    kind, inst = b["kind"], b["leader"].astype(np.int64) * (1 << 32) + b["number"]
    for i in range(limit):
        k = (int(inst[i]))
        if i > first and (kind[i] != kind[first] or k in seen or bool(b["by_id"][i]) != bool(b["by_id"][first])):
            out.append((first, i))
            first, seen = i, set()
        seen.add(k)
    if limit > first:
        out.append((first, limit))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["inbox", "perkind"], required=True)
    ap.add_argument("--form", choices=["host", "dev"], default="dev")
    ap.add_argument("--log2m", type=int, default=16)
    ap.add_argument("--limit", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import torch  # the HIP runtime both sides share

    from frankenpaxos_amd.epaxos import EPaxos

    m = 1 << a.log2m
    b = make_burst(m)
    deps_in = b["deps"].copy()
    deps_in[b["by_id"], 0] = -1
    ins = [b["kind"], b["to"], b["leader"], b["number"], b["bo"], b["br"], b["key"], b["is_set"], b["triple"], deps_in, b["dend"]]
    ms, extra = [], {}
    if a.mode == "inbox":
        stream = torch.cuda.Stream()
        T = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
        with torch.cuda.stream(stream):
            d = [T(v) for v in ins]
            outs = [torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(5)]
            odeps = torch.zeros((m, N), dtype=torch.int32, device="cuda")
        stream.synchronize()
        for it in range(a.warmup + a.rounds):
            e = EPaxos(N, NUM_KEYS, num_instances=b["per"])
            if a.form == "dev":
                e.set_stream(stream.cuda_stream)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                e.replica_inbox_dev(*d, outcome=outs[0], out_ballot=outs[1], out_status=outs[2], out_deps=odeps,
                                    out_values_end=outs[3], out_triple=outs[4])
                assert e.sync() == 0
                e1.record(stream)
                e1.synchronize()
                dt = e0.elapsed_time(e1)
                outcome = outs[0].cpu().numpy() if it == a.warmup + a.rounds - 1 else None
            else:
                t0 = time.perf_counter()
                res = e.replica_inbox(*ins)
                dt = (time.perf_counter() - t0) * 1e3
                assert res[0] == 0
                outcome = res[1]
            if it >= a.warmup:
                ms.append(dt)
            if outcome is not None:
                extra["outcomes"] = {int(k): int(v) for k, v in zip(*np.unique(outcome, return_counts=True))}
            e.close()
        extra["messages"] = m
    else:
        limit = a.limit or m
        runs = runs_of(b, limit)
        tgt = (1 << b["to"]).astype(np.uint8)
        for it in range(a.warmup + a.rounds):
            e = EPaxos(N, NUM_KEYS, num_instances=b["per"])
            t0 = time.perf_counter()
            for (s, z) in runs:
                k = int(b["kind"][s])
                sl = slice(s, z)
                if k == PRE_ACCEPT:
                    st = e.handle_preaccept(b["leader"][sl], b["number"][sl], b["bo"][sl], b["br"][sl], b["key"][sl], b["is_set"][sl],
                                            b["triple"][sl], b["deps"][sl], b["dend"][sl], tgt[sl])[0]
                elif k == COMMIT:
                    by_id = bool(b["by_id"][s])
                    st = e.handle_commit(b["leader"][sl], b["number"][sl], b["triple"][sl], tgt[sl], b["key"][sl], b["is_set"][sl],
                                         None if by_id else b["deps"][sl], None if by_id else b["dend"][sl])
                else:
                    st = e.prepare(b["leader"][sl], b["number"][sl], b["bo"][sl], b["br"][sl], tgt[sl])[0]
                assert st == 0, (s, z, k, st)
            dt = (time.perf_counter() - t0) * 1e3
            if it >= a.warmup:
                ms.append(dt)
            e.close()
        extra.update(messages=limit, calls=len(runs), mean_run=round(limit / len(runs), 3))
    med = statistics.median(ms)
    print(json.dumps(dict(mode=a.mode, form=a.form if a.mode == "inbox" else "host", log2m=a.log2m, rounds=len(ms),
                          ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                          us_per_message=round(med * 1e3 / extra["messages"], 4), **extra)))


if __name__ == "__main__":
    main()
