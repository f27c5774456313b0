"""A MultiPaxos replica's burst of Chosens and reads: fpx_replica_inbox_dev against fpx_replica_chosen_msgs_dev (what the
added passes cost when there is nothing to schedule) and against handling the messages one at a time on one host thread
(replica_inbox_host.cpp, the shape of multipaxos/Replica.scala).  The numbers of profiles/replica_inbox.md.

    python profiles/microbench/replica_inbox.py --mode chosen-msgs [--lib <libfpx.so of the PARENT commit>]
    python profiles/microbench/replica_inbox.py --mode chosen-null | chosen-out | mixed
    python profiles/microbench/replica_inbox.py --mode mixed --dump burst.bin     (writes the burst for the host program)

--mode chosen-msgs uses only entry points the parent commit has, through plain ctypes, so that it runs on that commit's
library: the code under test is never its own yardstick.  2^20 slots; the burst is 2^20 Chosens in a shuffled order
(mixed: with 2^18 reads inserted at random positions, aimed at random slots, a tenth eventual).  Every burst starts
from a fresh log (fpx_reset, outside the timed region); the timed region is enqueue to sync, between two HIP events on
the context's stream; the median of --bursts runs after --warmup.  One JSON line.  Per-kernel times: run --mode mixed
under rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
CHOSEN, READ_REQUEST, EVENTUAL_READ_REQUEST = 4, 12, 14
S, NREADS = 1 << 20, 1 << 18


def make_burst(mixed):
    rng = np.random.default_rng(1)
    c_slot = rng.permutation(S).astype(np.int32)
    if not mixed:
        return np.full(S, CHOSEN, np.int32), c_slot, (np.arange(S, dtype=np.int64) * 2654435761 % (1 << 30)).astype(np.int32)
    n = S + NREADS
    is_read = np.zeros(n, bool)
    is_read[rng.choice(n, NREADS, replace=False)] = True
    kind = np.where(is_read, READ_REQUEST, CHOSEN).astype(np.int32)
    kind[is_read & (rng.random(n) < 0.1)] = EVENTUAL_READ_REQUEST
    slot = np.zeros(n, np.int32)
    slot[~is_read] = c_slot
    slot[is_read] = rng.integers(-1, S, NREADS)
    value = np.where(is_read, -1, np.arange(n) % (1 << 30)).astype(np.int32)
    return kind, slot, value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["chosen-msgs", "chosen-null", "chosen-out", "mixed"], required=True)
    ap.add_argument("--lib", default=os.path.join(ROOT, "frankenpaxos_amd", "csrc", "libfpx.so"))
    ap.add_argument("--bursts", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dump", help="write the burst (n, then kind, slot, value as int32) here and exit")
    a = ap.parse_args()
    kind, slot, value = make_burst(a.mode == "mixed")
    n = len(kind)
    if a.dump:
        with open(a.dump, "wb") as f:
            np.array([n, S], np.int32).tofile(f)
            for x in (kind, slot, value):
                x.tofile(f)
        return
    import torch  # the HIP runtime both sides share

    from frankenpaxos_amd._lib import FpxConfig

    L = C.CDLL(a.lib, mode=C.RTLD_GLOBAL)
    cfg = FpxConfig(S, 3, 1, 1, 1, 0, 0, 0, 2, 0, 4, 0, 0, 0, 0)
    h = C.c_void_p()
    assert L.fpx_create(C.byref(cfg), C.byref(h)) == 0
    stream = torch.cuda.Stream()
    assert L.fpx_set_stream(h, C.c_void_p(stream.cuda_stream)) == 0
    with torch.cuda.stream(stream):
        d_kind, d_slot, d_value = (torch.from_numpy(x).cuda() for x in (kind, slot, value))
        outs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)] + [torch.zeros(4, dtype=torch.int32, device="cuda")]
    stream.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())

    def burst():
        if a.mode == "chosen-msgs":
            assert L.fpx_replica_chosen_msgs_dev(h, n, p(d_kind), p(d_slot), p(d_slot), p(d_value), None) == 0
        elif a.mode == "chosen-null":
            assert L.fpx_replica_inbox_dev(h, n, p(d_kind), p(d_slot), p(d_value), None, None, None, None, None) == 0
        else:
            assert L.fpx_replica_inbox_dev(h, n, p(d_kind), p(d_slot), p(d_value), None, *[p(o) for o in outs]) == 0
        assert L.fpx_sync(h) == 0

    ms = []
    for it in range(a.warmup + a.bursts):
        assert L.fpx_reset(h) == 0 and L.fpx_sync(h) == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        burst()
        e1.record(stream)
        e1.synchronize()
        if it >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    wm, num = C.c_int32(), C.c_int32()
    assert L.fpx_replica_state(h, C.byref(wm), C.byref(num)) == 0
    assert (wm.value, num.value) == (S, S)
    out = dict(mode=a.mode, lib=os.path.abspath(a.lib), messages=n, bursts=len(ms), ms_median=round(statistics.median(ms), 4),
               ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))
    if a.mode in ("chosen-out", "mixed"):
        counts = outs[3].cpu().numpy()
        out["counts"] = counts.tolist()
        ec = outs[0].cpu().numpy()
        out["ran_at_once_or_released"] = int((ec >= 0).sum())
        assert counts[2] == 0 and counts[3] == S and counts[0] == (NREADS if a.mode == "mixed" else 0)
    print(json.dumps(out))
    L.fpx_destroy(h)


if __name__ == "__main__":
    main()
