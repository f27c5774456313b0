"""A Mencius replica's burst of Chosens and ChosenNoopRanges: fpx_replica_chosen_msgs_dev (one call) against what the
library had before it -- one fpx_replica_chosen_dev call for the Chosens and one fpx_replica_chosen_noop_range call per
range.  The numbers of profiles/replica_msgs.md.

    python profiles/replica_msgs_bench.py --mode new    [--lib libfpx.so] [--shape band|chosens] [--bursts 20]
    python profiles/replica_msgs_bench.py --mode parent --lib <libfpx.so built from the parent commit>

--mode parent uses only entry points the parent commit has, through plain ctypes, so that it runs on that commit's
library: the code under test is never its own yardstick.  Every burst starts from a fresh log (fpx_reset, outside the
timed region); the timed region is enqueue to sync, between two HIP events on the context's stream.  One JSON line.

shape band (config 5): S = 2^22, L = 256; leader groups 0 .. 127 send the Chosens of their 16 384 slots each, groups
128 .. 255 one ChosenNoopRange over theirs; the groups' batches back to back.  shape chosens: 2^20 Chosens, L = 1.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHOSEN, CHOSEN_NOOP_RANGE = 4, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["new", "parent"], required=True)
    ap.add_argument("--lib", default=os.path.join(ROOT, "frankenpaxos_amd", "csrc", "libfpx.so"))
    ap.add_argument("--shape", choices=["band", "chosens"], default="band")
    ap.add_argument("--bursts", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch  # the HIP runtime both sides share

    from frankenpaxos_amd._lib import FpxConfig

    L = C.CDLL(a.lib, mode=C.RTLD_GLOBAL)
    S = 1 << 22 if a.shape == "band" else 1 << 20
    G = 256 if a.shape == "band" else 1
    cfg = FpxConfig(S, 3, 1, G, 1, 0, 0, 0, 2, 0, 4, 0, 0, 0, 0)
    h = C.c_void_p()
    assert L.fpx_create(C.byref(cfg), C.byref(h)) == 0
    stream = torch.cuda.Stream()
    assert L.fpx_set_stream(h, C.c_void_p(stream.cuda_stream)) == 0

    rows = S // G
    if a.shape == "band":
        groups = G // 2
        c_slot = (np.arange(groups, dtype=np.int32)[:, None] + np.arange(rows, dtype=np.int32)[None, :] * G).reshape(-1)
        r_start = np.arange(groups, G, dtype=np.int32)
    else:
        c_slot = np.random.default_rng(1).permutation(S).astype(np.int32)
        r_start = np.zeros(0, np.int32)
    nc, nr = len(c_slot), len(r_start)
    c_value = (np.arange(nc, dtype=np.int64) * 2654435761 % (1 << 30)).astype(np.int32)
    kind = np.concatenate([np.full(nc, CHOSEN, np.int32), np.full(nr, CHOSEN_NOOP_RANGE, np.int32)])
    slot = np.concatenate([c_slot, r_start])
    end = np.concatenate([np.zeros(nc, np.int32), np.full(nr, S, np.int32)])
    value = np.concatenate([c_value, np.zeros(nr, np.int32)])
    with torch.cuda.stream(stream):
        d_kind, d_slot, d_end, d_value = (torch.from_numpy(x).cuda() for x in (kind, slot, end, value))
    stream.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    wm, num = C.c_int32(), C.c_int32()

    def burst():
        if a.mode == "new":
            assert L.fpx_replica_chosen_msgs_dev(h, nc + nr, p(d_kind), p(d_slot), p(d_end), p(d_value), None) == 0
        else:
            assert L.fpx_replica_chosen_dev(h, nc, p(d_slot), p(d_value), None) == 0
            for g in r_start.tolist():
                assert L.fpx_replica_chosen_noop_range(h, g, S, C.byref(wm), C.byref(num)) == 0
        assert L.fpx_sync(h) == 0

    ms, wall = [], []
    for it in range(a.warmup + a.bursts):
        assert L.fpx_reset(h) == 0 and L.fpx_sync(h) == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        burst()
        e1.record(stream)
        e1.synchronize()
        t1 = time.perf_counter()
        if it >= a.warmup:
            ms.append(e0.elapsed_time(e1)), wall.append((t1 - t0) * 1e3)
    assert L.fpx_replica_state(h, C.byref(wm), C.byref(num)) == 0
    # the byte model: per Chosen 12 B read (kind, slot, value) and 5 B written (log value and flag); per slot of a range
    # 5 B written
    positions = nr * rows
    model = nc * 17 + positions * 5
    med = statistics.median(ms)
    print(json.dumps(dict(mode=a.mode, shape=a.shape, lib=os.path.basename(a.lib), messages=nc + nr, chosens=nc, ranges=nr,
                          range_slots=positions, bursts=len(ms), ms_median=round(med, 4), ms_min=round(min(ms), 4),
                          ms_max=round(max(ms), 4), wall_ms_median=round(statistics.median(wall), 4),
                          model_bytes=model, gb_per_s=round(model / med / 1e6, 1),
                          executed_watermark=wm.value, num_chosen=num.value)))
    assert num.value == nc + positions and wm.value == (S if a.shape == "band" else nc)
    L.fpx_destroy(h)


if __name__ == "__main__":
    main()
