"""Times fpx_epx_preaccept_mk_packed_dev at 2^20 commands, n = 5, 1024 keys, with 1 / 2 / 4 distinct keys per command, next
to fpx_epx_preaccept_packed_dev on the same single-key tick.  Prints one JSON line per configuration (median of the timed
ticks: wall time from the call to fpx_epx_sync returning, on one warm context).  Run from the repository root:
    python profiles/microbench/epx_multikey.py [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from frankenpaxos_amd.epaxos import EPaxos  # noqa: E402
from tests.workloads import random_tick  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--m", type=int, default=1 << 20)
    a = ap.parse_args()
    n, num_keys, m = 5, 1024, a.m
    rng = np.random.default_rng(1)
    leader, number, key, is_set, mask, rank = random_tick(rng, n, num_keys, m, [0] * n, 64.0)
    T = lambda x, dt=torch.int32: torch.from_numpy(np.ascontiguousarray(x)).to(dt).cuda()
    dl, dn, ds, dm, dr = T(leader), T(number), T(is_set, torch.uint8), T(mask, torch.uint8), T(rank)
    packed = torch.zeros((m, 16), dtype=torch.int32, device="cuda")
    configs = [("single_key_packed_dev", 1, False), ("mk_1key", 1, True), ("mk_2keys", 2, True), ("mk_4keys", 4, True)]
    for name, c, mk_form in configs:
        off = T(np.arange(m + 1, dtype=np.int64) * c)
        keys = np.empty(m * c, np.int32)
        keys[0::c] = key
        for j in range(1, c):   # distinct extra keys
            keys[j::c] = (key + 97 * j) % num_keys
        dk = T(keys)
        times = []
        e = EPaxos(n, num_keys)   # no command log: every tick is the same work on a warm context
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mk_form:
                e.preaccept_mk_packed_dev(dl, dn, off, dk, ds, dm, dr, packed)
            else:
                e.preaccept_packed_dev(dl, dn, dk, ds, dm, dr, packed)
            assert e.sync() == 0
            if it >= a.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        e.close()
        med = float(np.median(times))
        print(json.dumps({"config": name, "m": m, "n": n, "keys_per_command": c, "median_ms": round(med, 4),
                          "min_ms": round(float(np.min(times)), 4), "ns_per_command": round(med * 1e6 / m, 3)}), flush=True)


if __name__ == "__main__":
    main()
