"""A new leader's log from Phase1b messages: fpx_leader_phase1b_msgs_dev against what a caller had before it.

Setting (--shape headline, that of profiles/phase1_info.md): a 2^20 x 256 context, the lower half of the window voted by
every acceptor, the upper half by a thrifty run of f + 1 = 128 acceptors, watermark S / 4; the burst is the Phase1b of
those 128 acceptors, i.e. fpx_acceptor_phase1b_info_all_dev's output for them, left on the device.  --shape cfg5: 256
leader groups x 3 acceptors, leader group 0 recovers from f + 1 = 2 of its acceptors.  3 warm-ups, median of --reps:

  (a) fpx_leader_phase1b_msgs_dev, events on the context's stream: per call; with --one-call the script makes exactly one
      timed call and nothing else after the setup, for a kernel trace that gives the time per launch
  (b) the same fold by one host thread over the same arrays (numpy, one vectorised maximum per message on the key the
      kernel uses), the records already in host memory; and the time to bring them there
  (c) the floor: fpx_leader_phase1b_scan on the same votes and quorum inside the context (host call, wall clock)

Prints one JSON line (profiles/leader_phase1b.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import frankenpaxos_amd as fa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=["headline", "cfg5"], default="headline")
ap.add_argument("--log-slots", type=int, default=20)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--one-call", action="store_true")
args = ap.parse_args()
WARM = 0 if args.one_call else 3
REPS = 1 if args.one_call else args.reps
S = 1 << args.log_slots
dev = torch.device("cuda:0")

if args.shape == "headline":
    R, L = 256, 1
    cfg = fa.make_config(num_slots=S, num_replicas=R, f=127, ballot_mode=1)
else:
    R, L = 3, 256
    cfg = fa.make_config(num_slots=S, num_replicas=R, f=1, num_leader_groups=L, ballot_mode=1)
ctx = fa.Context(cfg)
ng, E, wm, f1, ROUND = L, L * R, S // 4, cfg.f + 1, 3

# the votes of profiles/microbench/phase1_info.py
slot = torch.arange(S, dtype=torch.int32, device=dev)
rnd = torch.zeros(S, dtype=torch.int32, device=dev)
tgt = np.zeros((S, 4), np.uint64)
for w in range(4):
    word = lambda n: np.uint64(sum(1 << k for k in range(64) if 64 * w + k < n))
    tgt[: S // 2, w] = word(R)
    tgt[S // 2:, w] = word(f1)
ch = torch.zeros(S, dtype=torch.uint8, device=dev)
cr, cv = torch.zeros_like(slot), torch.zeros_like(slot)
ctx.phase2_fused_dev(slot, rnd, slot, torch.from_numpy(tgt.view(np.int64)).to(dev), ch, cr, cv)
assert ctx.sync() == 0

# the quorum: acceptors 0 .. f of (leader) group 0; their Phase1b.info, left on the device
masks = np.zeros((ng, 4), np.uint64)
for a in range(f1):
    masks[0, a >> 6] |= np.uint64(1 << (a & 63))
tmask = torch.from_numpy(masks.view(np.int64)).to(dev)
off_h = ctx.acceptor_phase1b_info_all(wm, masks)[0]
total = int(off_h[-1])
d_off = torch.zeros(E + 1, dtype=torch.int64, device=dev)
d_rec = [torch.zeros(max(total, 1), dtype=torch.int32, device=dev) for _ in range(3)]
d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
ctx.acceptor_phase1b_info_all_dev(wm, tmask, total, d_off, d_rec[0], d_rec[1], d_rec[2], d_tot)
assert ctx.sync() == 0
e = torch.arange(E, device=dev)
grp, acc = (e // R).to(torch.int32), (e % R).to(torch.int32)
kind = torch.where((grp == 0) & (acc < f1), 9, 0).to(torch.int32)      # FPX_WIRE_PHASE1B for the quorum's entries
mround = torch.full_like(kind, ROUND)
hgroup = torch.zeros_like(kind)                                         # the acceptor group inside the leader's leader group
count = len(range(wm if L == 1 else -(-wm // L) * L, S, L))
result = torch.full((8,), -1, dtype=torch.int64, device=dev)
out = [torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(3)]

# (a)
stream = torch.cuda.Stream(device=dev)
ctx.set_stream(stream.cuda_stream)
ta = []
for rep in range(WARM + REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    ctx.leader_phase1b_msgs_dev(ROUND, wm, mround, acc, d_off, d_rec[0], d_rec[1], d_rec[2], result, kind=kind, group_index=hgroup,
                                cap=count, out_slot=out[0], safe_round=out[1], safe_value=out[2])
    e1.record(stream)
    e1.synchronize()
    if rep >= WARM:
        ta.append(e0.elapsed_time(e1))
assert ctx.sync() == 0
res = result.cpu().numpy()
assert res[0] == 1 and res[2] == count and res[3] == S - 1 - (S - 1) % L, res
ctx.set_stream(None)
got_round, got_value = out[1].cpu().numpy(), out[2].cpu().numpy()
med = lambda x: float(np.median(x))
line = dict(shape=args.shape, slots=S, replicas=R, leader_groups=L, watermark=wm, messages=int(kind.numel()), winners=f1,
            records=total, entries=count, a_call_ms_median=med(ta), a_call_ms_min=float(min(ta)),
            a_records_per_s=total / med(ta) * 1e3, reps=REPS)

if not args.one_call:
    # (b) one host thread, the records in host memory
    t0 = time.perf_counter()
    h_slot, h_vr, h_vv = (x.cpu().numpy() for x in d_rec)
    t_down = (time.perf_counter() - t0) * 1e3
    tb = []
    for rep in range(3):
        t0 = time.perf_counter()
        table = np.zeros(count, np.int64)
        first = int(res[3]) - (count - 1) * L              # the first output slot
        for a in range(f1):
            lo, hi = off_h[a], off_h[a + 1]
            s = h_slot[lo:hi]
            keep = (s >= first) & ((s - first) % L == 0)
            j = (s[keep] - first) // L
            key = ((h_vr[lo:hi][keep].astype(np.int64) + 1) << 8) | (255 - a)
            table[j] = np.maximum(table[j], key)                     # (slots of one message are distinct)
        sr = (table >> 8).astype(np.int32) - 1
        tb.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(sr, got_round)
    # (c) the in-context scan on the same votes
    tc = []
    for rep in range(WARM + min(REPS, 10)):
        t0 = time.perf_counter()
        st, mx, c_sr, c_sv = ctx.leader_phase1b_scan(wm, masks, S)
        t1 = time.perf_counter()
        assert st == 0
        if rep >= WARM:
            tc.append((t1 - t0) * 1e3)
    if L == 1:
        assert np.array_equal(c_sr, got_round) and np.array_equal(c_sv, got_value)
    line.update(b_host_fold_ms_median=med(tb), b_records_download_ms=t_down, c_scan_host_call_ms_median=med(tc),
                ratio_b_over_a=med(tb) / med(ta))
print(json.dumps(line))
ctx.close()
