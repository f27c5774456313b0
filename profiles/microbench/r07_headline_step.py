"""the headline step (2^20 fresh slots x 256 acceptors, PER_SLOT, fused, device pointers) timed with HIP events, for
A/B runs and rocprofv3 passes (profiles/r07_ballot_summary.md).  Imports frankenpaxos_amd from the current directory, so
that the same script times another checkout: `cd <tree> && python <this file>`.  AB_WINDOWS, AB_STEPS: log windows, timed steps"""
import json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import torch
import frankenpaxos_amd as fa

N = 1 << 20
WIN = int(os.environ.get("AB_WINDOWS", "12"))
K = int(os.environ.get("AB_STEPS", "10"))
dev = torch.device("cuda:0")
ctx = fa.Context(fa.make_config(num_slots=WIN * N, num_replicas=256, f=127, quorum_kind=fa.FPX_Q_THRESHOLD,
                                ballot_mode=fa.FPX_BALLOT_PER_SLOT, tally_ways=4, device=0, flags=fa.FPX_F_TRUSTED))
stream = torch.cuda.current_stream()
ctx.set_stream(stream.cuda_stream)
assert ctx.acceptor_phase1a(0, 0)[0] == 0
ctx.flush_promises()
steps = []
for w in range(WIN):
    slot = torch.arange(w * N, (w + 1) * N, dtype=torch.int32, device=dev)
    val = (slot * 7 + 3).to(torch.int32)
    steps.append((slot, torch.zeros(N, dtype=torch.int32, device=dev), val, torch.zeros(N, dtype=torch.uint8, device=dev),
                  torch.full((N,), -7, dtype=torch.int32, device=dev), torch.full((N,), -7, dtype=torch.int32, device=dev)))
def step(i):
    s, r, v, ch, cr, cv = steps[i]
    ctx.phase2_fused_dev(s, r, v, None, ch, cr, cv)
W = 2
for i in range(W):
    step(i)
assert ctx.sync() == 0
torch.cuda.synchronize()
ctx.profile_enable(True)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for i in range(W, W + K):
    step(i)
e1.record()
torch.cuda.synchronize()
per = ctx.profile_read_launches()
assert ctx.sync() == 0
for i in range(W, W + K):
    s, r, v, ch, cr, cv = steps[i]
    assert bool(ch.all()) and bool((cv == v).all()) and bool((cr == 0).all()), "step %d not all chosen" % i
ms = e0.elapsed_time(e1) / K
out = {"ms_per_step": ms, "slots_per_s": N / (ms * 1e-3), "kernel_ms": float(sum(per)) / max(1, len(per)), "launches": len(per)}
if hasattr(ctx, "ballot_summary_audit"):
    out["audit"] = ctx.ballot_summary_audit()
print(json.dumps(out), flush=True)
ctx.close()
