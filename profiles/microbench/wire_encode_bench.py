"""What does it cost to turn a tick's records back into wire bytes on the device?  The tick is r04_wire_decode.md's: n
canonical ProxyLeaderInbound{Phase2a} with 16-byte commands, all chosen (R = 3, f = 1).

  host_chosen     fpx_wire_encode_replica_chosen on one host thread: the C ABI has no batch form of it, so this is a python
                  loop over ctypes on a sample of the records, reported beside the rate of a call that writes nothing
  enc             fpx_wire_encode_replica_chosen_dev alone, records and bytes in HBM
  enc+d2h         ... plus the copy of the reply into page-locked memory
  to_records      copy up -> decode -> fused step, stopped at Chosen records   (r04_wire_decode.md row 4, re-measured)
  to_bytes        ... -> Chosen encode -> copy down, the same calls on the same stream
  tick            fpx_wire_phase2_tick on fpx_host_alloc buffers (synchronous, its own staging)
  p2b             fpx_wire_encode_phase2b_batch_dev against fpx_wire_encode_phase2b_batch on one thread: 2^20 x 3, 2^16 x 256

    python profiles/microbench/wire_encode_bench.py [log2 n]
Per-kernel times: rocprofv3 --kernel-trace --stats -- python profiles/microbench/wire_encode_bench.py  (a run of its own).
"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "profiles/microbench")
import frankenpaxos_amd as fa
from frankenpaxos_amd import wire
from frankenpaxos_amd.context import PinnedArray
from wire_decode_bench import tick, timed


def wall(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def main():
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n = 1 << lg
    buf, off, slot = tick(n)
    in_len = int(off[-1])
    dev = torch.device("cuda:0")
    gpu = fa.Context(fa.make_config(num_slots=n, num_replicas=3, f=1, flags=fa.FPX_F_TRUSTED))
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    res = {"n": n, "in_bytes": in_len}
    L = wire._L()

    d_buf, d_off = torch.from_numpy(buf).to(dev), torch.from_numpy(off).to(dev)
    d = gpu.wire_decode_dev("proxy_leader_inbound", d_buf, d_off)
    ch = torch.ones(n, dtype=torch.uint8, device=dev)
    out = torch.empty(in_len, dtype=torch.uint8, device=dev)
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    tot = torch.empty(2, dtype=torch.int64, device=dev)
    enc = lambda: gpu.wire_encode_chosen_dev(d["slot"], d["value_off"], d["value_len"], d_buf, emit=ch, is_noop=d["is_noop"],
                                             out=out, out_offsets=offs, totals=tot)
    enc()
    assert gpu.sync() == 0
    count, total = (int(x) for x in tot.cpu().numpy())
    assert count == n
    res["out_bytes"] = total
    # model bytes per message: record (emit 1 + slot 4 + is_noop 4 + value_off 8 + value_len 4) + value read, message + offset written
    res["model_bytes_per_message"] = 21 + 20 + total / n + 8
    o, of = out.cpu().numpy(), offs.cpu().numpy()
    voff, vlen = d["value_off"].cpu().numpy(), d["value_len"].cpu().numpy()

    # the host encoder on one thread, on a sample (python's call overhead measured beside it)
    sample = np.random.default_rng(2).integers(0, n, 200000)
    scratch = np.zeros(64, np.uint8)
    sp, bp = scratch.ctypes.data, buf.ctypes.data
    sl, vo, vl = slot.tolist(), voff.tolist(), vlen.tolist()
    t0 = time.perf_counter()
    for i in sample.tolist():
        L.fpx_wire_encode_replica_chosen(sp, 64, sl[i], bp + vo[i], vl[i], 0)
    t_host = (time.perf_counter() - t0) / len(sample)
    t0 = time.perf_counter()
    for i in sample.tolist():
        L.fpx_wire_encode_replica_chosen(None, 0, sl[i], bp + vo[i], vl[i], 0)   # sizes only: no byte written
    t_call = (time.perf_counter() - t0) / len(sample)
    res["host_chosen_per_s_incl_ctypes"], res["ctypes_call_per_s"] = 1 / t_host, 1 / t_call
    for i in sample[:64].tolist():   # and the device bytes are the host's
        k = L.fpx_wire_encode_replica_chosen(sp, 64, sl[i], bp + vo[i], vl[i], 0)
        assert o[of[i]:of[i + 1]].tobytes() == scratch[:k].tobytes()

    t = timed(enc, 20)
    res["enc_ms"], res["enc_msgs_per_s"], res["enc_model_GBs"] = t * 1e3, n / t, res["model_bytes_per_message"] * n / t / 1e9
    p_out = torch.empty(in_len, dtype=torch.uint8).pin_memory()
    p_offs = torch.empty(n + 1, dtype=torch.int64).pin_memory()

    def enc_down():
        enc()
        p_out[:total].copy_(out[:total], non_blocking=True)
        p_offs.copy_(offs, non_blocking=True)

    t = timed(enc_down, 10)
    res["enc_d2h_ms"], res["enc_d2h_msgs_per_s"] = t * 1e3, n / t

    p_buf, p_off = torch.from_numpy(buf).pin_memory(), torch.from_numpy(off).pin_memory()
    chz = torch.zeros(n, dtype=torch.uint8, device=dev)
    cv = torch.zeros(n, dtype=torch.int32, device=dev)
    p_ch, p_cv = torch.empty(n, dtype=torch.uint8).pin_memory(), torch.empty(n, dtype=torch.int32).pin_memory()

    def to_chosen():
        gpu.reset()
        d_buf.copy_(p_buf, non_blocking=True)
        d_off.copy_(p_off, non_blocking=True)
        dd = gpu.wire_decode_dev("proxy_leader_inbound", d_buf, d_off)
        gpu.phase2_fused_dev(dd["slot"], dd["round"], dd["value_id"], None, chz, None, cv)
        return dd

    def to_records():
        to_chosen()
        p_ch.copy_(chz, non_blocking=True)
        p_cv.copy_(cv, non_blocking=True)

    def to_bytes():
        dd = to_chosen()
        gpu.wire_encode_chosen_dev(dd["slot"], dd["value_off"], dd["value_len"], d_buf, emit=chz, is_noop=dd["is_noop"],
                                   out=out, out_offsets=offs, totals=tot)
        p_out[:total].copy_(out[:total], non_blocking=True)
        p_offs.copy_(offs, non_blocking=True)

    t = timed(to_records, 5)
    res["to_records_ms"], res["to_records_msgs_per_s"] = t * 1e3, n / t
    t = timed(to_bytes, 5)
    assert gpu.sync() == 0 and bool(chz.all())
    res["to_bytes_ms"], res["to_bytes_msgs_per_s"] = t * 1e3, n / t

    pin = [PinnedArray(in_len, np.uint8), PinnedArray(n + 1, np.int64), PinnedArray(in_len, np.uint8), PinnedArray(n + 1, np.int64)]
    pin[0].array[:], pin[1].array[:] = buf, off

    def tick_call():
        gpu.reset()
        st, c, need, bad = gpu.wire_phase2_tick(pin[0].array.ctypes.data, in_len, pin[1].array.ctypes.data, n,
                                                pin[2].array.ctypes.data, in_len, pin[3].array.ctypes.data)
        assert st == 0 and c == n

    t = wall(tick_call, 5)
    res["tick_ms"], res["tick_msgs_per_s"] = t * 1e3, n / t
    assert pin[2].array[:total].tobytes() == p_out[:total].numpy().tobytes()

    # Phase2b batches
    for m, R in ((1 << 20, 3), (1 << 16, 256)):
        s = np.arange(m, dtype=np.int32)
        r = np.zeros(m, np.int32)
        bits = np.zeros((m, 4), np.uint64)
        for w in range(4):
            k = min(64, max(0, R - 64 * w))
            bits[:, w] = np.uint64((1 << k) - 1 if k < 64 else 0xFFFFFFFFFFFFFFFF)
        msgs = m * R
        hb, ho = np.zeros(msgs * 16, np.uint8), np.zeros(msgs + 1, np.int64)
        t0 = time.perf_counter()
        k = L.fpx_wire_encode_phase2b_batch(m, s.ctypes.data, r.ctypes.data, bits.ctypes.data, None, 0, hb.ctypes.data, len(hb),
                                            ho.ctypes.data, msgs)
        th = time.perf_counter() - t0
        assert k == msgs
        ds, dr, db = torch.from_numpy(s).to(dev), torch.from_numpy(r).to(dev), torch.from_numpy(bits.view(np.int64)).to(dev)
        po = torch.empty(int(ho[k]), dtype=torch.uint8, device=dev)
        pf = torch.empty(msgs + 1, dtype=torch.int64, device=dev)
        f = lambda: gpu.wire_encode_phase2b_batch_dev(ds, dr, db, out=po, out_offsets=pf, totals=tot)
        f()
        assert gpu.sync() == 0 and po.cpu().numpy().tobytes() == hb[:ho[k]].tobytes() and (pf.cpu().numpy() == ho).all()
        t = timed(f, 10)
        key = "p2b_%dx%d" % (m, R)
        res[key + "_host_msgs_per_s"], res[key + "_dev_msgs_per_s"], res[key + "_dev_ms"] = msgs / th, msgs / t, t * 1e3
        res[key + "_dev_out_GBs"] = (int(ho[k]) + 8 * msgs) / t / 1e9
    print(json.dumps(res))


if __name__ == "__main__":
    main()
