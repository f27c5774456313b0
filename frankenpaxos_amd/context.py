"""Context: a Python handle on one libfpx context (= the acceptor groups + one proxy leader of
SURVEY.md section 8 living in the HBM of one MI355X).

Host-pointer methods take / return numpy arrays and accept any batch; `*_dev` methods take torch
CUDA tensors (already resident in HBM), enqueue on the context's stream and return immediately.
Every method ends up in a HIP kernel; nothing here computes protocol results on the CPU.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FpxConfig, FpxError


def make_config(num_slots, num_replicas, num_groups=1, num_leader_groups=1, f=0,
                quorum_kind=_lib.FPX_Q_THRESHOLD, grid_rows=0, grid_cols=0, num_leaders=2,
                ballot_mode=_lib.FPX_BALLOT_ACCEPTOR, tally_ways=4, replica_base=0, replicas_total=0,
                device=0, flags=0):
    return FpxConfig(num_slots, num_replicas, num_groups, num_leader_groups, f, quorum_kind,
                     grid_rows, grid_cols, num_leaders, ballot_mode, tally_ways, replica_base,
                     replicas_total, device, flags)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def _u64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint64)


def _hp(a):
    return None if a is None else a.ctypes.data


def _dp(t):
    """device pointer of a torch tensor (or None)"""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device entry points take contiguous CUDA tensors"
    return t.data_ptr()


class Context:
    def __init__(self, cfg):
        self.L = _lib.lib()
        self.cfg = cfg
        st = self.L.fpx_config_check(C.byref(cfg))
        if st:
            raise FpxError(st, "fpx_config_check")
        h = C.c_void_p()
        st = self.L.fpx_create(C.byref(cfg), C.byref(h))
        if st:
            raise FpxError(st, "fpx_create")
        self._h = h
        self.S, self.R = cfg.num_slots, cfg.num_replicas
        self.ngroups = cfg.num_groups * cfg.num_leader_groups

    def close(self):
        if getattr(self, "_h", None):
            self.L.fpx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- lifecycle -------------------------------------------------------------------------
    def reset(self):
        st = self.L.fpx_reset(self._h)
        if st:
            raise FpxError(st, "fpx_reset")

    def set_stream(self, hip_stream):
        """hip_stream: integer hipStream_t, e.g. torch.cuda.current_stream().cuda_stream (0 = the
        device's default stream); None selects the context's private stream (FPX_STREAM_OWN)"""
        st = self.L.fpx_set_stream(self._h, C.c_void_p(-1 if hip_stream is None else int(hip_stream)))
        if st:
            raise FpxError(st, "fpx_set_stream")

    def sync(self):
        """waits for the stream; returns the sticky device status of the _dev calls"""
        return self.L.fpx_sync(self._h)

    def error_detail(self):
        i, s, r = C.c_int32(), C.c_int32(), C.c_int32()
        self.L.fpx_error_detail(self._h, C.byref(i), C.byref(s), C.byref(r))
        return i.value, s.value, r.value

    def profile_enable(self, on=True):
        st = self.L.fpx_profile_enable(self._h, int(on))
        if st:
            raise FpxError(st, "fpx_profile_enable")

    def profile_read(self):
        """(launches, total_ms) of the dominant kernel since the last read (HIP events on the stream)"""
        n, ms = C.c_int32(), C.c_double()
        st = self.L.fpx_profile_read(self._h, C.byref(n), C.byref(ms))
        if st:
            raise FpxError(st, "fpx_profile_read")
        return n.value, ms.value

    def profile_read_launches(self, cap=4096):
        """durations in ms of the timed launches since the last read, in launch order"""
        out = (C.c_float * cap)()
        n = C.c_int32()
        st = self.L.fpx_profile_read_launches(self._h, cap, out, C.byref(n))
        if st:
            raise FpxError(st, "fpx_profile_read_launches")
        return [float(out[i]) for i in range(min(cap, n.value))]

    @property
    def device_bytes(self):
        return self.L.fpx_device_bytes(self._h)

    def acceptor_max_voted_in(self, group, replica, first_slot=0, count=None):
        """Acceptor.maxVotedSlot over the slots [first_slot, first_slot + count) of the acceptor's group (-1: no vote there)"""
        out = C.c_int32(-1)
        st = self.L.fpx_acceptor_max_voted_in(self._h, group, replica, first_slot, self.cfg.num_slots - first_slot if count is None else count,
                                              C.byref(out))
        if st:
            raise FpxError(st, "fpx_acceptor_max_voted_in")
        return out.value

    def placement_stats(self):
        """how fpx_create placed the cell arrays: {"chunks": bool, "windows": n, "probe_ms": (min, median, max)}"""
        out = (C.c_float * 5)()
        st = self.L.fpx_placement_stats(self._h, out)
        if st:
            raise FpxError(st, "fpx_placement_stats")
        pr, un, ms = C.c_int32(0), C.c_int32(0), C.c_float(0)
        st = self.L.fpx_placement_search(self._h, C.byref(pr), C.byref(un), C.byref(ms))
        if st:
            raise FpxError(st, "fpx_placement_search")
        return {"chunks": bool(out[0]), "windows": int(out[1]), "probe_ms": (float(out[2]), float(out[3]), float(out[4])),
                "search": {"probes": pr.value, "unprobed_decisions": un.value, "ms": float(ms.value)}}

    def deferred_folds(self):
        """diagnostic: fused steps whose launch carried the fold of the step before (include/fpx.h)"""
        return int(self.L.fpx_deferred_folds(self._h))

    def band_merged_steps(self):
        """diagnostic: the mencius_band_fused_dev steps that ran in the two-launch form"""
        return int(self.L.fpx_band_merged_steps(self._h))

    def vote_launch_census(self):
        """diagnostic: the vote launches since the context was created (include/fpx.h, fpx_vote_launch_census) --
        {"cells": {(G, mode, ps, fused, form): count} with the non-zero cells only, "capped": n, "sc_lds": n, "th_lds": n};
        form is one of _lib.CENSUS_FORMS"""
        out = (C.c_int64 * _lib.CENSUS_WORDS)()
        n = C.c_int32(0)
        st = self.L.fpx_vote_launch_census(self._h, _lib.CENSUS_WORDS, out, C.byref(n))
        if st:
            raise FpxError(st, "fpx_vote_launch_census")
        assert n.value == _lib.CENSUS_WORDS, "include/fpx.h and _lib.CENSUS_WORDS disagree"
        nf = len(_lib.CENSUS_FORMS)
        cells = {}
        for k in range(_lib.CENSUS_CELLS * nf):
            if out[k]:
                cell, form = divmod(k, nf)
                rest, fused = divmod(cell, 2)
                rest, ps = divmod(rest, 3)
                g_log2, mode = divmod(rest, 4)
                cells[(1 << g_log2, mode, ps, fused, _lib.CENSUS_FORMS[form])] = int(out[k])
        base = _lib.CENSUS_CELLS * nf
        return {"cells": cells, "capped": int(out[base]), "sc_lds": int(out[base + 1]), "th_lds": int(out[base + 2])}

    def range_launch_census(self):
        """diagnostic: the noop-range launches since the context was created (include/fpx.h, fpx_range_launch_census) --
        {form: count} over every form of _lib.RANGE_CENSUS_FORMS, zeros included"""
        nw = len(_lib.RANGE_CENSUS_FORMS)
        out = (C.c_int64 * nw)()
        n = C.c_int32(0)
        st = self.L.fpx_range_launch_census(self._h, out, nw, C.byref(n))
        if st:
            raise FpxError(st, "fpx_range_launch_census")
        assert n.value == nw, "include/fpx.h and _lib.RANGE_CENSUS_FORMS disagree"
        return {name: int(out[k]) for k, name in enumerate(_lib.RANGE_CENSUS_FORMS)}

    # ---- host-pointer entry points (numpy) ---------------------------------------------------
    def acceptor_phase2a(self, slot, round_, value, target_mask=None):
        slot, round_, value, target_mask = _i32(slot), _i32(round_), _i32(value), _u64(target_mask)
        n = len(slot)
        vb = np.zeros((n, 4), np.uint64)
        nb = np.zeros((n, 4), np.uint64)
        nr = np.zeros(n, np.int32)
        st = self.L.fpx_acceptor_phase2a(self._h, n, _hp(slot), _hp(round_), _hp(value),
                                         _hp(target_mask), _hp(vb), _hp(nb), _hp(nr))
        return st, vb, nb, nr

    def acceptor_phase1a(self, group, round_, watermark=0, target_mask=None):
        target_mask = _u64(target_mask)
        pb = np.zeros(4, np.uint64)
        nb = np.zeros(4, np.uint64)
        st = self.L.fpx_acceptor_phase1a(self._h, group, round_, watermark, _hp(target_mask),
                                         _hp(pb), _hp(nb))
        return st, pb, nb

    def acceptor_phase1a_dev(self, group, round_, watermark=0, target_mask=None, promised_bits=None,
                             nack_bits=None):
        """asynchronous Phase1a: torch CUDA tensors of 4 int64 words each (or None)"""
        st = self.L.fpx_acceptor_phase1a_dev(self._h, group, round_, watermark, _dp(target_mask),
                                             _dp(promised_bits), _dp(nack_bits))
        if st:
            raise FpxError(st, "fpx_acceptor_phase1a_dev")

    def flush_promises(self):
        st = self.L.fpx_acceptor_flush_promises(self._h)
        if st:
            raise FpxError(st, "fpx_acceptor_flush_promises")

    def proxy_open(self, slot, round_, value):
        slot, round_, value = _i32(slot), _i32(round_), _i32(value)
        n = len(slot)
        new = np.zeros(n, np.uint8)
        st = self.L.fpx_proxy_open(self._h, n, _hp(slot), _hp(round_), _hp(value), _hp(new))
        return st, new

    def proxy_phase2b(self, slot, round_, vote_bits):
        slot, round_, vote_bits = _i32(slot), _i32(round_), _u64(vote_bits)
        n = len(slot)
        ch = np.zeros(n, np.uint8)
        cr = np.zeros(n, np.int32)
        cv = np.zeros(n, np.int32)
        st = self.L.fpx_proxy_phase2b(self._h, n, _hp(slot), _hp(round_), _hp(vote_bits), _hp(ch),
                                      _hp(cr), _hp(cv))
        return st, ch, cr, cv

    def proxy_phase2b_msgs(self, acceptor_index, slot, round_, kind=None, group_index=None, grid_cols=0):
        """one Phase2b per (acceptor, slot), any order, duplicates allowed: = wire.phase2b_rows + proxy_phase2b, each
        row's outcome at the index of its first message (kind None: all are Phase2bs; group_index None: 0)"""
        acceptor_index, slot, round_ = _i32(acceptor_index), _i32(slot), _i32(round_)
        kind, group_index = _i32(kind), _i32(group_index)
        n = len(slot)
        ch = np.zeros(n, np.uint8)
        cr = np.zeros(n, np.int32)
        cv = np.zeros(n, np.int32)
        st = self.L.fpx_proxy_phase2b_msgs(self._h, n, _hp(kind), _hp(group_index), _hp(acceptor_index), _hp(slot),
                                           _hp(round_), grid_cols, _hp(ch), _hp(cr), _hp(cv))
        return st, ch, cr, cv

    def acceptor_inbox(self, kind, acceptor_index, slot, round_, value, group_index=None, grid_cols=0, replies=True):
        """a burst of AcceptorInbound messages in delivery order (kinds of frankenpaxos_amd.wire), each delivered to acceptor
        (group_index, acceptor_index) of this context, exactly as multipaxos.Acceptor handles them one by one:
        (status, reply_kind, reply_value).  group_index None: 0; replies False: both outputs NULL (returned as None)"""
        kind, acceptor_index, slot = _i32(kind), _i32(acceptor_index), _i32(slot)
        round_, value, group_index = _i32(round_), _i32(value), _i32(group_index)
        n = len(kind)
        assert len(acceptor_index) == len(slot) == len(round_) == len(value) == n
        rk = np.full(n, -9, np.int32) if replies else None
        rv = np.full(n, -9, np.int32) if replies else None
        st = self.L.fpx_acceptor_inbox(self._h, n, _hp(kind), _hp(group_index), _hp(acceptor_index), _hp(slot), _hp(round_),
                                       _hp(value), grid_cols, _hp(rk), _hp(rv))
        return st, rk, rv

    def mencius_acceptor_inbox(self, kind, acceptor_index, slot, slot_end, round_, value, group_index=None, replies=True):
        """a burst of Mencius AcceptorInbound messages in delivery order (Phase2a, Phase2aNoopRange with slot = start and
        slot_end = end, Phase1a), each delivered to acceptor acceptor_index of row group_index = leader_group * num_groups +
        acceptor_group, exactly as mencius.Acceptor handles them one by one: (status, reply_kind, reply_value).
        group_index None: 0; replies False: both outputs NULL (returned as None)"""
        kind, acceptor_index, slot, slot_end = _i32(kind), _i32(acceptor_index), _i32(slot), _i32(slot_end)
        round_, value, group_index = _i32(round_), _i32(value), _i32(group_index)
        n = len(kind)
        assert len(acceptor_index) == len(slot) == len(slot_end) == len(round_) == len(value) == n
        rk = np.full(n, -9, np.int32) if replies else None
        rv = np.full(n, -9, np.int32) if replies else None
        st = self.L.fpx_mencius_acceptor_inbox(self._h, n, _hp(kind), _hp(group_index), _hp(acceptor_index), _hp(slot),
                                               _hp(slot_end), _hp(round_), _hp(value), _hp(rk), _hp(rv))
        return st, rk, rv

    def mencius_acceptor_inbox_dev(self, kind, acceptor_index, slot, slot_end, round_, value, group_index=None,
                                   reply_kind=None, reply_value=None, n=None):
        """the same on device tensors (int32; either output may be None); errors surface at sync()"""
        st = self.L.fpx_mencius_acceptor_inbox_dev(self._h, kind.numel() if n is None else n, _dp(kind), _dp(group_index),
                                                   _dp(acceptor_index), _dp(slot), _dp(slot_end), _dp(round_), _dp(value),
                                                   _dp(reply_kind), _dp(reply_value))
        if st:
            raise FpxError(st, "fpx_mencius_acceptor_inbox_dev")

    def mencius_proxy_phase2b_msgs(self, acceptor_index, slot, round_, kind=None, group_index=None, slot_end=None):
        """one Phase2b / Phase2bNoopRange per (acceptor, key) in delivery order (mencius/ProxyLeader.scala:305-411): = the
        burst folded into rows + proxy_phase2b / proxy_phase2b_noop_ranges, each row's outcome at the index of its first
        message (kind None: all are Phase2bs; group_index None: 0; slot_end None: no range message)"""
        acceptor_index, slot, round_ = _i32(acceptor_index), _i32(slot), _i32(round_)
        kind, group_index, slot_end = _i32(kind), _i32(group_index), _i32(slot_end)
        n = len(slot)
        ch = np.zeros(n, np.uint8)
        cr = np.zeros(n, np.int32)
        cv = np.zeros(n, np.int32)
        st = self.L.fpx_mencius_proxy_phase2b_msgs(self._h, n, _hp(kind), _hp(group_index), _hp(acceptor_index),
                                                   _hp(slot), _hp(slot_end), _hp(round_), _hp(ch), _hp(cr), _hp(cv))
        return st, ch, cr, cv

    def mencius_phase2b_tick(self, acceptor_index, slot, round_, kind=None, group_index=None, slot_end=None, out_cap=None):
        """fpx_mencius_phase2b_tick: (status, count, records) with records = the first min(count, out_cap) newly chosen
        (kind, slot, slot_end or -1, round, value id or -1) in message order; the status is returned, not raised --
        FPX_ECAPACITY (count = the capacity needed) is an answer here.  out_cap None: n."""
        acceptor_index, slot, round_ = _i32(acceptor_index), _i32(slot), _i32(round_)
        kind, group_index, slot_end = _i32(kind), _i32(group_index), _i32(slot_end)
        n = len(slot)
        cap = n if out_cap is None else int(out_cap)
        outs = [np.full(max(cap, 1), -77, np.int32) for _ in range(5)]
        count = C.c_int32(0)
        st = self.L.fpx_mencius_phase2b_tick(self._h, n, _hp(kind), _hp(group_index), _hp(acceptor_index), _hp(slot),
                                             _hp(slot_end), _hp(round_), *[_hp(o) for o in outs], cap, C.byref(count))
        k = min(count.value, cap)
        return st, count.value, list(zip(*[o[:k].tolist() for o in outs]))

    def phase2_fused(self, slot, round_, value, target_mask=None):
        slot, round_, value, target_mask = _i32(slot), _i32(round_), _i32(value), _u64(target_mask)
        n = len(slot)
        ch = np.zeros(n, np.uint8)
        cr = np.zeros(n, np.int32)
        cv = np.zeros(n, np.int32)
        nr = np.zeros(n, np.int32)
        st = self.L.fpx_phase2_fused(self._h, n, _hp(slot), _hp(round_), _hp(value),
                                     _hp(target_mask), _hp(ch), _hp(cr), _hp(cv), _hp(nr))
        return st, ch, cr, cv, nr

    # ---- device-pointer entry points (torch CUDA tensors, async) ------------------------------
    def acceptor_phase2a_dev(self, slot, round_, value, target_mask=None, vote_bits=None,
                             nack_bits=None, nack_round=None):
        st = self.L.fpx_acceptor_phase2a_dev(self._h, slot.numel(), _dp(slot), _dp(round_),
                                             _dp(value), _dp(target_mask), _dp(vote_bits),
                                             _dp(nack_bits), _dp(nack_round))
        if st:
            raise FpxError(st, "fpx_acceptor_phase2a_dev")

    def proxy_open_dev(self, slot, round_, value, is_new=None):
        st = self.L.fpx_proxy_open_dev(self._h, slot.numel(), _dp(slot), _dp(round_), _dp(value),
                                       _dp(is_new))
        if st:
            raise FpxError(st, "fpx_proxy_open_dev")

    def proxy_phase2b_dev(self, slot, round_, vote_bits, newly_chosen=None, chosen_round=None,
                          chosen_value=None):
        st = self.L.fpx_proxy_phase2b_dev(self._h, slot.numel(), _dp(slot), _dp(round_),
                                          _dp(vote_bits), _dp(newly_chosen), _dp(chosen_round),
                                          _dp(chosen_value))
        if st:
            raise FpxError(st, "fpx_proxy_phase2b_dev")

    def proxy_phase2b_msgs_dev(self, acceptor_index, slot, round_, kind=None, group_index=None, grid_cols=0,
                               newly_chosen=None, chosen_round=None, chosen_value=None):
        st = self.L.fpx_proxy_phase2b_msgs_dev(self._h, slot.numel(), _dp(kind), _dp(group_index), _dp(acceptor_index),
                                               _dp(slot), _dp(round_), grid_cols, _dp(newly_chosen), _dp(chosen_round),
                                               _dp(chosen_value))
        if st:
            raise FpxError(st, "fpx_proxy_phase2b_msgs_dev")

    def acceptor_inbox_dev(self, kind, acceptor_index, slot, round_, value, group_index=None, grid_cols=0, reply_kind=None,
                           reply_value=None, n=None):
        """the same on device tensors (int32; either output may be None); errors surface at sync()"""
        st = self.L.fpx_acceptor_inbox_dev(self._h, kind.numel() if n is None else n, _dp(kind), _dp(group_index),
                                           _dp(acceptor_index), _dp(slot), _dp(round_), _dp(value), grid_cols,
                                           _dp(reply_kind), _dp(reply_value))
        if st:
            raise FpxError(st, "fpx_acceptor_inbox_dev")

    def mencius_proxy_phase2b_msgs_dev(self, acceptor_index, slot, round_, kind=None, group_index=None, slot_end=None,
                                       newly_chosen=None, chosen_round=None, chosen_value=None):
        st = self.L.fpx_mencius_proxy_phase2b_msgs_dev(self._h, slot.numel(), _dp(kind), _dp(group_index),
                                                       _dp(acceptor_index), _dp(slot), _dp(slot_end), _dp(round_),
                                                       _dp(newly_chosen), _dp(chosen_round), _dp(chosen_value))
        if st:
            raise FpxError(st, "fpx_mencius_proxy_phase2b_msgs_dev")

    def phase2_fused_dev(self, slot, round_, value, target_mask=None, chosen=None, chosen_round=None,
                         chosen_value=None, nack_round=None):
        st = self.L.fpx_phase2_fused_dev(self._h, slot.numel(), _dp(slot), _dp(round_), _dp(value),
                                         _dp(target_mask), _dp(chosen), _dp(chosen_round),
                                         _dp(chosen_value), _dp(nack_round))
        if st:
            raise FpxError(st, "fpx_phase2_fused_dev")

    # ---- the wire adapter on the device (include/fpx_wire.h) -------------------------------------------
    def wire_decode_dev(self, which, buf, offsets, value_id_base=0, buf_len=None):
        """which = "proxy_leader_inbound" | "acceptor_inbound"; buf: uint8 CUDA tensor holding the tick's messages back
        to back, offsets: int64 CUDA tensor [n + 1].  Returns a dict of CUDA tensors (the SoA batch), enqueued on the
        context's stream; errors surface at sync() like every _dev call."""
        import torch
        n = offsets.numel() - 1
        names = ["kind", "slot", "round", "is_noop", "value_off", "value_len"] + \
            (["group_index", "acceptor_index"] if which == "proxy_leader_inbound" else ["chosen_watermark"]) + ["value_id"]
        out = {k: torch.empty(max(n, 1), dtype=torch.int64 if k == "value_off" else torch.int32, device=buf.device)[:n]
               for k in names}
        from . import wire
        fn = getattr(wire._L(), "fpx_wire_decode_%s_dev" % which)
        st = fn(self._h, _dp(buf), buf.numel() if buf_len is None else buf_len, _dp(offsets), n,
                *[out[k].data_ptr() for k in names[:-1]], value_id_base, out["value_id"].data_ptr())
        if st:
            raise FpxError(st, "fpx_wire_decode_%s_dev" % which)
        return out

    def _wire_encode_out(self, device, cap, max_msgs, out, out_offsets, totals):
        import torch
        if out is None:
            out = torch.empty(max(int(cap), 1), dtype=torch.uint8, device=device)
        if out_offsets is None:
            out_offsets = torch.empty(int(max_msgs) + 1, dtype=torch.int64, device=device)
        if totals is None:
            totals = torch.empty(2, dtype=torch.int64, device=device)
        return out, out_offsets, totals

    def wire_encode_chosen_dev(self, slot, value_off, value_len, values, emit=None, is_noop=None, cap=None, out=None,
                               out_offsets=None, totals=None, values_len=None):
        """ReplicaInbound{Chosen} of every record with emit[i] != 0 (None: all), back to back: slot / value_len int32,
        value_off int64, is_noop int32, emit uint8 CUDA tensors as wire_decode_dev and phase2_fused_dev leave them; values =
        the tick's bytes (uint8 CUDA tensor).  Returns CUDA tensors (out, out_offsets[n + 1], totals[2] = count, bytes
        needed), enqueued on the context's stream; FPX_ECAPACITY / FPX_EINVAL surface at sync() and abort nothing.
        cap: capacity in bytes (default: out.numel(), or values.numel() + 24 n when out is None)."""
        n = slot.numel()
        nv = values.numel() if values_len is None else values_len
        if cap is None:
            cap = out.numel() if out is not None else nv + 24 * n
        out, out_offsets, totals = self._wire_encode_out(slot.device, cap, n, out, out_offsets, totals)
        from . import wire
        st = wire._L().fpx_wire_encode_replica_chosen_dev(self._h, n, _dp(emit), _dp(slot), _dp(is_noop), _dp(values), nv,
                                                          _dp(value_off), _dp(value_len), _dp(out), cap, _dp(out_offsets),
                                                          _dp(totals))
        if st:
            raise FpxError(st, "fpx_wire_encode_replica_chosen_dev")
        return out, out_offsets, totals

    def wire_encode_phase2b_batch_dev(self, slot, round_, vote_bits, group_of_slot=None, grid_cols=0, dialect=0, cap=None,
                                      max_msgs=None, out=None, out_offsets=None, totals=None):
        """ProxyLeaderInbound{Phase2b} per set bit of vote_bits (n x 4 words; int64 or uint64 CUDA tensor), as
        wire.encode_phase2b_batch on the host.  Defaults: max_msgs = 256 n, cap = 46 max_msgs (no Phase2b is longer)."""
        n = slot.numel()
        if max_msgs is None:
            max_msgs = out_offsets.numel() - 1 if out_offsets is not None else 256 * n
        if cap is None:
            cap = out.numel() if out is not None else 46 * max_msgs
        out, out_offsets, totals = self._wire_encode_out(slot.device, cap, max_msgs, out, out_offsets, totals)
        from . import wire
        st = wire._L().fpx_wire_encode_phase2b_batch_dev(self._h, dialect, n, _dp(slot), _dp(round_), _dp(vote_bits),
                                                         _dp(group_of_slot), grid_cols, _dp(out), cap, _dp(out_offsets),
                                                         max_msgs, _dp(totals))
        if st:
            raise FpxError(st, "fpx_wire_encode_phase2b_batch_dev")
        return out, out_offsets, totals

    def wire_encode_leader_nack_dev(self, nack_round, dialect=0, cap=None, max_msgs=None, out=None, out_offsets=None,
                                    totals=None):
        """LeaderInbound{Nack} of every record with nack_round[i] >= 0 (int32 CUDA tensor, as K1 / K3 report them)."""
        n = nack_round.numel()
        if max_msgs is None:
            max_msgs = out_offsets.numel() - 1 if out_offsets is not None else n
        if cap is None:
            cap = out.numel() if out is not None else 13 * max_msgs
        out, out_offsets, totals = self._wire_encode_out(nack_round.device, cap, max_msgs, out, out_offsets, totals)
        from . import wire
        st = wire._L().fpx_wire_encode_leader_nack_dev(self._h, dialect, n, _dp(nack_round), _dp(out), cap,
                                                       _dp(out_offsets), max_msgs, _dp(totals))
        if st:
            raise FpxError(st, "fpx_wire_encode_leader_nack_dev")
        return out, out_offsets, totals

    def wire_phase2_tick(self, in_ptr, in_len, in_offsets_ptr, n, out_ptr, out_cap, out_offsets_ptr, nack_round_ptr=None):
        """fpx_wire_phase2_tick on raw addresses of page-locked buffers (host_alloc): returns (status, count,
        bytes_needed, bad_index); the status is returned, not raised -- FPX_ECAPACITY is an answer here."""
        from . import wire
        count, need, bad = C.c_int64(0), C.c_int64(0), C.c_int32(-1)
        st = wire._L().fpx_wire_phase2_tick(self._h, in_ptr, in_len, in_offsets_ptr, n, out_ptr, out_cap, out_offsets_ptr,
                                            C.byref(count), nack_round_ptr, C.byref(need), C.byref(bad))
        return st, count.value, need.value, bad.value

    def wire_phase2b_tick(self, in_ptr, in_len, in_offsets_ptr, n, out_slot_ptr, out_round_ptr, out_value_ptr, out_cap,
                          grid_cols=0):
        """fpx_wire_phase2b_tick on raw addresses of page-locked buffers (host_alloc): returns (status, count, bad_index);
        the status is returned, not raised -- FPX_ECAPACITY (count = the capacity needed) is an answer here."""
        from . import wire
        count, bad = C.c_int32(0), C.c_int32(-1)
        st = wire._L().fpx_wire_phase2b_tick(self._h, in_ptr, in_len, in_offsets_ptr, n, grid_cols, out_slot_ptr,
                                             out_round_ptr, out_value_ptr, out_cap, C.byref(count), C.byref(bad))
        return st, count.value, bad.value

    # ---- multi-GPU: RCCL communicator behind the C ABI (fpx_comm_*) ----------------------------------
    def comm_create(self, unique_id, rank, world):
        """collective over the `world` contexts (one per GPU): unique_id = comm_unique_id() of one rank"""
        buf = (C.c_uint8 * _lib.FPX_COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        st = self.L.fpx_comm_create(self._h, buf, rank, world)
        if st:
            raise FpxError(st, "fpx_comm_create (rccl %d)" % self.L.fpx_last_rccl_error(self._h))

    def comm_destroy(self):
        st = self.L.fpx_comm_destroy(self._h)
        if st:
            raise FpxError(st, "fpx_comm_destroy")

    def comm_info(self):
        r, w = C.c_int32(), C.c_int32()
        self.L.fpx_comm_info(self._h, C.byref(r), C.byref(w))
        return r.value, w.value

    def phase2_replica_sharded_dev(self, slot, round_, value, target_mask=None, chosen=None,
                                   chosen_round=None, chosen_value=None, nack_round=None):
        """replica-axis sharded fused step: K1 on my acceptors -> ncclReduceScatter(sum) of the partial vote
        bitmaps -> open + K2 on my slice of the batch (outputs have n / world entries)"""
        st = self.L.fpx_phase2_replica_sharded_dev(self._h, slot.numel(), _dp(slot), _dp(round_), _dp(value),
                                                   _dp(target_mask), _dp(chosen), _dp(chosen_round),
                                                   _dp(chosen_value), _dp(nack_round))
        if st:
            raise FpxError(st, "fpx_phase2_replica_sharded_dev (rccl %d)" % self.L.fpx_last_rccl_error(self._h))

    def comm_allgather_chosen_dev(self, chosen, chosen_round, chosen_value, all_chosen, all_round, all_value):
        n = (chosen if chosen is not None else chosen_value).numel()
        st = self.L.fpx_comm_allgather_chosen_dev(self._h, n, _dp(chosen), _dp(chosen_round), _dp(chosen_value),
                                                  _dp(all_chosen), _dp(all_round), _dp(all_value))
        if st:
            raise FpxError(st, "fpx_comm_allgather_chosen_dev")

    def profile_read_collective(self):
        n, ms = C.c_int32(), C.c_double()
        st = self.L.fpx_profile_read_collective(self._h, C.byref(n), C.byref(ms))
        if st:
            raise FpxError(st, "fpx_profile_read_collective")
        return n.value, ms.value

    def proxy_forget(self, first_slot, count):
        """GC of the proxy leader's tallies of a slot range (async on the context's stream)"""
        st = self.L.fpx_proxy_forget(self._h, first_slot, count)
        if st:
            raise FpxError(st, "fpx_proxy_forget")

    def recycle_slots(self, first_slot, count):
        """the rows of a slot range become fresh: votes dropped, tallies forgotten, promises kept (async)"""
        st = self.L.fpx_recycle_slots(self._h, first_slot, count)
        if st:
            raise FpxError(st, "fpx_recycle_slots")

    # ---- K4: Mencius noop ranges ----------------------------------------------------------------
    def acceptor_phase2a_noop_range(self, slot_start, slot_end, round_, target_masks=None):
        A = self.cfg.num_groups
        target_masks = _u64(target_masks)
        vb = np.zeros((A, 4), np.uint64)
        nb = np.zeros((A, 4), np.uint64)
        nr = C.c_int32(-1)
        st = self.L.fpx_acceptor_phase2a_noop_range(self._h, slot_start, slot_end, round_,
                                                    _hp(target_masks), _hp(vb), _hp(nb), C.byref(nr))
        return st, vb, nb, nr.value

    def proxy_open_noop_range(self, slot_start, slot_end, round_):
        new = C.c_uint8(0)
        st = self.L.fpx_proxy_open_noop_range(self._h, slot_start, slot_end, round_, C.byref(new))
        return st, new.value

    def proxy_phase2b_noop_range(self, slot_start, slot_end, round_, vote_bits):
        vote_bits = _u64(vote_bits)
        ch = C.c_uint8(0)
        st = self.L.fpx_proxy_phase2b_noop_range(self._h, slot_start, slot_end, round_, _hp(vote_bits),
                                                 C.byref(ch))
        return st, ch.value

    # batched forms (n ranges per call; bitmaps n x num_groups x 4)
    def _ranges(self, slot_start, slot_end, round_):
        return _i32(np.atleast_1d(slot_start)), _i32(np.atleast_1d(slot_end)), _i32(np.atleast_1d(round_))

    def acceptor_phase2a_noop_ranges(self, slot_start, slot_end, round_, target_masks=None):
        s, e, r = self._ranges(slot_start, slot_end, round_)
        n, A = len(s), self.cfg.num_groups
        target_masks = _u64(target_masks)
        vb = np.zeros((n, A, 4), np.uint64)
        nb = np.zeros((n, A, 4), np.uint64)
        nr = np.full(n, -1, np.int32)
        st = self.L.fpx_acceptor_phase2a_noop_ranges(self._h, n, _hp(s), _hp(e), _hp(r), _hp(target_masks),
                                                     _hp(vb), _hp(nb), _hp(nr))
        return st, vb, nb, nr

    def proxy_open_noop_ranges(self, slot_start, slot_end, round_):
        s, e, r = self._ranges(slot_start, slot_end, round_)
        new = np.zeros(len(s), np.uint8)
        st = self.L.fpx_proxy_open_noop_ranges(self._h, len(s), _hp(s), _hp(e), _hp(r), _hp(new))
        return st, new

    def proxy_phase2b_noop_ranges(self, slot_start, slot_end, round_, vote_bits):
        s, e, r = self._ranges(slot_start, slot_end, round_)
        vote_bits = _u64(vote_bits)
        ch = np.zeros(len(s), np.uint8)
        st = self.L.fpx_proxy_phase2b_noop_ranges(self._h, len(s), _hp(s), _hp(e), _hp(r), _hp(vote_bits), _hp(ch))
        return st, ch

    def noop_ranges_fused(self, slot_start, slot_end, round_, target_masks=None):
        """open + acceptors + tally for n ranges: (status, vote_bits, nack_bits, nack_round, is_new, chosen)"""
        s, e, r = self._ranges(slot_start, slot_end, round_)
        n, A = len(s), self.cfg.num_groups
        target_masks = _u64(target_masks)
        vb = np.zeros((n, A, 4), np.uint64)
        nb = np.zeros((n, A, 4), np.uint64)
        nr = np.full(n, -1, np.int32)
        new = np.zeros(n, np.uint8)
        ch = np.zeros(n, np.uint8)
        st = self.L.fpx_noop_ranges_fused(self._h, n, _hp(s), _hp(e), _hp(r), _hp(target_masks), _hp(vb), _hp(nb),
                                          _hp(nr), _hp(new), _hp(ch))
        return st, vb, nb, nr, new, ch

    def noop_ranges_fused_dev(self, slot_start, slot_end, round_, target_masks=None, vote_bits=None,
                              nack_bits=None, nack_round=None, is_new=None, chosen=None):
        st = self.L.fpx_noop_ranges_fused_dev(self._h, slot_start.numel(), _dp(slot_start), _dp(slot_end),
                                              _dp(round_), _dp(target_masks), _dp(vote_bits), _dp(nack_bits),
                                              _dp(nack_round), _dp(is_new), _dp(chosen))
        if st:
            raise FpxError(st, "fpx_noop_ranges_fused_dev")

    def mencius_band_fused_dev(self, slot, round_, value, target_mask, chosen, chosen_round, chosen_value, nack_round,
                               slot_start, slot_end, range_round, range_target_masks=None, range_vote_bits=None,
                               range_nack_bits=None, range_nack_round=None, range_is_new=None, range_chosen=None,
                               independent=False):
        """one Mencius proxy-leader step: phase2_fused_dev on the commands + noop_ranges_fused_dev on the ranges; with
        independent (no leader group has both) and FPX_F_TRUSTED the step is two launches (or the halves side by side)"""
        st = self.L.fpx_mencius_band_fused_dev(
            self._h, slot.numel(), _dp(slot), _dp(round_), _dp(value), _dp(target_mask), _dp(chosen), _dp(chosen_round),
            _dp(chosen_value), _dp(nack_round), slot_start.numel(), _dp(slot_start), _dp(slot_end), _dp(range_round),
            _dp(range_target_masks), _dp(range_vote_bits), _dp(range_nack_bits), _dp(range_nack_round), _dp(range_is_new),
            _dp(range_chosen), 1 if independent else 0)
        if st:
            raise FpxError(st, "fpx_mencius_band_fused_dev")

    def read_range_tally(self, slot_start, slot_end, round_):
        state = C.c_int32()
        bits = np.zeros((self.cfg.num_groups, 4), np.uint64)
        st = self.L.fpx_read_range_tally(self._h, slot_start, slot_end, round_, C.byref(state), _hp(bits))
        if st:
            raise FpxError(st, "fpx_read_range_tally")
        return state.value, bits

    def read_range_position(self, slot_start, slot_end, round_):
        """where the tally of (slot_start, slot_end, round_) lives in the range table: (capacity, home bucket, bucket);
        bucket is -1 for an unknown key"""
        cap, home, at = C.c_int32(), C.c_int32(), C.c_int32()
        st = self.L.fpx_read_range_position(self._h, slot_start, slot_end, round_, C.byref(cap), C.byref(home), C.byref(at))
        if st:
            raise FpxError(st, "fpx_read_range_position")
        return cap.value, home.value, at.value

    # ---- f1: replica log / f2: Phase-1 recovery scan ----------------------------------------------
    def replica_chosen(self, slot, value, mask=None):
        slot, value = _i32(slot), _i32(value)
        mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        wm, nc = C.c_int32(), C.c_int32()
        st = self.L.fpx_replica_chosen(self._h, len(slot), _hp(slot), _hp(value), _hp(mask),
                                       C.byref(wm), C.byref(nc))
        return st, wm.value, nc.value

    def replica_chosen_noop_range(self, slot_start, slot_end):
        wm, nc = C.c_int32(), C.c_int32()
        st = self.L.fpx_replica_chosen_noop_range(self._h, slot_start, slot_end, C.byref(wm), C.byref(nc))
        return st, wm.value, nc.value

    def replica_chosen_dev(self, slot, value, mask=None):
        st = self.L.fpx_replica_chosen_dev(self._h, slot.numel(), _dp(slot), _dp(value), _dp(mask))
        if st:
            raise FpxError(st, "fpx_replica_chosen_dev")

    def replica_chosen_msgs(self, kind, slot, slot_end, value, mask=None):
        """a burst of Chosen / ChosenNoopRange messages in delivery order (kinds of frankenpaxos_amd.wire), exactly as a
        Mencius replica handles them one by one: (status, executed_watermark, num_chosen)"""
        kind, slot, slot_end, value = _i32(kind), _i32(slot), _i32(slot_end), _i32(value)
        assert len(kind) == len(slot) == len(slot_end) == len(value)
        mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        wm, nc = C.c_int32(), C.c_int32()
        st = self.L.fpx_replica_chosen_msgs(self._h, len(kind), _hp(kind), _hp(slot), _hp(slot_end), _hp(value),
                                            _hp(mask), C.byref(wm), C.byref(nc))
        return st, wm.value, nc.value

    def replica_chosen_msgs_dev(self, kind, slot, slot_end, value, mask=None, n=None):
        """the same on device tensors (n: the number of messages, default kind.numel()); errors surface at sync()"""
        st = self.L.fpx_replica_chosen_msgs_dev(self._h, kind.numel() if n is None else n, _dp(kind), _dp(slot),
                                                _dp(slot_end), _dp(value), _dp(mask))
        if st:
            raise FpxError(st, "fpx_replica_chosen_msgs_dev")

    def replica_inbox(self, kind, slot, value, mask=None, exec_count=None, reply_slot=None, order=None):
        """a MultiPaxos replica's burst of Chosens and reads in delivery order (kinds of frankenpaxos_amd.wire), exactly as
        the replica handles them one by one: (status, exec_count, reply_slot, order, counts, executed_watermark,
        num_chosen); counts = [reads, reads that ran, W0, W1], order's first counts[0] entries are valid.  The output
        arrays may be passed in (int32, len(kind)): on an error they are left as they were"""
        kind, slot, value = _i32(kind), _i32(slot), _i32(value)
        assert len(kind) == len(slot) == len(value)
        n = len(kind)
        mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        outs = [np.full(max(n, 1), -9, np.int32) if a is None else a for a in (exec_count, reply_slot, order)]
        counts = np.full(4, -9, np.int32)
        wm, nc = C.c_int32(), C.c_int32()
        st = self.L.fpx_replica_inbox(self._h, n, _hp(kind), _hp(slot), _hp(value), _hp(mask), _hp(outs[0]), _hp(outs[1]),
                                      _hp(outs[2]), _hp(counts), C.byref(wm), C.byref(nc))
        return st, outs[0][:n], outs[1][:n], outs[2][:n], counts, wm.value, nc.value

    def replica_inbox_dev(self, kind, slot, value, mask=None, exec_count=None, reply_slot=None, order=None, counts=None,
                          n=None):
        """the same on device tensors (the four outputs all given or all None: then the burst's Chosens are ingested and
        nothing is scheduled); errors surface at sync()"""
        st = self.L.fpx_replica_inbox_dev(self._h, kind.numel() if n is None else n, _dp(kind), _dp(slot), _dp(value),
                                          _dp(mask), _dp(exec_count), _dp(reply_slot), _dp(order), _dp(counts))
        if st:
            raise FpxError(st, "fpx_replica_inbox_dev")

    def replica_state(self):
        wm, nc = C.c_int32(), C.c_int32()
        st = self.L.fpx_replica_state(self._h, C.byref(wm), C.byref(nc))
        if st:
            raise FpxError(st, "fpx_replica_state")
        return wm.value, nc.value

    def replica_read_log(self, first, count):
        vals = np.zeros(count, np.int32)
        pres = np.zeros(count, np.uint8)
        st = self.L.fpx_replica_read_log(self._h, first, count, _hp(vals), _hp(pres))
        if st:
            raise FpxError(st, "fpx_replica_read_log")
        return vals, pres

    def leader_phase1b_scan(self, watermark, quorum_masks, cap):
        q = np.ascontiguousarray(quorum_masks, dtype=np.uint64).reshape(self.ngroups, 4)
        mx = C.c_int32()
        sr = np.full(cap, -7, np.int32)
        sv = np.full(cap, -7, np.int32)
        st = self.L.fpx_leader_phase1b_scan(self._h, watermark, _hp(q), cap, C.byref(mx), _hp(sr),
                                            _hp(sv))
        k = max(0, min(cap, mx.value - watermark + 1))
        return st, mx.value, sr[:k], sv[:k]

    def leader_phase1b_msgs(self, round_, watermark, msg_round, acceptor_index, offsets, info_slot, info_vote_round,
                            info_value_id, kind=None, group_index=None, leader_group=0, recover_slot=-1, flags=0,
                            grid_cols=0, cap=None):
        """Leader.handlePhase1b for a burst of Phase1b messages in delivery order (host arrays, synchronous).  Message i
        owns the records offsets[i]:offsets[i + 1] (offsets: n + 1 entries; or pass the decoder's info_first, n entries,
        and it is completed from the record count).  cap None: a sizing call first.  Returns (status, result) with
        result a dict: complete, decided_at, and -- when complete -- count, max_slot, next_slot, out_slot, safe_round,
        safe_value (the first min(count, cap) entries), held_bits (ngroups x 4)."""
        msg_round, acceptor_index = _i32(msg_round), _i32(acceptor_index)
        kind, group_index = _i32(kind), _i32(group_index)
        info_slot, info_vote_round, info_value_id = _i32(info_slot), _i32(info_vote_round), _i32(info_value_id)
        n = len(msg_round)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if len(offsets) == n:  # a prefix sum without its total (wire.decode_leader_inbound's info_first)
            offsets = np.concatenate([offsets, np.array([len(info_slot)], np.int64)])
        assert len(offsets) == n + 1, "offsets has n + 1 entries"

        def call(c, sl, sr, sv, held):
            res = np.full(_lib.FPX_P1B_RESULT_WORDS, -1, np.int64)
            st = self.L.fpx_leader_phase1b_msgs(self._h, round_, watermark, leader_group, recover_slot, flags, n, _hp(kind),
                                                _hp(msg_round), _hp(group_index), _hp(acceptor_index), _hp(offsets),
                                                _hp(info_slot), _hp(info_vote_round), _hp(info_value_id), grid_cols, c,
                                                _hp(sl), _hp(sr), _hp(sv), _hp(res), _hp(held))
            return st, res

        if cap is None:
            st, res = call(0, None, None, None, None)
            if res[0] != 1:  # refused, or no quorum yet (a complete result comes with FPX_ECAPACITY or FPX_EFATAL_PROTOCOL too)
                return st, self._p1b_result(res, None, None, None, None)
            cap = int(res[_lib.FPX_P1B_COUNT])
        sl, sr, sv = (np.full(cap, -7, np.int32) for _ in range(3))
        held = np.zeros((self.ngroups, 4), np.uint64)
        st, res = call(cap, sl, sr, sv, held)
        return st, self._p1b_result(res, sl, sr, sv, held)

    @staticmethod
    def _p1b_result(res, sl, sr, sv, held):
        out = {"complete": int(res[0]), "decided_at": int(res[1])}
        if res[0] == 1:
            w = int(res[_lib.FPX_P1B_WRITTEN])
            out.update(count=int(res[_lib.FPX_P1B_COUNT]), max_slot=int(res[_lib.FPX_P1B_MAX_SLOT]),
                       next_slot=int(res[_lib.FPX_P1B_NEXT_SLOT]), written=w, held_bits=held,
                       out_slot=None if sl is None else sl[:w], safe_round=None if sr is None else sr[:w],
                       safe_value=None if sv is None else sv[:w])
        return out

    def leader_phase1b_msgs_dev(self, round_, watermark, msg_round, acceptor_index, offsets, info_slot, info_vote_round,
                                info_value_id, result, kind=None, group_index=None, leader_group=0, recover_slot=-1,
                                flags=0, grid_cols=0, cap=0, out_slot=None, safe_round=None, safe_value=None,
                                held_bits=None):
        """asynchronous form on torch CUDA tensors: the headers int32 [n], offsets int64 [n + 1], the records int32,
        result int64 [FPX_P1B_RESULT_WORDS], the outputs int32 of at least cap elements (None with cap = 0), held_bits
        int64 [ngroups x 4] or None.  Errors surface at sync()."""
        st = self.L.fpx_leader_phase1b_msgs_dev(self._h, round_, watermark, leader_group, recover_slot, flags,
                                                msg_round.numel(), _dp(kind), _dp(msg_round), _dp(group_index),
                                                _dp(acceptor_index), _dp(offsets), _dp(info_slot), _dp(info_vote_round),
                                                _dp(info_value_id), grid_cols, cap, _dp(out_slot), _dp(safe_round),
                                                _dp(safe_value), _dp(result), _dp(held_bits))
        if st:
            raise FpxError(st, "fpx_leader_phase1b_msgs_dev")

    def acceptor_phase1b_info(self, group, replica, watermark=0):
        """Phase1b.info of one acceptor: (slot, vote_round, vote_value) of its votes in slots >= watermark, ascending"""
        k = C.c_int32()
        st = self.L.fpx_acceptor_phase1b_info(self._h, group, replica, watermark, 0, C.byref(k), None, None, None)
        if st:
            raise FpxError(st, "fpx_acceptor_phase1b_info")
        n = k.value
        sl, vr, vv = (np.zeros(n, np.int32) for _ in range(3))
        if n:
            st = self.L.fpx_acceptor_phase1b_info(self._h, group, replica, watermark, n, C.byref(k), _hp(sl), _hp(vr), _hp(vv))
            if st:
                raise FpxError(st, "fpx_acceptor_phase1b_info")
        return sl, vr, vv

    def _p1_masks(self, masks):
        return None if masks is None else np.ascontiguousarray(masks, dtype=np.uint64).reshape(self.ngroups, 4)

    def acceptor_phase1b_info_all(self, watermark=0, masks=None):
        """Phase1b.info of every selected acceptor in one device pass: (offsets, slot, vote_round, vote_value); entry
        e = group * R + replica owns offsets[e]:offsets[e + 1].  masks: ngroups x 4 uint64 (acceptor_phase1a's target
        bits) or None = all.  Sizes with one cap = 0 call."""
        masks = self._p1_masks(masks)
        off = np.zeros(self.ngroups * self.R + 1, np.int64)
        k = C.c_int64()
        st = self.L.fpx_acceptor_phase1b_info_all(self._h, watermark, _hp(masks), 0, _hp(off), None, None, None, C.byref(k))
        if st not in (0, _lib.FPX_ECAPACITY):
            raise FpxError(st, "fpx_acceptor_phase1b_info_all")
        return (off,) + self._p1_fill(watermark, masks, k.value, off)

    def _p1_fill(self, watermark, masks, n, off):
        """the records of a pass whose sizing call counted n: one call with cap = n"""
        sl, vr, vv = (np.zeros(n, np.int32) for _ in range(3))
        if n:
            k = C.c_int64()
            st = self.L.fpx_acceptor_phase1b_info_all(self._h, watermark, _hp(masks), n, _hp(off), _hp(sl), _hp(vr), _hp(vv),
                                                      C.byref(k))
            if st:
                raise FpxError(st, "fpx_acceptor_phase1b_info_all")
        return sl, vr, vv

    def acceptor_phase1b_info_all_dev(self, watermark, masks, cap, offsets, slot, vote_round, vote_value, totals):
        """asynchronous form on torch CUDA tensors: masks ngroups x 4 int64 words or None, offsets E + 1 int64, the
        record arrays int32 of at least cap elements (None with cap = 0), totals 2 int64 (needed, written)"""
        st = self.L.fpx_acceptor_phase1b_info_all_dev(self._h, watermark, _dp(masks), cap, _dp(offsets), _dp(slot),
                                                      _dp(vote_round), _dp(vote_value), _dp(totals))
        if st:
            raise FpxError(st, "fpx_acceptor_phase1b_info_all_dev")

    def acceptor_phase1(self, round_, watermark=0, masks=None):
        """A Leader's Phase1a at every acceptor it addresses: (promised_bits, nack_bits, offsets, slot, vote_round,
        vote_value), the bits ngroups x 4, the info of exactly the acceptors that promised.  The round moves once, in a
        sizing call; the records are fetched behind it by one fpx_acceptor_phase1b_info_all on the promised bits."""
        masks = self._p1_masks(masks)
        pb = np.zeros((self.ngroups, 4), np.uint64)
        nb = np.zeros((self.ngroups, 4), np.uint64)
        off = np.zeros(self.ngroups * self.R + 1, np.int64)
        k = C.c_int64()
        st = self.L.fpx_acceptor_phase1(self._h, round_, watermark, _hp(masks), _hp(pb), _hp(nb), 0, _hp(off), None, None,
                                        None, C.byref(k))
        if st not in (0, _lib.FPX_ECAPACITY):
            raise FpxError(st, "fpx_acceptor_phase1")
        return (pb, nb, off) + self._p1_fill(watermark, pb, k.value, off)

    # ---- readback ------------------------------------------------------------------------------
    def read_acceptor(self, group, replica):
        p, m = C.c_int32(), C.c_int32()
        vr = np.zeros(self.S, np.int32)
        vv = np.zeros(self.S, np.int32)
        bl = np.zeros(self.S, np.int32)
        st = self.L.fpx_read_acceptor(self._h, group, replica, C.byref(p), C.byref(m), _hp(vr),
                                      _hp(vv), _hp(bl))
        if st:
            raise FpxError(st, "fpx_read_acceptor")
        return p.value, m.value, vr, vv, bl

    def read_state(self):
        vr = np.zeros((self.S, self.R), np.int32)
        vv = np.zeros((self.S, self.R), np.int32)
        bl = np.zeros((self.S, self.R), np.int32)
        st = self.L.fpx_read_state(self._h, _hp(vr), _hp(vv), _hp(bl))
        if st:
            raise FpxError(st, "fpx_read_state")
        return vr, vv, bl

    def read_scalars(self):
        pr = np.zeros((self.ngroups, self.R), np.int32)
        mv = np.zeros((self.ngroups, self.R), np.int32)
        st = self.L.fpx_read_scalars(self._h, _hp(pr), _hp(mv))
        if st:
            raise FpxError(st, "fpx_read_scalars")
        return pr, mv

    def state_digest(self):
        """8 uint64 digests of the whole state (fpx_state_digest): equal states have equal digests; the converse holds up
        to a collision of a 64-bit additive hash of (position, value) terms -- improbable, not impossible"""
        out = np.zeros(8, np.uint64)
        st = self.L.fpx_state_digest(self._h, _hp(out))
        if st:
            raise FpxError(st, "fpx_state_digest")
        return out

    def ballot_summary_audit(self):
        """FPX_BALLOT_PER_SLOT: (uniform rows, mixed rows, violations) of the per-row ballot summaries
        (fpx_ballot_summary_audit); violations -- uniform rows with a cell that differs from the summary -- must be 0"""
        out = np.zeros(3, np.int64)
        st = self.L.fpx_ballot_summary_audit(self._h, _hp(out))
        if st:
            raise FpxError(st, "fpx_ballot_summary_audit")
        return int(out[0]), int(out[1]), int(out[2])

    def vote_summary_audit(self):
        """(fresh rows, rows kept as cells, compact rows) of the vote rows (fpx_vote_summary_audit).  Call it before
        read_state(), which turns every compact row back into cells"""
        out = np.zeros(3, np.int64)
        st = self.L.fpx_vote_summary_audit(self._h, _hp(out))
        if st:
            raise FpxError(st, "fpx_vote_summary_audit")
        return int(out[0]), int(out[1]), int(out[2])

    def read_tally(self, slot):
        n = C.c_int32()
        rounds = np.zeros(8, np.int32)
        states = np.zeros(8, np.int32)
        values = np.zeros(8, np.int32)
        bits = np.zeros((8, 4), np.uint64)
        st = self.L.fpx_read_tally(self._h, slot, C.byref(n), _hp(rounds), _hp(states), _hp(values),
                                   _hp(bits))
        if st:
            raise FpxError(st, "fpx_read_tally")
        return [(int(rounds[i]), int(states[i]), int(values[i]), tuple(int(x) for x in bits[i]))
                for i in range(n.value)]


def comm_unique_id():
    """ncclGetUniqueId through the C ABI: 128 opaque bytes for fpx_comm_create on every rank"""
    buf = (C.c_uint8 * _lib.FPX_COMM_ID_BYTES)()
    st = _lib.lib().fpx_comm_unique_id(buf)
    if st:
        raise FpxError(st, "fpx_comm_unique_id")
    return bytes(buf)


# ---- a5 / a7 free functions ----------------------------------------------------------------------
class PinnedArray:
    """A numpy array over page-locked host memory (fpx_host_alloc): batches built in it cross PCIe by
    DMA.  Keep the object alive while `array` is in use; `free()` (or garbage collection) releases it."""

    def __init__(self, shape, dtype):
        self._L = _lib.lib()
        dtype = np.dtype(dtype)
        nbytes = max(1, int(np.prod(shape)) * dtype.itemsize)
        p = C.c_void_p()
        st = self._L.fpx_host_alloc(nbytes, C.byref(p))
        if st:
            raise FpxError(st, "fpx_host_alloc")
        self._p = p
        buf = (C.c_char * nbytes).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if self._p is not None:
            self.array = None
            self._L.fpx_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def quorum_eval(cfg, nodes, strict=True, read=False):
    """isWriteQuorum / isReadQuorum (strict) or the isSuperSetOf* variants for n node sets
    (n x 4 uint64), evaluated by the device predicate the tally kernels use."""
    L = _lib.lib()
    nodes = np.ascontiguousarray(nodes, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros(len(nodes), np.uint8)
    fn = L.fpx_read_quorum_eval if read else L.fpx_quorum_eval
    st = fn(C.byref(cfg), len(nodes), _hp(nodes), int(strict), _hp(out))
    if st == _lib.FPX_EINVAL:
        raise ValueError("IllegalArgumentException (require failed)")
    if st:
        raise FpxError(st, "fpx_quorum_eval")
    return out.astype(bool)


def round_leader(num_leaders, round_):
    return _lib.lib().fpx_round_leader(num_leaders, round_)


def next_classic_round(num_leaders, leader_index, round_):
    return _lib.lib().fpx_next_classic_round(num_leaders, leader_index, round_)
