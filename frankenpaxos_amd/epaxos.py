"""EPaxos pre-accept fast path (K5) on the GPU: python handle on an fpx_epx context.

Every result is computed by the HIP kernels of csrc/fpx_epaxos.hip; there is no CPU path here."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FpxError


FPX_EPX_F_LEADER_STATE = 1
FPX_EPX_F_RECOVERY = 2
# fpx_epx_recover / fpx_epx_recovery_replies: per-message outcomes (include/fpx.h)
RV_PREPARING, RV_COMMITTED, RV_FATAL = range(3)
RC_IGNORED, RC_WAITING, RC_ACCEPT, RC_PRE_ACCEPT, RC_PRE_ACCEPT_NOOP, RC_FATAL = range(6)
# fpx_epx_leader_replies: message kinds and per-message outcomes (include/fpx.h)
PRE_ACCEPT_OK, ACCEPT_OK, NACK, SLOW_PATH_TIMER = 0, 1, 2, 3
(IGNORED, WAITING, START_SLOW_PATH_TIMER, FAST_COMMIT, ACCEPT, SLOW_COMMIT, NACK_RECOVER, NACK_IGNORED,
 FATAL) = range(9)
# fpx_epx_replica_inbox: message kinds and per-message outcomes (include/fpx.h)
IN_PRE_ACCEPT, IN_ACCEPT, IN_COMMIT, IN_PREPARE = 0, 1, 2, 3
(RI_IGNORED, RI_PRE_ACCEPT_OK, RI_PRE_ACCEPT_OK_AGAIN, RI_ACCEPT_OK, RI_ACCEPT_OK_AGAIN, RI_LEARNT, RI_PREPARE_OK, RI_NACK,
 RI_COMMIT_BACK) = range(9)
INBOX_MAX = 1 << 24
KEY_LIST = -2         # FPX_EPX_KEY_LIST: a leader state's key word for a list of two or more distinct keys


class FpxEpxConfig(C.Structure):
    _fields_ = [("num_replicas", C.c_int32), ("num_keys", C.c_int32), ("device", C.c_int32),
                ("flags", C.c_uint32), ("num_instances", C.c_int32)]


def _bind(L):
    if getattr(L, "_epx_bound", False):
        return
    VP = C.c_void_p
    L.fpx_epx_create.argtypes = [C.POINTER(FpxEpxConfig), C.POINTER(VP)]
    L.fpx_epx_destroy.argtypes = [VP]
    L.fpx_epx_set_stream.argtypes = [VP, VP]
    L.fpx_epx_sync.argtypes = [VP]
    # fpx_epx_preaccept[_dev]: the table in _lib.SIGNATURES (one place, checked against the header)
    L.fpx_epx_read_index.argtypes = [VP, C.c_int32, C.c_int32, VP, VP]
    L._epx_bound = True


class EPaxos:
    def __init__(self, num_replicas, num_keys, device=0, num_instances=0, leader_state=False, recovery=False):
        """num_instances > 0: every replica keeps its command log for instances (leader, number < num_instances):
        pre-accept records it, prepare() / accept() run the per-instance Paxos on it.
        leader_state (needs num_instances > 0): the context also keeps Replica.leaderStates, for lead() and
        leader_replies() -- hosted replicas that lead instances among peers in other processes.
        recovery (needs leader_state): the leader state has the Preparing phase, for recover(), recovery_replies() and
        lead_accept() -- hosted replicas that originate an instance's recovery"""
        self.L = _lib.lib()
        _bind(self.L)
        self.n, self.num_keys = num_replicas, num_keys
        flags = (FPX_EPX_F_LEADER_STATE if leader_state else 0) | (FPX_EPX_F_RECOVERY if recovery else 0)
        cfg = FpxEpxConfig(num_replicas, num_keys, device, flags, num_instances)
        h = C.c_void_p()
        st = self.L.fpx_epx_create(C.byref(cfg), C.byref(h))
        if st:
            raise FpxError(st, "fpx_epx_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.L.fpx_epx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, s):
        st = self.L.fpx_epx_set_stream(self._h, C.c_void_p(-1 if s is None else int(s)))
        if st:
            raise FpxError(st, "fpx_epx_set_stream")

    def sync(self):
        return self.L.fpx_epx_sync(self._h)

    def preaccept(self, leader, number, key, is_set, resp_mask, rank, seen_mask=None, triple_id=None):
        """seen_mask: the other replicas that process the PreAccept (None = resp_mask, a thrifty
        deployment; all n-1 others with the reference's default ThriftySystem.NotThrifty)"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        a8 = lambda x: np.ascontiguousarray(x, dtype=np.uint8)
        leader, number, key, rank = a32(leader), a32(number), a32(key), a32(rank)
        is_set, resp_mask = a8(is_set), a8(resp_mask)
        seen_mask = None if seen_mask is None else a8(seen_mask)
        triple_id = None if triple_id is None else a32(triple_id)
        m = len(leader)
        fast = np.zeros(m, np.uint8)
        deps = np.zeros((m, self.n), np.int32)
        ldeps = np.zeros((m, self.n), np.int32)
        own = np.zeros((m, 2), np.int32)
        p = lambda a: None if a is None else a.ctypes.data
        st = self.L.fpx_epx_preaccept(self._h, m, p(leader), p(number), p(key), p(is_set), p(resp_mask),
                                      p(seen_mask), p(rank), p(triple_id), p(fast), p(deps), p(ldeps), p(own))
        return st, fast, deps, ldeps, own

    def prepare(self, leader, number, ballot_ordering, ballot_replica, target_mask):
        """Replica.handlePrepare at the replicas of target_mask: (status, ok_bits, nack_bits, commit_bits,
        nack_ballot, reply_status[m, n], reply_vote[m, n], reply_triple[m, n])"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        leader, number, bo, br = a32(leader), a32(number), a32(ballot_ordering), a32(ballot_replica)
        tgt = np.ascontiguousarray(target_mask, dtype=np.uint8)
        m = len(leader)
        ok, nack, com = (np.zeros(m, np.uint8) for _ in range(3))
        nb = np.full(m, -1, np.int32)
        rs, rv, rt = (np.full((m, self.n), -1, np.int32) for _ in range(3))
        p = lambda a: a.ctypes.data
        st = self.L.fpx_epx_prepare(self._h, m, p(leader), p(number), p(bo), p(br), p(tgt), p(ok), p(nack), p(com),
                                    p(nb), p(rs), p(rv), p(rt))
        return st, ok, nack, com, nb, rs, rv, rt

    def handle_prepare_oks(self, leader, number, ballot_ordering, ballot_replica, resp_mask, reply_status, reply_vote,
                           reply_triple, as_intended=False):
        """Replica.handlePrepareOk, the recovering replica's decision: (status, action, source, triple) -- action 0 wait,
        1 Accept phase with `source`'s triple, 2 pre-accept again with its command, 3 pre-accept a Noop"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        leader, number, bo, br = a32(leader), a32(number), a32(ballot_ordering), a32(ballot_replica)
        mask = np.ascontiguousarray(resp_mask, dtype=np.uint8)
        rs, rv, rt = a32(reply_status), a32(reply_vote), a32(reply_triple)
        m = len(leader)
        act, src, tr = (np.full(m, -9, np.int32) for _ in range(3))
        p = lambda a: a.ctypes.data
        st = self.L.fpx_epx_handle_prepare_oks(self._h, m, p(leader), p(number), p(bo), p(br), p(mask), p(rs), p(rv), p(rt),
                                               int(as_intended), p(act), p(src), p(tr))
        return st, act, src, tr

    def accept(self, leader, number, ballot_ordering, ballot_replica, triple_id, target_mask, key=None, is_set=None):
        """the Accept phase: (status, ok_bits, nack_bits, commit_bits, nack_ballot, committed).  key / is_set: the
        triples' commands (updateConflictIndex wherever the triple is stored); key None = every triple is a Noop"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        leader, number, bo, br, tr = a32(leader), a32(number), a32(ballot_ordering), a32(ballot_replica), a32(triple_id)
        tgt = np.ascontiguousarray(target_mask, dtype=np.uint8)
        m = len(leader)
        key = np.full(m, -1, np.int32) if key is None else a32(key)
        is_set = np.zeros(m, np.uint8) if is_set is None else np.ascontiguousarray(is_set, dtype=np.uint8)
        ok, nack, com, done = (np.zeros(m, np.uint8) for _ in range(4))
        nb = np.full(m, -1, np.int32)
        p = lambda a: a.ctypes.data
        st = self.L.fpx_epx_accept(self._h, m, p(leader), p(number), p(bo), p(br), p(tr), p(key), p(is_set), p(tgt),
                                   p(ok), p(nack), p(com), p(nb), p(done))
        return st, ok, nack, com, nb, done

    def handle_commit(self, leader, number, triple_id, target_mask, key=None, is_set=None, deps=None, deps_values_end=None):
        """Replica.handleCommit at the replicas of target_mask: CommittedEntry(triple) whatever was there, the conflict
        index learns the command.  key None = Noops; deps None = the triple is known by its id alone.  -> status"""
        a32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int32)
        leader, number, tr = a32(leader), a32(number), a32(triple_id)
        m = len(leader)
        tgt = np.ascontiguousarray(target_mask, dtype=np.uint8)
        key = np.full(m, -1, np.int32) if key is None else a32(key)
        is_set = np.zeros(m, np.uint8) if is_set is None else np.ascontiguousarray(is_set, dtype=np.uint8)
        d, de = a32(deps), a32(deps_values_end)
        p = lambda a: None if a is None else a.ctypes.data
        return self.L.fpx_epx_handle_commit(self._h, m, p(leader), p(number), p(tr), p(key), p(is_set), p(d), p(de), p(tgt))

    def handle_preaccept(self, leader, number, ballot_ordering, ballot_replica, key, is_set, triple_id, deps_in,
                         deps_in_values_end, target_mask):
        """Replica.handlePreAccept in full at the replicas of target_mask (key -1 = Noop): (status, ok_bits,
        resend_bits, nack_bits, commit_bits, nack_ballot, reply_deps[m, n, n], reply_values_end[m, n],
        reply_triple[m, n])"""
        a32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int32)
        leader, number, bo, br, key = a32(leader), a32(number), a32(ballot_ordering), a32(ballot_replica), a32(key)
        is_set = np.ascontiguousarray(is_set, dtype=np.uint8)
        tr, din, dend = a32(triple_id), a32(deps_in), a32(deps_in_values_end)
        tgt = np.ascontiguousarray(target_mask, dtype=np.uint8)
        m = len(leader)
        ok, resend, nack, com = (np.zeros(m, np.uint8) for _ in range(4))
        nb = np.full(m, -1, np.int32)
        rd = np.zeros((m, self.n, self.n), np.int32)
        re = np.zeros((m, self.n), np.int32)
        rt = np.full((m, self.n), -1, np.int32)
        p = lambda a: None if a is None else a.ctypes.data
        st = self.L.fpx_epx_handle_preaccept(self._h, m, p(leader), p(number), p(bo), p(br), p(key), p(is_set), p(tr),
                                             p(din), p(dend), p(tgt), p(ok), p(resend), p(nack), p(com), p(nb), p(rd),
                                             p(re), p(rt))
        return st, ok, resend, nack, com, nb, rd, re, rt

    # ---- multi-key commands (the _mk entry points): key_lists = one list of keys per command, or (key_offsets, keys) ----
    @staticmethod
    def key_lists(key_lists):
        """[[k, ...], ...] or (key_offsets[m + 1], keys) -> the CSR pair of int32 arrays"""
        if isinstance(key_lists, tuple) and len(key_lists) == 2 and all(isinstance(a, np.ndarray) for a in key_lists):
            return np.ascontiguousarray(key_lists[0], np.int32), np.ascontiguousarray(key_lists[1], np.int32)
        off = np.zeros(len(key_lists) + 1, np.int32)
        off[1:] = np.cumsum([len(k) for k in key_lists])
        keys = np.ascontiguousarray([k for ks in key_lists for k in ks], np.int32)
        return off, keys

    def preaccept_mk(self, leader, number, key_lists, is_set, resp_mask, rank, seen_mask=None, triple_id=None):
        """preaccept() with any number of keys per command: (status, fast, deps, leader_deps, own_values_end)"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        a8 = lambda x: np.ascontiguousarray(x, dtype=np.uint8)
        off, keys = self.key_lists(key_lists)
        leader, number, rank = a32(leader), a32(number), a32(rank)
        is_set, resp_mask = a8(is_set), a8(resp_mask)
        seen_mask = None if seen_mask is None else a8(seen_mask)
        triple_id = None if triple_id is None else a32(triple_id)
        m = len(leader)
        fast = np.zeros(m, np.uint8)
        deps, ldeps = np.zeros((m, self.n), np.int32), np.zeros((m, self.n), np.int32)
        own = np.zeros((m, 2), np.int32)
        p = lambda a: None if a is None else a.ctypes.data
        st = self.L.fpx_epx_preaccept_mk(self._h, m, p(leader), p(number), p(off), p(keys), p(is_set), p(resp_mask),
                                         p(seen_mask), p(rank), p(triple_id), p(fast), p(deps), p(ldeps), p(own))
        return st, fast, deps, ldeps, own

    def preaccept_mk_dev(self, leader, number, key_offsets, keys, is_set, resp_mask, rank, fast=None, deps=None,
                         leader_deps=None, seen_mask=None, own_values_end=None, triple_id=None):
        d = lambda t: None if t is None else t.data_ptr()
        st = self.L.fpx_epx_preaccept_mk_dev(self._h, leader.numel(), d(leader), d(number), d(key_offsets), d(keys),
                                             d(is_set), d(resp_mask), d(seen_mask), d(rank), d(triple_id), d(fast), d(deps),
                                             d(leader_deps), d(own_values_end))
        if st:
            raise FpxError(st, "fpx_epx_preaccept_mk_dev")

    def preaccept_mk_packed_dev(self, leader, number, key_offsets, keys, is_set, resp_mask, rank, packed, seen_mask=None,
                                triple_id=None):
        d = lambda t: None if t is None else t.data_ptr()
        st = self.L.fpx_epx_preaccept_mk_packed_dev(self._h, leader.numel(), d(leader), d(number), d(key_offsets), d(keys),
                                                    d(is_set), d(resp_mask), d(seen_mask), d(rank), d(triple_id), d(packed))
        if st:
            raise FpxError(st, "fpx_epx_preaccept_mk_packed_dev")

    def handle_preaccept_mk(self, leader, number, ballot_ordering, ballot_replica, key_lists, is_set, triple_id, deps_in,
                            deps_in_values_end, target_mask):
        """handle_preaccept() with a key list per command (an empty list: no conflicts, no put)"""
        a32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int32)
        off, keys = self.key_lists(key_lists)
        leader, number, bo, br = a32(leader), a32(number), a32(ballot_ordering), a32(ballot_replica)
        is_set = np.ascontiguousarray(is_set, dtype=np.uint8)
        tr, din, dend = a32(triple_id), a32(deps_in), a32(deps_in_values_end)
        tgt = np.ascontiguousarray(target_mask, dtype=np.uint8)
        m = len(leader)
        ok, resend, nack, com = (np.zeros(m, np.uint8) for _ in range(4))
        nb = np.full(m, -1, np.int32)
        rd = np.zeros((m, self.n, self.n), np.int32)
        re = np.zeros((m, self.n), np.int32)
        rt = np.full((m, self.n), -1, np.int32)
        p = lambda a: None if a is None else a.ctypes.data
        st = self.L.fpx_epx_handle_preaccept_mk(self._h, m, p(leader), p(number), p(bo), p(br), p(off), p(keys), p(is_set),
                                                p(tr), p(din), p(dend), p(tgt), p(ok), p(resend), p(nack), p(com), p(nb),
                                                p(rd), p(re), p(rt))
        return st, ok, resend, nack, com, nb, rd, re, rt

    def accept_mk(self, leader, number, ballot_ordering, ballot_replica, triple_id, target_mask, key_lists, is_set):
        """accept() with a key list per triple: (status, ok_bits, nack_bits, commit_bits, nack_ballot, committed)"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        off, keys = self.key_lists(key_lists)
        leader, number, bo, br, tr = a32(leader), a32(number), a32(ballot_ordering), a32(ballot_replica), a32(triple_id)
        tgt = np.ascontiguousarray(target_mask, dtype=np.uint8)
        is_set = np.ascontiguousarray(is_set, dtype=np.uint8)
        m = len(leader)
        ok, nack, com, done = (np.zeros(m, np.uint8) for _ in range(4))
        nb = np.full(m, -1, np.int32)
        p = lambda a: a.ctypes.data
        st = self.L.fpx_epx_accept_mk(self._h, m, p(leader), p(number), p(bo), p(br), p(tr), p(off), p(keys), p(is_set),
                                      p(tgt), p(ok), p(nack), p(com), p(nb), p(done))
        return st, ok, nack, com, nb, done

    def handle_commit_mk(self, leader, number, triple_id, target_mask, key_lists, is_set, deps=None, deps_values_end=None):
        """handle_commit() with a key list per triple -> status"""
        a32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int32)
        off, keys = self.key_lists(key_lists)
        leader, number, tr = a32(leader), a32(number), a32(triple_id)
        m = len(leader)
        tgt = np.ascontiguousarray(target_mask, dtype=np.uint8)
        is_set = np.ascontiguousarray(is_set, dtype=np.uint8)
        d, de = a32(deps), a32(deps_values_end)
        p = lambda a: None if a is None else a.ctypes.data
        return self.L.fpx_epx_handle_commit_mk(self._h, m, p(leader), p(number), p(tr), p(off), p(keys), p(is_set), p(d), p(de),
                                               p(tgt))

    # ---- the leader half (leader_state=True) ----
    def lead(self, leader, number, at, ballot_ordering, key, is_set, triple_id, avoid_fast_path=None):
        """transitionToPreAcceptPhase of instance (leader, number) at replica `at` in ballot (ballot_ordering, at), key -1 =
        Noop: (status, deps[m, n], deps_values_end[m]) -- the dependencies of the PreAccept to send"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        leader, number, at, bo, key, tr = a32(leader), a32(number), a32(at), a32(ballot_ordering), a32(key), a32(triple_id)
        m = len(leader)
        is_set = np.ascontiguousarray(is_set, dtype=np.uint8)
        avoid = np.zeros(m, np.uint8) if avoid_fast_path is None else np.ascontiguousarray(avoid_fast_path, dtype=np.uint8)
        deps, dend = np.zeros((m, self.n), np.int32), np.zeros(m, np.int32)
        p = lambda a: a.ctypes.data
        st = self.L.fpx_epx_lead(self._h, m, p(leader), p(number), p(at), p(bo), p(key), p(is_set), p(tr), p(avoid), p(deps),
                                 p(dend))
        return st, deps, dend

    def lead_mk(self, leader, number, at, ballot_ordering, key_lists, is_set, triple_id, avoid_fast_path=None):
        """lead() with a key list per command (an empty list: no conflicts, no put); the leader state keeps the key, -1 or
        KEY_LIST for one / no / several distinct keys"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        off, keys = self.key_lists(key_lists)
        leader, number, at, bo, tr = a32(leader), a32(number), a32(at), a32(ballot_ordering), a32(triple_id)
        m = len(leader)
        is_set = np.ascontiguousarray(is_set, dtype=np.uint8)
        avoid = np.zeros(m, np.uint8) if avoid_fast_path is None else np.ascontiguousarray(avoid_fast_path, dtype=np.uint8)
        deps, dend = np.zeros((m, self.n), np.int32), np.zeros(m, np.int32)
        p = lambda a: a.ctypes.data
        st = self.L.fpx_epx_lead_mk(self._h, m, p(leader), p(number), p(at), p(bo), p(off), p(keys), p(is_set), p(tr), p(avoid),
                                    p(deps), p(dend))
        return st, deps, dend

    def leader_replies(self, kind, to, leader, number, ballot_ordering, ballot_replica, replica_index, sequence_number=None,
                       deps=None, deps_values_end=None):
        """one burst of PreAcceptOk (0) / AcceptOk (1) / Nack (2) / defaultToSlowPath-timer (3) events in delivery order:
        (status, outcome[m], out_seq[m], out_deps[m, n], out_values_end[m], out_triple[m], decided_index[num_decided])"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        kind, to, leader, number = a32(kind), a32(to), a32(leader), a32(number)
        bo, br, ridx = a32(ballot_ordering), a32(ballot_replica), a32(replica_index)
        m = len(kind)
        seq = None if sequence_number is None else a32(sequence_number)
        deps = np.zeros((m, self.n), np.int32) if deps is None else a32(deps)
        dend = None if deps_values_end is None else a32(deps_values_end)
        outcome, oseq, oend, otr, dec = (np.full(m, -9, np.int32) for _ in range(5))
        odeps = np.full((m, self.n), -9, np.int32)
        nd = np.full(1, -9, np.int32)
        p = lambda a: None if a is None else a.ctypes.data
        st = self.L.fpx_epx_leader_replies(self._h, m, p(kind), p(to), p(leader), p(number), p(bo), p(br), p(ridx), p(seq),
                                           p(deps), p(dend), p(outcome), p(oseq), p(odeps), p(oend), p(otr), p(dec), p(nd))
        return st, outcome, oseq, odeps, oend, otr, dec[:max(int(nd[0]), 0)]

    def leader_replies_dev(self, kind, to, leader, number, ballot_ordering, ballot_replica, replica_index, sequence_number,
                           deps, deps_values_end, outcome=None, out_seq=None, out_deps=None, out_values_end=None,
                           out_triple=None, decided_index=None, num_decided=None):
        """the same on device tensors (int32), enqueued on the context's stream; the status comes with sync()"""
        d = lambda t: None if t is None else t.data_ptr()
        st = self.L.fpx_epx_leader_replies_dev(self._h, kind.numel(), d(kind), d(to), d(leader), d(number), d(ballot_ordering),
                                               d(ballot_replica), d(replica_index), d(sequence_number), d(deps),
                                               d(deps_values_end), d(outcome), d(out_seq), d(out_deps), d(out_values_end),
                                               d(out_triple), d(decided_index), d(num_decided))
        if st:
            raise FpxError(st, "fpx_epx_leader_replies_dev")

    # ---- a leader's reply burst from wire bytes (include/fpx_wire.h) ----
    def wire_decode_dev_tensors(self, buf, buf_len, offsets, n, only_kind=False):
        """fpx_wire_epaxos_decode_replica_inbound_dev on device tensors (buf uint8, offsets int64), enqueued on the
        context's stream: a dict of device tensors (wire.EPX_FOLDED_NAMES, and bad_index[1]); the status comes with sync()"""
        import torch

        from . import wire
        L = wire._L()
        out = {}
        for k in wire.EPX_FOLDED_NAMES:
            if only_kind and k != "kind":
                continue
            shape = (n, self.n) if k == "deps_watermark" else (n,)
            out[k] = torch.zeros(shape, dtype=torch.int64 if k == "cmd_off" else torch.int32, device=buf.device)
        out["bad_index"] = torch.full((1,), -9, dtype=torch.int32, device=buf.device)
        st = L.fpx_wire_epaxos_decode_replica_inbound_dev(
            self._h, buf.data_ptr(), buf_len, offsets.data_ptr(), n,
            *[out[k].data_ptr() if k in out else None for k in wire.EPX_FOLDED_NAMES], out["bad_index"].data_ptr())
        if st:
            raise FpxError(st, "fpx_wire_epaxos_decode_replica_inbound_dev")
        return out

    def wire_decode_dev(self, messages, offsets=None, only_kind=False):
        """the device decoder on a tick of serialised ReplicaInbound messages: the bytes and offsets are uploaded, the
        arrays come back as numpy arrays, with status_code (what sync() gave) and bad_index"""
        import torch

        from . import wire
        buf, off = wire.pack(messages)
        n = len(messages)
        if offsets is not None:
            off = np.ascontiguousarray(offsets, np.int64)
            n = len(off) - 1
        dev = torch.device("cuda", torch.cuda.current_device())
        d_buf, d_off = torch.from_numpy(buf).to(dev), torch.from_numpy(off).to(dev)
        torch.cuda.synchronize()
        t = self.wire_decode_dev_tensors(d_buf, sum(len(m) for m in messages), d_off, n, only_kind)
        st = self.sync()
        out = {k: v.cpu().numpy() for k, v in t.items()}
        out["status_code"], out["bad_index"] = st, int(out["bad_index"][0])
        return out

    def wire_leader_tick(self, messages, to, offsets=None):
        """fpx_wire_epx_leader_tick: a burst of serialised PreAcceptOk / AcceptOk / Nack messages, to[i] the replica that
        received message i -> what leader_replies returns for the decoded burst, plus bad_index:
        (status, outcome[m], out_seq[m], out_deps[m, n], out_values_end[m], out_triple[m], decided_index[num_decided],
        bad_index); on FPX_EINVAL the outputs keep their fill of -9"""
        from . import wire
        L = wire._L()
        buf, off = wire.pack(messages)
        m = len(messages)
        if offsets is not None:
            off = np.ascontiguousarray(offsets, np.int64)
            m = len(off) - 1
        to = np.ascontiguousarray(to, dtype=np.int32)
        outcome, oseq, oend, otr, dec = (np.full(m, -9, np.int32) for _ in range(5))
        odeps = np.full((m, self.n), -9, np.int32)
        nd = np.full(1, -9, np.int32)
        bad = C.c_int32(-9)
        p = lambda a: a.ctypes.data
        st = L.fpx_wire_epx_leader_tick(self._h, p(buf), sum(len(x) for x in messages), p(off), m, p(to), p(outcome), p(oseq),
                                        p(odeps), p(oend), p(otr), p(dec), p(nd), C.byref(bad))
        return st, outcome, oseq, odeps, oend, otr, dec[:max(int(nd[0]), 0)], bad.value

    # ---- the key table and a replica's inbox from wire bytes (include/fpx.h fpx_epx_keys_*, include/fpx_wire.h) ----
    KEY_MAX_LEN = 4096    # FPX_EPX_KEY_MAX_LEN

    def keys_enable(self, arena_bytes):
        """fpx_epx_keys_enable: the context keeps the key strings -> key ids map on the device, arena_bytes for the strings"""
        st = self.L.fpx_epx_keys_enable(self._h, int(arena_bytes))
        if st:
            raise FpxError(st, "fpx_epx_keys_enable")

    def keys_count(self):
        """(ids handed out, arena bytes used)"""
        n, used = C.c_int32(0), C.c_int64(0)
        st = self.L.fpx_epx_keys_count(self._h, C.byref(n), C.byref(used))
        if st:
            raise FpxError(st, "fpx_epx_keys_count")
        return n.value, used.value

    @staticmethod
    def pack_keys(keys):
        """a list of bytes -> (bytes uint8, off int64, len int32), back to back"""
        ln = np.array([len(k) for k in keys], np.int32)
        off = np.zeros(len(keys), np.int64)
        if len(keys):
            off[1:] = np.cumsum(ln[:-1], dtype=np.int64)
        return np.frombuffer(b"".join(bytes(k) for k in keys), np.uint8).copy(), off, ln

    def keys_intern(self, keys=None, packed=None):
        """fpx_epx_keys_intern on a list of bytes (or packed = (bytes, off, len) arrays): (status, ids[P]); the ids of a
        refused batch keep their fill of -9"""
        buf, off, ln = self.pack_keys(keys) if packed is None else packed
        buf = np.ascontiguousarray(buf, np.uint8)
        off, ln = np.ascontiguousarray(off, np.int64), np.ascontiguousarray(ln, np.int32)
        ids = np.full(len(off), -9, np.int32)
        st = self.L.fpx_epx_keys_intern(self._h, buf.ctypes.data if len(buf) else None, len(buf), off.ctypes.data, ln.ctypes.data,
                                        len(off), ids.ctypes.data)
        return st, ids

    def keys_intern_dev(self, buf, off, ln, ids, buf_len=None):
        """fpx_epx_keys_intern_dev on device tensors (uint8, int64, int32 -> int32), enqueued; the status comes with sync()"""
        st = self.L.fpx_epx_keys_intern_dev(self._h, buf.data_ptr(), buf.numel() if buf_len is None else buf_len, off.data_ptr(),
                                            ln.data_ptr(), off.numel(), ids.data_ptr())
        if st:
            raise FpxError(st, "fpx_epx_keys_intern_dev")

    def keys_read(self, first_id=0, n=None):
        """fpx_epx_keys_read: the keys of ids first_id .. first_id + n - 1 (default: all) as a list of bytes"""
        if n is None:
            n = self.keys_count()[0] - first_id
        off = np.zeros(n + 1, np.int32)
        out = np.zeros(1, np.uint8)
        st = self.L.fpx_epx_keys_read(self._h, first_id, n, off.ctypes.data, out.ctypes.data, 0)
        if st == _lib.FPX_ECAPACITY:
            out = np.zeros(int(off[n]), np.uint8)
            st = self.L.fpx_epx_keys_read(self._h, first_id, n, off.ctypes.data, out.ctypes.data, len(out))
        if st:
            raise FpxError(st, "fpx_epx_keys_read")
        return [out[off[j]:off[j + 1]].tobytes() for j in range(n)]

    # ---- the command store (include/fpx.h fpx_epx_cmds_*) ----
    CMD_MAX_LEN = 1 << 16    # FPX_EPX_CMD_MAX_LEN

    def cmds_enable(self, max_triples, arena_bytes):
        """fpx_epx_cmds_enable: the context keeps the triples' serialised commands on the device, by triple id"""
        st = self.L.fpx_epx_cmds_enable(self._h, int(max_triples), int(arena_bytes))
        if st:
            raise FpxError(st, "fpx_epx_cmds_enable")

    def cmds_put(self, commands=None, triple_id=None, packed=None):
        """fpx_epx_cmds_put on a list of bytes (or packed = (bytes, off, len) arrays) and their triple ids:
        (status, result[4] = new commands, new bytes, skipped, refused; on FPX_EINVAL -1 and the bad index)"""
        buf, off, ln = self.pack_keys(commands) if packed is None else packed
        buf = np.ascontiguousarray(buf, np.uint8)
        off, ln = np.ascontiguousarray(off, np.int64), np.ascontiguousarray(ln, np.int32)
        tr = np.ascontiguousarray(triple_id, np.int32)
        assert len(tr) == len(off) == len(ln)
        res = np.full(4, -9, np.int64)
        st = self.L.fpx_epx_cmds_put(self._h, buf.ctypes.data if len(buf) else None, len(buf), off.ctypes.data, ln.ctypes.data,
                                     tr.ctypes.data, len(off), res.ctypes.data)
        return st, res

    def cmds_put_dev(self, buf, off, ln, triple_id, result, buf_len=None):
        """fpx_epx_cmds_put_dev on device tensors (uint8, int64, int32, int32 -> int64[4]), enqueued; the status comes with
        sync()"""
        st = self.L.fpx_epx_cmds_put_dev(self._h, buf.data_ptr(), buf.numel() if buf_len is None else buf_len, off.data_ptr(),
                                         ln.data_ptr(), triple_id.data_ptr(), off.numel(), result.data_ptr())
        if st:
            raise FpxError(st, "fpx_epx_cmds_put_dev")

    def cmds_read(self, triple_id):
        """fpx_epx_cmds_read: the stored bytes of one triple id, None when it has none"""
        n = C.c_int32(0)
        st = self.L.fpx_epx_cmds_read(self._h, int(triple_id), None, 0, C.byref(n))
        if st == _lib.FPX_ECAPACITY:
            out = np.zeros(n.value, np.uint8)
            st = self.L.fpx_epx_cmds_read(self._h, int(triple_id), out.ctypes.data, len(out), C.byref(n))
            if st == 0:
                return out.tobytes()
        if st:
            raise FpxError(st, "fpx_epx_cmds_read")
        return None if n.value < 0 else b""

    def cmds_stats(self):
        """fpx_epx_cmds_stats: (commands stored, arena bytes used, records skipped so far, bursts refused so far)"""
        out = np.zeros(4, np.int64)
        st = self.L.fpx_epx_cmds_stats(self._h, out.ctypes.data)
        if st:
            raise FpxError(st, "fpx_epx_cmds_stats")
        return tuple(int(x) for x in out)

    def wire_classify_dev(self, buf, cmd_off, cmd_len, max_pairs):
        """fpx_wire_epx_classify_dev on the serialised CommandOrNoops cmd_off / cmd_len locate in buf (uint8 array; all
        uploaded): a dict of numpy arrays key_offsets[m + 1], keys[num_pairs] (ids), is_set, is_noop, cmd_shape, result[4]
        (bad index, num_pairs, new keys, new bytes) and status_code (what sync() gave)"""
        import torch

        from . import wire
        L = wire._L()
        dev = torch.device("cuda", torch.cuda.current_device())
        up = lambda a, t: torch.from_numpy(np.array(a, dtype=t)).to(dev)
        m = len(cmd_off)
        d_buf = up(buf if len(buf) else np.zeros(1, np.uint8), np.uint8)
        d_off, d_len = up(cmd_off, np.int64), up(cmd_len, np.int32)
        z = lambda k, t: torch.full((max(k, 1),), -9, dtype=t, device=dev)
        koff, keys, iset = z(m + 1, torch.int32), z(max_pairs, torch.int32), z(m, torch.uint8)
        noop, shape, res = z(m, torch.int32), z(m, torch.int32), z(4, torch.int32)
        torch.cuda.synchronize()
        st = L.fpx_wire_epx_classify_dev(self._h, d_buf.data_ptr(), len(buf), d_off.data_ptr(), d_len.data_ptr(), m, max_pairs,
                                         koff.data_ptr(), keys.data_ptr(), iset.data_ptr(), noop.data_ptr(), shape.data_ptr(),
                                         res.data_ptr())
        if st:
            raise FpxError(st, "fpx_wire_epx_classify_dev")
        st = self.sync()
        res = res.cpu().numpy()
        P = int(res[1]) if st == 0 else 0
        return {"key_offsets": koff.cpu().numpy()[:m + 1], "keys": keys.cpu().numpy()[:P], "is_set": iset.cpu().numpy()[:m],
                "is_noop": noop.cpu().numpy()[:m], "cmd_shape": shape.cpu().numpy()[:m], "result": res, "status_code": st}

    def wire_replica_tick(self, messages, to, max_pairs, triple_base=0, triple_id=None, offsets=None):
        """fpx_wire_epx_replica_tick: a burst of serialised PreAccept / Accept / Commit / Prepare messages, to[i] the replica
        that received message i -> what replica_inbox_mk returns for the decoded burst, plus bad_index and num_pairs:
        (status, outcome[m], out_ballot[m], out_status[m], out_deps[m, n], out_values_end[m], out_triple[m], bad_index,
        num_pairs); on a refusal the outputs keep their fill of -9"""
        from . import wire
        L = wire._L()
        buf, off = wire.pack(messages)
        m = len(messages)
        if offsets is not None:
            off = np.ascontiguousarray(offsets, np.int64)
            m = len(off) - 1
        to = np.ascontiguousarray(to, dtype=np.int32)
        tr = None if triple_id is None else np.ascontiguousarray(triple_id, dtype=np.int32)
        outcome, ob, os_, oend, otr = (np.full(m, -9, np.int32) for _ in range(5))
        odeps = np.full((m, self.n), -9, np.int32)
        bad, npairs = C.c_int32(-9), C.c_int32(-9)
        p = lambda a: None if a is None else a.ctypes.data
        st = L.fpx_wire_epx_replica_tick(self._h, p(buf), sum(len(x) for x in messages), p(off), m, p(to), triple_base, p(tr),
                                         max_pairs, p(outcome), p(ob), p(os_), p(odeps), p(oend), p(otr), C.byref(bad),
                                         C.byref(npairs))
        return st, outcome, ob, os_, odeps, oend, otr, bad.value, npairs.value

    def wire_replica_tick_dev(self, buf, buf_len, offsets, to, max_pairs, triple_base=0, triple_id=None, outcome=None,
                              out_ballot=None, out_status=None, out_deps=None, out_values_end=None, out_triple=None,
                              bad_index=None, num_pairs=None):
        """the same on device tensors (buf uint8, offsets int64[m + 1], the rest int32); bad_index[1] is required.  ONE host
        wait inside (the pair count); the status comes with sync()"""
        from . import wire
        L = wire._L()
        d = lambda t: None if t is None else t.data_ptr()
        st = L.fpx_wire_epx_replica_tick_dev(self._h, d(buf), buf_len, d(offsets), offsets.numel() - 1, d(to), triple_base,
                                             d(triple_id), max_pairs, d(outcome), d(out_ballot), d(out_status), d(out_deps),
                                             d(out_values_end), d(out_triple), d(bad_index), d(num_pairs))
        if st:
            raise FpxError(st, "fpx_wire_epx_replica_tick_dev")

    # ---- a replica tick's replies as wire bytes ----
    def encode_replica_replies_dev(self, to, leader, number, ballot_ordering, ballot_replica, outcome, out_ballot, out_status,
                                   out_deps, out_values_end, out, cap, out_offsets, reply_kind, totals, m=None):
        """fpx_wire_epx_encode_replica_replies_dev on device tensors (the ten record arrays int32, out uint8 or None for the
        sizing call, out_offsets int64[m + 1], reply_kind uint8[m], totals int64[4]), enqueued: no host wait, the status comes
        with sync().  m: the number of records (default: to.numel())"""
        from . import wire
        L = wire._L()
        d = lambda t: None if t is None else t.data_ptr()
        st = L.fpx_wire_epx_encode_replica_replies_dev(
            self._h, to.numel() if m is None else m, d(to), d(leader), d(number), d(ballot_ordering), d(ballot_replica), d(outcome),
            d(out_ballot), d(out_status), d(out_deps), d(out_values_end), d(out), cap, d(out_offsets), d(reply_kind), d(totals))
        if st:
            raise FpxError(st, "fpx_wire_epx_encode_replica_replies_dev")

    def encode_replica_replies_cmds_dev(self, to, leader, number, ballot_ordering, ballot_replica, outcome, out_ballot,
                                        out_status, out_deps, out_values_end, out_triple, out, cap, out_offsets, reply_kind,
                                        totals, m=None):
        """fpx_wire_epx_encode_replica_replies_cmds_dev: encode_replica_replies_dev with out_triple (int32[m]); the replies
        that carry a stored command are encoded from the context's command store"""
        from . import wire
        L = wire._L()
        d = lambda t: None if t is None else t.data_ptr()
        st = L.fpx_wire_epx_encode_replica_replies_cmds_dev(
            self._h, to.numel() if m is None else m, d(to), d(leader), d(number), d(ballot_ordering), d(ballot_replica), d(outcome),
            d(out_ballot), d(out_status), d(out_deps), d(out_values_end), d(out_triple), d(out), cap, d(out_offsets), d(reply_kind),
            d(totals))
        if st:
            raise FpxError(st, "fpx_wire_epx_encode_replica_replies_cmds_dev")

    def encode_replica_replies(self, cap=None, base_offset=0, out_triple=None, **arrays):
        """the device encoder on host arrays (the ten of wire.EPX_REPLY_RECORDS): upload, encode, sync, download.  The result
        is wire.epx_encode_replica_replies's dict, with the same fills where the call writes nothing.  cap None: sized by a
        first call; base_offset: the output starts that many bytes behind a 256-byte boundary; out_triple: the _cmds_dev
        call with these triple ids"""
        import torch

        from . import wire
        rec = wire.epx_reply_records(self.n, **arrays)
        m = len(rec[0])
        dev = torch.device("cuda", torch.cuda.current_device())
        up = [torch.from_numpy(a.reshape(-1) if a.size else np.zeros(1, np.int32)).to(dev) for a in rec]
        if out_triple is not None:
            tr = np.ascontiguousarray(out_triple, np.int32)
            up.append(torch.from_numpy(tr if tr.size else np.zeros(1, np.int32)).to(dev))
            encode = self.encode_replica_replies_cmds_dev
        else:
            encode = self.encode_replica_replies_dev
        off = torch.full((m + 1,), -9, dtype=torch.int64, device=dev)
        kind = torch.full((max(m, 1),), 9, dtype=torch.uint8, device=dev)
        totals = torch.full((4,), -9, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        if cap is None:
            encode(*up, None, 0, off, kind, totals, m=m)
            st = self.sync()
            if st not in (0, _lib.FPX_ECAPACITY):
                return {"status_code": st, "out": np.zeros(0, np.uint8), "out_offsets": off.cpu().numpy(),
                        "reply_kind": kind.cpu().numpy()[:m], "totals": totals.cpu().numpy(), "replies": []}
            cap = int(totals.cpu()[1])
            off.fill_(-9), kind.fill_(9)
        buf = torch.full((base_offset + cap + 16,), 0xEE, dtype=torch.uint8, device=dev)
        out = buf[base_offset:]
        torch.cuda.synchronize()
        encode(*up, out if cap > 0 else None, cap, off, kind, totals, m=m)
        st = self.sync()
        whole = buf.cpu().numpy()
        o, off = whole[base_offset:base_offset + cap], off.cpu().numpy()
        replies = [o[int(off[i]):int(off[i + 1])].tobytes() for i in range(m)] if st == 0 else []
        return {"status_code": st, "out": o, "out_offsets": off, "reply_kind": kind.cpu().numpy()[:m],
                "totals": totals.cpu().numpy(), "replies": replies, "around": (whole[:base_offset], whole[base_offset + cap:])}

    def wire_replica_tick_bytes(self, messages, to, max_pairs, out_cap=None, triple_base=0, triple_id=None, offsets=None,
                                soa=True):
        """fpx_wire_epx_replica_tick_bytes: wire_replica_tick, and the replies as wire bytes.  A dict: status_code, out
        (uint8[out_cap]), out_offsets, reply_kind, totals, replies (per-message bytes, on FPX_OK), bad_index, num_pairs, and
        with soa the six struct-of-arrays outputs of wire_replica_tick (outcome, out_ballot, out_status, out_deps,
        out_values_end, out_triple); what the call leaves alone keeps its fill (-9; kinds 9; bytes 0xEE).  out_cap None:
        len(messages) x wire.EPX_REPLY_MAX"""
        from . import wire
        L = wire._L()
        buf, off = wire.pack(messages)
        m = len(messages)
        if offsets is not None:
            off = np.ascontiguousarray(offsets, np.int64)
            m = len(off) - 1
        to = np.ascontiguousarray(to, dtype=np.int32)
        tr = None if triple_id is None else np.ascontiguousarray(triple_id, dtype=np.int32)
        cap = m * wire.EPX_REPLY_MAX if out_cap is None else out_cap
        out, ooff, kind = np.full(max(cap, 1), 0xEE, np.uint8), np.full(m + 1, -9, np.int64), np.full(max(m, 1), 9, np.uint8)
        totals = np.full(4, -9, np.int64)
        names = ("outcome", "out_ballot", "out_status", "out_deps", "out_values_end", "out_triple")
        arr = {k: (np.full((m, self.n) if k == "out_deps" else m, -9, np.int32) if soa else None) for k in names}
        bad, npairs = C.c_int32(-9), C.c_int32(-9)
        p = lambda a: None if a is None else a.ctypes.data
        st = L.fpx_wire_epx_replica_tick_bytes(self._h, p(buf), sum(len(x) for x in messages), p(off), m, p(to), triple_base, p(tr),
                                               max_pairs, p(out) if cap > 0 else None, cap, p(ooff), p(kind), p(totals),
                                               *[p(arr[k]) for k in names], C.byref(bad), C.byref(npairs))
        replies = [out[int(ooff[i]):int(ooff[i + 1])].tobytes() for i in range(m)] if st == 0 else []
        res = {"status_code": st, "out": out[:cap], "out_offsets": ooff, "reply_kind": kind[:m], "totals": totals,
               "replies": replies, "bad_index": bad.value, "num_pairs": npairs.value}
        res.update(arr)
        return res

    def wire_replica_tick_bytes_dev(self, buf, buf_len, offsets, to, max_pairs, out, out_cap, out_offsets, reply_kind, totals,
                                    triple_base=0, triple_id=None, outcome=None, out_ballot=None, out_status=None,
                                    out_deps=None, out_values_end=None, out_triple=None, bad_index=None, num_pairs=None):
        """the same on device tensors (buf, out, reply_kind uint8; offsets, out_offsets, totals int64; the rest int32);
        bad_index[1] is required, the six struct-of-arrays outputs are optional.  ONE host wait inside (the pair count);
        the status comes with sync()"""
        from . import wire
        L = wire._L()
        d = lambda t: None if t is None else t.data_ptr()
        st = L.fpx_wire_epx_replica_tick_bytes_dev(self._h, d(buf), buf_len, d(offsets), offsets.numel() - 1, d(to), triple_base,
                                                   d(triple_id), max_pairs, d(out), out_cap, d(out_offsets), d(reply_kind),
                                                   d(totals), d(outcome), d(out_ballot), d(out_status), d(out_deps),
                                                   d(out_values_end), d(out_triple), d(bad_index), d(num_pairs))
        if st:
            raise FpxError(st, "fpx_wire_epx_replica_tick_bytes_dev")

    # ---- originating recovery (recovery=True) ----
    def recover(self, leader, number, at):
        """transitionToPreparePhase of instance (leader, number) at replica `at`, its own Prepare delivered at once:
        (status, outcome[m], ballot_ordering[m] of the Prepare to send, and the own PrepareOk: status[m], vote_ballot[m]
        encoded, triple[m]); on FPX_EINVAL the outputs keep their fill of -9"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        leader, number, at = a32(leader), a32(number), a32(at)
        m = len(leader)
        outcome, ord_, os_, ov, ot = (np.full(m, -9, np.int32) for _ in range(5))
        p = lambda a: a.ctypes.data
        st = self.L.fpx_epx_recover(self._h, m, p(leader), p(number), p(at), p(outcome), p(ord_), p(os_), p(ov), p(ot))
        return st, outcome, ord_, os_, ov, ot

    def recovery_replies(self, to, leader, number, ballot_ordering, ballot_replica, replica_index, status,
                         vote_ballot_ordering, vote_ballot_replica, triple_id, sequence_number=None, deps=None,
                         deps_values_end=None, as_intended=False):
        """one burst of PrepareOks in delivery order: (status, outcome[m], source[m], triple[m], ballot[m], out_seq[m],
        out_deps[m, n], out_values_end[m], decided_index[num_decided])"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        to, leader, number = a32(to), a32(leader), a32(number)
        bo, br, ridx, stt = a32(ballot_ordering), a32(ballot_replica), a32(replica_index), a32(status)
        vo, vr, tr = a32(vote_ballot_ordering), a32(vote_ballot_replica), a32(triple_id)
        m = len(to)
        seq = None if sequence_number is None else a32(sequence_number)
        deps = np.zeros((m, self.n), np.int32) if deps is None else a32(deps)
        dend = None if deps_values_end is None else a32(deps_values_end)
        outcome, src, otr, ob, oseq, oend, dec = (np.full(m, -9, np.int32) for _ in range(7))
        odeps = np.full((m, self.n), -9, np.int32)
        nd = np.full(1, -9, np.int32)
        p = lambda a: None if a is None else a.ctypes.data
        st = self.L.fpx_epx_recovery_replies(self._h, m, p(to), p(leader), p(number), p(bo), p(br), p(ridx), p(stt), p(vo), p(vr),
                                             p(tr), p(seq), p(deps), p(dend), 1 if as_intended else 0, p(outcome), p(src),
                                             p(otr), p(ob), p(oseq), p(odeps), p(oend), p(dec), p(nd))
        return st, outcome, src, otr, ob, oseq, odeps, oend, dec[:max(int(nd[0]), 0)]

    def recovery_replies_dev(self, to, leader, number, ballot_ordering, ballot_replica, replica_index, status,
                             vote_ballot_ordering, vote_ballot_replica, triple_id, sequence_number, deps, deps_values_end,
                             as_intended=False, outcome=None, out_source=None, out_triple=None, out_ballot=None, out_seq=None,
                             out_deps=None, out_values_end=None, decided_index=None, num_decided=None):
        """the same on device tensors (int32), enqueued on the context's stream; the status comes with sync()"""
        d = lambda t: None if t is None else t.data_ptr()
        st = self.L.fpx_epx_recovery_replies_dev(self._h, to.numel(), d(to), d(leader), d(number), d(ballot_ordering),
                                                 d(ballot_replica), d(replica_index), d(status), d(vote_ballot_ordering),
                                                 d(vote_ballot_replica), d(triple_id), d(sequence_number), d(deps),
                                                 d(deps_values_end), 1 if as_intended else 0, d(outcome), d(out_source),
                                                 d(out_triple), d(out_ballot), d(out_seq), d(out_deps), d(out_values_end),
                                                 d(decided_index), d(num_decided))
        if st:
            raise FpxError(st, "fpx_epx_recovery_replies_dev")

    def lead_accept(self, leader, number, at, ballot_ordering, key, is_set, triple_id, sequence_number, deps,
                    deps_values_end=None):
        """transitionToAcceptPhase of instance (leader, number) at replica `at` in ballot (ballot_ordering, at) with the triple
        (triple_id, sequence_number, deps[m, n], deps_values_end) -> status"""
        a32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int32)
        leader, number, at, bo, key, tr = a32(leader), a32(number), a32(at), a32(ballot_ordering), a32(key), a32(triple_id)
        m = len(leader)
        is_set = np.ascontiguousarray(is_set, dtype=np.uint8)
        seq, dend = a32(sequence_number), a32(deps_values_end)
        deps = a32(deps).reshape(m, self.n)
        p = lambda a: None if a is None else a.ctypes.data
        return self.L.fpx_epx_lead_accept(self._h, m, p(leader), p(number), p(at), p(bo), p(key), p(is_set), p(tr), p(seq),
                                          p(deps), p(dend))

    def lead_accept_mk(self, leader, number, at, ballot_ordering, key_lists, is_set, triple_id, sequence_number, deps,
                       deps_values_end=None):
        """lead_accept() with a key list per triple -> status"""
        a32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int32)
        off, keys = self.key_lists(key_lists)
        leader, number, at, bo, tr = a32(leader), a32(number), a32(at), a32(ballot_ordering), a32(triple_id)
        m = len(leader)
        is_set = np.ascontiguousarray(is_set, dtype=np.uint8)
        seq, dend = a32(sequence_number), a32(deps_values_end)
        deps = a32(deps).reshape(m, self.n)
        p = lambda a: None if a is None else a.ctypes.data
        return self.L.fpx_epx_lead_accept_mk(self._h, m, p(leader), p(number), p(at), p(bo), p(off), p(keys), p(is_set), p(tr),
                                             p(seq), p(deps), p(dend))

    def read_recovery_state(self, replica, leader, number):
        """[n, 3]: per responder the PrepareOk's status, voteBallot (encoded) and triple id; -1s where there is none"""
        out = np.zeros((self.n, 3), np.int32)
        st = self.L.fpx_epx_read_recovery_state(self._h, replica, leader, number, out.ctypes.data)
        if st:
            raise FpxError(st, "fpx_epx_read_recovery_state")
        return out

    # ---- the replica half, a burst at a time ----
    def replica_inbox(self, kind, to, leader, number, ballot_ordering, ballot_replica, key, is_set, triple_id, deps,
                      deps_values_end=None):
        """one burst of PreAccept (0) / Accept (1) / Commit (2) / Prepare (3) messages from peer replicas in delivery order,
        message i to replica to[i]: (status, outcome[m], out_ballot[m], out_status[m], out_deps[m, n], out_values_end[m],
        out_triple[m]); on a status other than 0 the outputs keep their fill of -9"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        kind, to, leader, number = a32(kind), a32(to), a32(leader), a32(number)
        bo, br, key, tr = a32(ballot_ordering), a32(ballot_replica), a32(key), a32(triple_id)
        is_set = np.ascontiguousarray(is_set, dtype=np.uint8)
        m = len(kind)
        deps = a32(deps).reshape(m, self.n)
        dend = None if deps_values_end is None else a32(deps_values_end)
        outcome, ob, os_, oend, otr = (np.full(m, -9, np.int32) for _ in range(5))
        odeps = np.full((m, self.n), -9, np.int32)
        p = lambda a: None if a is None else a.ctypes.data
        st = self.L.fpx_epx_replica_inbox(self._h, m, p(kind), p(to), p(leader), p(number), p(bo), p(br), p(key), p(is_set),
                                          p(tr), p(deps), p(dend), p(outcome), p(ob), p(os_), p(odeps), p(oend), p(otr))
        return st, outcome, ob, os_, odeps, oend, otr

    def replica_inbox_dev(self, kind, to, leader, number, ballot_ordering, ballot_replica, key, is_set, triple_id, deps,
                          deps_values_end=None, outcome=None, out_ballot=None, out_status=None, out_deps=None,
                          out_values_end=None, out_triple=None):
        """the same on device tensors (int32; is_set uint8), enqueued on the context's stream; the status comes with sync()"""
        d = lambda t: None if t is None else t.data_ptr()
        st = self.L.fpx_epx_replica_inbox_dev(self._h, kind.numel(), d(kind), d(to), d(leader), d(number), d(ballot_ordering),
                                              d(ballot_replica), d(key), d(is_set), d(triple_id), d(deps), d(deps_values_end),
                                              d(outcome), d(out_ballot), d(out_status), d(out_deps), d(out_values_end),
                                              d(out_triple))
        if st:
            raise FpxError(st, "fpx_epx_replica_inbox_dev")

    def replica_inbox_mk(self, kind, to, leader, number, ballot_ordering, ballot_replica, key_lists, is_set, triple_id, deps,
                         deps_values_end=None):
        """replica_inbox() with a key list per message (a Prepare's is not read; an empty list behaves as a Noop)"""
        a32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        off, keys = self.key_lists(key_lists)
        kind, to, leader, number = a32(kind), a32(to), a32(leader), a32(number)
        bo, br, tr = a32(ballot_ordering), a32(ballot_replica), a32(triple_id)
        is_set = np.ascontiguousarray(is_set, dtype=np.uint8)
        m = len(kind)
        deps = a32(deps).reshape(m, self.n)
        dend = None if deps_values_end is None else a32(deps_values_end)
        outcome, ob, os_, oend, otr = (np.full(m, -9, np.int32) for _ in range(5))
        odeps = np.full((m, self.n), -9, np.int32)
        p = lambda a: None if a is None else a.ctypes.data
        st = self.L.fpx_epx_replica_inbox_mk(self._h, m, p(kind), p(to), p(leader), p(number), p(bo), p(br), p(off), p(keys),
                                             p(is_set), p(tr), p(deps), p(dend), p(outcome), p(ob), p(os_), p(odeps), p(oend),
                                             p(otr))
        return st, outcome, ob, os_, odeps, oend, otr

    def replica_inbox_mk_dev(self, kind, to, leader, number, ballot_ordering, ballot_replica, key_offsets, keys, is_set,
                             triple_id, deps, deps_values_end=None, outcome=None, out_ballot=None, out_status=None,
                             out_deps=None, out_values_end=None, out_triple=None, num_pairs=None):
        """the same on device tensors (int32; is_set uint8): key_offsets[m + 1] and keys; num_pairs (default: keys.numel())
        is checked against key_offsets[m] on the device.  Enqueued on the context's stream; the status comes with sync()"""
        d = lambda t: None if t is None else t.data_ptr()
        num_pairs = keys.numel() if num_pairs is None else int(num_pairs)
        st = self.L.fpx_epx_replica_inbox_mk_dev(self._h, kind.numel(), d(kind), d(to), d(leader), d(number), d(ballot_ordering),
                                                 d(ballot_replica), d(key_offsets), d(keys), num_pairs, d(is_set), d(triple_id),
                                                 d(deps), d(deps_values_end), d(outcome), d(out_ballot), d(out_status),
                                                 d(out_deps), d(out_values_end), d(out_triple))
        if st:
            raise FpxError(st, "fpx_epx_replica_inbox_mk_dev")

    def read_leader_state(self, replica, leader, number):
        """(phase [0 when not live], ballot, avoid_fast_path, triple id, key [-1: none, KEY_LIST: two or more distinct keys,
        the caller holds the list], is_set, response mask, stored phase),
        responses[n, n + 2] (row q: sequence number, n watermarks, values_end)"""
        out = np.zeros(8, np.int32)
        resp = np.zeros((self.n, self.n + 2), np.int32)
        st = self.L.fpx_epx_read_leader_state(self._h, replica, leader, number, out.ctypes.data, resp.ctypes.data)
        if st:
            raise FpxError(st, "fpx_epx_read_leader_state")
        return tuple(int(x) for x in out), resp

    def read_cmdlog_deps(self, replica, leader, number):
        """the dependencies kept with a command-log entry: (watermarks[n], values_end)"""
        deps, end = np.zeros(self.n, np.int32), np.zeros(1, np.int32)
        st = self.L.fpx_epx_read_cmdlog_deps(self._h, replica, leader, number, deps.ctypes.data, end.ctypes.data)
        if st:
            raise FpxError(st, "fpx_epx_read_cmdlog_deps")
        return deps, int(end[0])

    def read_cmdlog(self, replica, leader, number):
        """(kind, ballot, voteBallot, triple id, the replica's largestBallot); ballots encoded ordering * 8 + index"""
        out = np.zeros(5, np.int32)
        st = self.L.fpx_epx_read_cmdlog(self._h, replica, leader, number, out.ctypes.data)
        if st:
            raise FpxError(st, "fpx_epx_read_cmdlog")
        return tuple(int(x) for x in out)

    def preaccept_dev(self, leader, number, key, is_set, resp_mask, rank, fast=None, deps=None,
                      leader_deps=None, seen_mask=None, own_values_end=None, triple_id=None):
        d = lambda t: None if t is None else t.data_ptr()
        st = self.L.fpx_epx_preaccept_dev(self._h, leader.numel(), d(leader), d(number), d(key), d(is_set),
                                          d(resp_mask), d(seen_mask), d(rank), d(triple_id), d(fast), d(deps),
                                          d(leader_deps), d(own_values_end))
        if st:
            raise FpxError(st, "fpx_epx_preaccept_dev")

    def packed_stride(self):
        return int(self.L.fpx_epx_packed_stride(self.n))

    def preaccept_packed_dev(self, leader, number, key, is_set, resp_mask, rank, packed, seen_mask=None, triple_id=None):
        """one line of packed_stride() ints per command: deps | leader_deps | own_values_end[2] | fast (see unpack)"""
        d = lambda t: None if t is None else t.data_ptr()
        st = self.L.fpx_epx_preaccept_packed_dev(self._h, leader.numel(), d(leader), d(number), d(key), d(is_set),
                                                 d(resp_mask), d(seen_mask), d(rank), d(triple_id), d(packed))
        if st:
            raise FpxError(st, "fpx_epx_preaccept_packed_dev")

    def execute_dev(self, leader, number, packed, first, count, order, component, committed=None):
        """fpx_epx_execute_dev: the tick's commits through the device dependency graph.  Returns (num_executed,
        num_components, needs_host_path); order / component are filled on the device"""
        d = lambda t: None if t is None else t.data_ptr()
        f = np.ascontiguousarray(first, np.int32)
        c = np.ascontiguousarray(count, np.int32)
        ne, nc, nh = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        st = self.L.fpx_epx_execute_dev(self._h, leader.numel(), d(leader), d(number), d(packed), d(committed), f.ctypes.data,
                                        c.ctypes.data, d(order), d(component), C.addressof(ne), C.addressof(nc), C.addressof(nh))
        if st:
            raise FpxError(st, "fpx_epx_execute_dev")
        return ne.value, nc.value, nh.value

    def execute(self, leader, number, deps, first, count, deps_values_end=None, committed=None):
        """fpx_epx_execute: the same on host (numpy) arrays.  Returns (order, component, num_components, needs_host_path);
        order / component hold the num_executed entries"""
        leader, number = np.ascontiguousarray(leader, np.int32), np.ascontiguousarray(number, np.int32)
        deps = np.ascontiguousarray(deps, np.int32)
        m = len(leader)
        ends = None if deps_values_end is None else np.ascontiguousarray(deps_values_end, np.int32)
        cm = None if committed is None else np.ascontiguousarray(committed, np.uint8)
        f, c = np.ascontiguousarray(first, np.int32), np.ascontiguousarray(count, np.int32)
        order, comp = np.full(m, -1, np.int32), np.full(m, -1, np.int32)
        ne, nc, nh = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        p = lambda a: None if a is None else a.ctypes.data
        st = self.L.fpx_epx_execute(self._h, m, p(leader), p(number), p(deps), p(ends), p(cm), p(f), p(c), p(order), p(comp),
                                    C.addressof(ne), C.addressof(nc), C.addressof(nh))
        if st:
            raise FpxError(st, "fpx_epx_execute")
        return order[:ne.value], comp[:ne.value], nc.value, nh.value

    def unpack(self, packed):
        """packed [m, stride] (numpy or torch) -> fast [m], deps [m, n], leader_deps [m, n], own_values_end [m, 2]"""
        n = self.n
        return packed[:, 2 * n + 2], packed[:, :n], packed[:, n:2 * n], packed[:, 2 * n:2 * n + 2]

    def limits(self):
        """the exact-fit limits of the pre-accept tick for this n (include/fpx.h, fpx_epx_limits): {"kp_tc": commands of
        one key the second form holds on chip, "key_tc": the first form's, "nbk", "kp_max_occ", "kp_maxb", "kp_waves"}"""
        nw = len(_lib.EPX_LIMIT_WORDS)
        out = (C.c_int32 * nw)()
        n = C.c_int32(0)
        st = self.L.fpx_epx_limits(self._h, nw, out, C.byref(n))
        if st or n.value != nw:
            raise FpxError(st, "fpx_epx_limits")
        return dict(zip(_lib.EPX_LIMIT_WORDS, (int(x) for x in out)))

    def tick_census(self):
        """diagnostic: the paths the single-key pre-accept ticks took since the context was created (include/fpx.h,
        fpx_epx_tick_census), as {word name: count}; waits for the context's stream"""
        nw = len(_lib.EPX_CENSUS_WORDS)
        out = (C.c_int64 * nw)()
        n = C.c_int32(0)
        st = self.L.fpx_epx_tick_census(self._h, nw, out, C.byref(n))
        if st or n.value != nw:
            raise FpxError(st, "fpx_epx_tick_census")
        return dict(zip(_lib.EPX_CENSUS_WORDS, (int(x) for x in out)))

    def read_index(self, replica, key):
        g = np.zeros(self.n, np.int32)
        s = np.zeros(self.n, np.int32)
        st = self.L.fpx_epx_read_index(self._h, replica, key, g.ctypes.data, s.ctypes.data)
        if st:
            raise FpxError(st, "fpx_epx_read_index")
        return g, s
