// epx_reply_host.cpp -- what a caller of the existing replica tick does with its struct-of-arrays outputs today, from plain C:
// one fpx_wire_epaxos_encode_replica_inbound call per message (include/fpx_wire.h), one thread.  The yardstick of
// profiles/microbench/epx_wire_replica_replies.py; built by that script against libfpx.so.  Deferred records (a Commit sent
// back, a PrepareOk that carries a command, a triple stored by id) are skipped, as the device encoder skips them.
#include <cstdint>

#include "../../include/fpx.h"
#include "../../include/fpx_wire.h"

extern "C" int64_t mb_encode_replies(int32_t n, int32_t m, const int32_t* to, const int32_t* leader, const int32_t* number,
                                     const int32_t* b_ord, const int32_t* b_rep, const int32_t* outcome, const int32_t* out_ballot,
                                     const int32_t* out_status, const int32_t* out_deps, const int32_t* out_end, uint8_t* out,
                                     int64_t cap, int64_t* offsets, int64_t* encoded) {
  int32_t vl[FPX_WIRE_EPX_FOLD_MAX], vi[FPX_WIRE_EPX_FOLD_MAX];
  int64_t at = 0, count = 0;
  for (int32_t i = 0; i < m; ++i) {
    offsets[i] = at;
    fpx_wire_epx_msg msg = {};
    msg.instance_leader = leader[i], msg.instance_number = number[i];
    msg.ballot_ordering = b_ord[i], msg.ballot_replica = b_rep[i];
    msg.replica_index = to[i], msg.is_noop = -1, msg.num_replicas = -1;
    switch (outcome[i]) {
      case FPX_EPX_RI_PRE_ACCEPT_OK:
      case FPX_EPX_RI_PRE_ACCEPT_OK_AGAIN: {
        const int32_t* w = out_deps + (int64_t)i * n;
        const int64_t ids = out_end[i] > 0 ? (int64_t)out_end[i] - number[i] - 1 : 0;
        if (w[0] < 0 || ids > FPX_WIRE_EPX_FOLD_MAX) continue;
        msg.kind = FPX_WIRE_EPX_PRE_ACCEPT_OK, msg.has_sequence_number = 1, msg.sequence_number = 0;
        msg.num_replicas = n, msg.deps_watermark = w;
        for (int64_t k = 0; k < ids; ++k) vl[k] = leader[i], vi[k] = (int32_t)(number[i] + 1 + k);
        msg.num_values = ids > 0 ? (int32_t)ids : 0, msg.values_leader = vl, msg.values_id = vi;
        break;
      }
      case FPX_EPX_RI_ACCEPT_OK:
      case FPX_EPX_RI_ACCEPT_OK_AGAIN: msg.kind = FPX_WIRE_EPX_ACCEPT_OK; break;
      case FPX_EPX_RI_NACK:
        msg.kind = FPX_WIRE_EPX_NACK, msg.ballot_ordering = out_ballot[i] >> 3, msg.ballot_replica = out_ballot[i] & 7;
        break;
      case FPX_EPX_RI_PREPARE_OK:
        if (out_status[i] != 0) continue;
        msg.kind = FPX_WIRE_EPX_PREPARE_OK, msg.status = 0;
        msg.vote_ballot_ordering = out_ballot[i] < 0 ? -1 : out_ballot[i] >> 3;
        msg.vote_ballot_replica = out_ballot[i] < 0 ? -1 : out_ballot[i] & 7;
        break;
      default: continue;
    }
    const int64_t len = fpx_wire_epaxos_encode_replica_inbound(out + at, cap - at, &msg);
    if (len < 0) return -1;
    at += len, ++count;
  }
  offsets[m] = at;
  *encoded = count;
  return at;
}
