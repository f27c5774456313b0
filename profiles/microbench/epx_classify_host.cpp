// epx_classify_host.cpp -- the yardstick of profiles/microbench/epx_wire_replica_tick.py: what a host does today between
// "here are the command's bytes" and "here are its key ids" -- the parser of csrc/fpx_epx_cmd_parse.hpp (the header the
// device classify runs) and a std::unordered_map<std::string, int> that hands out ids in order of first occurrence, as
// GpuEPaxosEngine.keyOf does.  Built by the microbenchmark into profiles/microbench/build/; not part of libfpx.so.
#include <cstdint>
#include <string>
#include <unordered_map>

#include "../../frankenpaxos_amd/csrc/fpx_epx_cmd_parse.hpp"

namespace {
std::unordered_map<std::string, int32_t> table;
struct Sink {
  int32_t* keys;
  int64_t first, cap;
  void key(int32_t j, const uint8_t* at, int32_t len) {
    if (first + j >= cap) return;
    const auto it = table.emplace(std::string(reinterpret_cast<const char*>(at), (size_t)len), (int32_t)table.size());
    keys[first + j] = it.first->second;
  }
};
}  // namespace

extern "C" {

void mb_reset() { table.clear(); }
int32_t mb_count() { return (int32_t)table.size(); }

// key_offsets[m + 1], keys[cap], is_set[m]; returns the pairs, or -1 - i for a command i that is malformed or not canonical
int64_t mb_classify(const uint8_t* buf, const int64_t* cmd_off, const int32_t* cmd_len, int32_t m, int32_t* key_offsets,
                    int32_t* keys, uint8_t* is_set, int64_t cap) {
  int64_t total = 0;
  for (int32_t i = 0; i < m; ++i) {
    key_offsets[i] = (int32_t)total;
    is_set[i] = 0;
    if (cmd_len[i] < 0) continue;
    const fpxw::Reader r{buf + cmd_off[i], buf + cmd_off[i] + cmd_len[i]};
    fpxw::EpxCmd c;
    fpxw::EpxNoKeys none;
    if (!fpxw::epx_parse_command(r, &c, none) || c.shape != 1) return -1 - (int64_t)i;
    if (c.num_keys > 0) {
      Sink s{keys, total, cap};
      fpxw::EpxCmd again;
      (void)fpxw::epx_parse_command(r, &again, s);
    }
    is_set[i] = (uint8_t)c.is_set;
    total += c.num_keys;
  }
  key_offsets[m] = (int32_t)total;
  return total;
}
}
