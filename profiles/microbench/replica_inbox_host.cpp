// A MultiPaxos replica's inbox handled ONE MESSAGE AT A TIME on one host thread, in the shape of multipaxos/Replica.scala
// (handleChosen + executeLog :394-413, 572-590; handleDeferrableRead :455-476; executeRead :513-529): the yardstick of
// profiles/replica_inbox.md for fpx_replica_inbox_dev.  The log is a flat array (kinder than the reference's BufferMap),
// the deferred reads a hash map of vectors as there.  Reads the burst profiles/microbench/replica_inbox.py --dump wrote.
//
//   g++ -O2 -std=c++17 -o replica_inbox_host replica_inbox_host.cpp && ./replica_inbox_host burst.bin [runs]
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <vector>

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[2];
  if (std::fread(hdr, 4, 2, f) != 2) return 2;
  const int32_t n = hdr[0], S = hdr[1];
  std::vector<int32_t> kind(n), slot(n), value(n);
  if (std::fread(kind.data(), 4, n, f) != (size_t)n || std::fread(slot.data(), 4, n, f) != (size_t)n ||
      std::fread(value.data(), 4, n, f) != (size_t)n)
    return 2;
  std::fclose(f);
  const int runs = argc > 2 ? std::atoi(argv[2]) : 20;
  std::vector<double> ms;
  long long checksum = 0;
  for (int run = 0; run < runs + 3; ++run) {
    std::vector<int32_t> log_value(S, -1), exec(n, -2), reply(n, -2), order;
    std::vector<uint8_t> present(S, 0);
    std::unordered_map<int32_t, std::vector<int32_t>> deferred;
    order.reserve(n / 4);
    int32_t wm = 0, num_chosen = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int32_t i = 0; i < n; ++i) {
      const int32_t k = kind[i], s = slot[i];
      if (k == 4) {  // Chosen
        if (present[s]) continue;
        present[s] = 1, log_value[s] = value[i], ++num_chosen;
        while (wm < S && present[wm]) {  // executeLog
          auto it = deferred.find(wm);
          if (it != deferred.end()) {
            for (int32_t r : it->second) exec[r] = wm + 1, reply[r] = wm - 1, order.push_back(r);
            deferred.erase(it);
          }
          ++wm;
        }
      } else if (k == 14 || k == 26 || s < wm) {  // an eventual read, or a deferrable one whose slot has executed
        exec[i] = wm, reply[i] = wm - 1, order.push_back(i);
      } else {
        exec[i] = reply[i] = -1;
        deferred[s].push_back(i);
      }
    }
    const auto t1 = std::chrono::steady_clock::now();
    if (run >= 3) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    checksum += wm + num_chosen + (long long)order.size() + exec[n / 2];
  }
  std::sort(ms.begin(), ms.end());
  std::printf("{\"mode\": \"host message at a time\", \"messages\": %d, \"runs\": %zu, \"ms_median\": %.3f, \"ms_min\": %.3f, "
              "\"ms_max\": %.3f, \"checksum\": %lld}\n",
              n, ms.size(), ms[ms.size() / 2], ms.front(), ms.back(), checksum);
  return 0;
}
