// A Mencius acceptor's inbox handled ONE MESSAGE AT A TIME on one host thread, in the shape of mencius/Acceptor.scala
// (handlePhase1a :166-200 without the info, handlePhase2a :202-235, handlePhase2aNoopRange :237-291): the yardstick of
// profiles/mencius_acceptor_inbox.md for fpx_mencius_acceptor_inbox_dev.  Every acceptor's `states` is a flat array over
// the rows of its leader group (kinder than the reference's SortedMap).  Reads the burst
// profiles/microbench/mencius_acceptor_inbox.py --dump wrote.
//
//   g++ -O2 -std=c++17 -o mencius_acceptor_inbox_host mencius_acceptor_inbox_host.cpp && ./mencius_acceptor_inbox_host burst.bin [runs]
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Acceptor {
  int32_t round = -1, maxVotedSlot = -1;
  std::vector<int32_t> voteRound, voteValue;  // by row q = slot / L
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[5];
  if (std::fread(hdr, 4, 5, f) != 5) return 2;
  const int32_t n = hdr[0], S = hdr[1], L = hdr[2], A = hdr[3], R = hdr[4], rows = S / L;
  std::vector<int32_t> kind(n), group(n), acc(n), slot(n), end(n), round(n), value(n);
  for (std::vector<int32_t>* a : {&kind, &group, &acc, &slot, &end, &round, &value})
    if (std::fread(a->data(), 4, n, f) != (size_t)n) return 2;
  std::fclose(f);
  const int runs = argc > 2 ? std::atoi(argv[2]) : 20;
  std::vector<double> ms;
  long long checksum = 0;
  for (int run = 0; run < runs + 3; ++run) {
    std::vector<Acceptor> as((size_t)L * A * R);
    for (Acceptor& a : as) a.voteRound.assign(rows, -1), a.voteValue.assign(rows, -1);
    std::vector<int32_t> replyKind(n, 0), replyValue(n, -1);
    const auto t0 = std::chrono::steady_clock::now();
    for (int32_t i = 0; i < n; ++i) {
      if (kind[i] != 1 && kind[i] != 6 && kind[i] != 3) continue;
      Acceptor& a = as[(size_t)group[i] * R + acc[i]];
      if (round[i] < a.round) {  // :173, :210, :245
        replyKind[i] = 5, replyValue[i] = a.round;
        continue;
      }
      a.round = round[i], replyValue[i] = round[i];
      if (kind[i] == 1) {  // Phase2a
        a.voteRound[slot[i] / L] = round[i], a.voteValue[slot[i] / L] = value[i];
        a.maxVotedSlot = std::max(a.maxVotedSlot, slot[i]);
        replyKind[i] = 2;
      } else if (kind[i] == 6) {  // Phase2aNoopRange: :261-277
        const int ag = group[i] % A;
        int32_t s = slot[i];
        while ((s / L) % A != ag) s += L;
        for (; s < end[i]; s += L * A) {
          a.voteRound[s / L] = round[i], a.voteValue[s / L] = -1;
          a.maxVotedSlot = std::max(a.maxVotedSlot, s);
        }
        replyKind[i] = 7;
      } else {
        replyKind[i] = 9;
      }
    }
    const auto t1 = std::chrono::steady_clock::now();
    if (run >= 3) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    for (const Acceptor& a : as) checksum += a.round + a.maxVotedSlot + a.voteValue[rows / 2];
    checksum += replyKind[n / 2] + replyValue[n / 3];
  }
  std::sort(ms.begin(), ms.end());
  std::printf("{\"mode\": \"host message at a time\", \"messages\": %d, \"runs\": %zu, \"ms_median\": %.3f, \"ms_min\": %.3f, "
              "\"ms_max\": %.3f, \"checksum\": %lld}\n",
              n, ms.size(), ms[ms.size() / 2], ms.front(), ms.back(), checksum);
  return 0;
}
