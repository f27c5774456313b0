// The acceptors' inbox handled ONE MESSAGE AT A TIME on one host thread, in the shape of multipaxos/Acceptor.scala
// (handlePhase1a :148-182 without the info, handlePhase2a :184-220, the two read handlers :222-254): the yardstick of
// profiles/acceptor_inbox.md for fpx_acceptor_inbox_dev.  Every acceptor's `states` is a flat array over the window
// (kinder than the reference's SortedMap).  Reads the burst profiles/microbench/acceptor_inbox.py --dump wrote.
//
//   g++ -O2 -std=c++17 -o acceptor_inbox_host acceptor_inbox_host.cpp && ./acceptor_inbox_host burst.bin [runs]
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Acceptor {
  int32_t round = -1, maxVotedSlot = -1;
  std::vector<int32_t> voteRound, voteValue;
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[2];
  if (std::fread(hdr, 4, 2, f) != 2) return 2;
  const int32_t n = hdr[0], S = hdr[1], R = 3;
  std::vector<int32_t> kind(n), acc(n), slot(n), round(n), value(n);
  for (std::vector<int32_t>* a : {&kind, &acc, &slot, &round, &value})
    if (std::fread(a->data(), 4, n, f) != (size_t)n) return 2;
  std::fclose(f);
  const int runs = argc > 2 ? std::atoi(argv[2]) : 20;
  std::vector<double> ms;
  long long checksum = 0;
  for (int run = 0; run < runs + 3; ++run) {
    std::vector<Acceptor> as(R);
    for (Acceptor& a : as) a.voteRound.assign(S, -1), a.voteValue.assign(S, -1);
    std::vector<int32_t> replyKind(n, 0), replyValue(n, -1);
    const auto t0 = std::chrono::steady_clock::now();
    for (int32_t i = 0; i < n; ++i) {
      Acceptor& a = as[acc[i]];
      switch (kind[i]) {
        case 1:  // Phase2a
          if (round[i] < a.round) {
            replyKind[i] = 5, replyValue[i] = a.round;
          } else {
            a.round = round[i];
            a.voteRound[slot[i]] = round[i], a.voteValue[slot[i]] = value[i];
            a.maxVotedSlot = std::max(a.maxVotedSlot, slot[i]);
            replyKind[i] = 2, replyValue[i] = round[i];
          }
          break;
        case 3:  // Phase1a
          if (round[i] < a.round) replyKind[i] = 5, replyValue[i] = a.round;
          else a.round = round[i], replyKind[i] = 9, replyValue[i] = round[i];
          break;
        case 10:
        case 11: replyKind[i] = 10, replyValue[i] = a.maxVotedSlot; break;
        default: break;
      }
    }
    const auto t1 = std::chrono::steady_clock::now();
    if (run >= 3) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    for (const Acceptor& a : as) checksum += a.round + a.maxVotedSlot + a.voteValue[S / 2];
    checksum += replyKind[n / 2] + replyValue[n / 3];
  }
  std::sort(ms.begin(), ms.end());
  std::printf("{\"mode\": \"host message at a time\", \"messages\": %d, \"runs\": %zu, \"ms_median\": %.3f, \"ms_min\": %.3f, "
              "\"ms_max\": %.3f, \"checksum\": %lld}\n",
              n, ms.size(), ms[ms.size() / 2], ms.front(), ms.back(), checksum);
  return 0;
}
