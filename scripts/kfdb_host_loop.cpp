// What a caller has without the device database: a compiled loop over orbx_bow_score, one query against N BowVectors held in host
// memory, on `threads` host threads (entries dealt out in contiguous ranges).  Built and loaded by scripts/kfdb_rate.py.
#include <cstdint>
#include <thread>
#include <vector>

#include "orbx.h"

extern "C" int kfdb_host_loop(const uint32_t* words, const double* weights, const long long* offsets, int n_entries, const uint32_t* q_word,
                              const double* q_weight, int nq, int threads, double* scores) {
  std::vector<int> rc((size_t)threads, 0);
  auto work = [&](int t) {
    const int lo = (int)((long long)n_entries * t / threads), hi = (int)((long long)n_entries * (t + 1) / threads);
    for (int i = lo; i < hi; ++i)
      rc[(size_t)t] |= orbx_bow_score(q_word, q_weight, nq, words + offsets[i], weights + offsets[i], (int)(offsets[i + 1] - offsets[i]), &scores[i]);
  };
  std::vector<std::thread> th;
  for (int t = 1; t < threads; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
  int all = 0;
  for (int r : rc) all |= r;
  return all;
}
