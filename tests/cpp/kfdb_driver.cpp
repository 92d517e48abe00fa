// Driver of the compiled host mirror's place-recognition entries (include/orbx.hpp: orbx::KeyFrameDatabase, ConsistencyChecker) for
// tests/test_place_recognition_gpu.py.
//   kfdb_driver <in.bin> <out.bin>
//   in:  int32 N | per entry: u64 id, i32 map, i32 bad, i32 n, words [n] u32, weights [n] f64
//        int32 Q | per query: u64 current id, i32 scoring (0 L1, 1 DOT), i32 n_connected, connected [n_connected] u64
//        int32 R | per relocalisation query: i32 exclude_map (-1: none), i32 max_results, i32 n, words [n] u32, weights [n] f64
//   out: per query: i32 count, then count x (u64 id, f64 score); per relocalisation query: i32 count, then count x (u64 id, i32 map, f64 score);
//        last, one byte: 1 when the reference's two ConsistencyChecker unit tests (detector.rs:394-455) hold on orbx::ConsistencyChecker
#include <cstdio>
#include <vector>

#include "orbx.hpp"

template <class T> static bool rd(FILE* f, T* p, size_t n = 1) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
template <class T> static void wr(FILE* f, const T* p, size_t n = 1) { if (n) std::fwrite(p, sizeof(T), n, f); }

static bool consistency_checker_unit_tests() {
  using namespace orbx;
  LoopDetectorConfig cfg;
  cfg.consistency_threshold = 3;
  ConsistencyChecker a(cfg);
  if (a.add_and_check(10, {LoopCandidate{10, 1, 0.8, {2, 3}}})) return false;
  if (a.add_and_check(11, {LoopCandidate{11, 1, 0.85, {2}}})) return false;
  const auto r = a.add_and_check(12, {LoopCandidate{12, 1, 0.9, {}}});
  if (!r || r->loop_kf_id != 1 || a.history_len() != 0) return false;
  ConsistencyChecker b(cfg);
  for (uint64_t i = 10; i < 15; ++i)
    if (b.add_and_check(i, {LoopCandidate{i, i - 9, 0.8, {}}})) return false;
  return b.history_len() == 5;
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: kfdb_driver in.bin out.bin\n"); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  FILE* o = std::fopen(argv[2], "wb");
  if (!f || !o) return 2;
  const orbx::CameraModel cam{458.654, 457.296, 367.215, 248.375, 0.11007};
  try {
    orbx::Handle h(cam, 1000, 0, 752, 480, 1);
    orbx::KeyFrameDatabase db(h);
    int N = 0;
    if (!rd(f, &N)) return 2;
    for (int i = 0; i < N; ++i) {
      uint64_t id; int map, bad, n;
      if (!rd(f, &id) || !rd(f, &map) || !rd(f, &bad) || !rd(f, &n) || n < 0) return 2;
      std::vector<uint32_t> w((size_t)n); std::vector<double> v((size_t)n);
      if (!rd(f, w.data(), (size_t)n) || !rd(f, v.data(), (size_t)n)) return 2;
      db.add(id, w, v, (size_t)map, bad != 0);
    }
    int Q = 0;
    if (!rd(f, &Q)) return 2;
    for (int q = 0; q < Q; ++q) {
      uint64_t cur; int scoring, nc;
      if (!rd(f, &cur) || !rd(f, &scoring) || !rd(f, &nc) || nc < 0) return 2;
      std::vector<uint64_t> conn((size_t)nc);
      if (!rd(f, conn.data(), (size_t)nc)) return 2;
      const auto r = db.detect_loop_candidates(cur, conn, orbx::LoopDetectorConfig{}, scoring ? orbx::BowScoring::Dot : orbx::BowScoring::L1);
      const int cnt = (int)r.size();
      wr(o, &cnt);
      for (const auto& c : r) { wr(o, &c.loop_kf_id); wr(o, &c.bow_score); }
    }
    int R = 0;
    if (!rd(f, &R)) return 2;
    for (int q = 0; q < R; ++q) {
      int ex, mr, n;
      if (!rd(f, &ex) || !rd(f, &mr) || !rd(f, &n) || n < 0 || mr < 0) return 2;
      std::vector<uint32_t> w((size_t)n); std::vector<double> v((size_t)n);
      if (!rd(f, w.data(), (size_t)n) || !rd(f, v.data(), (size_t)n)) return 2;
      const auto r = db.detect_candidates(w, v, ex < 0 ? std::nullopt : std::optional<size_t>((size_t)ex), (size_t)mr);
      const int cnt = (int)r.size();
      wr(o, &cnt);
      for (const auto& c : r) { const int m = (int)c.map_index; wr(o, &c.keyframe_id); wr(o, &m); wr(o, &c.score); }
    }
    const unsigned char ok = consistency_checker_unit_tests() ? 1 : 0;
    wr(o, &ok);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "kfdb_driver: %s\n", e.what());
    return 1;
  }
  std::fclose(f);
  std::fclose(o);
  return 0;
}
