// Host-only check of UploadPlan, OutputPlan and the host-only helpers (node sort, node ranges, pose inverse) of orbx_internal.hpp: built and run by tests/test_plans.py, once more under
// -fsanitize=address,undefined.  The ring, the host-call skeleton and orbx_fail are this program's own: every buffer they hand out is a
// heap block of exactly the bytes asked for, "device" memory included, so a piece that is placed or copied wrongly is an out-of-bounds
// access the sanitizer sees, and what travels is compared byte by byte.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../orb-slam3-rust_amd/csrc/orbx_internal.hpp"

static int g_fails = 0, g_ring_begins = 0, g_call_begins = 0;
static size_t g_committed = 0, g_downloaded = 0;
static std::vector<uint8_t*> g_blocks;

static uint8_t* block(size_t bytes, int fill) {
  uint8_t* p = (uint8_t*)std::malloc(bytes ? bytes : 1);
  std::memset(p, fill, bytes);
  g_blocks.push_back(p);
  return p;
}

int orbx_fail(orbx_handle*, int code, const char*, ...) { ++g_fails; return code; }

static uint8_t *g_slot, *g_dev;
int orbx_ring_begin(orbx_handle*, UploadRing&, DevBuf& dev, size_t bytes, uint8_t** host, uint8_t** device) {
  ++g_ring_begins;
  g_slot = *host = block(bytes, 0xAB);                                    // what a slot holds before it is filled
  g_dev = *device = block(bytes, 0xCD);
  dev.p = g_dev; dev.bytes = bytes;
  return ORBX_OK;
}
int orbx_ring_commit(orbx_handle*, UploadRing&, const DevBuf& dev, size_t bytes) {
  std::memcpy(dev.p, g_slot, bytes);
  g_committed = bytes;
  return ORBX_OK;
}
int orbx_host_call_begin(orbx_handle*, PinnedBuf& pin, DevBuf& dev, size_t in_bytes, size_t out_bytes, HostCall& c) {
  ++g_call_begins;
  pin.p = block(in_bytes + out_bytes, 0xAB); pin.bytes = in_bytes + out_bytes;
  dev.p = block(in_bytes + out_bytes, 0xCD); dev.bytes = in_bytes + out_bytes;
  c.hi = (uint8_t*)pin.p; c.ho = c.hi + in_bytes; c.di = (uint8_t*)dev.p; c.dout = c.di + in_bytes; c.in_bytes = in_bytes;
  return ORBX_OK;
}
int orbx_host_call_download(orbx_handle*, const HostCall& c, size_t bytes) {
  std::memcpy(c.ho, c.dout, bytes);
  g_downloaded = bytes;
  return ORBX_OK;
}

static int bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); ++bad; } } while (0)

static bool all(const uint8_t* p, size_t n, int v) {
  for (size_t i = 0; i < n; ++i) if (p[i] != (uint8_t)v) return false;
  return true;
}

static void upload() {
  UploadRing ring; DevBuf dev;
  uint8_t* a = block(1, 0x11); uint8_t* b = block(257, 0x22); uint8_t* d = block(3, 0x44);
  UploadPlan up;
  const size_t o_a = up.put(a, 1), o_b = up.put(b, 257), o_r = up.put(nullptr, 100), o_e = up.put(a, 0), o_n = up.put(nullptr, 0), o_d = up.put(d, 3);
  CHECK(o_a == 0 && o_b == 256 && o_r == 768 && o_e == 1024 && o_n == 1024 && o_d == 1024 && up.c.off == 1280 && up.n == 3);
  CHECK(up.send(nullptr, ring, dev) == ORBX_OK && g_committed == 1280 && up.device == g_dev && up.host == g_slot);
  CHECK(g_dev[o_a] == 0x11 && all(g_dev + 1, 255, 0xAB));                 // one byte, and nothing beside it
  CHECK(all(g_dev + o_b, 257, 0x22) && all(g_dev + o_b + 257, 255, 0xAB));
  CHECK(all(g_dev + o_r, 256, 0xAB));                                     // reserved: nothing was copied into it
  CHECK(all(g_dev + o_d, 3, 0x44) && all(g_dev + o_d + 3, 253, 0xAB));
  // a piece made in place between begin and commit
  UploadPlan in_place;
  const size_t o_t = in_place.put(nullptr, 8), o_s = in_place.put(b, 257);
  CHECK(in_place.begin(nullptr, ring, dev) == ORBX_OK && all(in_place.host + o_s, 257, 0x22));
  std::memset(in_place.host + o_t, 0x77, 8);
  CHECK(in_place.commit(nullptr, ring, dev) == ORBX_OK && g_committed == 768 && all(in_place.device + o_t, 8, 0x77) && all(in_place.device + o_s, 257, 0x22));
  // no piece at all
  UploadPlan none;
  CHECK(none.send(nullptr, ring, dev) == ORBX_OK && g_committed == 0);
  // one piece too many: refused before the ring is touched, nothing dropped
  UploadPlan many;
  for (int i = 0; i < UploadPlan::CAP + 1; ++i) many.put(a, 1);
  const int begins = g_ring_begins, fails = g_fails;
  CHECK(many.send(nullptr, ring, dev) == ORBX_ERR_HIP && g_ring_begins == begins && g_fails == fails + 1);
  UploadPlan full;
  for (int i = 0; i < UploadPlan::CAP; ++i) full.put(a, 1);
  CHECK(full.send(nullptr, ring, dev) == ORBX_OK && g_dev[256 * (UploadPlan::CAP - 1)] == 0x11);
}

static void output() {
  PinnedBuf pin; DevBuf dev;
  uint8_t* one = block(1, 0); uint8_t* big = block(257, 0); int* part = (int*)block(40, 0x5A);
  OutputPlan out;
  const auto p_one = out.add(one, 1), p_big = out.add(big, 257);
  const auto p_head = out.add((int*)nullptr, 2), p_part = out.add(part, 10, true);
  const auto p_none = out.add((double*)nullptr, 0), p_empty = out.add((double*)one, 0);
  const size_t o_keep = out.keep(100);
  CHECK(out.down == 1280 && o_keep == 1280 && out.c.off == 1536 && out.n == 6);
  CHECK(out.begin(nullptr, pin, dev, 256) == ORBX_OK && out.call.dout == (uint8_t*)dev.p + 256 && pin.bytes == 256 + 1536);
  CHECK((uint8_t*)out.dev(p_one) == out.call.dout && out.dev(p_big) == out.call.dout + 256 && (uint8_t*)out.dev(p_head) == out.call.dout + 768);
  CHECK((uint8_t*)out.dev(p_part) == out.call.dout + 1024 && (uint8_t*)out.dev(p_none) == out.call.dout + 1280 && (uint8_t*)out.dev(p_empty) == out.call.dout + 1280);
  // what the launches would write
  *out.dev(p_one) = 0x11; std::memset(out.dev(p_big), 0x22, 257);
  out.dev(p_head)[0] = 0; out.dev(p_head)[1] = 4;
  for (int i = 0; i < 10; ++i) out.dev(p_part)[i] = 100 + i;
  std::memset(out.call.dout + o_keep, 0x33, 256);
  CHECK(out.finish(nullptr) == ORBX_OK && g_downloaded == 1280);
  CHECK(one[0] == 0x11 && all(big, 257, 0x22));
  CHECK(all((const uint8_t*)part, 40, 0x5A));                             // left to copy()
  CHECK(all(out.call.ho + o_keep, 256, 0xAB));                            // stayed on the device
  const size_t n = (size_t)out.host(p_head)[1];                           // the length the download tells
  CHECK(n == 4 && out.copy(nullptr, p_part, n) == ORBX_OK);
  CHECK(part[0] == 100 && part[3] == 103 && all((const uint8_t*)(part + 4), 24, 0x5A));
  const int fails = g_fails;
  CHECK(out.copy(nullptr, p_part, 11) == ORBX_ERR_HIP && g_fails == fails + 1 && part[3] == 103 && all((const uint8_t*)(part + 4), 24, 0x5A));
  CHECK(out.copy(nullptr, p_part, 0) == ORBX_OK && out.copy(nullptr, p_none, 0) == ORBX_OK && out.copy(nullptr, p_part, 10) == ORBX_OK && part[9] == 109);
  // one piece too many: refused before anything is reserved
  OutputPlan many;
  for (int i = 0; i < OutputPlan::CAP + 1; ++i) many.add(one, 1);
  const int begins = g_call_begins;
  CHECK(many.begin(nullptr, pin, dev) == ORBX_ERR_HIP && g_call_begins == begins && g_fails == fails + 2);
}

// orbx_sort_by_node / orbx_node_ranges / orbx_pose_inverse: every array is a heap block of exactly its size
static void helpers() {
  const uint32_t none = 0xffffffffu;
  const uint32_t n2v[7] = {5, none, 2, 5, 2, none, 9};
  uint32_t* node2 = (uint32_t*)block(sizeof n2v, 0); std::memcpy(node2, n2v, sizeof n2v);
  int* sorted = (int*)block(7 * sizeof(int), 0x5A);
  const int m = orbx_sort_by_node(node2, 7, sorted);
  const int want[7] = {2, 4, 0, 3, 6, 1, 5};                               // by node, then by index; the features in no list last
  CHECK(m == 5 && std::memcmp(sorted, want, sizeof want) == 0);
  const uint32_t n1v[5] = {2, none, 7, 9, 5};
  uint32_t* node1 = (uint32_t*)block(sizeof n1v, 0); std::memcpy(node1, n1v, sizeof n1v);
  int* lo = (int*)block(5 * sizeof(int), 0x5A); int* hi = (int*)block(5 * sizeof(int), 0x5A);
  orbx_node_ranges(node1, 5, node2, sorted, m, lo, hi);
  const int want_lo[5] = {0, 0, 4, 4, 2}, want_hi[5] = {2, 0, 4, 5, 4};   // in no list: (0, 0); node 7 is not in keyframe 2: empty where it would be
  CHECK(std::memcmp(lo, want_lo, sizeof want_lo) == 0 && std::memcmp(hi, want_hi, sizeof want_hi) == 0);
  // all in no list, and none at all
  uint32_t* all_none = (uint32_t*)block(3 * sizeof(uint32_t), 0xFF);
  CHECK(orbx_sort_by_node(all_none, 3, sorted) == 0 && sorted[0] == 0 && sorted[2] == 2);
  CHECK(orbx_sort_by_node(all_none, 0, (int*)block(0, 0)) == 0);
  orbx_node_ranges(node1, 5, all_none, sorted, 0, lo, hi);
  for (int i = 0; i < 5; ++i) CHECK(lo[i] == 0 && hi[i] == 0);
  // the inverse of a pose, applied to the pose's translation, is the origin; a quarter turn about z
  const double r = 0.70710678118654757;
  const double pv[7] = {r, 0.0, 0.0, r, 1.0, 2.0, 3.0};
  double* pose = (double*)block(sizeof pv, 0); std::memcpy(pose, pv, sizeof pv);
  double* inv = (double*)block(7 * sizeof(double), 0);
  orbx_pose_inverse(pose, inv);
  CHECK(inv[0] == r && inv[1] == 0.0 && inv[2] == 0.0 && inv[3] == -r);
  const double want_t[3] = {-2.0, 1.0, -3.0};                              // -(R^T t)
  for (int i = 0; i < 3; ++i) CHECK(inv[4 + i] > want_t[i] - 1e-15 && inv[4 + i] < want_t[i] + 1e-15);
}

int main() {
  upload();
  output();
  helpers();
  for (uint8_t* p : g_blocks) std::free(p);
  std::printf("plans %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
