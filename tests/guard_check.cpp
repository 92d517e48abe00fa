// Host-only check of orbx_guard (orbx_internal.hpp): built and run by tests/test_guard.py.  orbx_fail is this program's own: it
// records the code and the formatted text where the library's keeps them on the handle.
#include <cstdarg>
#include <cstdio>
#include <new>
#include <stdexcept>
#include <string>

#include "../orb-slam3-rust_amd/csrc/orbx_internal.hpp"

static int g_calls = 0, g_code = 0;
static std::string g_text;

int orbx_fail(orbx_handle*, int code, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  ++g_calls; g_code = code; g_text = buf;
  return code;
}

// one guarded call: its return value, how often orbx_fail ran, and what it was handed
template <class F>
static bool check(orbx_handle* h, F&& body, int want_rc, int want_calls, const char* want_text) {
  g_calls = 0; g_code = 0; g_text.clear();
  const int rc = orbx_guard(h, "who_calls", body);
  const bool ok = rc == want_rc && g_calls == want_calls && g_text == want_text && (want_calls == 0 || g_code == want_rc);
  if (!ok) std::printf("got rc %d, %d calls, '%s'; want rc %d, %d calls, '%s'\n", rc, g_calls, g_text.c_str(), want_rc, want_calls, want_text);
  return ok;
}

int main() {
  int (*const plain)() = [] { return 0; };
  static_assert(noexcept(orbx_guard((orbx_handle*)nullptr, "", plain)), "orbx_guard is noexcept: an escape would terminate");
  orbx_handle* h = new orbx_handle();
  int bad = 0;
  // a body's return value passes through, whatever it is
  for (int v : {0, 5, (int)ORBX_ERR_INVALID, (int)ORBX_ERR_EMPTY}) bad += !check(h, [&] { return v; }, v, 0, "");
  bad += !check(nullptr, [] { return 3; }, 3, 0, "");
  // the two texts
  bad += !check(h, []() -> int { throw std::bad_alloc(); }, ORBX_ERR_HIP, 1, "who_calls: out of host memory");
  bad += !check(h, []() -> int { throw 7; }, ORBX_ERR_HIP, 1, "who_calls: unexpected C++ exception");
  bad += !check(h, []() -> int { throw std::runtime_error("x"); }, ORBX_ERR_HIP, 1, "who_calls: unexpected C++ exception");
  // (thrown from a frame below the body, with a container alive in between: it is unwound, not leaked — the sanitizer build says so)
  bad += !check(h, []() -> int { std::string s(1000, 'x'); return std::stoi(s); }, ORBX_ERR_HIP, 1, "who_calls: unexpected C++ exception");
  // no handle: the code, and nowhere to keep a message
  bad += !check(nullptr, []() -> int { throw std::bad_alloc(); }, ORBX_ERR_HIP, 0, "");
  bad += !check(nullptr, []() -> int { throw 7; }, ORBX_ERR_HIP, 0, "");
  delete h;
  std::printf("guard %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
