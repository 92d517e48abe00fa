// Compiles and links the C++ mirrors of the whole-map global BA (include/orbx.hpp, include/orbx_map.hpp) against liborbx_hip.so: taking
// their addresses makes the compiler emit their bodies, so every C entry point they call must resolve.  prints GLOBAL_BA_MAP_DRIVER_OK.
#include <cstdio>

#include "orbx.hpp"
#include "orbx_map.hpp"

int main(int argc, char**) {
  const void* fn[] = {
      reinterpret_cast<const void*>(&orbx::solve_global_ba_map), reinterpret_cast<const void*>(&orbx::solve_global_ba),
      reinterpret_cast<const void*>(&orbx::map_collect_global_device), reinterpret_cast<const void*>(&orbx::map_collect_global),
      reinterpret_cast<const void*>(&orbx::map_global_ba), reinterpret_cast<const void*>(&orbx::global_map_bounds),
      reinterpret_cast<const void*>(&orbx::run_global_ba)};
  for (const void* f : fn)
    if (!f) return 1;
  // the cap is a plain getter: callable without a device
  if (orbx_ba_global_map_max_keyframes() < 1024) return 2;
  std::printf("GLOBAL_BA_MAP_DRIVER_OK %d %d\n", orbx_ba_global_map_max_keyframes(), argc);
  return 0;
}
