// Driver of the compiled host mirror's PnP entry (include/orbx.hpp: orbx::solve_pnp_ransac_detailed) for tests/test_pnp_*.py.
//   pnp_driver <in.bin> <out.bin>
//   in:  int32 n | prior T_wc [7] f64 | points3d [n][3] f64 | points2d [n][2] f32   (camera: EuRoC cam0)
//   out: pose T_wc [7] f64 | inlier_mask [n] u8 | reproj_errors [n] f64
#include <cstdio>
#include <vector>

#include "orbx.hpp"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: pnp_driver in.bin out.bin\n"); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n = 0;
  double prior[7];
  if (std::fread(&n, 4, 1, f) != 1 || n < 0 || std::fread(prior, 8, 7, f) != 7) return 2;
  std::vector<std::array<double, 3>> p3(n);
  std::vector<std::array<float, 2>> p2(n);
  if (n && (std::fread(p3.data(), 24, n, f) != (size_t)n || std::fread(p2.data(), 8, n, f) != (size_t)n)) return 2;
  std::fclose(f);
  const orbx::CameraModel cam{458.654, 457.296, 367.215, 248.375, 0.11007};
  try {
    orbx::Handle h(cam, 1000, 0, 752, 480, 1);
    orbx::SE3 pr;
    pr.rotation = {prior[0], prior[1], prior[2], prior[3]};
    pr.translation = {prior[4], prior[5], prior[6]};
    const orbx::PnPResult r = orbx::solve_pnp_ransac_detailed(h, p3, p2, cam, pr);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(r.pose.rotation.data(), 8, 4, o);
    std::fwrite(r.pose.translation.data(), 8, 3, o);
    for (bool b : r.inlier_mask) std::fputc(b ? 1 : 0, o);
    std::fwrite(r.reproj_errors.data(), 8, r.reproj_errors.size(), o);
    std::fclose(o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "pnp_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
