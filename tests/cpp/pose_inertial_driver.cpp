// Driver of the compiled host mirror's pose-inertial entry (include/orbx.hpp: orbx::pose_inertial_optimization) for
// tests/test_pose_inertial_*.py.
//   pose_inertial_driver <in.bin> <out.bin>
//   in:  int32 n | pose T_wc [7] | velocity [3] | bias [6] | prev_kf_pose T_wc [7] | prev_kf_velocity [3] | preint [11] (f64) |
//        points3d [n][3] f64 | points2d [n][2] f32 | is_stereo [n] u8   (camera: EuRoC cam0; default config)
//   out: pose T_wc [7] | velocity [3] | bias [6] (f64) | num_inliers, num_observations, iterations (u64)
#include <cstdio>
#include <vector>

#include "orbx.hpp"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: pose_inertial_driver in.bin out.bin\n"); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n = 0;
  double s[37];
  if (std::fread(&n, 4, 1, f) != 1 || n < 0 || std::fread(s, 8, 37, f) != 37) return 2;
  std::vector<double> p3(3 * (size_t)n);
  std::vector<float> p2(2 * (size_t)n);
  std::vector<uint8_t> st(n);
  if (n && (std::fread(p3.data(), 24, n, f) != (size_t)n || std::fread(p2.data(), 8, n, f) != (size_t)n ||
            std::fread(st.data(), 1, n, f) != (size_t)n))
    return 2;
  std::fclose(f);
  const orbx::CameraModel cam{458.654, 457.296, 367.215, 248.375, 0.11007};
  const auto se3 = [](const double* p) {
    orbx::SE3 r;
    r.rotation = {p[0], p[1], p[2], p[3]};
    r.translation = {p[4], p[5], p[6]};
    return r;
  };
  orbx::ImuBias bias;
  for (int k = 0; k < 3; ++k) { bias.gyro[k] = s[10 + k]; bias.accel[k] = s[13 + k]; }
  orbx::PreintegratedState pre;
  for (int k = 0; k < 4; ++k) pre.delta_rot[k] = s[26 + k];
  for (int k = 0; k < 3; ++k) { pre.delta_vel[k] = s[30 + k]; pre.delta_pos[k] = s[33 + k]; }
  pre.dt = s[36];
  std::vector<orbx::PoseObservation> obs((size_t)n);
  for (int i = 0; i < n; ++i) {
    obs[(size_t)i].uv = {p2[2 * (size_t)i], p2[2 * (size_t)i + 1]};
    obs[(size_t)i].point_world = {p3[3 * (size_t)i], p3[3 * (size_t)i + 1], p3[3 * (size_t)i + 2]};
    obs[(size_t)i].is_stereo = st[(size_t)i] != 0;
    obs[(size_t)i].index = (size_t)i;
  }
  try {
    orbx::Handle h(cam, 1000, 0, 752, 480, 1);
    const orbx::PoseInertialResult r = orbx::pose_inertial_optimization(
        h, se3(s), {s[7], s[8], s[9]}, bias, se3(s + 16), {s[23], s[24], s[25]}, orbx::ImuBias{}, pre, obs, cam, orbx::PoseInertialConfig{});
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(r.pose.rotation.data(), 8, 4, o);
    std::fwrite(r.pose.translation.data(), 8, 3, o);
    std::fwrite(r.velocity.data(), 8, 3, o);
    std::fwrite(r.bias.gyro.data(), 8, 3, o);
    std::fwrite(r.bias.accel.data(), 8, 3, o);
    const uint64_t c[3] = {r.num_inliers, r.num_observations, r.iterations};
    std::fwrite(c, 8, 3, o);
    std::fclose(o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "pose_inertial_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
