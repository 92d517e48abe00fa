"""The cameras and image sizes the camera tests run (tests/test_cameras_cpu.py, tests/test_cameras_gpu.py).

Every geometric search of the library takes the camera or the image size as an argument; the rest of the suite exercises them at
EuRoC cam0 and 752 x 480.  One dict per case: name, camera (fx, fy, cx, cy, baseline), w, h (the image the keypoints lie in — not
always 2cx x 2cy), regime (what the case reaches).  The values are fixed: what matters is the regime, not a dataset's third decimal.

  max_disp = f32(fx b / 0.1), min_disp = f32(fx b / 40)                            stereo_match
  guided grid: 64 x 48 cells of img_w / 64 x img_h / 48 px                          guided_match, track_frames
  triangulation grid: min(64, ceil(u32(2cx) / 32)) x min(64, ceil(u32(2cy) / 32))   search_for_triangulation (`grid`, cols x rows)

Non-vacuity floors, each half of what the CPU oracle returned when the table was written (the observed figure stands beside it):
  pairs   search_for_triangulation on camera_scenes.two_view(case);
  corner  of those, the pairs whose partner lies in grid row 63 (kp2.y >= 2016) with a window that reaches column 63
          (ceil((kp1.x + 100) / 32) >= 63): the ones that read the 64 x 64 grid's end sentinel.  At least 20 at grid64 and big;
  stereo  stereo_match on camera_scenes.stereo_features(case, 0, 2100, 2300).
"""

EUROC = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, baseline=0.11007)

CASES = [
    dict(name="euroc", camera=dict(EUROC), w=752, h=480, grid=(23, 16),
         regime="the control: max_disp 504.8, min_disp 1.26; its results equal what the existing tests get"),
    dict(name="kitti", camera=dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, baseline=0.5372), w=1241, h=376, grid=(38, 12),
         regime="max_disp 3861.7 exceeds the width (min_u always 0), min_disp 9.65, 64 / 1241 inexact in binary, the large baseline "
                "moves the stereo-parallax branch"),
    dict(name="square512", camera=dict(fx=190.978, fy=190.978, cx=254.9, cy=255.6, baseline=0.101), w=512, h=512, grid=(16, 16),
         regime="short focal length: the fuse radius scale z / fx leaves its lower clamp (10) at 178 m and sits at the upper one (50) "
                "from 889 m on (EuRoC: 427 m and 2134 m), so most far points search the full 50 px"),
    dict(name="anisotropic", camera=dict(fx=400.0, fy=800.0, cx=128.0, cy=336.0, baseline=0.12), w=640, h=480, grid=(8, 21),
         regime="fx != fy, cx = 0.2 w, cy = 0.7 h: any swap shows; 2cx = 256 != w separates the bounds rule (2cx, 2cy) from the "
                "grid rule (img_w, img_h)"),
    dict(name="tiny", camera=dict(fx=60.0, fy=60.0, cx=16.0, cy=16.0, baseline=0.05), w=64, h=64, grid=(1, 1),
         regime="1 x 1 triangulation grid; guided cells of 1 px and 1.33 px, radius 15 spans 31 cells; every index clamps"),
    dict(name="grid63", camera=dict(fx=1500.0, fy=1500.0, cx=1008.0, cy=1008.0, baseline=0.2), w=2200, h=2200, grid=(63, 63),
         regime="u32(2cx) = 2016: 63 x 63 cells, the last grid below the 64 x 64 one"),
    dict(name="grid64", camera=dict(fx=1500.0, fy=1500.0, cx=1008.5, cy=1008.5, baseline=0.2), w=2200, h=2200, grid=(64, 64),
         regime="u32(2cx) = 2017: 64 x 64 = 4096 cells, the first camera whose end sentinel cell_start[4096] lies past the build "
                "kernel's 1024 x 4 slots; differs from grid63 in the principal point only"),
    dict(name="big", camera=dict(fx=1500.0, fy=1500.0, cx=1150.0, cy=1150.0, baseline=0.2), w=2300, h=2300, grid=(64, 64),
         regime="64 x 64 grid whose saturated last row and column are 284 px wide: many keypoints in cell (63, 63)"),
    dict(name="tall", camera=dict(fx=500.0, fy=500.0, cx=320.0, cy=2047.5, baseline=0.1), w=640, h=4095, grid=(20, 64),
         regime="keypoint rows up to 4094.x, against the stereo matcher's last row bucket (4095)"),
]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]

# 2cx < 1: u32(2cx) = 0 columns.  The reference's grid would have no cell; the library refuses the call.
REFUSED = dict(name="refused", camera=dict(fx=400.0, fy=400.0, cx=0.4, cy=240.0, baseline=0.1), w=640, h=480, grid=(0, 15),
               regime="zero grid columns: search_for_triangulation raises OrbxError and the handle stays usable")

# name -> (pairs observed, corner observed, stereo observed); floors are half of these
OBSERVED = {
    "euroc": (1476, 0, 1605), "kitti": (1517, 0, 1596), "square512": (1352, 0, 1607), "anisotropic": (549, 0, 1605), "tiny": (1112, 0, 1611),
    "grid63": (1140, 0, 1600), "grid64": (1251, 212, 1600), "big": (992, 73, 1600), "tall": (561, 0, 1605),
}


def floor(name, what):
    return OBSERVED[name][("pairs", "corner", "stereo").index(what)] // 2
