"""The C++ mirror of triangulate_from_neighbors (include/orbx.hpp: TriangulationConfig, TriangulationResult, NewMapPoint,
triangulate_pairs, triangulate_from_neighbors) — tests/cpp/triangulate_driver.cpp built with g++ against liborbx_hip.so.
CPU: it compiles and links.  GPU: its new points are the Python mirror's, byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import triangulation_scenes as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam3-rust_amd")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")


def _build(tmp):
    exe = os.path.join(tmp, "triangulate_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "triangulate_driver.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lorbx_hip", "-L", ROCM_LIB, "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ROCM_LIB], check=True)
    return exe


def test_triangulate_driver_compiles_and_links(pkg, tmp_path):
    pkg.load_library()
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_triangulate_driver_equals_python_mirror(pkg, tmp_path):
    import torch
    tmp = str(tmp_path)
    exe = _build(tmp)
    name, inertial = "t3_nodes", 1
    sc = G.fused_scene(name)
    cam = sc["camera"]
    with open(os.path.join(tmp, "tri_in.bin"), "wb") as f:
        f.write(struct.pack("<ii5d", len(sc["neighbours"]), inertial, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["baseline"]))
        for kf in [sc["current"]] + sc["neighbours"]:
            f.write(struct.pack("<ii7d", len(kf["kp"]), int(kf.get("node") is not None), *[float(v) for v in kf["pose"]]))
            for key, t in (("kp", G.KEYPOINT), ("desc", np.uint8), ("pts", np.float64), ("has", np.uint8), ("mp", np.uint8)):
                f.write(np.ascontiguousarray(kf[key], t).tobytes())
            if kf.get("node") is not None:
                f.write(np.ascontiguousarray(kf["node"], np.uint32).tobytes())
    r = subprocess.run([exe, tmp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "TRIANGULATE_DRIVER_OK" in r.stdout, (r.stdout, r.stderr)
    buf = open(os.path.join(tmp, "tri_nb_out.bin"), "rb").read()
    head = struct.unpack_from("<6Q", buf, 0)
    rec = np.frombuffer(buf, np.dtype([("nb", "<i4"), ("i1", "<i4"), ("i2", "<i4"), ("pad", "<i4"), ("p", "<f8", 3)]), head[0], 48)
    # the Python mirror on the same scene
    h = pkg.Handle(pkg.CameraModel(**cam), 1000, device=0, max_w=752, max_h=480, max_batch=1)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kfs = []
    for kf in [sc["current"]] + sc["neighbours"]:
        k = pkg.KeyFrame(h, d(np.ascontiguousarray(kf["kp"]).view(np.float32).reshape(-1, 7).copy()), d(kf["desc"]), len(kf["kp"]), d(kf["pts"]), d(kf["has"]),
                         pose_wc=kf["pose"])
        k.set_map_points([7 if m else None for m in kf["mp"]])
        if kf.get("node") is not None:
            k.set_feature_nodes(kf["node"])
        kfs.append(k)
    nb, i1, i2, pts, res = kfs[0].triangulate_from_neighbors(pkg.CameraModel(**cam), kfs[1:], is_inertial=bool(inertial))
    for k in kfs:
        k.close()
    h.close()
    assert head == (len(nb), res.num_new_points, res.num_pairs_checked, res.num_matches_found, res.num_triangulated, res.num_validated) and len(nb) > 40
    assert np.array_equal(rec["nb"], nb) and np.array_equal(rec["i1"], i1) and np.array_equal(rec["i2"], i2) and rec["p"].tobytes() == pts.tobytes()
