"""The C++ mirror of loop-candidate verification (include/orbx.hpp: LoopKeyFrame, VerifiedLoop, verify_loop_candidate, Sim3SolverConfig,
Sim3Result, compute_sim3_ransac, compute_sim3_from_matches) — tests/cpp/loop_verify_driver.cpp built with g++ against
liborbx_hip.so.  CPU (tests/test_loop_verify_cpu.py): it compiles and links.  GPU: its results are the Python mirror's, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import loop_verify_scenes as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam3-rust_amd")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
PAIR_NAMES = ["ok_bf", "ok_fv", "few_points", "few_matches", "few_pairs", "no_model", "few_verified"]
SET_NAMES = ["n2", "n14", "n16_o30", "n64_o30", "free_scale"]


def _build(tmp):
    exe = os.path.join(tmp, "loop_verify_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "loop_verify_driver.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lorbx_hip", "-L", ROCM_LIB, "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ROCM_LIB], check=True)
    return exe


class _Reader:
    def __init__(self, buf):
        self.buf, self.pos = buf, 0

    def take(self, dtype, n):
        a = np.frombuffer(self.buf, dtype, n, self.pos)
        self.pos += a.nbytes
        return a

    def vec(self, dtype):
        return self.take(dtype, int(self.take("<u8", 1)[0]))


def _map_points(n, salt):
    return np.array([-1 if (i + salt) % 3 == 0 else 10 * i + salt for i in range(n)], np.int64)


@pytest.mark.gpu
def test_driver_equals_python_mirror(gpu_handle, pkg, tmp_path):
    cam = pkg.CameraModel(**Z.CAMERA)
    exe = _build(str(tmp_path))
    with open(tmp_path / "lv_in.bin", "wb") as f:
        f.write(np.array([len(PAIR_NAMES), len(SET_NAMES)], "<i4").tobytes())
        f.write(np.array([Z.CAMERA[k] for k in ("fx", "fy", "cx", "cy", "baseline")], "<f8").tobytes())
        for name in PAIR_NAMES:
            for salt, d in enumerate(Z.pair(name)):
                n = len(d["desc"])
                f.write(np.array([n, 1 if "node" in d else 0], "<i4").tobytes() + np.asarray(d["pose_wc"], "<f8").tobytes())
                f.write(np.ascontiguousarray(d["kp"]).tobytes() + np.ascontiguousarray(d["desc"]).tobytes())
                f.write(np.ascontiguousarray(d["points_cam"], "<f8").tobytes() + np.ascontiguousarray(d["has_point"], np.uint8).tobytes())
                if "node" in d:
                    f.write(np.ascontiguousarray(d["node"], "<u4").tobytes())
                f.write(_map_points(n, salt).tobytes())
        for name in SET_NAMES:
            p1, p2, _ = Z.sim3_set(name)
            f.write(np.array([len(p1), 1 if Z.SIM3_SETS[name][1].get("fix_scale", True) else 0], "<i4").tobytes())
            f.write(np.ascontiguousarray(p1, "<f8").tobytes() + np.ascontiguousarray(p2, "<f8").tobytes())
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "LOOP_VERIFY_DRIVER_OK" in out.stdout, out.stderr
    r = _Reader(open(tmp_path / "lv_out.bin", "rb").read())
    for b, name in enumerate(PAIR_NAMES):
        cur, loop = Z.pair(name)
        cur = dict(cur, map_points=_map_points(len(cur["desc"]), 0)); loop = dict(loop, map_points=_map_points(len(loop["desc"]), 1))
        g = gpu_handle.verify_loop_candidates(cam, [(cur, loop)])[0]
        v = pkg.verify_loop_candidate(cur, loop, cam, 100 + b, 200 + b, handle=gpu_handle)
        some = int(r.take("u1", 1)[0]); rec = r.take(pkg.LOOP_VERIFY_RESULT, 1); sim3 = r.take("<f8", 8); ids = r.take("<u8", 2)
        matches, fm, inl, mmp = r.vec(pkg.DMATCH), r.vec("<i4"), r.vec("u1"), r.vec("<i8")
        assert some == (1 if v is not None else 0) == (1 if g["status"] == pkg.LOOP_OK else 0), name
        assert rec.tobytes() == g["record"].tobytes() and sim3.tobytes() == g["sim3"].tobytes() and list(ids) == [100 + b, 200 + b], name
        assert matches.tobytes() == g["matches"].tobytes() and fm.tobytes() == g["feature_matches"].tobytes() and inl.tobytes() == g["inlier"].tobytes()
        want = [(int(cur["map_points"][i]), int(loop["map_points"][j])) for i, j in g["feature_matches"]
                if cur["map_points"][i] >= 0 and loop["map_points"][j] >= 0]
        assert [tuple(x) for x in mmp.reshape(-1, 2)] == want, name
        if v is not None:
            assert v.matched_map_points == want and want
    for name in SET_NAMES:
        p1, p2, _ = Z.sim3_set(name)
        m = pkg.Sim3SolverConfig(**Z.SIM3_SETS[name][1])
        s, i, rec = gpu_handle.compute_sim3_ransac_batch([(p1, p2)], m)
        some = int(r.take("u1", 1)[0]); sim3 = r.take("<f8", 8); crec = r.take(pkg.SIM3_RESULT, 1); idx = r.vec("<u8")
        assert some == (1 if int(rec[0]["status"]) == pkg.SIM3_OK else 0), name
        if some:
            assert sim3.tobytes() == s[0].tobytes() and crec.tobytes() == rec[:1].tobytes() and list(idx) == list(np.flatnonzero(i[0])), name
    assert int(r.take("<i4", 1)[0]) == 1 and r.pos == len(r.buf)
