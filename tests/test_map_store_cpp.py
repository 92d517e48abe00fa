"""The C++ mirror of the resident map-point store (include/orbx.hpp: MapPointStore, MapTrackFrame, MapTrackResult, map_track_frames
and the track_local_map / track_with_motion_model overloads that take a store) — tests/cpp/map_store_driver.cpp built with g++
against liborbx_hip.so.  CPU: it compiles and links.  GPU: its results are the Python mirror's, byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import map_store_scenes as M
import tracking_scenes as G
from test_track_cpp import _Reader, _assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam3-rust_amd")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")


def _build(tmp):
    exe = os.path.join(tmp, "map_store_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "map_store_driver.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lorbx_hip", "-L", ROCM_LIB, "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ROCM_LIB], check=True)
    return exe


def test_map_store_driver_compiles_and_links(pkg, tmp_path):
    pkg.load_library()
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_map_store_driver_equals_python_mirror(pkg, tmp_path):
    import torch
    tmp = str(tmp_path)
    exe = _build(tmp)
    store, scs, frames_kf = M.shared_batch()
    cam = G.CAMERA
    tables = [t for sc in scs for t in sc["tables"]]
    first = np.cumsum([0] + [len(sc["tables"]) for sc in scs])
    frame_kfs = [[int(first[s] + k) for s, k in fk] for fk in frames_kf]
    frames = [scs[0]["frame"], scs[1]["frame"], scs[0]["frame"]]
    live = store.live_slots()
    with open(os.path.join(tmp, "map_store_in.bin"), "wb") as f:
        f.write(struct.pack("<iiii5d", store.capacity, len(live), len(tables), len(frames), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["baseline"]))
        f.write(live.astype(np.int32).tobytes()); f.write(store.positions[live].tobytes()); f.write(store.desc[live].tobytes())
        for t in tables:
            f.write(struct.pack("<i", len(t))); f.write(np.ascontiguousarray(t, np.int32).tobytes())
        for (kp, desc, sp, pr), ks in zip(frames, frame_kfs):
            f.write(struct.pack("<ii14d", len(kp), len(ks), *[float(v) for v in sp], *[float(v) for v in pr]))
            f.write(np.array(ks, np.int32).tobytes()); f.write(np.ascontiguousarray(kp, G.KEYPOINT).tobytes()); f.write(np.ascontiguousarray(desc, np.uint8).tobytes())
    r = subprocess.run([exe, tmp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MAP_STORE_DRIVER_OK" in r.stdout, (r.stdout, r.stderr)
    rd = _Reader(open(os.path.join(tmp, "map_store_out.bin"), "rb").read())

    def same(t, ls, ms):
        _assert_same(pkg, rd.result(pkg), t)
        assert rd.vec("<i4").tolist() == ls.tolist() and rd.vec("<i4").tolist() == ms.tolist()

    h = pkg.Handle(pkg.CameraModel(**cam), 1000, device=0, max_w=752, max_h=480, max_batch=1)
    mp = pkg.MapPointStore(h, store.capacity)
    kfs = []
    try:
        c = pkg.CameraModel(**cam)
        mp.set(live, store.positions[live], store.desc[live])
        for t in tables:
            n = len(t)
            kf = pkg.KeyFrame(h, torch.zeros((max(n, 1), 7), dtype=torch.float32, device="cuda"), torch.zeros((max(n, 1), 32), dtype=torch.uint8, device="cuda"), n)
            kf.set_map_point_slots(mp, t)
            kfs.append(kf)
        ks = [[kfs[i] for i in fk] for fk in frame_kfs]
        one = h.map_track_frames(c, mp, frames, keyframes=ks, cfg=pkg.TrackConfig.for_mode(1))
        for t, ls, ms in one:
            same(t, ls, ms)
            assert t.status == pkg.TRACK_OK
        frames0 = [(f[0], f[1], f[2], f[2]) for f in frames]
        for t, ls, ms in h.map_track_frames(c, mp, frames0, src_slots=[x[2] for x in one], cfg=pkg.TrackConfig.for_mode(0)):
            same(t, ls, ms)
            assert t.status == pkg.TRACK_OK
        same(*h.map_track_frames(c, mp, frames[:1], keyframes=ks[:1], cfg=pkg.TrackConfig.for_mode(1))[0])
        same(*h.map_track_frames(c, mp, frames0[:1], src_slots=[one[0][2]], cfg=pkg.TrackConfig.for_mode(0))[0])
        assert rd.take("<i4", 2).tolist() == [store.capacity, len(live)] and rd.pos == len(rd.buf)
    finally:
        h.synchronize()
        for k in kfs:
            k.close()
        mp.close()
        h.close()
