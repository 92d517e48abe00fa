"""The local-BA window collected from the resident map on the GPU against tests/ba_collect_spec.py: everything discrete is byte-equal
to the spec.  The solver with its observations in device memory equals, bit for bit, the solver on a host copy; orbx_map_local_ba
returns exactly that result, writes exactly those positions into the store, and is held to the oracle at the project's BA bar."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ba_collect_scenes as B
import ba_collect_spec as S
import covisibility_scenes as V
import map_store_scenes as M
import tracking_scenes as G
from conftest import assert_ba_close
from test_ba_collect_cpu import build_driver
from test_map_store_gpu import _World, _d, _same, _select
from test_track_cpp import _Reader

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.CameraModel(**G.CAMERA)


@pytest.fixture(scope="module")
def rows():
    return M.random_rows(8)


class _BaWorld(_World):
    """_World whose keyframes carry keypoints (f32 x, y) and a pose"""

    def keyframe(self, table, xy, pose_wc=(1.0, 0, 0, 0, 0, 0, 0)):
        import torch
        n = len(xy)
        kp = G.keypoints(xy) if n else np.zeros(1, G.KEYPOINT)
        kf = self.pkg.KeyFrame(self.h, _d(kp.view(np.uint8).reshape(-1, G.KEYPOINT.itemsize)), torch.zeros((max(n, 1), 32), dtype=torch.uint8, device="cuda"), n,
                               pose_wc=pose_wc)
        if table is not None:
            kf.set_map_point_slots(self.mp, table)
        self.kfs.append(kf)
        return kf


def _world(h, pkg, rows, tables, counts, live, seed, capacity=M.CAPACITY):
    xy = B.keypoints(seed, counts)
    w = _BaWorld(h, pkg, rows[0][:capacity], rows[1][:capacity], live, capacity=capacity)
    for t, p in zip(tables, xy):
        w.keyframe(t, p)
    return w, xy


def _collect(h, pkg, mp, kfs, cur, max_cov):
    """the device form's outputs as numpy, cut to their sizes"""
    import torch
    o = h.map_collect_ba_window_device(mp, kfs, cur, max_cov)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in o.items()}
    K, F, M_, N = (int(x) for x in r["counts"])
    return dict(counts=r["counts"], local_kf=r["local_kf"], fixed_kf=r["fixed_kf"][:F - 1], list_slot=r["list_slot"][:M_], positions=r["positions"][:M_],
                obs32=np.ascontiguousarray(r["obs32"][:N]).view(pkg.BA_OBS32).reshape(-1), raw=o)


def _assert_spec(got, want, positions):
    for k in ("counts", "local_kf", "fixed_kf", "list_slot", "obs32"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, got["counts"], want["counts"])
    assert got["positions"].tobytes() == np.ascontiguousarray(positions[want["list_slot"]]).tobytes()


def _curs(tables):
    n = len(tables)
    none = [k for k, t in enumerate(tables) if t is None]
    return sorted({0, n - 1, n // 2} | set(none[:1]))


# ---- the collection against the specification ------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kfs", V.N_KFS)
def test_collection_equals_spec(gpu_handle, pkg, rows, n_kfs):
    """feature counts from {0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025}; max_covisible in {0, 1, 20}; cur = the first, the
    last, a keyframe without a table, one in the middle"""
    tables, counts, live = V.world(20 + n_kfs, n_kfs)
    w, xy = _world(gpu_handle, pkg, rows, tables, counts, live, 20 + n_kfs)
    try:
        seen = set()
        for max_cov in (0, 1, 20):
            for cur in _curs(tables):
                want = S.collect(tables, xy, live, cur, max_cov)
                _assert_spec(_collect(gpu_handle, pkg, w.mp, w.kfs, cur, max_cov), want, rows[0])
                seen.add((bool(want["empty"]), int(want["counts"][1]) > 1))
        if n_kfs >= 11:
            assert {(True, False), (False, True)} <= seen and set(counts) == set(V.SIZES)       # empty windows (cur without a table) and windows with fixed observers
    finally:
        w.close()


def test_collection_where_the_capacity_is_no_multiple_of_64(gpu_handle, pkg, rows):
    tables, counts, live = V.world(77, 11, capacity=1000)
    w, xy = _world(gpu_handle, pkg, rows, tables, counts, live, 77, capacity=1000)
    try:
        for cur, max_cov in ((0, 3), (10, 20), (4, 0)):
            want = S.collect(tables, xy, live, cur, max_cov)
            assert want["counts"][3] > 100
            _assert_spec(_collect(gpu_handle, pkg, w.mp, w.kfs, cur, max_cov), want, rows[0])
    finally:
        w.close()


def test_collection_where_the_tie_order_decides_the_local_keyframes(gpu_handle, pkg, rows):
    tables, counts, live = V.row_world("equal", 65)
    w, xy = _world(gpu_handle, pkg, rows, tables, counts, live, 65)
    try:
        for max_cov in (5, 20, 70):
            want = S.collect(tables, xy, live, 0, max_cov)
            assert want["local_kf"][:1 + min(max_cov, 64)].tolist() == list(range(1 + min(max_cov, 64)))     # a 64-way tie: position order
            _assert_spec(_collect(gpu_handle, pkg, w.mp, w.kfs, 0, max_cov), want, rows[0])
    finally:
        w.close()


# ---- the tables are left as found ------------------------------------------------------------------------------------------

def test_calls_leave_the_tables_as_found_and_repeat_themselves(gpu_handle, pkg, rows):
    tables, counts, live = V.world(31, 11)
    w, xy = _world(gpu_handle, pkg, rows, tables, counts, live, 31)
    try:
        with_table = [k for k in w.kfs if k is not w.kfs[5]]
        cov = lambda: gpu_handle.map_covisibility(w.mp, w.kfs, range(11), 5)
        sel1, cov1 = _select(gpu_handle, w.mp, keyframes=[with_table, w.kfs[:3]]), cov()
        a = _collect(gpu_handle, pkg, w.mp, w.kfs, 2, 4)
        assert _same(_select(gpu_handle, w.mp, keyframes=[with_table, w.kfs[:3]]), sel1) and _same(cov(), cov1)
        b = _collect(gpu_handle, pkg, w.mp, w.kfs, 2, 4)
        for k in ("counts", "local_kf", "fixed_kf", "list_slot", "positions", "obs32"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert all(a["raw"][k].cpu().numpy().tobytes() == b["raw"][k].cpu().numpy().tobytes() for k in ("counts", "local_kf", "fixed_kf"))
        _assert_spec(_collect(gpu_handle, pkg, w.mp, w.kfs, 7, 2), S.collect(tables, xy, live, 7, 2), rows[0])    # another window sees no trace of it
    finally:
        w.close()


# ---- host form, caps, refusals ---------------------------------------------------------------------------------------------

def test_host_form_equals_device_form_and_refusals_touch_nothing(gpu_handle, pkg, rows):
    import torch
    tables, counts, live = V.world(31, 11)
    w, xy = _world(gpu_handle, pkg, rows, tables, counts, live, 31)
    other = pkg.MapPointStore(gpu_handle, 64)
    stranger = None
    try:
        dev = _collect(gpu_handle, pkg, w.mp, w.kfs, 2, 4)
        host = gpu_handle.map_collect_ba_window(w.mp, w.kfs, 2, 4)
        for k in ("counts", "local_kf", "fixed_kf", "list_slot", "positions", "obs32"):
            assert host[k].dtype == dev[k].dtype and host[k].tobytes() == dev[k].tobytes(), k
        assert gpu_handle.map_collect_ba_window(w.mp, w.kfs, 5, 4) is None and S.collect(tables, xy, live, 5, 4)["empty"]      # cur without a table
        # a cap one below its bound: refused, the outputs untouched
        L = gpu_handle._L
        arr = (C.c_void_p * 11)(*[k._p for k in w.kfs])
        cap, ocap = gpu_handle._ba_window_bounds(w.mp, w.kfs, 2, 4)
        assert ocap == sum(counts) and cap == min(counts[2] + sum(sorted(counts[:2] + counts[3:], reverse=True)[:4]), M.CAPACITY)
        o = {k: torch.full_like(v, 0x5a) for k, v in dev["raw"].items()}
        p = lambda t: C.c_void_p(t.data_ptr())
        call = lambda c, oc: L.orbx_map_collect_ba_window_device(gpu_handle._h, w.mp._p, C.c_int(11), arr, C.c_int(2), C.c_int(4), C.c_int(c), C.c_int(oc), p(o["counts"]),
                                                                 p(o["local_kf"]), p(o["fixed_kf"]), p(o["list_slot"]), p(o["positions"]), p(o["obs32"]))
        torch.cuda.synchronize()
        assert call(cap - 1, ocap) == -1 and call(cap, ocap - 1) == -1
        torch.cuda.synchronize()
        assert all(bool((v == torch.full_like(v, 0x5a)).all()) for v in o.values())
        hc = np.full(4, 7, np.int32); hl = np.full(5, 7, np.int32); hf = np.full(11, 7, np.int32); hs = np.full(cap, 7, np.int32); hp = np.full((cap, 3), 7.0)
        ho = np.full(ocap * 16, 7, np.uint8)
        v = lambda a: a.ctypes.data_as(C.c_void_p)
        hcall = lambda c, oc: L.orbx_map_collect_ba_window(gpu_handle._h, w.mp._p, C.c_int(11), arr, C.c_int(2), C.c_int(4), C.c_int(c), C.c_int(oc), v(hc), v(hl), v(hf),
                                                           v(hs), v(hp), v(ho))
        assert hcall(cap - 1, ocap) == -1 and hcall(cap, ocap - 1) == -1
        assert all((a == 7).all() for a in (hc, hl, hf, hs, hp, ho))
        assert call(cap, ocap) == 0 and hcall(cap, ocap) == 0
        torch.cuda.synchronize()
        assert o["counts"].cpu().numpy().tobytes() == dev["counts"].tobytes() == hc.tobytes()
        # what is refused before anything is enqueued
        stranger = w.keyframe(np.array([1, 2], np.int32), np.zeros((2, 2), np.float32)); w.kfs.pop()
        stranger.set_map_point_slots(other, [1, 2])
        bad = [lambda: gpu_handle.map_collect_ba_window_device(w.mp, w.kfs, 11, 4), lambda: gpu_handle.map_collect_ba_window_device(w.mp, w.kfs, -1, 4),
               lambda: gpu_handle.map_collect_ba_window_device(w.mp, w.kfs, 0, -1), lambda: gpu_handle.map_collect_ba_window_device(w.mp, [], 0, 4),
               lambda: gpu_handle.map_collect_ba_window_device(w.mp, w.kfs + [stranger], 0, 4), lambda: gpu_handle.map_collect_ba_window(w.mp, w.kfs, 11, 4),
               lambda: gpu_handle.map_collect_ba_window(w.mp, [], 0, 4), lambda: gpu_handle.map_collect_ba_window(w.mp, w.kfs + [stranger], 0, 4),
               lambda: gpu_handle.map_local_ba(pkg.CameraModel(**G.CAMERA), w.mp, w.kfs, 11), lambda: gpu_handle.map_local_ba(pkg.CameraModel(**G.CAMERA), w.mp, w.kfs + [stranger], 0)]
        for i, f in enumerate(bad):
            with pytest.raises(pkg.OrbxError) as e:
                f()
            assert e.value.code == -1, i
        assert "another store" in str(e.value)
        _assert_spec(_collect(gpu_handle, pkg, w.mp, w.kfs, 2, 4), S.collect(tables, xy, live, 2, 4), rows[0])               # the next valid call is exact
    finally:
        gpu_handle.synchronize()
        if stranger is not None:
            stranger.close()
        other.close()
        w.close()


# ---- the solver on device observations, and the driver -----------------------------------------------------------------------

def _scene_world(h, pkg):
    sc = B.ba_scene()
    st = sc["store"]
    w = _BaWorld(h, pkg, st.positions, st.desc, st.live)
    for t, kp, pose in zip(sc["tables"], sc["kps"], sc["poses_wc"]):
        w.keyframe(t, np.stack([kp["x"], kp["y"]], 1), pose_wc=pose)
    return sc, w


def _window_arrays(pkg, sc, c):
    """the collection's outputs as orbx_ba_solve_visual_obs32's arguments: T_cw of local[1..] and of [local[0]] ++ fixed"""
    K = int(c["counts"][0])
    poses_cw = np.array([pkg.se3_inverse(sc["poses_wc"][k]) for k in c["local_kf"][1:1 + K]]).reshape(-1, 7)
    fixed_cw = np.array([pkg.se3_inverse(sc["poses_wc"][k]) for k in [c["local_kf"][0]] + c["fixed_kf"].tolist()]).reshape(-1, 7)
    return poses_cw, fixed_cw


def _solve_bytes(r):
    return (r["poses_wc"].tobytes(), r["points"].tobytes(), r["iterations"], struct.pack("<2d", r["initial_error"], r["final_error"]))


def test_solver_on_device_observations_equals_solver_on_their_host_copy(gpu_handle, pkg, cam):
    sc, w = _scene_world(gpu_handle, pkg)
    try:
        cfg = pkg.LocalBAConfigLM(max_covisible_keyframes=sc["max_covisible"])
        c = _collect(gpu_handle, pkg, w.mp, w.kfs, sc["cur"], sc["max_covisible"])
        xy = [np.stack([k["x"], k["y"]], 1) for k in sc["kps"]]
        _assert_spec(c, S.collect(sc["tables"], xy, sc["store"].live, sc["cur"], sc["max_covisible"]), sc["store"].positions)
        poses_cw, fixed_cw = _window_arrays(pkg, sc, c)
        N = int(c["counts"][3])
        dev = gpu_handle.ba_solve_visual_obs32_device(cam, cfg, poses_cw, fixed_cw, c["positions"], c["raw"]["obs32"], N)
        host = gpu_handle.ba_solve_visual(cam, cfg, poses_cw, fixed_cw, c["positions"], c["obs32"])
        assert _solve_bytes(dev) == _solve_bytes(host) and host["iterations"] > 0 and host["final_error"] < host["initial_error"]
        assert _solve_bytes(gpu_handle.ba_solve_visual_obs32_device(cam, cfg, poses_cw, fixed_cw, c["positions"], c["raw"]["obs32"], N)) == _solve_bytes(host)
        # with an all-reduce hook installed the observations would be read on the host: refused
        gpu_handle.set_allreduce(lambda ptr, n, stream: None)
        try:
            with pytest.raises(pkg.OrbxError) as e:
                gpu_handle.ba_solve_visual_obs32_device(cam, cfg, poses_cw, fixed_cw, c["positions"], c["raw"]["obs32"], N)
            assert e.value.code == -1
            with pytest.raises(pkg.OrbxError) as e:
                gpu_handle.map_local_ba(cam, w.mp, w.kfs, sc["cur"], cfg)
            assert e.value.code == -1
        finally:
            gpu_handle.set_allreduce(None)
        assert _same(w.mp.download(), (sc["store"].positions, sc["store"].desc, sc["store"].live))
    finally:
        w.close()


def test_map_local_ba_returns_that_result_and_writes_it_into_the_store(gpu_handle, pkg, cam, oracle):
    sc, w = _scene_world(gpu_handle, pkg)
    try:
        st = sc["store"]
        cfg = pkg.LocalBAConfigLM(max_covisible_keyframes=sc["max_covisible"])
        c = _collect(gpu_handle, pkg, w.mp, w.kfs, sc["cur"], sc["max_covisible"])
        poses_cw, fixed_cw = _window_arrays(pkg, sc, c)
        want = gpu_handle.ba_solve_visual(cam, cfg, poses_cw, fixed_cw, c["positions"], c["obs32"])
        K, F, M_, N = (int(x) for x in c["counts"])
        r = gpu_handle.map_local_ba(cam, w.mp, w.kfs, sc["cur"], cfg)
        assert r.counts.tobytes() == c["counts"].tobytes() and r.local_kf.tobytes() == c["local_kf"].tobytes() and r.list_slot.tobytes() == c["list_slot"].tobytes()
        assert list(r.optimized_poses) == c["local_kf"][1:1 + K].tolist() and list(r.optimized_points) == c["list_slot"].tolist()
        got = dict(poses_wc=np.array([r.optimized_poses[k] for k in r.optimized_poses]), points=r.points, iterations=r.iterations, initial_error=r.initial_error,
                   final_error=r.final_error)
        assert _solve_bytes(got) == _solve_bytes(want)
        assert r.final_error < r.initial_error and r.iterations > 0
        # the store: the window's positions are the returned points, everything else is as it was
        P = c["list_slot"]
        assert w.mp.download(P)[0].tobytes() == want["points"].tobytes()
        pos, desc, lv = w.mp.download()
        rest = np.setdiff1d(np.arange(M.CAPACITY), P)
        assert pos[rest].tobytes() == st.positions[rest].tobytes() and desc.tobytes() == st.desc.tobytes() and lv.tobytes() == st.live.tobytes()
        assert not np.array_equal(pos[P], st.positions[P])
        # the oracle on the same flattened window, at the project's BA bar (tests/test_ba_gpu.py)
        obs = np.zeros(N, pkg.BA_OBS)
        k = c["obs32"]["kf_idx"]
        obs["kf_idx"] = np.where(k >= 0, k, -1); obs["fixed_idx"] = np.where(k >= 0, -1, -1 - k); obs["mp_idx"] = c["obs32"]["mp_idx"]
        obs["u"] = c["obs32"]["u"]; obs["v"] = c["obs32"]["v"]
        assert pkg.ba_obs_to_obs32(obs, F).tobytes() == c["obs32"].tobytes()
        ocfg = oracle.ba_config()
        o = oracle.ba_solve_schur(oracle.Camera(**G.CAMERA), ocfg, poses_cw, fixed_cw, c["positions"], obs)
        assert_ba_close(got, o, 1e-6)
    finally:
        w.close()


def test_an_empty_window_leaves_the_store_unchanged(gpu_handle, pkg, cam, rows):
    tables, counts, live = V.world(31, 11)
    w, xy = _world(gpu_handle, pkg, rows, tables, counts, live, 31)
    try:
        before = w.mp.download()
        assert tables[5] is None and gpu_handle.map_local_ba(cam, w.mp, w.kfs, 5) is None
        assert _same(w.mp.download(), before)
        _assert_spec(_collect(gpu_handle, pkg, w.mp, w.kfs, 2, 4), S.collect(tables, xy, live, 2, 4), rows[0])
    finally:
        w.close()


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------

def test_ba_collect_driver_equals_python_mirror(pkg, tmp_path):
    tmp = str(tmp_path)
    exe = build_driver(tmp)
    sc = B.ba_scene()
    st, cam = sc["store"], G.CAMERA
    live = st.live_slots()
    with open(os.path.join(tmp, "ba_collect_in.bin"), "wb") as f:
        f.write(struct.pack("<iiiii5d", st.capacity, len(live), len(sc["tables"]), sc["cur"], sc["max_covisible"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["baseline"]))
        f.write(live.astype(np.int32).tobytes()); f.write(st.positions[live].tobytes()); f.write(st.desc[live].tobytes())
        for t, kp, pose in zip(sc["tables"], sc["kps"], sc["poses_wc"]):
            f.write(struct.pack("<i", len(t))); f.write(np.ascontiguousarray(t, np.int32).tobytes()); f.write(np.ascontiguousarray(kp, G.KEYPOINT).tobytes())
            f.write(np.ascontiguousarray(pose, np.float64).tobytes())
    r = subprocess.run([exe, tmp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "BA_COLLECT_DRIVER_OK" in r.stdout, (r.stdout, r.stderr)
    rd = _Reader(open(os.path.join(tmp, "ba_collect_out.bin"), "rb").read())
    h = pkg.Handle(pkg.CameraModel(**cam), 1000, device=0, max_w=752, max_h=480, max_batch=1)
    sc2, w = _scene_world(h, pkg)
    try:
        c = h.map_collect_ba_window(w.mp, w.kfs, sc["cur"], sc["max_covisible"])
        assert rd.vec("<i4").tobytes() == c["counts"].tobytes() and rd.vec("<i4").tobytes() == c["local_kf"].tobytes() and rd.vec("<i4").tobytes() == c["fixed_kf"].tobytes()
        assert rd.vec("<i4").tobytes() == c["list_slot"].tobytes() and rd.vec(("<f8", 3)).tobytes() == c["positions"].tobytes()
        assert rd.vec(pkg.BA_OBS32).tobytes() == c["obs32"].tobytes()
        res = h.map_local_ba(pkg.CameraModel(**cam), w.mp, w.kfs, sc["cur"], pkg.LocalBAConfigLM(max_covisible_keyframes=sc["max_covisible"]))
        assert rd.vec("<i4").tobytes() == res.counts.tobytes() and rd.vec("<i4").tobytes() == res.local_kf.tobytes()
        assert rd.vec("<f8").tobytes() == np.array([res.optimized_poses[k] for k in res.optimized_poses]).tobytes()
        assert rd.vec("<f8").tobytes() == np.array([res.iterations, res.initial_error, res.final_error], np.float64).tobytes()
        assert rd.vec(("<f8", 3)).tobytes() == res.points.tobytes() == w.mp.download(c["list_slot"])[0].tobytes()
        assert rd.pos == len(rd.buf) and res.iterations > 0
    finally:
        w.close()
        h.close()
