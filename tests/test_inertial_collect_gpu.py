"""The inertial local-BA window collected from the resident map on the GPU against tests/inertial_collect_spec.py: everything discrete is
byte-equal to the spec.  The inertial solver on 16-byte observations, host and device, equals the solver on the widened observations bit
for bit; orbx_map_local_inertial_ba returns exactly the result of the collection followed by that solver, writes exactly those positions
into the store, and is held to the oracle at tests/test_inertial_ba.py's tolerances."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ba_collect_scenes as B
import covisibility_scenes as V
import inertial_collect_scenes as I
import inertial_collect_spec as S
import inertial_edge_windows as W
import map_store_scenes as M
import tracking_scenes as G
from test_inertial_collect_cpu import build_driver
from test_map_store_gpu import _World, _d, _same, _select
from test_track_cpp import _Reader

pytestmark = pytest.mark.gpu
EMPTY = -6                            # ORBX_ERR_EMPTY


@pytest.fixture(scope="module")
def rows():
    return M.random_rows(8)


class _IWorld(_World):
    """_World whose keyframes carry keypoints (f32 x, y), stereo bytes (None: made without stereo points) and a pose"""

    def keyframe(self, table, xy, has=None, pose_wc=(1.0, 0, 0, 0, 0, 0, 0)):
        import torch
        n = len(xy)
        kp = G.keypoints(xy) if n else np.zeros(1, G.KEYPOINT)
        stereo = {} if has is None else dict(d_points_cam=torch.zeros((max(n, 1), 3), dtype=torch.float64, device="cuda"),
                                             d_has_point=_d(np.asarray(has, np.uint8) if n else np.zeros(1, np.uint8)))
        kf = self.pkg.KeyFrame(self.h, _d(kp.view(np.uint8).reshape(-1, G.KEYPOINT.itemsize)), torch.zeros((max(n, 1), 32), dtype=torch.uint8, device="cuda"), n,
                               pose_wc=pose_wc, **stereo)
        if table is not None:
            kf.set_map_point_slots(self.mp, table)
        self.kfs.append(kf)
        return kf


def _world(h, pkg, rows, tables, counts, live, seed, capacity=M.CAPACITY):
    """one keyframe (the last but one, a member of every tail) is made without has_point"""
    xy = B.keypoints(seed, counts)
    has = I.has_points(seed, counts)
    if len(tables) >= 2:
        has[len(tables) - 2] = None
    w = _IWorld(h, pkg, rows[0][:capacity], rows[1][:capacity], live, capacity=capacity)
    for t, p, hp in zip(tables, xy, has):
        w.keyframe(t, p, hp)
    return w, xy, has


def _collect(h, pkg, mp, kfs, chain):
    """the device form's outputs as numpy, cut to their sizes"""
    import torch
    o = h.map_collect_inertial_window_device(mp, kfs, chain)
    if o is None:
        return None
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in o.items()}
    K, F, M_, N = (int(x) for x in r["counts"])
    return dict(counts=r["counts"], fixed_kf=r["fixed_kf"][:F - 1], fixed_raw=r["fixed_kf"], list_slot=r["list_slot"][:M_], positions=r["positions"][:M_],
                obs32=np.ascontiguousarray(r["obs32"][:N]).view(pkg.BA_OBS32).reshape(-1), raw=o)


def _assert_spec(got, want, positions, n_kfs):
    for k in ("counts", "fixed_kf", "list_slot", "obs32"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, got["counts"], want["counts"])
    F = int(want["counts"][1])
    assert got["fixed_raw"].tolist() == want["fixed_kf"].tolist() + [-1] * (n_kfs - (F - 1))                   # entries [0, F - 1), then -1
    assert got["positions"].tobytes() == np.ascontiguousarray(positions[want["list_slot"]]).tobytes()


# ---- the collection against the specification ------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kfs", V.N_KFS)
def test_collection_equals_spec(gpu_handle, pkg, rows, n_kfs):
    """feature counts from {0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025}; chains of length 2, 3 and min(10, n_kfs), each as a tail,
    reversed and scattered; a chain whose anchor has no table; the chain of every keyframe; one keyframe without has_point"""
    tables, counts, live = V.world(40 + n_kfs, n_kfs)
    w, xy, has = _world(gpu_handle, pkg, rows, tables, counts, live, 40 + n_kfs)
    try:
        names, seen = set(), set()
        for name, chain in I.chains(n_kfs, tables, seed=n_kfs):
            want = S.collect(tables, xy, has, live, chain)
            _assert_spec(_collect(gpu_handle, pkg, w.mp, w.kfs, chain), want, rows[0], n_kfs)
            st = (want["obs32"]["mp_idx"] & S.STEREO) != 0
            names.add(name.rstrip("0123456789")); seen.add((bool(want["empty"]), int(want["counts"][1]) > 1, bool(st.any() and not st.all())))
        if n_kfs == 1:
            assert not names and _collect(gpu_handle, pkg, w.mp, w.kfs, [0]) is None                          # no chain of two: EMPTY
        if n_kfs >= 11:
            assert names >= {"tail", "reversed", "scattered", "anchor_without_table"} and (False, True, True) in seen and set(counts) == set(V.SIZES)
        if 11 <= n_kfs <= 65:
            assert "all" in names
    finally:
        w.close()


def test_collection_where_the_capacity_is_no_multiple_of_64(gpu_handle, pkg, rows):
    tables, counts, live = V.world(77, 11, capacity=1000)
    w, xy, has = _world(gpu_handle, pkg, rows, tables, counts, live, 77, capacity=1000)
    try:
        for chain in ([9, 10], [0, 4, 8, 2], list(range(11))):
            want = S.collect(tables, xy, has, live, chain)
            assert want["counts"][3] > 100
            _assert_spec(_collect(gpu_handle, pkg, w.mp, w.kfs, chain), want, rows[0], 11)
    finally:
        w.close()


def test_calls_leave_the_tables_as_found_and_repeat_themselves(gpu_handle, pkg, rows):
    tables, counts, live = V.world(31, 11)
    w, xy, has = _world(gpu_handle, pkg, rows, tables, counts, live, 31)
    try:
        with_table = [k for k in w.kfs if k is not w.kfs[5]]
        sel1 = _select(gpu_handle, w.mp, keyframes=[with_table, w.kfs[:3]])
        a = _collect(gpu_handle, pkg, w.mp, w.kfs, [8, 9, 10])
        assert _same(_select(gpu_handle, w.mp, keyframes=[with_table, w.kfs[:3]]), sel1)
        b = _collect(gpu_handle, pkg, w.mp, w.kfs, [8, 9, 10])
        for k in ("counts", "fixed_raw", "list_slot", "positions", "obs32"):
            assert a[k].tobytes() == b[k].tobytes(), k
        _assert_spec(_collect(gpu_handle, pkg, w.mp, w.kfs, [7, 2]), S.collect(tables, xy, has, live, [7, 2]), rows[0], 11)   # another window sees no trace of it
    finally:
        w.close()


def test_host_form_equals_device_form_and_refusals_touch_nothing(gpu_handle, pkg, rows):
    import torch
    tables, counts, live = V.world(31, 11)
    w, xy, has = _world(gpu_handle, pkg, rows, tables, counts, live, 31)
    other = pkg.MapPointStore(gpu_handle, 64)
    stranger = None
    try:
        chain = [8, 9, 10]
        dev = _collect(gpu_handle, pkg, w.mp, w.kfs, chain)
        host = gpu_handle.map_collect_inertial_window(w.mp, w.kfs, chain)
        for k in ("counts", "fixed_kf", "list_slot", "positions", "obs32"):
            assert host[k].dtype == dev[k].dtype and host[k].tobytes() == dev[k].tobytes(), k
        # M = 0 in the host form: EMPTY, counts and fixed_kf written
        e = {}
        t2 = [np.full(3, -1, np.int32), None]
        w2 = _IWorld(gpu_handle, pkg, rows[0], rows[1], live)
        try:
            for t in t2:
                w2.keyframe(t, np.zeros((3, 2), np.float32))
            assert gpu_handle.map_collect_inertial_window(w2.mp, w2.kfs, [0, 1], empty_info=e) is None
            assert e["counts"].tolist() == [2, 1, 0, 0] and e["fixed_kf"].tolist() == [-1, -1]
            assert gpu_handle.map_collect_inertial_window(w2.mp, w2.kfs, [0]) is None                          # n_chain = 1
        finally:
            w2.close()
        # a cap one below its bound: refused, the outputs untouched
        L = gpu_handle._L
        arr = (C.c_void_p * 11)(*[k._p for k in w.kfs])
        ch = np.array(chain, np.int32)
        cap, ocap = gpu_handle._inertial_window_bounds(w.mp, w.kfs, chain)
        assert ocap == sum(counts) and cap == min(sum(counts[k] for k in chain), M.CAPACITY)
        o = {k: torch.full_like(v, 0x5a) for k, v in dev["raw"].items()}
        p = lambda t: C.c_void_p(t.data_ptr())
        v = lambda a: a.ctypes.data_as(C.c_void_p)
        call = lambda c, oc, n=3: L.orbx_map_collect_inertial_window_device(gpu_handle._h, w.mp._p, C.c_int(11), arr, C.c_int(n), v(ch), C.c_int(c), C.c_int(oc),
                                                                            p(o["counts"]), p(o["fixed_kf"]), p(o["list_slot"]), p(o["positions"]), p(o["obs32"]))
        torch.cuda.synchronize()
        assert call(cap - 1, ocap) == -1 and call(cap, ocap - 1) == -1 and call(cap, ocap, 1) == EMPTY
        torch.cuda.synchronize()
        assert all(bool((t == torch.full_like(t, 0x5a)).all()) for t in o.values())
        hc = np.full(4, 7, np.int32); hf = np.full(11, 7, np.int32); hs = np.full(cap, 7, np.int32); hp = np.full((cap, 3), 7.0)
        ho = np.full(ocap * 16, 7, np.uint8)
        hcall = lambda c, oc, n=3: L.orbx_map_collect_inertial_window(gpu_handle._h, w.mp._p, C.c_int(11), arr, C.c_int(n), v(ch), C.c_int(c), C.c_int(oc), v(hc), v(hf),
                                                                      v(hs), v(hp), v(ho))
        assert hcall(cap - 1, ocap) == -1 and hcall(cap, ocap - 1) == -1 and hcall(cap, ocap, 1) == EMPTY
        assert all((a == 7).all() for a in (hc, hf, hs, hp, ho))
        assert call(cap, ocap) == 0 and hcall(cap, ocap) == 0
        torch.cuda.synchronize()
        assert o["counts"].cpu().numpy().tobytes() == dev["counts"].tobytes() == hc.tobytes()
        # what is refused before anything is enqueued
        stranger = w.keyframe(np.array([1, 2], np.int32), np.zeros((2, 2), np.float32)); w.kfs.pop()
        stranger.set_map_point_slots(other, [1, 2])
        before = w.mp.download()
        cam = pkg.CameraModel(**G.CAMERA)
        z = lambda n, m: np.zeros((n, m))
        local = lambda kfs, chain, ek=((0, 1),): gpu_handle.map_local_inertial_ba(cam, w.mp, kfs, chain, z(len(chain), 3), z(len(chain), 6), np.array(ek, np.int32).reshape(-1, 2),
                                                                                 np.tile([1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.25], (len(ek), 1)))
        bad = [lambda: gpu_handle.map_collect_inertial_window_device(w.mp, w.kfs, [9, 11]), lambda: gpu_handle.map_collect_inertial_window_device(w.mp, w.kfs, [-1, 9]),
               lambda: gpu_handle.map_collect_inertial_window_device(w.mp, w.kfs, [9, 10, 9]), lambda: gpu_handle.map_collect_inertial_window(w.mp, w.kfs, [9, 11]),
               lambda: gpu_handle.map_collect_inertial_window(w.mp, w.kfs, [3, 3]), lambda: gpu_handle.map_collect_inertial_window(w.mp, w.kfs + [stranger], [8, 9]),
               lambda: local(w.kfs, [9, 11]), lambda: local(w.kfs, [9, 9]), lambda: local(w.kfs, [8, 9, 10], ((0, 3),)), lambda: local(w.kfs, [8, 9, 10], ((-1, 1),)),
               lambda: local(w.kfs, [8, 9, 10], ((0, 1), (2, 2))), lambda: local(list(w.kfs) * 5, list(range(52))),
               lambda: gpu_handle.map_collect_inertial_window_device(w.mp, w.kfs + [stranger], [8, 9]), lambda: local(w.kfs + [stranger], [8, 9])]
        for i, f in enumerate(bad):
            with pytest.raises(pkg.OrbxError) as e:
                f()
            assert e.value.code == -1, i
        assert "another store" in str(e.value)
        assert local(w.kfs, [9]) is None                                                                       # n_chain = 1: EMPTY
        gpu_handle.set_allreduce(lambda ptr, n, stream: None)
        try:
            with pytest.raises(pkg.OrbxError) as e:
                local(w.kfs, [8, 9, 10])
            assert e.value.code == -1
        finally:
            gpu_handle.set_allreduce(None)
        assert _same(w.mp.download(), before)
        _assert_spec(_collect(gpu_handle, pkg, w.mp, w.kfs, chain), S.collect(tables, xy, has, live, chain), rows[0], 11)     # the next valid call is exact
    finally:
        gpu_handle.synchronize()
        if stranger is not None:
            stranger.close()
        other.close()
        w.close()


# ---- the solver's 16-byte forms -------------------------------------------------------------------------------------------------

def _solve_bytes(r):
    return (r["poses_wc"].tobytes(), r["velocities"].tobytes(), r["biases"].tobytes(), r["points"].tobytes(), r["iterations"],
            struct.pack("<2d", r["initial_error"], r["final_error"]))


@pytest.mark.parametrize("name,K", [("shuffled", 5), ("shuffled", 13), ("descending", 22)])
def test_inertial_obs32_forms_equal_the_solver_on_widened_observations(gpu_handle, pkg, name, K):
    """K = 5: the tiled assembly; 13: the global one; 22: one launch per panel"""
    w = pkg.synth.keypoint_precision(W.build(name, W.SEEDS[0], K, W.POINTS[K]))
    cam, cfg = pkg.CameraModel(**w["camera"]), pkg.LocalInertialBAConfig()
    F = len(w["fixed_cw"])
    o32 = pkg.ba_obs_to_obs32(w["obs"], F, inertial=True)
    st = (o32["mp_idx"] & S.STEREO) != 0
    assert st.any() and not st.all() and S.widen(o32, F).tobytes() == np.ascontiguousarray(w["obs"], S.BA_OBS).tobytes()
    args = (w["poses_wc"], w["velocities"], w["biases"], w["fixed_cw"], w["points"])
    want = gpu_handle.ba_solve_inertial(cam, cfg, *args, w["obs"], w["edge_kf"], w["preint"])
    host = gpu_handle.ba_solve_inertial_obs32(cam, cfg, *args, o32, w["edge_kf"], w["preint"])
    d_obs = _d(o32.view(np.uint8).reshape(-1, 16))
    dev = gpu_handle.ba_solve_inertial_obs32_device(cam, cfg, *args, d_obs, len(o32), w["edge_kf"], w["preint"])
    assert want["iterations"] > 0 and want["final_error"] < want["initial_error"]
    assert _solve_bytes(host) == _solve_bytes(want) and _solve_bytes(dev) == _solve_bytes(want)
    if K == 5:
        # the visual form reads mp_idx whole: a flagged index is out of range, never silently dropped
        vis = pkg.LocalBAConfigLM()
        poses_cw = np.array([pkg.se3_inverse(p) for p in w["poses_wc"]])
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.ba_solve_visual(cam, vis, poses_cw, w["fixed_cw"], w["points"], o32)
        assert e.value.code == -1 and "out of range" in str(e.value)
        plain = o32.copy(); plain["mp_idx"] &= ~S.STEREO
        assert gpu_handle.ba_solve_visual(cam, vis, poses_cw, w["fixed_cw"], w["points"], plain)["iterations"] > 0
        # an index out of range in the device form is named without being read; a hook refuses the device form
        badobs = o32.copy(); badobs["mp_idx"][7] = len(w["points"]) | (o32["mp_idx"][7] & S.STEREO)
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.ba_solve_inertial_obs32_device(cam, cfg, *args, _d(badobs.view(np.uint8).reshape(-1, 16)), len(o32), w["edge_kf"], w["preint"])
        assert e.value.code == -1 and "observation 7 (device memory)" in str(e.value)
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.ba_solve_inertial_obs32(cam, cfg, *args, badobs, w["edge_kf"], w["preint"])
        assert e.value.code == -1 and "mp %d/%d" % (len(w["points"]), len(w["points"])) in str(e.value)
        gpu_handle.set_allreduce(lambda ptr, n, stream: None)
        try:
            with pytest.raises(pkg.OrbxError) as e:
                gpu_handle.ba_solve_inertial_obs32_device(cam, cfg, *args, d_obs, len(o32), w["edge_kf"], w["preint"])
            assert e.value.code == -1
        finally:
            gpu_handle.set_allreduce(None)
        assert _solve_bytes(gpu_handle.ba_solve_inertial_obs32_device(cam, cfg, *args, d_obs, len(o32), w["edge_kf"], w["preint"])) == _solve_bytes(want)


# ---- orbx_map_local_inertial_ba -----------------------------------------------------------------------------------------------

def _scene_world(h, pkg, sc):
    st = sc["store"]
    w = _IWorld(h, pkg, st.positions, st.desc, st.live)
    for t, xy, hp, pose in zip(sc["tables"], sc["xy"], sc["has"], sc["poses_wc"]):
        w.keyframe(t, xy, hp, pose_wc=pose)
    return w


@pytest.mark.parametrize("K", [5, 11])
def test_map_local_inertial_ba_returns_that_result_and_writes_it_into_the_store(gpu_handle, pkg, K):
    sc, win, spec, o = I.solved_scene(I.SCENE_SEEDS[K], K)
    w = _scene_world(gpu_handle, pkg, sc)
    try:
        st = sc["store"]
        cam, cfg = pkg.CameraModel(**sc["camera"]), pkg.LocalInertialBAConfig()
        c = gpu_handle.map_collect_inertial_window(w.mp, w.kfs, sc["chain"])
        for k in ("counts", "fixed_kf", "list_slot", "obs32"):
            assert c[k].tobytes() == spec[k].tobytes(), k
        assert c["positions"].tobytes() == win["points"].tobytes()
        want = gpu_handle.ba_solve_inertial_obs32(cam, cfg, win["poses_wc"], win["velocities"], win["biases"], win["fixed_cw"], c["positions"], c["obs32"],
                                                  win["edge_kf"], win["preint"])
        r = gpu_handle.map_local_inertial_ba(cam, w.mp, w.kfs, sc["chain"], win["velocities"], win["biases"], win["edge_kf"], win["preint"], cfg)
        assert r["counts"].tobytes() == c["counts"].tobytes() and r["fixed_kf"].tobytes() == c["fixed_kf"].tobytes()
        P = c["list_slot"]
        got = dict(r, points=w.mp.download(P)[0])
        assert _solve_bytes(got) == _solve_bytes(want) and r["iterations"] > 0 and r["final_error"] < r["initial_error"]
        # the store: the window's positions are the returned points, everything else is as it was
        pos, desc, lv = w.mp.download()
        rest = np.setdiff1d(np.arange(M.CAPACITY), P)
        assert pos[rest].tobytes() == st.positions[rest].tobytes() and desc.tobytes() == st.desc.tobytes() and lv.tobytes() == st.live.tobytes()
        assert not np.array_equal(pos[P], st.positions[P])
        # the oracle on the spec's window, at tests/test_inertial_ba.py's tolerances
        print("K %d: iterations %d / %d, initial %.3e, final %.3e, outputs %s" % (
            K, got["iterations"], o["iterations"], abs(got["initial_error"] - o["initial_error"]) / o["initial_error"],
            abs(got["final_error"] - o["final_error"]) / o["final_error"], ["%.2e" % W.rel(got[k], o[k]) for k in W.OUTPUTS]))
        assert got["iterations"] == o["iterations"]
        assert abs(got["initial_error"] - o["initial_error"]) < 1e-10 * o["initial_error"]
        assert abs(got["final_error"] - o["final_error"]) < 1e-7 * o["final_error"]
        for key in W.OUTPUTS:
            assert W.rel(got[key], o[key]) < 1e-6, key
    finally:
        w.close()


def test_no_write_back_without_an_iteration(gpu_handle, pkg):
    sc, win, spec, o = I.solved_scene(I.SCENE_SEEDS[5], 5)
    w = _scene_world(gpu_handle, pkg, sc)
    try:
        cam = pkg.CameraModel(**sc["camera"])
        before = w.mp.download()
        r = gpu_handle.map_local_inertial_ba(cam, w.mp, w.kfs, sc["chain"], win["velocities"], win["biases"], win["edge_kf"], win["preint"], should_stop=lambda: True)
        assert r is not None and r["iterations"] == 0 and r["counts"].tobytes() == spec["counts"].tobytes()
        assert _same(w.mp.download(), before)
        r = gpu_handle.map_local_inertial_ba(cam, w.mp, w.kfs, sc["chain"], win["velocities"], win["biases"], win["edge_kf"][:0], win["preint"][:0])   # E = 0
        assert r["iterations"] > 0 and not _same(w.mp.download(), before)
    finally:
        w.close()


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------

def test_inertial_collect_driver_equals_python_mirror(pkg, tmp_path):
    tmp = str(tmp_path)
    exe = build_driver(tmp)
    sc, win, spec, o = I.solved_scene(I.SCENE_SEEDS[5], 5)
    st, cam = sc["store"], sc["camera"]
    live = st.live_slots()
    with open(os.path.join(tmp, "inertial_collect_in.bin"), "wb") as f:
        f.write(struct.pack("<iiiii5d", st.capacity, len(live), len(sc["tables"]), len(sc["chain"]), len(win["edge_kf"]), cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                            cam["baseline"]))
        f.write(live.astype(np.int32).tobytes()); f.write(st.positions[live].tobytes()); f.write(st.desc[live].tobytes())
        for t, xy, hp, pose in zip(sc["tables"], sc["xy"], sc["has"], sc["poses_wc"]):
            f.write(struct.pack("<i", len(t))); f.write(np.ascontiguousarray(t, np.int32).tobytes()); f.write(np.ascontiguousarray(G.keypoints(xy), G.KEYPOINT).tobytes())
            f.write(np.ascontiguousarray(hp, np.uint8).tobytes()); f.write(np.ascontiguousarray(pose, np.float64).tobytes())
        f.write(np.array(sc["chain"], np.int32).tobytes()); f.write(np.ascontiguousarray(win["velocities"]).tobytes()); f.write(np.ascontiguousarray(win["biases"]).tobytes())
        f.write(np.ascontiguousarray(win["edge_kf"], np.int32).tobytes()); f.write(np.ascontiguousarray(win["preint"]).tobytes())
    r = subprocess.run([exe, tmp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "INERTIAL_COLLECT_DRIVER_OK" in r.stdout, (r.stdout, r.stderr)
    rd = _Reader(open(os.path.join(tmp, "inertial_collect_out.bin"), "rb").read())
    h = pkg.Handle(pkg.CameraModel(**cam), 1000, device=0, max_w=752, max_h=480, max_batch=1)
    w = _scene_world(h, pkg, sc)
    try:
        c = h.map_collect_inertial_window(w.mp, w.kfs, sc["chain"])
        assert rd.vec("<i4").tobytes() == c["counts"].tobytes() == spec["counts"].tobytes() and rd.vec("<i4").tobytes() == c["fixed_kf"].tobytes()
        assert rd.vec("<i4").tobytes() == c["list_slot"].tobytes() and rd.vec(("<f8", 3)).tobytes() == c["positions"].tobytes()
        assert rd.vec(pkg.BA_OBS32).tobytes() == c["obs32"].tobytes() == spec["obs32"].tobytes()
        res = h.map_local_inertial_ba(pkg.CameraModel(**cam), w.mp, w.kfs, sc["chain"], win["velocities"], win["biases"], win["edge_kf"], win["preint"])
        assert rd.vec("<i4").tobytes() == res["counts"].tobytes() and rd.vec("<i4").tobytes() == res["fixed_kf"].tobytes()
        assert rd.vec("<f8").tobytes() == res["poses_wc"].tobytes() and rd.vec(("<f8", 3)).tobytes() == res["velocities"].tobytes()
        assert rd.vec("<f8").tobytes() == res["biases"].tobytes()
        assert rd.vec("<f8").tobytes() == np.array([res["iterations"], res["initial_error"], res["final_error"]], np.float64).tobytes()
        assert rd.vec(("<f8", 3)).tobytes() == w.mp.download(c["list_slot"])[0].tobytes()
        assert rd.pos == len(rd.buf) and res["iterations"] > 0
    finally:
        w.close()
        h.close()
