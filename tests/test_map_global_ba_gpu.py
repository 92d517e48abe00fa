"""Global BA from the resident map on the GPU (orbx_map_collect_global[_device], orbx_map_global_ba): the whole map's problem collected
where the slot tables lie equals tests/map_global_spec.py byte for byte, and the driver equals the sequence collect, then
ba_solve_global_map_obs32 on the downloaded arrays, then MapPointStore.set — byte for byte in poses, store positions and scalars.

The discrete world has dead slots, a keyframe without a table, slots repeated inside a keyframe, features without a point and, through
the device form of set_map_point_slots, a slot out of range (which a table stores as -1: no table can hold one).  A second, geometric
world of 140 small keyframes shows that the resident call crosses the window solver's 128.
"""
import struct

import numpy as np
import pytest

import ba_collect_scenes as B
import covisibility_scenes as V
import map_global_spec as S
import map_store_scenes as M
import tracking_scenes as G
from test_ba_collect_gpu import _BaWorld, _world
from test_map_store_gpu import _d, _same

pytestmark = pytest.mark.gpu

SIZES = [257, 64, 255, 1, 300, 65, 256, 0]            # features per keyframe of the discrete world (keyframe 5 has no table)


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.CameraModel(**G.CAMERA)


@pytest.fixture(scope="module")
def rows():
    return M.random_rows(8)


def _collect_dev(h, pkg, mp, kfs, **caps):
    """the device form's outputs as numpy, cut to their sizes"""
    import torch
    o = h.map_collect_global_device(mp, kfs, **caps)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in o.items()}
    K, F, M_, N = (int(x) for x in r["counts"])
    return dict(counts=r["counts"], list_slot=r["list_slot"][:M_], positions=r["positions"][:M_],
                obs32=np.ascontiguousarray(r["obs32"][:N]).view(pkg.BA_OBS32).reshape(-1), raw=o)


def _assert_spec(got, want, positions):
    for k in ("counts", "list_slot", "obs32"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, got["counts"], want["counts"])
    assert got["positions"].tobytes() == np.ascontiguousarray(positions[want["list_slot"]]).tobytes()


def _discrete_world(h, pkg, rows):
    tables, counts, live = V.world(41, 8, sizes=SIZES)
    assert tables[5] is None and sorted(counts) == sorted(SIZES)
    w, xy = _world(h, pkg, rows, tables, counts, live, 41)
    # a slot out of range, handed over in device memory: the table keeps -1 in its place
    k = next(i for i, t in enumerate(tables) if t is not None and len(t) > 100)
    t = tables[k].copy(); t[3] = M.CAPACITY + 3
    w.kfs[k].set_map_point_slots(w.mp, _d(t))
    tables = list(tables); tables[k] = np.where(t >= M.CAPACITY, -1, t).astype(np.int32)
    assert w.kfs[k].get_map_point_slots().tolist() == tables[k].tolist()
    return w, xy, tables, live


def test_collection_equals_spec_host_and_device_twice(gpu_handle, pkg, rows):
    w, xy, tables, live = _discrete_world(gpu_handle, pkg, rows)
    try:
        want = S.collect(tables, xy, live)
        K, F, M_, N = (int(x) for x in want["counts"])
        dead = sum(int(((t >= 0) & (live[np.maximum(t, 0)] == 0)).sum()) for t in tables if t is not None)
        assert K == 7 and F == 1 and M_ > 200 and N > M_ and dead > 10              # points seen more than once, features on dead slots
        before = w.mp.download()
        tabs = [k.get_map_point_slots() for k in w.kfs]
        for _ in range(2):
            _assert_spec(_collect_dev(gpu_handle, pkg, w.mp, w.kfs), want, rows[0])
            host = gpu_handle.map_collect_global(w.mp, w.kfs)
            _assert_spec(host, want, rows[0])
        # the store and the tables are left as found
        assert _same(w.mp.download(), before) and all(np.array_equal(k.get_map_point_slots(), t) for k, t in zip(w.kfs, tabs))
        # one keyframe: the anchor alone (K = 0) still collects
        one = S.collect(tables[:1], xy[:1], live)
        _assert_spec(_collect_dev(gpu_handle, pkg, w.mp, w.kfs[:1]), one, rows[0])
        assert int(one["counts"][0]) == 0
    finally:
        w.close()


def test_refusals(gpu_handle, pkg, rows):
    w, xy, tables, live = _discrete_world(gpu_handle, pkg, rows)
    other = pkg.MapPointStore(gpu_handle, 64)
    stranger = None
    try:
        want = S.collect(tables, xy, live)
        cap, ocap = gpu_handle._global_bounds(w.mp, w.kfs)
        assert ocap == sum(SIZES) and cap == min(ocap, M.CAPACITY)
        before = w.mp.download()
        for kw in (dict(list_cap=cap - 1), dict(obs_cap=ocap - 1)):
            for call in (gpu_handle.map_collect_global_device, gpu_handle.map_collect_global):
                with pytest.raises(pkg.OrbxError) as e:
                    call(w.mp, w.kfs, **kw)
                assert e.value.code == -1 and "bound" in str(e.value)
        for call in (gpu_handle.map_collect_global_device, gpu_handle.map_collect_global, lambda mp, kfs: gpu_handle.map_global_ba(pkg.CameraModel(**G.CAMERA), mp, kfs)):
            with pytest.raises(pkg.OrbxError) as e:
                call(w.mp, [])
            assert e.value.code == -1 and "n_kfs" in str(e.value)
        import torch
        stranger = pkg.KeyFrame(gpu_handle, torch.zeros((4, 7), dtype=torch.float32, device="cuda"), torch.zeros((4, 32), dtype=torch.uint8, device="cuda"), 4)
        stranger.set_map_point_slots(other, np.array([0, 1, -1, 2], np.int32))
        for call in (gpu_handle.map_collect_global_device, gpu_handle.map_collect_global):
            with pytest.raises(pkg.OrbxError) as e:
                call(w.mp, w.kfs + [stranger])
            assert e.value.code == -1 and "another store" in str(e.value)
        assert _same(w.mp.download(), before)
        _assert_spec(_collect_dev(gpu_handle, pkg, w.mp, w.kfs), want, rows[0])        # the next valid call is exact
    finally:
        gpu_handle.synchronize()
        if stranger is not None:
            stranger.close()
        other.close()
        w.close()


def _scene_world(h, pkg, **kw):
    sc = B.ba_scene(**kw)
    st = sc["store"]
    w = _BaWorld(h, pkg, st.positions, st.desc, st.live)
    for t, kp, pose in zip(sc["tables"], sc["kps"], sc["poses_wc"]):
        w.keyframe(t, np.stack([kp["x"], kp["y"]], 1), pose_wc=pose)
    return sc, w


def _solve_bytes(r):
    return (np.asarray(r["poses_wc"]).tobytes(), r["iterations"], struct.pack("<2d", r["initial_error"], r["final_error"]))


def _assert_driver_equals_sequence(h, pkg, cam, sc, w):
    st = sc["store"]
    xy = [np.stack([k["x"], k["y"]], 1) for k in sc["kps"]]
    c = h.map_collect_global(w.mp, w.kfs)
    _assert_spec(c, S.collect(sc["tables"], xy, st.live), st.positions)
    K, F, M_, N = (int(x) for x in c["counts"])
    assert K == len(w.kfs) - 1 and F == 1
    poses_cw = np.array([pkg.se3_inverse(p) for p in sc["poses_wc"][1:]]).reshape(-1, 7)
    fixed_cw = pkg.se3_inverse(sc["poses_wc"][0])
    want = h.ba_solve_global_map_obs32(cam, pkg.GlobalBAConfig(), poses_cw, fixed_cw, c["positions"], c["obs32"])
    r = h.map_global_ba(cam, w.mp, w.kfs)
    assert r["counts"].tobytes() == c["counts"].tobytes()
    assert _solve_bytes(r) == _solve_bytes(want)
    assert r["iterations"] > 0 and r["final_error"] < r["initial_error"]
    # the store: P's positions are the solver's points, as MapPointStore.set would write them; everything else is as it was
    P = c["list_slot"]
    assert w.mp.download(P)[0].tobytes() == want["points"].tobytes()
    pos, desc, lv = w.mp.download()
    rest = np.setdiff1d(np.arange(M.CAPACITY), P)
    assert pos[rest].tobytes() == st.positions[rest].tobytes() and desc.tobytes() == st.desc.tobytes() and lv.tobytes() == st.live.tobytes()
    assert not np.array_equal(pos[P], st.positions[P])
    w.mp.set(P, want["points"])
    assert w.mp.download()[0].tobytes() == pos.tobytes()
    return r, c


def test_map_global_ba_equals_collect_solve_set(gpu_handle, pkg, cam, oracle):
    sc, w = _scene_world(gpu_handle, pkg, seed=300, n_kf=8, n_mp=300)
    try:
        r, c = _assert_driver_equals_sequence(gpu_handle, pkg, cam, sc, w)
        # an all-reduce hook installed: refused, the store untouched
        before = w.mp.download()
        gpu_handle.set_allreduce(lambda ptr, n, stream: None)
        try:
            with pytest.raises(pkg.OrbxError) as e:
                gpu_handle.map_global_ba(cam, w.mp, w.kfs)
            assert e.value.code == -1
        finally:
            gpu_handle.set_allreduce(None)
        assert _same(w.mp.download(), before)
    finally:
        w.close()


def test_an_all_dead_map_is_empty_and_leaves_the_store_untouched(gpu_handle, pkg, cam, rows):
    tables, counts, live = V.world(41, 8, sizes=SIZES)
    dead = np.zeros_like(live)
    dead[np.setdiff1d(np.arange(M.CAPACITY), np.concatenate([t[t >= 0] for t in tables if t is not None]))[:5]] = 1     # live slots that nobody observes
    w, xy = _world(gpu_handle, pkg, rows, tables, counts, dead, 41)
    try:
        before = w.mp.download()
        assert S.collect(tables, xy, dead)["empty"]
        assert gpu_handle.map_collect_global(w.mp, w.kfs) is None
        assert gpu_handle.map_global_ba(cam, w.mp, w.kfs) is None
        assert _same(w.mp.download(), before)
    finally:
        w.close()


def test_the_resident_call_crosses_128_keyframes(gpu_handle, pkg, cam):
    sc, w = _scene_world(gpu_handle, pkg, seed=301, n_kf=140, n_mp=80)
    try:
        assert len(w.kfs) == 140 and 20 <= np.median([k.n for k in w.kfs]) <= 60
        r, c = _assert_driver_equals_sequence(gpu_handle, pkg, cam, sc, w)
        assert int(c["counts"][0]) == 139
    finally:
        w.close()
