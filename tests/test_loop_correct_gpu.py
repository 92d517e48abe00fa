"""The loop correction on the resident map on the GPU against tests/loop_correct_spec.py.

Byte equality: counts, affected bytes, list, goner / keeper, every table and d_mp_uniq (read through the covisibility weights made
from it), every unaffected store row, every unaffected pose.
Numeric: a corrected position or pose translation is s_c (R_c p) + t_c — a chain of about 30 f64 operations, each good to 2^-53
of the magnitude s_c |p| + |t_c|, so the device and numpy differ by some 3e-15 of it; the tolerance is 1e-13 (s_c |p| + |t_c|) per
component, a 30-fold margin for contraction and ordering.  Quaternion components (products of unit quaternions): within 1e-13."""
import numpy as np
import pytest

import covisibility_spec as CS
import loop_correct_scenes as Z
import loop_correct_spec as S
from test_map_store_gpu import _World, _d

pytestmark = pytest.mark.gpu

KEYS = ("counts", "affected", "list_slot", "goner", "keeper")


class _LoopWorld(_World):
    def keyframe(self, table, n, pose_wc):
        import torch
        kf = self.pkg.KeyFrame(self.h, torch.zeros((max(n, 1), 7), dtype=torch.float32, device="cuda"), torch.zeros((max(n, 1), 32), dtype=torch.uint8, device="cuda"), n,
                               pose_wc=pose_wc)
        if table is not None:
            # the host form refuses an entry outside [-1, capacity); the device form stores it as -1: the only way such an entry arrives
            out = np.asarray(table).max(initial=-1) >= self.mp.capacity
            kf.set_map_point_slots(self.mp, _d(np.asarray(table, np.int32)) if out and n else table)
        self.kfs.append(kf)
        return kf


def _world(h, pkg, sc):
    w = _LoopWorld(h, pkg, sc["positions"], sc["desc"], sc["live"], capacity=sc["capacity"])
    for t, n, p in zip(sc["tables"], sc["n"], sc["poses"]):
        w.keyframe(t, n, p)
    return w


def _cfg(pkg, sc):
    return pkg.LoopCorrectConfig(sc["min_weight"], sc["max_depth"])


def _spec(sc):
    return S.correct_loop(sc["tables"], sc["live"], sc["positions"], sc["poses"], sc["parent"], sc["cur"], sc["loop"], sc["sim3"], sc["matches"], sc["min_weight"],
                          sc["max_depth"])


def _device(h, pkg, w, sc):
    import torch
    o = h.map_correct_loop_device(w.mp, w.kfs, sc["parent"], sc["cur"], sc["loop"], sc["sim3"], sc["matches"], _cfg(pkg, sc))
    torch.cuda.synchronize()
    c = o["counts"].cpu().numpy()
    return dict(counts=c, affected=o["affected"].cpu().numpy(), poses_wc=o["poses_wc"].cpu().numpy(), list_slot=o["list_slot"].cpu().numpy()[:c[1]],
                goner=o["goner"].cpu().numpy()[:c[3]], keeper=o["keeper"].cpu().numpy()[:c[3]])


def _tables(w):
    return [k.get_map_point_slots() for k in w.kfs]


def _as_arrays(tables, counts, capacity):
    """the tables as they lie on the device: no table reads as -1 everywhere, an out-of-range entry was stored as -1"""
    return [np.full(n, -1, np.int32) if t is None else np.where(np.asarray(t) >= capacity, -1, t).astype(np.int32) for t, n in zip(tables, counts)]


def _check_numbers(sc, want, got_poses, got_pos):
    """poses and store positions: bytes where nothing is corrected, the docstring's tolerances where something is"""
    aff = want["affected"] == 1
    assert got_poses[~aff].tobytes() == np.asarray(sc["poses"])[~aff].tobytes()
    if aff.any():
        dq = np.abs(got_poses[aff, :4] - want["poses_wc"][aff, :4]).max()
        dt = np.abs(got_poses[aff, 4:] - want["poses_wc"][aff, 4:]).max(axis=1)
        tol = S.tolerance(sc["sim3"], np.asarray(sc["poses"])[aff, 4:])
        print("quaternions within %.2e; translations within %.2e of their tolerance" % (dq, (dt / tol).max()))
        assert dq <= 1e-13 and np.all(dt <= tol)
    moved = np.zeros(len(sc["live"]), bool); moved[want["list_slot"]] = True
    on = sc["live"] == 1
    assert got_pos[on & ~moved].tobytes() == sc["positions"][on & ~moved].tobytes()
    if moved.any():
        dp = np.abs(got_pos[moved] - want["positions"][moved]).max(axis=1)
        tol = S.tolerance(sc["sim3"], sc["positions"][moved])
        print("positions within %.2e of their tolerance" % (dp / tol).max())
        assert np.all(dp <= tol)


def _check_device(h, pkg, sc, want=None, weights=True):
    want = want or _spec(sc)
    w = _world(h, pkg, sc)
    try:
        got = _device(h, pkg, w, sc)
        for k in KEYS:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, got["counts"], want["counts"])
        new = _as_arrays(want["tables"], sc["n"], sc["capacity"])
        for k, (a, b) in enumerate(zip(_tables(w), new)):
            assert a.tobytes() == b.tobytes(), k
        pos, desc, lv = w.mp.download()
        on = sc["live"] == 1
        assert lv.tobytes() == sc["live"].tobytes() and desc[on].tobytes() == sc["desc"][on].tobytes()      # the device form erases nothing
        _check_numbers(sc, want, got["poses_wc"], pos)
        for kf, p in zip(w.kfs, sc["poses"]):                                      # ... and applies no pose
            assert kf.info()["pose_wc"].tobytes() == np.asarray(p, np.float64).tobytes()
        if weights:
            # d_mp_uniq was made again and the store's index / mark tables were left as found: what is derived from the tables
            # afterwards equals its specification on the new tables
            q = list(range(len(w.kfs)))[:16]
            assert h.map_covisibility(w.mp, w.kfs, q)[0].tobytes() == CS.weights(want["tables"], sc["live"], q).tobytes()
        return got
    finally:
        w.close()


# ---- reach -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(Z.REACH))
def test_reach(gpu_handle, pkg, name):
    got = _check_device(gpu_handle, pkg, Z.REACH[name]())
    assert np.flatnonzero(got["affected"]).tolist() == Z.REACH_WANT[name]


@pytest.fixture(scope="module")
def random_specs():
    cache = {}

    def get(N):
        if N not in cache:
            cache[N] = _spec(Z.random_graph(N))
        return cache[N]
    return get


@pytest.mark.parametrize("N", Z.RANDOM_N)
def test_random_graphs_across_wave_and_block_edges(gpu_handle, pkg, random_specs, N):
    want = random_specs(N)
    assert 1 < want["counts"][0] < N and want["counts"][3] > 0
    _check_device(gpu_handle, pkg, Z.random_graph(N), want)


# ---- points and Sim3 ---------------------------------------------------------------------------------------------------------

def test_points_inside_and_outside(gpu_handle, pkg):
    got = _check_device(gpu_handle, pkg, Z.points())
    assert got["list_slot"].tolist() == [0, 1, 2, 4, 3]
    assert _check_device(gpu_handle, pkg, Z.no_points())["counts"].tolist() == [2, 0, 0, 0]


@pytest.mark.parametrize("i,name", list(enumerate(Z.SIM3S)))
def test_sim3_and_orientations(gpu_handle, pkg, i, name):
    poses = Z.orientation_poses()
    _check_device(gpu_handle, pkg, Z.points(Z.SIM3S[name], poses[i % len(poses)]), weights=False)


# ---- fuse --------------------------------------------------------------------------------------------------------------------

def test_fuse_rules(gpu_handle, pkg):
    got = _check_device(gpu_handle, pkg, Z.fuse_scene())
    assert got["counts"].tolist() == [3, 26, 7, 6]
    assert _check_device(gpu_handle, pkg, Z.no_pairs())["counts"].tolist() == [2, 3, 0, 0]
    sc = dict(Z.fuse_scene()); sc["matches"] = np.zeros((0, 2), np.int32)       # zero matches: the fuse launches are not made at all
    assert _check_device(gpu_handle, pkg, sc)["counts"].tolist() == [3, 26, 0, 0]


@pytest.mark.parametrize("seed", [0, 1])
def test_agreement_worlds(gpu_handle, pkg, seed):
    _check_device(gpu_handle, pkg, Z.agree_world(seed))


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_touch_nothing(gpu_handle, pkg):
    h = gpu_handle
    sc = Z.fuse_scene()
    w = _world(h, pkg, sc)
    other = pkg.MapPointStore(h, 64)
    stranger = _LoopWorld(h, pkg, sc["positions"][:64], sc["desc"][:64], np.ones(64, np.uint8), capacity=64)
    stranger.keyframe(np.array([1, 2, 3], np.int32), 3, sc["poses"][0])
    bare = _LoopWorld(h, pkg, sc["positions"], sc["desc"], sc["live"], capacity=sc["capacity"])
    for k, (t, n, p) in enumerate(zip(sc["tables"], sc["n"], sc["poses"])):
        bare.keyframe(None if k == 1 else t, n, p)
    try:
        before = (_tables(w), w.mp.download())
        K = len(w.kfs)
        ok = dict(mp=w.mp, kfs=w.kfs, parent=sc["parent"], cur=0, loop=1, sim3=sc["sim3"], m=sc["matches"], cfg=_cfg(pkg, sc))

        def call(form, **kw):
            a = dict(ok); a.update(kw)
            return getattr(h, form)(a["mp"], a["kfs"], a["parent"], a["cur"], a["loop"], a["sim3"], a["m"], a["cfg"])

        def par(k, v):
            p = sc["parent"].copy(); p[k] = v
            return p
        s3 = lambda i, v: np.concatenate([sc["sim3"][:i], [v], sc["sim3"][i + 1:]])
        bad = [dict(cur=-1), dict(cur=K), dict(loop=K), dict(loop=-1), dict(loop=-2), dict(cur=1), dict(parent=par(2, K)), dict(parent=par(2, -2)), dict(parent=par(3, 3)),
               dict(kfs=w.kfs + [w.kfs[2]], parent=np.append(sc["parent"], -1)), dict(kfs=w.kfs[:3] + stranger.kfs, parent=sc["parent"]), dict(mp=other),
               dict(sim3=s3(7, 0.0)), dict(sim3=s3(7, -1.0)), dict(sim3=s3(7, np.inf)), dict(sim3=s3(7, np.nan)),
               dict(cfg=pkg.LoopCorrectConfig(-1, 100)), dict(cfg=pkg.LoopCorrectConfig(15, -1))]
        for form in ("map_correct_loop_device", "map_correct_loop"):
            for kw in bad:
                with pytest.raises(pkg.OrbxError) as e:
                    call(form, **kw)
                assert e.value.code == pkg.api.ORBX_ERR_INVALID, (form, kw)
        # a match outside its keyframe: refused by the host form; no pair to the device form (below)
        out = sc["matches"].copy(); out[4] = (sc["n"][0], 0)
        with pytest.raises(pkg.OrbxError):
            call("map_correct_loop", m=out)
        out[4] = (0, -1)
        with pytest.raises(pkg.OrbxError):
            call("map_correct_loop", m=out)
        # cur or loop without a table while there are matches; list_cap below its bound; n_matches < 0; too many keyframes
        with pytest.raises(pkg.OrbxError):
            h.map_correct_loop(bare.mp, bare.kfs, sc["parent"], 0, 1, sc["sim3"], sc["matches"], _cfg(pkg, sc))
        import ctypes as C
        from orb_slam3_rust_amd.api import _vp
        c = _cfg(pkg, sc)._c()
        o = h._loop_host_outputs(K, len(sc["matches"]), sum(sc["n"]))
        fm = np.ascontiguousarray(sc["matches"], np.int32)
        par_, s3_ = np.ascontiguousarray(sc["parent"], np.int32), np.ascontiguousarray(sc["sim3"], np.float64)

        def raw(n_kfs, n_matches, list_cap):
            return h._L.orbx_map_correct_loop(h._h, C.byref(c), w.mp._p, C.c_int(n_kfs), h._kf_array(w.kfs), _vp(par_), C.c_int(0), C.c_int(1), _vp(s3_), C.c_int(n_matches), _vp(fm),
                                              C.c_int(list_cap), _vp(o["counts"]), _vp(o["affected"]), _vp(o["poses_wc"]), _vp(o["list_slot"]), _vp(o["goner"]), _vp(o["keeper"]))
        bound = min(sum(sc["n"]), sc["capacity"])
        assert raw(K, len(fm), bound - 1) == raw(K, -1, bound) == raw(h._L.orbx_map_loop_max_keyframes() + 1, len(fm), bound) == pkg.api.ORBX_ERR_INVALID
        assert raw(0, 0, 0) == 0                                                 # n_kfs = 0: ORBX_OK, nothing done
        after = (_tables(w), w.mp.download())
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before[0], after[0])) and all(a.tobytes() == b.tobytes() for a, b in zip(before[1], after[1]))
        assert all(kf.info()["pose_wc"].tobytes() == np.asarray(p).tobytes() for kf, p in zip(w.kfs, sc["poses"]))
        # the world still answers as a fresh one does; the device form reads an out-of-range match as no pair
        want = _spec(sc)
        sc2 = dict(sc); sc2["matches"] = sc["matches"].copy(); sc2["matches"][4] = (sc["n"][0], 0)
        assert _device(h, pkg, w, sc)["counts"].tolist() == want["counts"].tolist()
        assert _check_device(h, pkg, sc2)["counts"][2] == want["counts"][2] - 1
    finally:
        w.close(); stranger.close(); bare.close(); other.close()


# ---- the same bytes, and the host form -----------------------------------------------------------------------------------------

def test_two_runs_give_the_same_bytes(gpu_handle, pkg, random_specs):
    sc = Z.random_graph(130)
    w1, w2 = _world(gpu_handle, pkg, sc), _world(gpu_handle, pkg, sc)
    try:
        a, b = _device(gpu_handle, pkg, w1, sc), _device(gpu_handle, pkg, w2, sc)
        assert all(a[k].tobytes() == b[k].tobytes() for k in KEYS + ("poses_wc",))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(_tables(w1), _tables(w2)))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(w1.mp.download(), w2.mp.download()))
    finally:
        w1.close(); w2.close()


@pytest.mark.parametrize("scene", ["fuse", "random65"])
def test_host_form_equals_device_form_with_the_download_done_by_hand(gpu_handle, pkg, scene):
    h = gpu_handle
    sc = Z.fuse_scene() if scene == "fuse" else Z.random_graph(65)
    w1, w2 = _world(h, pkg, sc), _world(h, pkg, sc)
    try:
        got = h.map_correct_loop(w1.mp, w1.kfs, sc["parent"], sc["cur"], sc["loop"], sc["sim3"], sc["matches"], _cfg(pkg, sc))
        dev = _device(h, pkg, w2, sc)
        assert all(got[k].dtype == dev[k].dtype and got[k].tobytes() == dev[k].tobytes() for k in KEYS + ("poses_wc",))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(_tables(w1), _tables(w2)))
        # by hand: the poses of A applied, the goners erased
        for kf, a, p in zip(w2.kfs, dev["affected"], dev["poses_wc"]):
            if a:
                kf.set_pose(p)
        if len(dev["goner"]):
            w2.mp.erase(dev["goner"])
        assert all(x.info()["pose_wc"].tobytes() == y.info()["pose_wc"].tobytes() for x, y in zip(w1.kfs, w2.kfs))
        assert any(x.info()["pose_wc"].tobytes() != np.asarray(p).tobytes() for x, p in zip(w1.kfs, sc["poses"]))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(w1.mp.download(), w2.mp.download()))
        live = sc["live"].copy(); live[dev["goner"]] = 0
        assert w1.mp.download()[2].tobytes() == live.tobytes() and w1.mp.info()["n_live"] == int(live.sum()) == int(sc["live"].sum()) - int(dev["counts"][3]) < int(sc["live"].sum())
    finally:
        w1.close(); w2.close()


# ---- one session -----------------------------------------------------------------------------------------------------------------

def _session_world(h, pkg, sc):
    import torch
    w = _World(h, pkg, sc["positions"], sc["desc"], sc["live"], capacity=sc["capacity"])
    for d, t in zip(sc["kfs"], sc["tables"]):
        n = len(t)
        kf = pkg.KeyFrame(h, _d(np.ascontiguousarray(d["kp"]).view(np.uint8).reshape(n, 28)), _d(d["desc"]), n, _d(d["points_cam"]), _d(d["has_point"]), pose_wc=d["pose_wc"])
        kf.set_map_point_slots(w.mp, t)
        w.kfs.append(kf)
    return w


def test_session_verify_then_close_loop_equals_correct_loop_then_global_ba(gpu_handle, pkg):
    """twelve keyframes of 200 features on a circle with drift: the loop verified on the resident keyframes, then closed in one call —
    against the sequence a caller could already make of the parts"""
    h = gpu_handle
    sc = Z.session()
    cam = pkg.CameraModel(**Z.CAMERA)
    w1, w2 = _session_world(h, pkg, sc), _session_world(h, pkg, sc)
    try:
        v = pkg.KeyFrame.verify_loop_candidates(h, cam, [w1.kfs[11]], [w1.kfs[0]])[0]
        assert v["status"] == pkg.LOOP_OK and len(v["feature_matches"]) >= 100
        args = (sc["parent"], 11, 0, v["sim3"], v["feature_matches"])
        one = h.map_close_loop(cam, w1.mp, w1.kfs, *args)
        two = h.map_correct_loop(w2.mp, w2.kfs, *args)
        ba = h.map_global_ba(cam, w2.mp, w2.kfs)
        want = S.correct_loop(sc["tables"], sc["live"], sc["positions"], sc["poses"], sc["parent"], 11, 0, v["sim3"], v["feature_matches"])
        assert all(one[k].tobytes() == two[k].tobytes() == want[k].tobytes() for k in KEYS) and one["poses_wc"].tobytes() == two["poses_wc"].tobytes()
        assert one["counts"][3] >= 100 and one["counts"][0] > 1
        assert all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(_tables(w1), _tables(w2), want["tables"]))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(w1.mp.download(), w2.mp.download()))
        assert all(x.info()["pose_wc"].tobytes() == y.info()["pose_wc"].tobytes() for x, y in zip(w1.kfs, w2.kfs))
        g = one["global_ba"]
        assert g is not None and ba is not None and g["poses_wc"].tobytes() == ba["poses_wc"].tobytes() and g["counts"].tobytes() == ba["counts"].tobytes()
        assert (g["iterations"], g["initial_error"], g["final_error"]) == (ba["iterations"], ba["initial_error"], ba["final_error"])
        assert g["iterations"] > 0 and g["final_error"] < g["initial_error"]
        # without the global BA the call is map_correct_loop
        w3 = _session_world(h, pkg, sc)
        try:
            three = h.map_close_loop(cam, w3.mp, w3.kfs, *args, global_ba=False)
            assert three["global_ba"] is None and all(three[k].tobytes() == two[k].tobytes() for k in KEYS)
        finally:
            w3.close()
    finally:
        w1.close(); w2.close()
