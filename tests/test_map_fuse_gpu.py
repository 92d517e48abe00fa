"""Fuse and merge on the resident map on the GPU against tests/map_fuse_spec.py: byte equality everywhere.  The search the
specification is given is the oracle's fuse_search, which the GPU search equals bit for bit (tests/test_fuse_search.py)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import covisibility_spec as CS
import map_fuse_scenes as F
import map_fuse_spec as S
import map_observations_spec as OSP
from test_map_fuse_cpu import build_driver
from test_map_store_gpu import _World, _d, _same
from test_track_cpp import _Reader

pytestmark = pytest.mark.gpu

PASSES = {"out": ([0], F.TGT), "back": ([1, 2, 3, 6, 7, 8], [0]), "one": ([0], [1]), "twice": ([0, 1, 0], [6, 3])}


@pytest.fixture(scope="module")
def scenes():
    return {seed: F.world(seed) for seed in (1, 2)}


@pytest.fixture(scope="module")
def spec(scenes, oracle):
    """every pass's specification, computed once"""
    cache = {}

    def get(seed, name):
        if (seed, name) not in cache:
            sc = scenes[seed]
            src, tgt = PASSES[name]
            cache[(seed, name)] = S.fuse(sc["tables"], sc["live"], sc["positions"], sc["desc"], src, tgt, F.oracle_search(oracle, sc))
        return cache[(seed, name)]
    return get


class _FuseWorld(_World):
    def keyframe(self, table, xy, desc, pose_wc):
        import torch
        n = len(desc)
        kp = F.keypoints(xy, self.pkg.KEYPOINT)
        d_kp = _d(kp.view(np.uint8).reshape(-1, self.pkg.KEYPOINT.itemsize)) if n else torch.zeros((1, 28), dtype=torch.uint8, device="cuda")
        kf = self.pkg.KeyFrame(self.h, d_kp, _d(desc) if n else torch.zeros((1, 32), dtype=torch.uint8, device="cuda"), n, pose_wc=pose_wc)
        if table is not None:
            kf.set_map_point_slots(self.mp, table)
        self.kfs.append(kf)
        return kf


def _world(h, pkg, sc):
    w = _FuseWorld(h, pkg, sc["positions"], sc["desc"], sc["live"], capacity=sc["capacity"])
    for t, xy, d, p in zip(sc["tables"], sc["xy"], sc["descs"], sc["poses"]):
        w.keyframe(t, xy, d, p)
    return w


def _cam(pkg):
    return pkg.CameraModel(**F.CAMERA)


def _device(h, pkg, w, src, tgt):
    import torch
    o = h.map_fuse_device(_cam(pkg), w.mp, w.kfs, src, tgt, F.RADIUS_SCALE)
    torch.cuda.synchronize()
    c = o["counts"].cpu().numpy()
    return dict(counts=c, list_slot=o["list_slot"].cpu().numpy()[:c[0]], match=o["match"].cpu().numpy()[:c[0]], goner=o["goner"].cpu().numpy()[:c[3]],
                keeper=o["keeper"].cpu().numpy()[:c[3]])


KEYS = ("counts", "list_slot", "match", "goner", "keeper")


def _tables(w):
    return [k.get_map_point_slots() for k in w.kfs]


def _as_arrays(tables, counts):
    return [np.full(n, -1, np.int32) if t is None else np.asarray(t, np.int32) for t, n in zip(tables, counts)]


# ---- the device form against the specification ---------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,name", [(1, "out"), (2, "out"), (1, "back"), (1, "one"), (2, "twice")])
def test_device_form_equals_spec(gpu_handle, pkg, scenes, spec, seed, name):
    """out: P = 234 (no multiple of a block), targets of 2100 features, without a table and without features; back: six sources, one
    target; twice: a source listed twice"""
    sc, want = scenes[seed], spec(seed, name)
    src, tgt = PASSES[name]
    w = _world(gpu_handle, pkg, sc)
    try:
        # the search alone, before the pass touches the tables: the rows of the pairs that are not skipped
        pos, desc, _ = w.mp.download(want["list_slot"])
        idx, _ = pkg.KeyFrame.fuse_search(gpu_handle, _cam(pkg), pos, desc, [w.kfs[t] for t in tgt], F.RADIUS_SCALE, 50)
        obs = [OSP.observed_at(t, sc["live"]) for t in sc["tables"]]
        seen = np.array([[int(s) in obs[t] for t in tgt] for s in want["list_slot"]], bool).reshape(len(want["list_slot"]), len(tgt))
        assert np.array_equal(np.where(seen, -1, idx), want["match"]) and seen.sum() == want["skipped"]
        got = _device(gpu_handle, pkg, w, src, tgt)
        for k in KEYS:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, got["counts"], want["counts"])
        new = _as_arrays(want["tables"], sc["tables"].counts)
        for k, (a, b) in enumerate(zip(_tables(w), new)):
            assert a.tobytes() == b.tobytes(), k
        if name == "out":
            assert all(v >= F.REQUIRED[k] for k, v in F.scene_counts(sc, want, tgt).items())
        # the live bytes, positions and descriptors are untouched
        pos, desc, lv = w.mp.download()
        on = sc["live"] == 1
        assert lv.tobytes() == sc["live"].tobytes() and pos[on].tobytes() == sc["positions"][on].tobytes() and desc[on].tobytes() == sc["desc"][on].tobytes()
        assert w.mp.info()["n_live"] == int(sc["live"].sum())
        # what is derived from the tables afterwards equals its specification on the new tables: d_mp_uniq was made again, and the
        # store's first / mark tables were left as found
        n_kf = len(w.kfs)
        wt, best, cnt = gpu_handle.map_covisibility(w.mp, w.kfs, range(n_kf), 4)
        want_w = CS.weights(new, sc["live"], range(n_kf))
        assert wt.tobytes() == want_w.tobytes() and _same((best, cnt), CS.best_rows(want_w, 4))
        slots = np.flatnonzero(sc["live"]).astype(np.int32)[::-1].copy()
        assert _same(gpu_handle.map_observations(w.mp, w.kfs, slots), OSP.observations(new, sc["live"], slots))
        assert OSP.n_observers(new, sc["live"])[want["goner"]].sum() == 0   # no table names a goner
    finally:
        w.close()


def test_host_form_equals_device_form_erases_the_goners_and_repeats(gpu_handle, pkg, scenes, spec):
    sc, want = scenes[1], spec(1, "out")
    w, w2 = _world(gpu_handle, pkg, sc), _world(gpu_handle, pkg, sc)
    try:
        got = gpu_handle.map_fuse(_cam(pkg), w.mp, w.kfs, [0], F.TGT, F.RADIUS_SCALE)
        again = _device(gpu_handle, pkg, w2, [0], F.TGT)                   # a fresh identical world: the same bytes
        for k in KEYS:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes() == again[k].tobytes(), k
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_tables(w), _tables(w2)))
        live = sc["live"].copy(); live[want["goner"]] = 0
        assert w.mp.info()["n_live"] == int(live.sum()) == int(sc["live"].sum()) - int(want["counts"][3])
        assert w.mp.download()[2].tobytes() == live.tobytes() and w2.mp.download()[2].tobytes() == sc["live"].tobytes()
        # nothing to do: counts written and nothing else
        for src, tgt in (([], [1]), ([0], []), ([8], [1])):
            r = gpu_handle.map_fuse(_cam(pkg), w2.mp, w2.kfs, src, tgt, F.RADIUS_SCALE)
            assert r["counts"].tolist()[1:] == [0, 0, 0] and len(r["goner"]) == 0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_tables(w), _tables(w2)))
    finally:
        w.close(); w2.close()


def test_search_in_neighbors_equals_the_composition(gpu_handle, pkg, scenes, oracle):
    sc = scenes[2]
    want = S.search_in_neighbors(sc["tables"], sc["live"], sc["positions"], sc["desc"], 0, F.ALL_NB, F.oracle_search(oracle, sc))
    assert want["b"]["counts"][1] >= 20 and want["b"]["counts"][3] >= 3
    normals = np.random.default_rng(4).normal(size=(sc["capacity"], 3))
    w, w2 = _world(gpu_handle, pkg, sc), _world(gpu_handle, pkg, sc)
    try:
        got = gpu_handle.map_search_in_neighbors(_cam(pkg), w.mp, w.kfs, 0, F.ALL_NB, F.RADIUS_SCALE, F.SCALE_RANGE, slot_normals=normals)
        assert got["counts"].tobytes() == np.stack([want["a"]["counts"], want["b"]["counts"]]).tobytes()
        for p in "ab":
            assert got["goner_" + p].tobytes() == want[p]["goner"].tobytes() and got["keeper_" + p].tobytes() == want[p]["keeper"].tobytes()
        assert got["affected"].dtype == np.int32 and got["affected"].tobytes() == want["affected"].tobytes()
        new = _as_arrays(want["tables"], sc["tables"].counts)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_tables(w), new))
        assert w.mp.download()[2].tobytes() == want["live"].tobytes() and w.mp.info()["n_live"] == int(want["live"].sum())
        # the refresh: orbx_map_refresh_points on the returned list, on a world brought to the same state by the two passes
        gpu_handle.map_fuse(_cam(pkg), w2.mp, w2.kfs, [0], F.ALL_NB, F.RADIUS_SCALE)
        gpu_handle.map_fuse(_cam(pkg), w2.mp, w2.kfs, F.ALL_NB, [0], F.RADIUS_SCALE)
        ref = gpu_handle.map_refresh_points(w2.mp, w2.kfs, got["affected"], F.SCALE_RANGE, normals[got["affected"]])
        for k in ("mp_desc", "normals", "min_distance", "max_distance", "records"):
            assert getattr(got["refresh"], k).tobytes() == getattr(ref, k).tobytes(), k
        spec_r, _ = OSP.refresh(new, want["live"], want["affected"], sc["positions"], sc["desc"], sc["poses"], sc["descs"], F.SCALE_RANGE, normals[want["affected"]])
        assert got["refresh"].mp_desc.tobytes() == spec_r["mp_desc"].tobytes() and got["refresh"].records.tobytes() == spec_r["records"].tobytes()
        assert _same(w.mp.download(), w2.mp.download()) and got["refresh"].num_descriptors_updated > 100
    finally:
        w.close(); w2.close()


def test_refusals_touch_nothing(gpu_handle, pkg, scenes, spec):
    import torch
    sc, want = scenes[1], spec(1, "one")
    w = _world(gpu_handle, pkg, sc)
    other = pkg.MapPointStore(gpu_handle, 64)
    h2 = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), 500, device=0, max_w=752, max_h=480, max_batch=1)
    stranger = foreign = None
    try:
        cam = _cam(pkg)
        before, store = _tables(w), w.mp.download()
        stranger = w.keyframe(np.array([1, 2], np.int32), sc["xy"][1][:2], sc["descs"][1][:2], sc["poses"][0]); w.kfs.pop()
        stranger.set_map_point_slots(other, [1, 2])
        foreign = pkg.KeyFrame(h2, torch.zeros((2, 28), dtype=torch.uint8, device="cuda"), torch.zeros((2, 32), dtype=torch.uint8, device="cuda"), 2)
        bad = []
        for f in (gpu_handle.map_fuse, gpu_handle.map_fuse_device):
            bad += [lambda f=f: f(cam, w.mp, w.kfs, [9], [1], F.RADIUS_SCALE), lambda f=f: f(cam, w.mp, w.kfs, [0], [-1], F.RADIUS_SCALE),
                    lambda f=f: f(cam, w.mp, w.kfs, [0], [1, 2, 1], F.RADIUS_SCALE), lambda f=f: f(cam, w.mp, w.kfs, [0], [1], F.RADIUS_SCALE, 257),
                    lambda f=f: f(cam, w.mp, w.kfs + [stranger], [0], [1], F.RADIUS_SCALE), lambda f=f: f(cam, w.mp, w.kfs + [foreign], [0], [1], F.RADIUS_SCALE),
                    lambda f=f: f(cam, w.mp, w.kfs + [w.kfs[2]], [0], [1], F.RADIUS_SCALE), lambda f=f: f(cam, w.mp, [w.kfs[8]] * 65536, [0], [1], F.RADIUS_SCALE)]
        bad += [lambda: gpu_handle.map_search_in_neighbors(cam, w.mp, w.kfs, 0, [1, 0], F.RADIUS_SCALE, F.SCALE_RANGE),
                lambda: gpu_handle.map_search_in_neighbors(cam, w.mp, w.kfs, 9, [1], F.RADIUS_SCALE, F.SCALE_RANGE),
                lambda: gpu_handle.map_search_in_neighbors(cam, w.mp, w.kfs, 0, [1, 1], F.RADIUS_SCALE, F.SCALE_RANGE)]
        for i, f in enumerate(bad):
            with pytest.raises(pkg.OrbxError) as e:
                f()
            assert e.value.code == -1, i
        # a cap below its bound, raw, with the outputs watched
        L = gpu_handle._L
        arr = (C.c_void_p * 9)(*[k._p for k in w.kfs])
        c_ = cam._c()
        o = [torch.full((n,), 0x5a5a5a5a, dtype=torch.int32, device="cuda") for n in (4, 299, 299, 600, 600)]
        src, tgt = np.array([0], np.int32), np.array([1], np.int32)
        p = lambda t: C.c_void_p(t.data_ptr())
        v = lambda a: a.ctypes.data_as(C.c_void_p)
        torch.cuda.synchronize()
        call = lambda cap: L.orbx_map_fuse_device(gpu_handle._h, C.byref(c_), w.mp._p, C.c_int(9), arr, C.c_int(1), v(src), C.c_int(1), v(tgt), C.c_double(F.RADIUS_SCALE),
                                                  C.c_uint(50), C.c_int(cap), p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]))
        assert call(298) == -1
        torch.cuda.synchronize()
        assert all(bool((t == 0x5a5a5a5a).all()) for t in o)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_tables(w), before)) and _same(w.mp.download(), store)
        # the next valid call is exact
        assert call(299) == 0
        torch.cuda.synchronize()
        P, G = int(want["counts"][0]), int(want["counts"][3])
        assert o[0].cpu().numpy().tobytes() == want["counts"].tobytes() and o[1].cpu().numpy()[:P].tobytes() == want["list_slot"].tobytes()
        assert o[2].cpu().numpy()[:P].tobytes() == want["match"].tobytes() and o[3].cpu().numpy()[:G].tobytes() == want["goner"].tobytes()
        assert o[4].cpu().numpy()[:G].tobytes() == want["keeper"].tobytes()
    finally:
        gpu_handle.synchronize()
        for k in (stranger, foreign):
            if k is not None:
                k.close()
        h2.close()
        other.close()
        w.close()


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------

def test_map_fuse_driver_equals_python_mirror(pkg, scenes, tmp_path):
    tmp = str(tmp_path)
    exe = build_driver(tmp)
    sc = scenes[1]
    ls = np.flatnonzero(sc["live"]).astype(np.int32)
    nb = np.array(F.ALL_NB, np.int32)
    normals = np.random.default_rng(6).normal(size=(sc["capacity"], 3))
    with open(os.path.join(tmp, "map_fuse_in.bin"), "wb") as f:
        f.write(struct.pack("<5i2d", sc["capacity"], len(ls), len(sc["tables"]), 0, len(nb), F.RADIUS_SCALE, F.SCALE_RANGE))
        f.write(ls.tobytes()); f.write(sc["positions"][ls].tobytes()); f.write(sc["desc"][ls].tobytes()); f.write(nb.tobytes()); f.write(normals.tobytes())
        for t, xy, d, pose in zip(sc["tables"], sc["xy"], sc["descs"], sc["poses"]):
            f.write(struct.pack("<ii", len(xy), 0 if t is None else 1))
            f.write((np.full(len(xy), -1, np.int32) if t is None else np.ascontiguousarray(t, np.int32)).tobytes())
            f.write(F.keypoints(xy, pkg.KEYPOINT).tobytes()); f.write(np.ascontiguousarray(d).tobytes()); f.write(np.ascontiguousarray(pose).tobytes())
    r = subprocess.run([exe, tmp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MAP_FUSE_DRIVER_OK" in r.stdout, (r.stdout, r.stderr)
    rd = _Reader(open(os.path.join(tmp, "map_fuse_out.bin"), "rb").read())
    h = pkg.Handle(pkg.CameraModel(**F.CAMERA), 1000, device=0, max_w=752, max_h=480, max_batch=1)
    w, w2 = _world(h, pkg, sc), _world(h, pkg, sc)

    def world_equals(wd):
        for k in wd.kfs:
            assert rd.vec("<i4").tobytes() == k.get_map_point_slots().tobytes()
        _, desc, live = wd.mp.download()
        assert rd.vec("u1").tobytes() == live.tobytes() and rd.vec("u1").tobytes() == desc.tobytes()
    try:
        a = h.map_fuse(_cam(pkg), w.mp, w.kfs, [0], nb, F.RADIUS_SCALE)
        assert rd.vec("<i4").tobytes() == a["counts"].tobytes() and a["counts"][3] > 50
        for k in ("list_slot", "match", "goner", "keeper"):
            assert rd.vec("<i4").tobytes() == a[k].tobytes(), k
        world_equals(w)
        b = h.map_search_in_neighbors(_cam(pkg), w2.mp, w2.kfs, 0, nb, F.RADIUS_SCALE, F.SCALE_RANGE, slot_normals=normals)
        assert rd.vec("<i4").tobytes() == b["counts"].tobytes()
        for k in ("goner_a", "keeper_a", "goner_b", "keeper_b", "affected"):
            assert rd.vec("<i4").tobytes() == b[k].tobytes(), k
        rf = b["refresh"]
        assert rd.vec("u1").tobytes() == rf.mp_desc.tobytes() and rd.vec(("<f8", 3)).tobytes() == rf.normals.tobytes()
        assert rd.vec("<f8").tobytes() == rf.min_distance.tobytes() and rd.vec("<f8").tobytes() == rf.max_distance.tobytes()
        assert rd.vec(pkg.MP_REFRESH_RECORD).tobytes() == rf.records.tobytes()
        assert rd.vec("<i4").tolist() == [len(b["goner_a"]) + len(b["goner_b"]), int(b["counts"][0, 2] + b["counts"][1, 2])]
        world_equals(w2)
        assert rd.pos == len(rd.buf)
    finally:
        w.close(); w2.close()
        h.close()
