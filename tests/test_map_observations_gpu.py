"""The observation calls on the resident map on the GPU against tests/map_observations_spec.py: byte equality everywhere.  The lists
and the redundancy equal the numpy spec; map_refresh_points equals, output for output, KeyFrame.refresh_map_points fed the spec's
lists and the store's rows (composition: the new call adds no arithmetic), and leaves its descriptors in the store."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import covisibility_scenes as V
import map_observations_scenes as OS
import map_observations_spec as S
import map_store_scenes as M
from test_map_observations_cpu import build_driver
from test_map_store_gpu import _World, _d, _same, _select
from test_track_cpp import _Reader

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows():
    return M.random_rows(9)


class _ObsWorld(_World):
    """_World whose keyframes carry descriptors and a pose"""

    def keyframe(self, table, desc, pose_wc):
        import torch
        n = len(desc)
        kf = self.pkg.KeyFrame(self.h, torch.zeros((max(n, 1), 7), dtype=torch.float32, device="cuda"),
                               _d(desc) if n else torch.zeros((1, 32), dtype=torch.uint8, device="cuda"), n, pose_wc=pose_wc)
        if table is not None:
            kf.set_map_point_slots(self.mp, table)
        self.kfs.append(kf)
        return kf


def _world(h, pkg, rows, tables, counts, live, seed, capacity=M.CAPACITY):
    descs, poses = OS.keyframe_rows(seed, counts)
    w = _ObsWorld(h, pkg, rows[0][:capacity], rows[1][:capacity], live, capacity=capacity)
    for t, d, p in zip(tables, descs, poses):
        w.keyframe(t, d, p)
    w.descs, w.poses = descs, poses
    return w


def _lists(h, w, slots):
    """the device form's lists as numpy, cut to their sizes"""
    import torch
    o = h.map_observations_device(w.mp, w.kfs, slots)
    torch.cuda.synchronize()
    start = o["obs_start"].cpu().numpy()
    N = int(start[-1])
    return start, o["obs_kf"].cpu().numpy()[:N], o["obs_feat"].cpu().numpy()[:N]


def _refresh_device(h, pkg, w, slots, normals):
    import torch
    nr = _d(np.array(normals, np.float64))
    o = h.map_refresh_points_device(w.mp, w.kfs, slots, OS.SCALE_RANGE, nr)
    torch.cuda.synchronize()
    return (o["mp_desc"].cpu().numpy(), nr.cpu().numpy(), o["min_distance"].cpu().numpy(), o["max_distance"].cpu().numpy(),
            o["records"].cpu().numpy().view(pkg.MP_REFRESH_RECORD).reshape(-1))


def _existing_refresh(h, pkg, w, tables, live, slots, desc_rows, normals):
    """KeyFrame.refresh_map_points fed the specification's lists and the store's rows"""
    start, kf, feat = S.observations(tables, live, slots)
    r = pkg.KeyFrame.refresh_map_points(h, w.kfs, w.positions[slots], start, kf, feat, OS.SCALE_RANGE, desc_rows[slots], normals)
    return (r.mp_desc, r.normals, r.min_distance, r.max_distance, r.records)


def _redundancy(h, w, cand, min_obs, threshold):
    import torch
    o = h.map_keyframe_redundancy_device(w.mp, w.kfs, cand, min_obs, threshold)
    torch.cuda.synchronize()
    return o["total"].cpu().numpy(), o["redundant"].cpu().numpy(), o["cull"].cpu().numpy()


def _normals(seed, n):
    v = np.random.default_rng(seed + 50).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _slot_sets(seed, live, lonely):
    ls = np.random.default_rng(seed).permutation(np.flatnonzero(live)).astype(np.int32)
    return [ls, ls[:1], np.array([lonely], np.int32)]


# ---- the lists against the specification ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kfs,capacity", [(n, M.CAPACITY) for n in V.N_KFS] + [(11, 1000)])
def test_lists_equal_spec(gpu_handle, pkg, rows, n_kfs, capacity):
    """feature counts from {0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025}; slots shuffled: all live slots, one slot, a live slot
    nobody observes"""
    seed = 40 + n_kfs + capacity
    tables, counts, live = V.world(seed, n_kfs, capacity=capacity)
    live, lonely = OS.with_unobserved(tables, live)
    w = _world(gpu_handle, pkg, rows, tables, counts, live, seed, capacity=capacity)
    try:
        for slots in _slot_sets(seed, live, lonely):
            want = S.observations(tables, live, slots)
            got = _lists(gpu_handle, w, slots)
            assert _same(got, want), (len(slots), got[0][-1], want[0][-1])
        assert want[0].tolist() == [0, 0]                                   # the lonely slot: live, and observed by nobody
        few = np.diff(_lists(gpu_handle, w, _slot_sets(seed, live, lonely)[0])[0]) < 3
        assert few.tolist() == (S.n_observers(tables, live)[_slot_sets(seed, live, lonely)[0]] < 3).tolist()       # map-point culling's observation test
        if n_kfs >= 11:
            assert set(counts) == set(V.SIZES) and any(t is None for t in tables)
    finally:
        w.close()


def test_rising_world_lists_refresh_and_redundancy(gpu_handle, pkg, rows):
    """row_world("rising", 258): slot j < 257 has 258 - j observers, the slots behind them one — every length from 1 to 258: the
    ranking's 64 / 65 edge, the refresh kernels' 64 / 65 and 256 / 257, min_observations at 3 / 4 / 5"""
    tables, counts, live = V.row_world("rising", 258)
    w = _world(gpu_handle, pkg, rows, tables, counts, live, 258)
    try:
        _rising_checks(gpu_handle, pkg, rows, w, tables, live)
    finally:
        w.close()


def _rising_checks(gpu_handle, pkg, rows, w, tables, live):
    rng = np.random.default_rng(3)
    slots = rng.permutation(np.concatenate([np.arange(800), 800 + rng.permutation(M.CAPACITY - 800)[:1700]])).astype(np.int32)        # three chunks of the scan
    want = S.observations(tables, live, slots)
    assert set(np.diff(want[0]).tolist()) == set(range(0, 259))
    assert _same(_lists(gpu_handle, w, slots), want)
    # the refresh: every output equals the existing call's on those lists
    nr = _normals(1, len(slots))
    ref = _existing_refresh(gpu_handle, pkg, w, tables, live, slots, rows[1], nr)
    got = _refresh_device(gpu_handle, pkg, w, slots, nr)
    assert _same(got, ref)
    assert set(got[4]["n_observers"].tolist()) >= set(range(0, 259)) and (got[4]["chosen"] >= 0).sum() == (np.diff(want[0]) > 0).sum()
    spec, _ = S.refresh(tables, live, slots, rows[0], rows[1], w.poses, w.descs, OS.SCALE_RANGE, nr)
    assert got[0].tobytes() == spec["mp_desc"].tobytes() and got[4].tobytes() == spec["records"].tobytes()
    pos, desc, lv = w.mp.download()
    assert desc[slots].tobytes() == got[0].tobytes() and pos.tobytes() == rows[0].tobytes() and lv.tobytes() == live.tobytes()
    rest = np.setdiff1d(np.arange(M.CAPACITY), slots)
    assert desc[rest].tobytes() == rows[1][rest].tobytes()
    # the redundancy: every keyframe a candidate
    cand = np.arange(258, dtype=np.int32)
    for min_obs, thr in ((0, 0.5), (3, 0.5), (3, 0.9), (257, 0.5)):
        want_r = S.redundancy(tables, live, cand, min_obs, thr)
        assert _same(_redundancy(gpu_handle, w, cand, min_obs, thr), want_r), (min_obs, thr)
    assert 0 < S.redundancy(tables, live, cand, 3, 0.9)[2].sum() < 258


# ---- the refresh against the existing call ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kfs,capacity", [(11, 1000), (65, M.CAPACITY)])
def test_refresh_equals_the_existing_call(gpu_handle, pkg, rows, n_kfs, capacity):
    seed = 60 + n_kfs
    tables, counts, live = V.world(seed, n_kfs, capacity=capacity)
    live, lonely = OS.with_unobserved(tables, live)
    w = _world(gpu_handle, pkg, rows, tables, counts, live, seed, capacity=capacity)
    try:
        desc_now = rows[1][:capacity].copy()
        for i, slots in enumerate(_slot_sets(seed, live, lonely)):
            nr = _normals(seed + i, len(slots))
            ref = _existing_refresh(gpu_handle, pkg, w, tables, live, slots, desc_now, nr)
            got = _refresh_device(gpu_handle, pkg, w, slots, nr)
            assert _same(got, ref), i
            desc_now[slots] = got[0]
            pos, desc, lv = w.mp.download()
            assert desc[live == 1].tobytes() == desc_now[live == 1].tobytes() and pos[live == 1].tobytes() == rows[0][:capacity][live == 1].tobytes()
            assert lv.tobytes() == live.tobytes() and w.mp.download(slots)[1].tobytes() == got[0].tobytes()
            # the host form, and the call again: the same bytes
            host = gpu_handle.map_refresh_points(w.mp, w.kfs, slots, OS.SCALE_RANGE, nr)
            assert _same((host.mp_desc, host.normals, host.min_distance, host.max_distance, host.records), got), i
            assert _same(_refresh_device(gpu_handle, pkg, w, slots, nr), got), i
        assert got[4]["chosen"].tolist() == [-1] and got[0].tobytes() == rows[1][lonely].tobytes() and got[2][0] == np.inf        # the lonely slot keeps its descriptor
        assert len(gpu_handle.map_refresh_points(w.mp, w.kfs, [], OS.SCALE_RANGE, np.zeros((0, 3))).records) == 0
    finally:
        w.close()


# ---- the redundancy against the specification -------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kfs,capacity", [(n, M.CAPACITY) for n in V.N_KFS] + [(11, 1000)])
def test_redundancy_equals_spec(gpu_handle, pkg, rows, n_kfs, capacity):
    """candidates: every keyframe in shuffled order — one without a table and one without features among them where the world has
    them — and one index twice"""
    seed = 80 + n_kfs + capacity
    tables, counts, live = V.world(seed, n_kfs, capacity=capacity)
    w = _world(gpu_handle, pkg, rows, tables, counts, live, seed, capacity=capacity)
    try:
        cand = np.random.default_rng(seed).permutation(n_kfs).astype(np.int32)
        cand = np.concatenate([cand, cand[:1]])
        if n_kfs >= 11:
            assert any(tables[c] is None for c in cand) and any(counts[c] == 0 for c in cand)
        for min_obs in (0, 3):
            for thr in (0.5, 0.9):
                want = S.redundancy(tables, live, cand, min_obs, thr)
                assert _same(_redundancy(gpu_handle, w, cand, min_obs, thr), want), (min_obs, thr)
                assert _same(gpu_handle.map_keyframe_redundancy(w.mp, w.kfs, cand, min_obs, thr), want), (min_obs, thr)
        assert _same(_redundancy(gpu_handle, w, cand[:1], 3, 0.9), S.redundancy(tables, live, cand[:1], 3, 0.9))
        assert all(len(x) == 0 for x in gpu_handle.map_keyframe_redundancy(w.mp, w.kfs, [], 3, 0.9))
    finally:
        w.close()


def test_a_ratio_at_the_threshold_is_not_culled_and_one_feature_above_it_is(gpu_handle, pkg, rows):
    tables, counts, live, want = OS.ratio_world()
    w = _world(gpu_handle, pkg, rows, tables, counts, live, 7)
    try:
        cand = [3, 4, 5, 6, 0]
        for thr, cull in ((0.5, [0, 1, 1, 1, 0]), (0.9, [0, 0, 0, 1, 0])):
            got = _redundancy(gpu_handle, w, cand, 3, thr)
            assert _same(got, S.redundancy(tables, live, cand, 3, thr))
            assert got[2].tolist() == cull and [(int(t), int(r)) for t, r in zip(got[0][:4], got[1][:4])] == [want[k] for k in (3, 4, 5, 6)]
    finally:
        w.close()


# ---- the tables are left as found --------------------------------------------------------------------------------------------

def test_calls_leave_the_tables_as_found_and_repeat_themselves(gpu_handle, pkg, rows):
    import torch
    tables, counts, live = V.world(31, 11)
    w = _world(gpu_handle, pkg, rows, tables, counts, live, 31)
    try:
        with_table = [k for k in w.kfs if k is not w.kfs[5]]
        slots = np.random.default_rng(1).permutation(np.flatnonzero(live)).astype(np.int32)
        nr = _normals(2, len(slots))

        def others():
            sel = _select(gpu_handle, w.mp, keyframes=[with_table, w.kfs[:3]])
            cov = gpu_handle.map_covisibility(w.mp, w.kfs, range(11), 5)
            ba = gpu_handle.map_collect_ba_window_device(w.mp, w.kfs, 2, 4)
            torch.cuda.synchronize()
            n = [int(x) for x in ba["counts"].cpu().numpy()]
            return list(sel) + list(cov) + [ba["counts"].cpu().numpy(), ba["local_kf"].cpu().numpy(), ba["fixed_kf"].cpu().numpy()[:n[1] - 1],
                                           ba["list_slot"].cpu().numpy()[:n[2]], ba["obs32"].cpu().numpy()[:n[3]]]

        before = others()
        calls = [lambda: _lists(gpu_handle, w, slots), lambda: _redundancy(gpu_handle, w, np.arange(11), 3, 0.5), lambda: _refresh_device(gpu_handle, pkg, w, slots, nr)]
        for i, f in enumerate(calls):
            a = f()
            after = others()
            if i == 2:                                                      # the refresh changes the store's descriptors, and so the rows a selection gathers
                assert not _same(after[3:4], before[3:4])
                after[3] = before[3]
            assert _same(after, before), i
            assert _same(f(), a), i
        assert _same(_lists(gpu_handle, w, slots[:7]), S.observations(tables, live, slots[:7]))       # another call sees no trace of them
    finally:
        w.close()


# ---- host form, refusals ----------------------------------------------------------------------------------------------------

def test_host_form_equals_device_form_and_refusals_touch_nothing(gpu_handle, pkg, rows):
    import torch
    tables, counts, live = V.world(31, 11)
    w = _world(gpu_handle, pkg, rows, tables, counts, live, 31)
    other = pkg.MapPointStore(gpu_handle, 64)
    h2 = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), 500, device=0, max_w=752, max_h=480, max_batch=1)
    stranger = foreign = None
    try:
        slots = np.random.default_rng(1).permutation(np.flatnonzero(live)).astype(np.int32)
        assert _same(gpu_handle.map_observations(w.mp, w.kfs, slots), _lists(gpu_handle, w, slots))
        assert _same(gpu_handle.map_observations(w.mp, w.kfs, []), (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)))
        assert _same(gpu_handle.map_observations(w.mp, [], slots[:3]), (np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)))
        before = w.mp.download()
        stranger = w.keyframe(np.array([1, 2], np.int32), np.zeros((2, 32), np.uint8), w.poses[0]); w.kfs.pop()
        stranger.set_map_point_slots(other, [1, 2])
        foreign = pkg.KeyFrame(h2, torch.zeros((2, 7), dtype=torch.float32, device="cuda"), torch.zeros((2, 32), dtype=torch.uint8, device="cuda"), 2)
        dead = int(np.flatnonzero(live == 0)[0])
        bad_slots = [np.array([slots[0], M.CAPACITY], np.int32), np.array([slots[0], -1], np.int32), np.array([slots[0], slots[1], slots[0]], np.int32),
                     np.array([slots[0], dead], np.int32)]
        nr3 = np.zeros((3, 3))
        bad = [lambda s=s: gpu_handle.map_observations_device(w.mp, w.kfs, s) for s in bad_slots]
        bad += [lambda s=s: gpu_handle.map_observations(w.mp, w.kfs, s) for s in bad_slots]
        bad += [lambda s=s: gpu_handle.map_refresh_points(w.mp, w.kfs, s, OS.SCALE_RANGE, nr3[:len(s)]) for s in bad_slots]
        bad += [lambda s=s: gpu_handle.map_refresh_points_device(w.mp, w.kfs, s, OS.SCALE_RANGE, _d(nr3[:len(s)])) for s in bad_slots]
        for kfs in (w.kfs + [stranger], w.kfs + [foreign], [w.kfs[0]] * 65536):
            bad += [lambda k=kfs: gpu_handle.map_observations_device(w.mp, k, slots[:3]), lambda k=kfs: gpu_handle.map_observations(w.mp, k, slots[:3]),
                    lambda k=kfs: gpu_handle.map_refresh_points(w.mp, k, slots[:3], OS.SCALE_RANGE, nr3),
                    lambda k=kfs: gpu_handle.map_refresh_points_device(w.mp, k, slots[:3], OS.SCALE_RANGE, _d(nr3)),
                    lambda k=kfs: gpu_handle.map_keyframe_redundancy(w.mp, k, [0], 3, 0.9), lambda k=kfs: gpu_handle.map_keyframe_redundancy_device(w.mp, k, [0], 3, 0.9)]
        bad += [lambda: gpu_handle.map_keyframe_redundancy(w.mp, w.kfs, [11], 3, 0.9), lambda: gpu_handle.map_keyframe_redundancy(w.mp, w.kfs, [-1], 3, 0.9),
                lambda: gpu_handle.map_keyframe_redundancy(w.mp, w.kfs, [0], -1, 0.9), lambda: gpu_handle.map_keyframe_redundancy_device(w.mp, w.kfs, [11], 3, 0.9),
                lambda: gpu_handle.map_keyframe_redundancy_device(w.mp, w.kfs, [0], -1, 0.9), lambda: gpu_handle.map_keyframe_redundancy(w.mp, [], [0], 3, 0.9)]
        for i, f in enumerate(bad):
            with pytest.raises(pkg.OrbxError) as e:
                f()
            assert e.value.code == -1, i
        # raw calls whose outputs are watched: a refusal writes nothing
        L = gpu_handle._L
        arr = (C.c_void_p * 11)(*[k._p for k in w.kfs])
        cap = sum(counts)
        p = lambda t: C.c_void_p(t.data_ptr())
        v = lambda a: a.ctypes.data_as(C.c_void_p)
        o = [torch.full((n,), 0x5a5a5a5a, dtype=torch.int32, device="cuda") for n in (4, cap, cap)]
        ho = [np.full(n, 7, np.int32) for n in (4, cap, cap)]
        s3 = np.ascontiguousarray(slots[:3])
        torch.cuda.synchronize()
        twice = np.array([slots[0], slots[0], slots[1]], np.int32)
        assert L.orbx_map_observations_device(gpu_handle._h, w.mp._p, C.c_int(11), arr, C.c_int(3), v(s3), C.c_int(cap - 1), p(o[0]), p(o[1]), p(o[2])) == -1
        assert L.orbx_map_observations_device(gpu_handle._h, w.mp._p, C.c_int(11), arr, C.c_int(3), v(twice), C.c_int(cap), p(o[0]), p(o[1]), p(o[2])) == -1
        assert L.orbx_map_observations(gpu_handle._h, w.mp._p, C.c_int(11), arr, C.c_int(3), v(s3), C.c_int(cap - 1), v(ho[0]), v(ho[1]), v(ho[2])) == -1
        assert L.orbx_map_observations(gpu_handle._h, w.mp._p, C.c_int(11), arr, C.c_int(3), v(twice), C.c_int(cap), v(ho[0]), v(ho[1]), v(ho[2])) == -1
        r = [torch.full((3,), 0x5a5a5a5a, dtype=torch.int32, device="cuda"), torch.full((3,), 0x5a5a5a5a, dtype=torch.int32, device="cuda"),
             torch.full((3,), 0x5a, dtype=torch.uint8, device="cuda")]
        c_bad = np.array([0, 11, 1], np.int32)
        assert L.orbx_map_keyframe_redundancy_device(gpu_handle._h, w.mp._p, C.c_int(11), arr, C.c_int(3), v(c_bad), C.c_int(3), C.c_double(0.9), p(r[0]), p(r[1]),
                                                     p(r[2])) == -1
        md = torch.full((3, 32), 0x5a, dtype=torch.uint8, device="cuda"); nrm = torch.full((3, 3), 7.0, dtype=torch.float64, device="cuda")
        mn = torch.full((3,), 7.0, dtype=torch.float64, device="cuda"); mx = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
        rec = torch.full((3, 16), 0x5a, dtype=torch.uint8, device="cuda")
        assert L.orbx_map_refresh_points_device(gpu_handle._h, w.mp._p, C.c_int(11), arr, C.c_int(3), v(twice), C.c_double(OS.SCALE_RANGE), p(md), p(nrm), p(mn), p(mx),
                                                p(rec)) == -1
        torch.cuda.synchronize()
        assert all(bool((t == 0x5a5a5a5a).all()) for t in o + r[:2]) and bool((r[2] == 0x5a).all()) and all((a == 7).all() for a in ho)
        assert bool((md == 0x5a).all()) and bool((rec == 0x5a).all()) and all(bool((t == 7.0).all()) for t in (nrm, mn, mx))
        assert _same(w.mp.download(), before)
        # the next valid calls are exact
        assert L.orbx_map_observations_device(gpu_handle._h, w.mp._p, C.c_int(11), arr, C.c_int(3), v(s3), C.c_int(cap), p(o[0]), p(o[1]), p(o[2])) == 0
        torch.cuda.synchronize()
        want = S.observations(tables, live, s3)
        assert o[0].cpu().numpy().tobytes() == want[0].tobytes() and o[1].cpu().numpy()[:want[0][-1]].tobytes() == want[1].tobytes()
        assert _same(_redundancy(gpu_handle, w, [0, 10, 1], 3, 0.9), S.redundancy(tables, live, [0, 10, 1], 3, 0.9))
    finally:
        gpu_handle.synchronize()
        for k in (stranger, foreign):
            if k is not None:
                k.close()
        h2.close()
        other.close()
        w.close()


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------

def test_map_observations_driver_equals_python_mirror(pkg, rows, tmp_path):
    tmp = str(tmp_path)
    exe = build_driver(tmp)
    tables, counts, live = V.world(31, 11)
    descs, poses = OS.keyframe_rows(31, counts)
    ls = np.flatnonzero(live).astype(np.int32)
    ask = np.random.default_rng(5).permutation(ls).astype(np.int32)
    nr = _normals(5, len(ask))
    cand = np.array([0, 5, 10, 3, 3], np.int32)
    with open(os.path.join(tmp, "map_obs_in.bin"), "wb") as f:
        f.write(struct.pack("<6i2d", M.CAPACITY, len(ls), 11, len(ask), len(cand), 3, 0.5, OS.SCALE_RANGE))
        f.write(ls.tobytes()); f.write(rows[0][ls].tobytes()); f.write(rows[1][ls].tobytes()); f.write(ask.tobytes()); f.write(nr.tobytes()); f.write(cand.tobytes())
        for t, n, d, pose in zip(tables, counts, descs, poses):
            f.write(struct.pack("<ii", n, 0 if t is None else 1))
            f.write((np.full(n, -1, np.int32) if t is None else np.ascontiguousarray(t, np.int32)).tobytes()); f.write(d.tobytes()); f.write(pose.tobytes())
    r = subprocess.run([exe, tmp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MAP_OBSERVATIONS_DRIVER_OK" in r.stdout, (r.stdout, r.stderr)
    rd = _Reader(open(os.path.join(tmp, "map_obs_out.bin"), "rb").read())
    h = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), 1000, device=0, max_w=752, max_h=480, max_batch=1)
    w = _world(h, pkg, rows, tables, counts, live, 31)
    try:
        start, kf, feat = h.map_observations(w.mp, w.kfs, ask)
        assert rd.vec("<i4").tobytes() == start.tobytes() and rd.vec("<i4").tobytes() == kf.tobytes() and rd.vec("<i4").tobytes() == feat.tobytes()
        assert rd.vec("u1").tolist() == (np.diff(start) < 3).astype(np.uint8).tolist()
        total, red, cull = h.map_keyframe_redundancy(w.mp, w.kfs, cand, 3, 0.5)
        assert rd.vec("<i4").tobytes() == total.tobytes() and rd.vec("<i4").tobytes() == red.tobytes() and rd.vec("u1").tobytes() == cull.tobytes()
        res = h.map_refresh_points(w.mp, w.kfs, ask, OS.SCALE_RANGE, nr)
        assert rd.vec("u1").tobytes() == res.mp_desc.tobytes() and rd.vec(("<f8", 3)).tobytes() == res.normals.tobytes()
        assert rd.vec("<f8").tobytes() == res.min_distance.tobytes() and rd.vec("<f8").tobytes() == res.max_distance.tobytes()
        assert rd.vec(pkg.MP_REFRESH_RECORD).tobytes() == res.records.tobytes()
        assert rd.vec("u1").tobytes() == w.mp.download(ask)[1].tobytes() == res.mp_desc.tobytes()
        assert rd.pos == len(rd.buf) and (res.records["chosen"] >= 0).sum() > 100
    finally:
        w.close()
        h.close()
