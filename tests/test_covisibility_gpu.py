"""Covisibility on the resident map on the GPU against tests/covisibility_spec.py: exact equality everywhere.  Weights, best lists
and the chosen local keyframes equal the spec; every other output of map_track_local[_device] equals, byte for byte, what
map_track_frames_device returns for the spec's keyframe lists (composition: the new calls add no arithmetic)."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import covisibility_scenes as V
import covisibility_spec as S
import map_store_scenes as M
import map_store_spec as MS
import tracking_scenes as G
from test_covisibility_cpu import build_driver
from test_map_store_gpu import _World, _d, _frame_tensors, _np, _same, _select
from test_track_cpp import _Reader, _assert_same
from test_tracking_gpu import _frame_bytes_device, _frame_bytes_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.CameraModel(**G.CAMERA)


@pytest.fixture(scope="module")
def rows():
    return M.random_rows(6)


def _cov(h, mp, kfs, queries, n_best=0):
    import torch
    o = h.map_covisibility_device(mp, kfs, queries, n_best)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _world(h, pkg, rows, tables, counts, live, capacity=M.CAPACITY):
    w = _World(h, pkg, rows[0][:capacity], rows[1][:capacity], live, capacity=capacity)
    for t, n in zip(tables, counts):
        w.keyframe(t, n=n)
    return w


def _queries(n_kfs):
    """every keyframe where they are few; else seven of them (not a multiple of the count kernel's query group): a keyframe
    without a table, the ends, and one keyframe twice"""
    return list(range(n_kfs)) if n_kfs <= 11 else [0, 5, n_kfs - 1, 3, 17, 0, n_kfs // 2]


# ---- weights ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kfs", V.N_KFS)
def test_weights_equal_spec_and_rows_equal_their_single_calls(gpu_handle, pkg, rows, n_kfs):
    """feature counts from {0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025}, keyframes without a table, repeats inside a table,
    dead slots and -1 entries; several queries in one call that share keyframes"""
    tables, counts, live = V.world(20 + n_kfs, n_kfs)
    w = _world(gpu_handle, pkg, rows, tables, counts, live)
    try:
        q = _queries(n_kfs)
        want = S.weights(tables, live, q)
        got = _cov(gpu_handle, w.mp, w.kfs, q)["weights"]
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
        for i in range(min(len(q), 5)):
            one = _cov(gpu_handle, w.mp, w.kfs, [q[i]])["weights"]
            assert one.tobytes() == want[i:i + 1].tobytes(), i
    finally:
        w.close()


def test_weights_where_the_capacity_is_no_multiple_of_64(gpu_handle, pkg, rows):
    tables, counts, live = V.world(77, 11, capacity=1000)
    w = _world(gpu_handle, pkg, rows, tables, counts, live, capacity=1000)
    try:
        q = list(range(11))
        r = _cov(gpu_handle, w.mp, w.kfs, q, 4)
        want = S.weights(tables, live, q)
        assert want.max() > 10 and _same((r["weights"], r["best"], r["n_best"]), (want,) + S.best_rows(want, 4))
    finally:
        w.close()


def test_known_answers(gpu_handle, pkg):
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "covisibility_known_answers.json")))
    desc = np.arange(12 * 32, dtype=np.uint32).astype(np.uint8).reshape(12, 32)
    w = _World(gpu_handle, pkg, np.zeros((12, 3)), desc, k["live"], capacity=k["capacity"])
    try:
        for t, n in zip(k["tables"], k["n_features"]):
            w.keyframe(None if t is None else np.array(t, np.int32), n=n)
        r = _cov(gpu_handle, w.mp, w.kfs, list(range(7)), 3)
        assert r["weights"].tolist() == k["weights"] and r["best"].tolist() == k["best_3"] and r["n_best"].tolist() == k["n_best_3"]
        r = _cov(gpu_handle, w.mp, w.kfs, [0], 10)
        assert r["best"][0].tolist() == k["best_10_row_0"] and r["n_best"].tolist() == [k["n_best_10_row_0"]]
    finally:
        w.close()


# ---- best lists ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_best", [0, 1, 10, 20, 65, 68])
def test_best_lists_equal_spec(gpu_handle, pkg, rows, n_best):
    """n_kfs = 65: n_best in {0, 1, 10, 20, n_kfs, n_kfs + 3}; d_n_best and the -1 padding exact"""
    tables, counts, live = V.world(85, 65)
    w = _world(gpu_handle, pkg, rows, tables, counts, live)
    try:
        q = _queries(65)
        want = S.weights(tables, live, q)
        r = _cov(gpu_handle, w.mp, w.kfs, q, n_best)
        assert r["weights"].tobytes() == want.tobytes()
        if n_best == 0:
            assert set(r) == {"weights"}
            return
        b, n = S.best_rows(want, n_best)
        assert _same((r["best"], r["n_best"]), (b, n)) and n[1] == 0 and 0 < n.max() <= min(n_best, 64)       # (query 5 has no table: an all-zero row)
        import torch
        only = gpu_handle.map_covisibility_device(w.mp, w.kfs, q, n_best, weights=False)                       # d_weights NULL: the rows live in the workspace
        torch.cuda.synchronize()
        assert set(only) == {"best", "n_best"} and _same((only["best"].cpu().numpy(), only["n_best"].cpu().numpy()), (b, n))
    finally:
        w.close()


@pytest.mark.parametrize("n_kfs", [3, 257])
@pytest.mark.parametrize("kind", ["equal", "zero", "rising"])
def test_rows_all_equal_all_zero_and_rising_with_the_index(gpu_handle, pkg, rows, kind, n_kfs):
    """a row whose weights are all equal (index order), all zero (nothing but padding), or strictly decreasing in reverse index
    order; 257 keyframes are more than one pass of the ranking workgroup"""
    tables, counts, live = V.row_world(kind, n_kfs)
    w = _world(gpu_handle, pkg, rows, tables, counts, live)
    try:
        for n_best in (10, n_kfs + 3):
            r = _cov(gpu_handle, w.mp, w.kfs, [0, n_kfs - 1], n_best)
            want = S.weights(tables, live, [0, n_kfs - 1])
            assert _same((r["weights"], r["best"], r["n_best"]), (want,) + S.best_rows(want, n_best)), n_best
        n = {"equal": n_kfs - 1, "zero": 0, "rising": n_kfs - 1}[kind]
        assert r["n_best"][0] == n and (r["best"][0, n:] == -1).all()
        if kind == "rising":
            assert r["best"][0, :n].tolist() == list(range(n_kfs - 1, 0, -1))
        if kind == "equal":
            assert r["best"][0, :n].tolist() == list(range(1, n_kfs))
    finally:
        w.close()


# ---- the tables are left clean ---------------------------------------------------------------------------------------------

def test_calls_leave_the_tables_clean_and_erase_lowers_the_weights(gpu_handle, pkg, rows):
    tables, counts, live = V.world(31, 11)
    w = _world(gpu_handle, pkg, rows, tables, counts, live)
    try:
        q = list(range(11))
        with_table = [k for k in w.kfs if k is not w.kfs[5]]
        sel1 = _select(gpu_handle, w.mp, keyframes=[with_table, w.kfs[:3]])
        a = _cov(gpu_handle, w.mp, w.kfs, q, 5)
        b = _cov(gpu_handle, w.mp, w.kfs, q, 5)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)                                # the same call twice
        # other queries over the same tables see no marks of the earlier ones
        assert _cov(gpu_handle, w.mp, w.kfs, [7, 2])["weights"].tobytes() == S.weights(tables, live, [7, 2]).tobytes()
        assert _same(_select(gpu_handle, w.mp, keyframes=[with_table, w.kfs[:3]]), sel1)         # and the selection's tables are untouched
        # erase slots that keyframes share: the weights drop as the spec says
        want = S.weights(tables, live, q)
        k0, k1 = np.unravel_index(np.argmax(want), want.shape)
        shared = sorted(S.observed(tables[k0], live) & S.observed(tables[k1], live))
        gone = np.array(shared[:max(len(shared) // 2, 1)], np.int32)
        w.mp.erase(gone)
        live2 = live.copy(); live2[gone] = 0
        want2 = S.weights(tables, live2, q)
        assert want2[k0, k1] == want[k0, k1] - len(gone)
        r = _cov(gpu_handle, w.mp, w.kfs, q, 5)
        assert _same((r["weights"], r["best"], r["n_best"]), (want2,) + S.best_rows(want2, 5))
        w.kfs[k1].set_map_point_slots(w.mp, None)                                              # a table cleared: the keyframe observes nothing
        t3 = list(tables); t3[k1] = None
        assert _cov(gpu_handle, w.mp, w.kfs, q)["weights"].tobytes() == S.weights(t3, live2, q).tobytes()
    finally:
        w.close()


# ---- tracking with the local keyframes chosen on the device ----------------------------------------------------------------

def _tracking(gpu_handle, pkg):
    store, scs, tables, first = V.tracking_world()
    w = _World(gpu_handle, pkg, store.positions, store.desc, store.live)
    for t in tables:
        w.keyframe(t)
    # a reference with more covisibles than n_best, one with none, no reference at all
    cases = [(scs[0]["frame"], first[0]), (scs[2]["frame"], first[2]), (scs[1]["frame"], -1)]
    return w, store, tables, cases


@pytest.mark.parametrize("mode", [0, 1])
def test_map_track_local_device_equals_map_track_frames_device(gpu_handle, pkg, cam, mode):
    w, store, tables, cases = _tracking(gpu_handle, pkg)
    try:
        cfg = pkg.TrackConfig.for_mode(mode)
        n_best = 2
        local = lambda cs: _np(pkg, gpu_handle.map_track_local_device(cam, w.mp, w.kfs, [r for _, r in cs], n_best, cfg=cfg, **_frame_tensors([f for f, _ in cs])))
        spec = [S.local_keyframes(tables, store.live, r, n_best) for _, r in cases]
        assert [len(s[0]) for s in spec] == [3, 1, 9]
        subsets = [cases[:1], cases[1:2], cases[2:], cases]                                    # every case alone, then the batch mixing all three
        got = [local(cs) for cs in subsets]
        for cs, r, idx in zip(subsets, got, [[0], [1], [2], [0, 1, 2]]):
            frames = [f for f, _ in cs]
            want = _np(pkg, gpu_handle.map_track_frames_device(cam, w.mp, keyframes=[[w.kfs[i] for i in spec[j][0]] for j in idx], cfg=cfg, **_frame_tensors(frames)))
            assert r["local_kf"].dtype == np.int32 and r["local_kf"].tolist() == [spec[j][1].tolist() for j in idx]
            n = int(want["list_offsets"][-1])
            lists = [MS.select_keyframes([tables[i] for i in spec[j][0]], store.live) for j in idx]
            assert r["list_offsets"].tolist() == want["list_offsets"].tolist() == np.cumsum([0] + [len(x) for x in lists]).tolist()
            assert r["list_slot"][:n].tolist() == np.concatenate(lists).tolist()
            for k in ("list_slot", "positions", "mp_desc"):
                assert r[k][:n].tobytes() == want[k][:n].tobytes(), k
            assert r["offsets"].tolist() == want["offsets"].tolist() and r["matched_slot"].tobytes() == want["matched_slot"].tobytes()
            for b, f in enumerate(frames):
                assert _frame_bytes_device(r, b, len(f[0])) == _frame_bytes_device(want, b, len(f[0])), (mode, b)
        assert got[3]["results"]["status"][2] == pkg.TRACK_OK and got[3]["offsets"][1] > 0        # (the frame over every keyframe sees all its points)
        # batch-composition independence: frame b alone equals frame b in the batch
        full = got[3]
        for b, one in enumerate(got[:3]):
            nf = len(cases[b][0][0])
            s = slice(int(full["list_offsets"][b]), int(full["list_offsets"][b + 1]))
            assert _frame_bytes_device(one, 0, nf) == _frame_bytes_device(full, b, nf), b
            assert one["list_slot"][:s.stop - s.start].tolist() == full["list_slot"][s].tolist() and one["local_kf"][0].tolist() == full["local_kf"][b].tolist()
            assert one["matched_slot"][0, :nf].tolist() == full["matched_slot"][b, :nf].tolist()
        again = local(cases)
        assert all(_frame_bytes_device(again, b, len(c[0][0])) == _frame_bytes_device(full, b, len(c[0][0])) for b, c in enumerate(cases))
    finally:
        w.close()


def test_host_forms_equal_device_forms(gpu_handle, pkg, cam):
    w, store, tables, cases = _tracking(gpu_handle, pkg)
    try:
        q = [0, 6, 8, 3, 0]
        dev = _cov(gpu_handle, w.mp, w.kfs, q, 4)
        wt, best, cnt = gpu_handle.map_covisibility(w.mp, w.kfs, q, 4)
        assert _same((wt, best, cnt), (dev["weights"], dev["best"], dev["n_best"])) and wt.tobytes() == S.weights(tables, store.live, q).tobytes()
        start, ids = pkg.covisibility_lists(np.arange(100, 109), *gpu_handle.map_covisibility(w.mp, w.kfs, range(9), 3)[1:])
        want = [S.best(r, 3) for r in S.weights(tables, store.live, range(9))]
        assert np.diff(start).tolist() == [n for _, n in want] and ids.tolist() == [100 + int(i) for b, n in want for i in b[:n]]
        cfg = pkg.TrackConfig.for_mode(1)
        frames, ref = [f for f, _ in cases], [r for _, r in cases]
        r = _np(pkg, gpu_handle.map_track_local_device(cam, w.mp, w.kfs, ref, 2, cfg=cfg, **_frame_tensors(frames)))
        for b, (t, ls, ms, lk) in enumerate(gpu_handle.map_track_local(cam, w.mp, frames, w.kfs, ref, 2, cfg=cfg)):
            nf = len(frames[b][0])
            assert _frame_bytes_host(pkg, t) == _frame_bytes_device(r, b, nf), b
            assert ls.tolist() == r["list_slot"][r["list_offsets"][b]:r["list_offsets"][b + 1]].tolist() and ms.tolist() == r["matched_slot"][b, :nf].tolist()
            assert lk.dtype == np.int32 and lk.tolist() == r["local_kf"][b].tolist()
    finally:
        w.close()


# ---- validation ------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_store_usable_and_the_next_call_exact(gpu_handle, pkg, cam):
    import torch
    w, store, tables, cases = _tracking(gpu_handle, pkg)
    other = pkg.MapPointStore(gpu_handle, 64)
    try:
        frames, a = [cases[0][0]], _frame_tensors([cases[0][0]])
        stranger = w.keyframe(np.array([1, 2], np.int32)); w.kfs.pop()
        stranger.set_map_point_slots(other, [1, 2])
        bad = [lambda: gpu_handle.map_covisibility_device(w.mp, w.kfs, [9]), lambda: gpu_handle.map_covisibility_device(w.mp, w.kfs, [0, -1], 2),
               lambda: gpu_handle.map_covisibility_device(w.mp, w.kfs, [0], -1), lambda: gpu_handle.map_covisibility(w.mp, w.kfs, [9], 2),
               lambda: gpu_handle.map_covisibility(w.mp, w.kfs, [0], -1), lambda: gpu_handle.map_covisibility_device(w.mp, w.kfs + [stranger], [0], 2),
               lambda: gpu_handle.map_covisibility(w.mp, w.kfs + [stranger], [0], 2),
               lambda: gpu_handle.map_track_local_device(cam, w.mp, w.kfs, [9], 2, **a), lambda: gpu_handle.map_track_local_device(cam, w.mp, w.kfs, [-2], 2, **a),
               lambda: gpu_handle.map_track_local_device(cam, w.mp, w.kfs, [0], -1, **a),
               lambda: gpu_handle.map_track_local_device(cam, w.mp, w.kfs + [stranger], [0], 2, **a),
               lambda: gpu_handle.map_track_local(cam, w.mp, frames, w.kfs, [9], 2), lambda: gpu_handle.map_track_local(cam, w.mp, frames, w.kfs, [0], -1),
               lambda: gpu_handle.map_track_local(cam, w.mp, frames, w.kfs + [stranger], [-1], 2)]
        for i, f in enumerate(bad):
            with pytest.raises(pkg.OrbxError) as e:
                f()
            assert e.value.code == -1, i
        assert "another store" in str(e.value)
        # a list_cap below the host-known bound
        o = gpu_handle.map_track_local_device(cam, w.mp, w.kfs, [0], 2, **a)
        L = gpu_handle._L
        arr = (C.c_void_p * 9)(*[k._p for k in w.kfs])
        ref = np.array([0], np.int32)
        bound = w.kfs[0].n + sum(sorted([k.n for k in w.kfs[1:]], reverse=True)[:2])
        tc = pkg.TrackConfig()._c(); pc = pkg.PnPConfig()._c(); cc = cam._c()
        p = lambda t: C.c_void_p(t.data_ptr())
        call = lambda cap: L.orbx_map_track_local_device(
            gpu_handle._h, C.byref(cc), C.byref(tc), C.byref(pc), w.mp._p, C.c_int(1), C.c_int(9), arr, ref.ctypes.data_as(C.c_void_p), C.c_int(2), p(a["kp"]), p(a["desc"]),
            p(a["feat_start"]), p(a["feat_count"]), C.c_int(1), C.c_int(a["max_feat"]), p(a["search_poses_wc"]), p(a["priors_wc"]), C.c_int(cap), p(o["local_kf"]),
            p(o["list_offsets"]), p(o["list_slot"]), p(o["positions"]), p(o["mp_desc"]), p(o["offsets"]), p(o["points3d"]), p(o["points2d"]), p(o["mp_idx"]),
            p(o["feat_idx"]), p(o["poses"]), p(o["inlier"]), p(o["err"]), p(o["pnp_results"]), p(o["matched"]), p(o["matched_slot"]), p(o["results"]))
        torch.cuda.synchronize()
        assert len(o["list_slot"]) == bound and call(bound - 1) == -1 and call(bound) == 0
        # nothing to do is no error
        assert gpu_handle.map_covisibility_device(w.mp, w.kfs, [], 3)["best"].shape == (0, 3)
        assert gpu_handle.map_covisibility_device(w.mp, [], [], 3)["weights"].shape == (0, 0)
        assert gpu_handle.map_covisibility(w.mp, w.kfs, [], 2)[0].shape == (0, 9) and gpu_handle.map_covisibility(w.mp, [], [], 2)[2].shape == (0,)
        # the next valid calls are exact
        want = S.weights(tables, store.live, range(9))
        r = _cov(gpu_handle, w.mp, w.kfs, range(9), 3)
        assert _same((r["weights"], r["best"], r["n_best"]), (want,) + S.best_rows(want, 3))
        r = _np(pkg, gpu_handle.map_track_local_device(cam, w.mp, w.kfs, [0], 2, **a))
        lst, row = S.local_keyframes(tables, store.live, 0, 2)
        assert r["local_kf"][0].tolist() == row.tolist()
        assert r["list_slot"][:r["list_offsets"][1]].tolist() == MS.select_keyframes([tables[i] for i in lst], store.live).tolist()
        assert w.mp.info()["n_live"] == int(store.live.sum())
    finally:
        gpu_handle.synchronize()
        stranger.close(); other.close()
        w.close()


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------

def test_covisibility_driver_equals_python_mirror(pkg, tmp_path):
    import torch
    tmp = str(tmp_path)
    exe = build_driver(tmp)
    store, scs, tables, first = V.tracking_world()
    cam = G.CAMERA
    frames = [scs[0]["frame"], scs[2]["frame"], scs[1]["frame"]]
    ref, n_best = [first[0], first[2], -1], 2
    live = store.live_slots()
    with open(os.path.join(tmp, "covisibility_in.bin"), "wb") as f:
        f.write(struct.pack("<iiiii5d", store.capacity, len(live), len(tables), len(frames), n_best, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["baseline"]))
        f.write(live.astype(np.int32).tobytes()); f.write(store.positions[live].tobytes()); f.write(store.desc[live].tobytes())
        for t in tables:
            f.write(struct.pack("<i", len(t))); f.write(np.ascontiguousarray(t, np.int32).tobytes())
        for (kp, desc, sp, pr), r in zip(frames, ref):
            f.write(struct.pack("<ii14d", len(kp), r, *[float(v) for v in sp], *[float(v) for v in pr]))
            f.write(np.ascontiguousarray(kp, G.KEYPOINT).tobytes()); f.write(np.ascontiguousarray(desc, np.uint8).tobytes())
    r = subprocess.run([exe, tmp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "COVISIBILITY_DRIVER_OK" in r.stdout, (r.stdout, r.stderr)
    rd = _Reader(open(os.path.join(tmp, "covisibility_out.bin"), "rb").read())
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
        wt, best, cnt = h.map_covisibility(mp, kfs, range(len(kfs)), n_best)
        assert rd.vec("<i4").tolist() == wt.reshape(-1).tolist() and rd.vec("<i4").tolist() == best.reshape(-1).tolist() and rd.vec("<i4").tolist() == cnt.tolist()
        assert rd.vec("<i4").tolist() == best[0, :cnt[0]].tolist()
        res = h.map_track_local(c, mp, frames, kfs, ref, n_best, cfg=pkg.TrackConfig.for_mode(1))
        for t, ls, ms, lk in res + h.map_track_local(c, mp, frames[:1], kfs, ref[:1], n_best, cfg=pkg.TrackConfig.for_mode(1)):
            _assert_same(pkg, rd.result(pkg), t)
            assert rd.vec("<i4").tolist() == ls.tolist() and rd.vec("<i4").tolist() == ms.tolist() and rd.vec("<i4").tolist() == lk.tolist()
        assert rd.pos == len(rd.buf) and res[2][0].status == pkg.TRACK_OK
    finally:
        h.synchronize()
        for k in kfs:
            k.close()
        mp.close()
        h.close()
