"""The resident map on the GPU at the size of a real map, against the numpy specifications: byte equality everywhere, no tolerance.
Every scene of tests/map_scale_scenes.py enters a path of map_store_kernels.hip that the other map tests stop short of (more than
256 selection workgroups before one, a second and third tile of the covisibility ranking, tracks longer than 512, more than 256
fixed observers, more than 256 goners, slot numbers past 2^20); tests/test_map_scale_cpu.py shows from the specifications alone
that each scene gets there.  The worlds are built once per module: creating a thousand keyframes is most of the time."""
import numpy as np
import pytest

import ba_collect_spec as BSP
import covisibility_scenes as V
import covisibility_spec as CS
import map_fuse_scenes as F
import map_fuse_spec as FSP
import map_observations_spec as OSP
import map_scale_scenes as Z
import map_store_scenes as M
import map_store_spec as MSP
import tracking_scenes as G
from test_ba_collect_gpu import _BaWorld, _assert_spec, _collect
from test_map_fuse_gpu import KEYS, _as_arrays, _cam, _device, _tables
from test_map_fuse_gpu import _world as _fuse_world
from test_map_store_gpu import _World, _d, _expected_lists, _frame_tensors, _np, _same, _select
from test_tracking_gpu import _frame_bytes_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.CameraModel(**G.CAMERA)


@pytest.fixture(scope="module")
def rows():
    return M.random_rows(11, capacity=Z.RANK_CAPACITY)


def _table_world(h, pkg, rows, tables, counts, live, capacity=M.CAPACITY):
    w = _World(h, pkg, rows[0][:capacity], rows[1][:capacity], live, capacity=capacity)
    for t, n in zip(tables, counts):
        w.keyframe(t, n=n)
    return w


class _BigWorld(_World):
    """the big store, filled by ONE set call that names its 300000 slots in shuffled order, and 40 keyframes over it"""

    def __init__(self, h, pkg, big):
        self.h, self.pkg = h, pkg
        self.positions, self.desc = big["positions"], big["desc"]
        self.mp = pkg.MapPointStore(h, big["capacity"])
        self.kfs = []
        assert self.mp.info() == dict(capacity=big["capacity"], n_live=0)
        self.mp.set(big["slots"], self.positions[big["slots"]], self.desc[big["slots"]])


@pytest.fixture(scope="module")
def big():
    return Z.big_store()


@pytest.fixture(scope="module")
def big_world(gpu_handle, pkg, big):
    w = _BigWorld(gpu_handle, pkg, big)
    try:
        w.tables = Z.big_tables(big)
        for t in w.tables:
            w.keyframe(t)
        yield w
    finally:
        w.close()


# ---- scene 1: the big store -------------------------------------------------------------------------------------------------------

def _assert_store(mp, big, live):
    P, D, L = mp.download()
    on = live == 1
    assert L.tobytes() == live.tobytes() and mp.info() == dict(capacity=big["capacity"], n_live=int(on.sum()))
    assert P[on].tobytes() == big["positions"][on].tobytes() and D[on].tobytes() == big["desc"][on].tobytes()
    return P, D


def test_big_store_set_download_erase_and_a_selection_of_293_chunks(gpu_handle, big, big_world):
    """capacity 2^20 + 7, 300000 slots set by one call (blocks at 0, across 65536 and across 2^20 up to capacity - 1), half of them
    erased by one call; one frame's slot source lists all 300000: 293 workgroups, so the base sums take a second stride"""
    cap, slots, gone, mp = big["capacity"], big["slots"], big["gone"], big_world.mp
    live = Z.live_bytes(cap, slots)
    P, D = _assert_store(mp, big, live)
    assert not P[live == 0].any() and not D[live == 0].any()                # nothing was written beside the named slots
    p, d, l = mp.download(slots)
    assert p.tobytes() == big["positions"][slots].tobytes() and d.tobytes() == big["desc"][slots].tobytes() and l.all()
    src = _d(np.concatenate([slots, [0]]).astype(np.int32))
    for lv, erase in ((live, None), (Z.live_bytes(cap, slots, gone), gone)):
        if erase is not None:
            mp.erase(erase)
            _assert_store(mp, big, lv)
            assert mp.download(erase)[2].sum() == 0
        want = MSP.select_slots(slots, lv)
        got = _select(gpu_handle, mp, src_slots=src, src_offsets=[0, len(slots)])
        assert got[0].tolist() == [0, len(want)] and got[1].tobytes() == want.tobytes()
        assert _same(got[2:], MSP.gathered(want, big["positions"], big["desc"]))
    assert len(want) == len(slots) - len(gone) and want.max() == cap - 1
    mp.set(gone, big["positions"][gone], big["desc"][gone])                 # back, for the tests that share the store
    _assert_store(mp, big, live)


# ---- scene 2: many frames, many chunks ----------------------------------------------------------------------------------------------

def test_300_frames_of_one_chunk_and_3_frames_of_91_chunks_in_one_store(gpu_handle, pkg, rows):
    """B * n_chunk is 300 and 273: the workgroups of the later frames sum more than 256 chunk counts; frames without keyframes,
    frames sharing keyframes, a wide frame without candidates between two; the first-sighting rows of the 300 are re-used by the 3
    and again by the 300"""
    sc = Z.frames_scene()
    w = _World(gpu_handle, pkg, rows[0][:M.CAPACITY], rows[1][:M.CAPACITY], sc["live"])
    try:
        small = [w.keyframe(t, n=n) for t, n in zip(sc["small"], sc["small_n"])]
        wide = [w.keyframe(t, n=n) for t, n in zip(sc["wide"], sc["wide_n"])]
        r4 = (rows[0][:M.CAPACITY], rows[1][:M.CAPACITY])
        want_s = _expected_lists([[sc["small"][k] for k in f] for f in sc["small_frames"]], sc["live"], *r4)
        want_w = _expected_lists([[sc["wide"][k] for k in f] for f in sc["wide_frames"]], sc["live"], *r4)
        sel_s = lambda: _select(gpu_handle, w.mp, keyframes=[[small[k] for k in f] for f in sc["small_frames"]])
        sel_w = lambda: _select(gpu_handle, w.mp, keyframes=[[wide[k] for k in f] for f in sc["wide_frames"]])
        for sel, want in ((sel_s, want_s), (sel_w, want_w), (sel_s, want_s), (sel_w, want_w)):
            got = sel()
            assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and _same(got, want)
        assert want_w[0][1] == want_w[0][2] > 1000 and want_s[0][-1] > 3000
    finally:
        w.close()


# ---- scene 3: keyframes past the ranking tile -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kfs", Z.RANK_N_KFS)
@pytest.mark.parametrize("kind", Z.RANK_KINDS)
def test_covisibility_of_1023_to_2049_keyframes_equals_spec_and_rows_equal_their_single_calls(gpu_handle, pkg, rows, kind, n_kfs):
    """the ranking's second and third tile; `equal`: every rank decision is an index tie-break, across the tile borders, and n_best
    cuts inside the tie; weights, best, n_best and the -1 padding"""
    tables, counts, live = Z.rank_world(kind, n_kfs)
    w = _table_world(gpu_handle, pkg, rows, tables, counts, live, capacity=Z.RANK_CAPACITY)
    try:
        q = Z.rank_queries(n_kfs)
        want = CS.weights(tables, live, q)
        for n_best in Z.rank_n_best(n_kfs):
            wt, best, cnt = gpu_handle.map_covisibility(w.mp, w.kfs, q, n_best)
            b, n = CS.best_rows(want, n_best)
            assert wt.tobytes() == want.tobytes(), n_best
            assert _same((best, cnt), (b, n)), (n_best, cnt.tolist(), n.tolist())
            assert all((best[i, n[i]:] == -1).all() for i in range(len(q)))
        b, n = CS.best_rows(want, 1024)
        for i in range(len(q)):
            one = gpu_handle.map_covisibility(w.mp, w.kfs, [q[i]], 1024)
            assert _same(one, (want[i:i + 1], b[i:i + 1], n[i:i + 1])), i
        if kind != "mixed":
            assert n[0] == min(n_kfs - 1, 1024)
            assert b[0, :n[0]].tolist() == (list(range(1, n_kfs)) if kind == "equal" else list(range(n_kfs - 1, 0, -1)))[:1024]
    finally:
        w.close()


# ---- scene 4: a local map over every keyframe -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kfs", Z.LOCAL_N_KFS)
def test_local_map_over_every_keyframe_equals_the_listed_form(gpu_handle, pkg, cam, n_kfs):
    """ref_kf = -1 over 600 / 1025 keyframes: more than one scan round of segments; beside it a frame with a reference keyframe,
    whose neighbours are ranked among them all.  Everything equals map_track_frames_device given the specification's keyframes."""
    sc = Z.local_scene(n_kfs)
    st, tables = sc["store"], sc["tables"]
    w = _World(gpu_handle, pkg, st.positions, st.desc, st.live)
    try:
        for t in tables:
            w.keyframe(t)
        n_best, refs = 2, [-1, max(range(n_kfs), key=lambda k: len(tables[k]))]
        frames = [sc["frame"], sc["frame"]]
        cfg = pkg.TrackConfig.for_mode(1)
        spec = [CS.local_keyframes(tables, st.live, r, n_best) for r in refs]
        assert len(spec[0][0]) == n_kfs and len(spec[1][0]) == 3
        r = _np(pkg, gpu_handle.map_track_local_device(cam, w.mp, w.kfs, refs, n_best, cfg=cfg, **_frame_tensors(frames)))
        want = _np(pkg, gpu_handle.map_track_frames_device(cam, w.mp, keyframes=[[w.kfs[i] for i in s[0]] for s in spec], cfg=cfg, **_frame_tensors(frames)))
        assert r["local_kf"].dtype == np.int32 and r["local_kf"].tolist() == [s[1].tolist() for s in spec]
        lists = [MSP.select_keyframes([tables[i] for i in s[0]], st.live) for s in spec]
        n = int(want["list_offsets"][-1])
        assert r["list_offsets"].tolist() == want["list_offsets"].tolist() == np.cumsum([0] + [len(x) for x in lists]).tolist()
        assert r["list_slot"][:n].tolist() == np.concatenate(lists).tolist()
        pos, de = MSP.gathered(np.concatenate(lists), st.positions, st.desc)
        assert r["positions"][:n].tobytes() == pos.tobytes() and r["mp_desc"][:n].tobytes() == de.tobytes()
        for k in ("list_slot", "positions", "mp_desc"):
            assert r[k][:n].tobytes() == want[k][:n].tobytes(), k
        assert r["offsets"].tolist() == want["offsets"].tolist() and r["matched_slot"].tobytes() == want["matched_slot"].tobytes()
        for b, f in enumerate(frames):
            assert _frame_bytes_device(r, b, len(f[0])) == _frame_bytes_device(want, b, len(f[0])), b
        assert r["results"]["status"][0] == pkg.TRACK_OK and int(r["results"][0]["n_inliers"]) > 100       # (every point of the frame is in the list)
    finally:
        w.close()


# ---- scene 5: long tracks and many points -----------------------------------------------------------------------------------------

def test_tracks_of_every_length_to_1026_lists_and_redundancy(gpu_handle, pkg, rows):
    """row_world("rising", 1026): the long-track ranking takes up to five rounds of 256 either way; min_observations = 1025 is met
    by one point only"""
    tables, counts, live = V.row_world("rising", Z.RISING_N_KFS)
    w = _table_world(gpu_handle, pkg, rows, tables, counts, live)
    try:
        slots = Z.rising_slots()
        want = OSP.observations(tables, live, slots)
        assert set(np.diff(want[0]).tolist()) == set(range(0, 1027))
        assert _same(gpu_handle.map_observations(w.mp, w.kfs, slots), want)
        cand = np.arange(Z.RISING_N_KFS, dtype=np.int32)
        for min_obs in (3, 1025):
            for thr in (0.5, 0.9):
                want_r = OSP.redundancy(tables, live, cand, min_obs, thr)
                assert _same(gpu_handle.map_keyframe_redundancy(w.mp, w.kfs, cand, min_obs, thr), want_r), (min_obs, thr)
        assert want_r[1].max() == 1 and 0 < OSP.redundancy(tables, live, cand, 3, 0.9)[2].sum() < Z.RISING_N_KFS
    finally:
        w.close()


def test_observations_of_300000_points_on_the_big_store(gpu_handle, big, big_world):
    """n_list = 300000: 293 chunks of points, so the scan's `before` sum takes a second stride; slots past 2^20 index the table"""
    slots = big["slots"]
    live = Z.live_bytes(big["capacity"], slots)
    want = Z.observations_sorted(big_world.tables, live, slots)
    got = gpu_handle.map_observations(big_world.mp, big_world.kfs, slots)
    assert got[0].tobytes() == want[0].tobytes() and _same(got, want)
    some = slots[::1000]                                                    # and a short list against the looped specification itself
    assert _same(gpu_handle.map_observations(big_world.mp, big_world.kfs, some), OSP.observations(big_world.tables, live, some))
    cand = np.arange(len(big_world.kfs), dtype=np.int32)
    assert _same(gpu_handle.map_keyframe_redundancy(big_world.mp, big_world.kfs, cand, 1, 0.1), OSP.redundancy(big_world.tables, live, cand, 1, 0.1))


# ---- scene 6: many fixed observers ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def window(gpu_handle, pkg, rows):
    tables, counts, live, xy = Z.window_world()
    w = _BaWorld(gpu_handle, pkg, rows[0][:M.CAPACITY], rows[1][:M.CAPACITY], live)
    try:
        for t, p in zip(tables, xy):
            w.keyframe(t, p)
        yield w, tables, live, xy
    finally:
        w.close()


@pytest.mark.parametrize("max_covisible", [3, 20])
def test_window_with_more_than_600_fixed_observers_equals_spec(gpu_handle, pkg, rows, window, max_covisible):
    w, tables, live, xy = window
    want = BSP.collect(tables, xy, live, 0, max_covisible)
    assert int(want["counts"][1]) - 1 >= 600
    _assert_spec(_collect(gpu_handle, pkg, w.mp, w.kfs, 0, max_covisible), want, rows[0][:M.CAPACITY])
    host = gpu_handle.map_collect_ba_window(w.mp, w.kfs, 0, max_covisible)
    assert all(host[k].tobytes() == want[k].tobytes() for k in ("counts", "local_kf", "fixed_kf", "list_slot", "obs32"))


# ---- scene 7: many merges ---------------------------------------------------------------------------------------------------------

def test_one_pass_with_560_merges_equals_spec_and_the_host_form_erases_exactly_the_goners(gpu_handle, pkg, oracle):
    """three tiles and three workgroups of the goners' ranking; classes of two, every one kept by the projected point"""
    sc = Z.merge_world()
    want = FSP.fuse(sc["tables"], sc["live"], sc["positions"], sc["desc"], [Z.MERGE_CUR], Z.MERGE_TGT, F.oracle_search(oracle, sc))
    assert int(want["counts"][3]) >= 520
    w, w2 = _fuse_world(gpu_handle, pkg, sc), _fuse_world(gpu_handle, pkg, sc)
    try:
        got = _device(gpu_handle, pkg, w, [Z.MERGE_CUR], Z.MERGE_TGT)
        for k in KEYS:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, got["counts"], want["counts"])
        new = _as_arrays(want["tables"], sc["tables"].counts)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_tables(w), new))
        assert w.mp.download()[2].tobytes() == sc["live"].tobytes()         # the device form erases nothing
        # d_mp_uniq was made again: covisibility on the new tables
        wt, best, cnt = gpu_handle.map_covisibility(w.mp, w.kfs, range(len(w.kfs)), 4)
        want_w = CS.weights(new, sc["live"], range(len(w.kfs)))
        assert wt.tobytes() == want_w.tobytes() and _same((best, cnt), CS.best_rows(want_w, 4))
        assert OSP.n_observers(new, sc["live"])[want["goner"]].sum() == 0   # no table names a goner
        host = gpu_handle.map_fuse(_cam(pkg), w2.mp, w2.kfs, [Z.MERGE_CUR], Z.MERGE_TGT, F.RADIUS_SCALE)
        for k in KEYS:
            assert host[k].tobytes() == want[k].tobytes(), k
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_tables(w2), new))
        live = sc["live"].copy(); live[want["goner"]] = 0
        assert w2.mp.download()[2].tobytes() == live.tobytes() and w2.mp.info()["n_live"] == int(sc["live"].sum()) - int(want["counts"][3])
    finally:
        w.close(); w2.close()


# ---- scene 8: the frame count as a grid row -----------------------------------------------------------------------------------------

def test_more_than_65535_frames_are_refused_before_anything_runs(gpu_handle, pkg, cam, rows):
    """every call whose frame is a grid row: 65536 frames without keyframes or entries are ORBX_ERR_INVALID; the store, the tables
    and the first-sighting rows are as they were (the selection that follows is exact), and 65535 frames are served"""
    import torch
    live = np.zeros(64, np.uint8); live[[3, 4, 9, 63]] = 1
    w = _World(gpu_handle, pkg, rows[0][:64], rows[1][:64], live, capacity=64)
    try:
        t0, t1 = np.array([3, -1, 9, 3, 5], np.int32), np.array([63, 4, 9], np.int32)
        k0, k1 = w.keyframe(t0), w.keyframe(t1)
        want = _expected_lists([[t0, t1], [t1]], live, rows[0][:64], rows[1][:64])
        assert _same(_select(gpu_handle, w.mp, keyframes=[[k0, k1], [k1]]), want)
        before = w.mp.download()
        B = Z.MAX_GRID_ROWS + 1
        f0 = G.frame(3, 4, 6)
        frame = (f0[0][:0], f0[1][:0], f0[4], f0[5])
        dev = dict(kp=torch.zeros((1, 7), dtype=torch.float32, device="cuda"), desc=torch.zeros((1, 32), dtype=torch.uint8, device="cuda"),
                   feat_start=torch.zeros(B, dtype=torch.int32, device="cuda"), feat_count=torch.zeros(B, dtype=torch.int32, device="cuda"), max_feat=1)
        poses = _d(np.tile(f0[4], (B, 1)))
        empty = _d(np.zeros(1, np.int32))
        bad = [lambda: gpu_handle.map_select_points_device(w.mp, keyframes=[[]] * B),
               lambda: gpu_handle.map_select_points_device(w.mp, src_slots=empty, src_offsets=np.zeros(B + 1, np.int32)),
               lambda: gpu_handle.map_track_frames_device(cam, w.mp, keyframes=[[]] * B, search_poses_wc=poses, priors_wc=poses, **dev),
               lambda: gpu_handle.map_track_frames(cam, w.mp, [frame] * B, keyframes=[[]] * B),
               lambda: gpu_handle.map_track_local_device(cam, w.mp, [k0, k1], [-1] * B, 1, search_poses_wc=poses, priors_wc=poses, **dev),
               lambda: gpu_handle.map_track_local(cam, w.mp, [frame] * B, [k0, k1], [0] * B, 1),
               lambda: gpu_handle.map_track_reference_device(cam, w.mp, [k1] * B, priors_wc=poses, **dev)]
        for i, f in enumerate(bad):
            with pytest.raises(pkg.OrbxError) as e:
                f()
            assert e.value.code == -1 and "at most 65535 frames per call" in str(e.value), (i, str(e.value))
        gpu_handle.synchronize()
        assert _same(w.mp.download(), before) and w.mp.info() == dict(capacity=64, n_live=4)
        assert k0.get_map_point_slots().tolist() == t0.tolist() and k1.get_map_point_slots().tolist() == t1.tolist()
        assert _same(_select(gpu_handle, w.mp, keyframes=[[k0, k1], [k1]]), want)
        # the largest count that is served: 65535 frames, the last one with keyframes
        most = [[]] * (Z.MAX_GRID_ROWS - 1) + [[k0, k1]]
        got = _select(gpu_handle, w.mp, keyframes=most)
        one = _expected_lists([[t0, t1]], live, rows[0][:64], rows[1][:64])
        assert got[0].tolist() == [0] * Z.MAX_GRID_ROWS + [int(one[0][1])] and _same(got[1:], one[1:])
        assert _same(_select(gpu_handle, w.mp, keyframes=[[k0, k1], [k1]]), want)
    finally:
        w.close()
