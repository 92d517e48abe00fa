"""The resident map-point store on the GPU against tests/map_store_spec.py: exact equality everywhere.  Lists, offsets, gathered
rows and matched_slot equal the spec; every output of map_track_frames[_device] equals, byte for byte, what track_frames_device
returns for the spec's gathered rows on the same frames, and map_track_reference_device what keyframe_track_reference returns for
the spec's rows (composition: the new calls add no arithmetic)."""
import json
import os

import numpy as np
import pytest

import map_store_scenes as M
import map_store_spec as S
import track_reference_scenes as R
import tracking_scenes as G
from test_tracking_gpu import _frame_bytes_device, _frame_bytes_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOTALS = [0, 1, 63, 64, 65, 255, 256, 257, M.CHUNK - 1, M.CHUNK, M.CHUNK + 1, 2 * M.CHUNK - 1, 2 * M.CHUNK, 2 * M.CHUNK + 1]


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.CameraModel(**G.CAMERA)


@pytest.fixture(scope="module")
def rows():
    return M.random_rows(5)


def _d(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _World:
    """a device store filled from a host image, and keyframes with slot tables; everything is closed at the end"""

    def __init__(self, h, pkg, positions, desc, live, capacity=M.CAPACITY):
        self.h, self.pkg = h, pkg
        self.positions, self.desc, self.live = np.asarray(positions), np.asarray(desc), np.asarray(live, np.uint8).copy()
        self.mp = pkg.MapPointStore(h, capacity)
        ls = np.flatnonzero(self.live).astype(np.int32)
        self.mp.set(ls, self.positions[ls], self.desc[ls])
        self.kfs = []

    def keyframe(self, table, n=None, desc=None):
        import torch
        n = len(table) if n is None else n
        d = _d(desc) if desc is not None and n else torch.zeros((max(n, 1), 32), dtype=torch.uint8, device="cuda")
        kf = self.pkg.KeyFrame(self.h, torch.zeros((max(n, 1), 7), dtype=torch.float32, device="cuda"), d, n)
        if table is not None:
            kf.set_map_point_slots(self.mp, table)
        self.kfs.append(kf)
        return kf

    def close(self):
        self.h.synchronize()
        for k in self.kfs:
            k.close()
        self.mp.close()


def _expected_lists(tables_per_frame, live, positions, desc):
    lists = [S.select_keyframes(t, live) for t in tables_per_frame]
    off = np.zeros(len(lists) + 1, np.int32); off[1:] = np.cumsum([len(x) for x in lists])
    cat = np.concatenate(lists + [np.zeros(0, np.int32)]).astype(np.int32)
    pos, de = S.gathered(cat, positions, desc)
    return off, cat, pos, de


def _select(h, mp, **src):
    import torch
    o = h.map_select_points_device(mp, **src)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in o.items()}
    n = int(r["list_offsets"][-1])
    return r["list_offsets"], r["list_slot"][:n], r["positions"][:n], r["mp_desc"][:n]


def _same(got, want):
    return all(np.asarray(g).dtype == np.asarray(w).dtype and np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


# ---- the store itself ----------------------------------------------------------------------------------------------------

def test_set_download_erase_round_trip(gpu_handle, pkg, rows):
    pos, desc = rows
    mp = pkg.MapPointStore(gpu_handle, 300)
    try:
        assert mp.info() == dict(capacity=300, n_live=0)
        slots = np.array([7, 0, 299, 150, 151], np.int32)
        mp.set(slots, pos[:5], desc[:5])
        p, d, l = mp.download(slots)
        assert p.tobytes() == pos[:5].tobytes() and d.tobytes() == desc[:5].tobytes() and l.tolist() == [1] * 5 and mp.info()["n_live"] == 5
        P, D, Lv = mp.download()
        assert Lv.sum() == 5 and not P[Lv == 0].any() and not D[Lv == 0].any()
        mp.set(slots[:2], positions=pos[10:12])                              # positions only: BA's apply
        mp.set(slots[2:4], descriptors=desc[20:22])                          # descriptors only: the refresh
        p, d, l = mp.download(slots)
        assert p.tobytes() == np.concatenate([pos[10:12], pos[2:5]]).tobytes()
        assert d.tobytes() == np.concatenate([desc[:2], desc[20:22], desc[4:5]]).tobytes() and l.all()
        mp.erase([150, 150, 3])                                              # a repeat and a slot that never lived
        assert mp.download(slots)[2].tolist() == [1, 1, 1, 0, 1] and mp.info()["n_live"] == 4
        mp.set([], np.zeros((0, 3)), np.zeros((0, 32), np.uint8)); mp.erase([])
        # set_device equals set
        other = pkg.MapPointStore(gpu_handle, 300)
        try:
            s2 = np.array([1, 298, 64, 65, 2], np.int32)
            mp.set(s2, pos[30:35], desc[30:35])
            other.set_device(slots, _d(pos[:5]), _d(desc[:5]))
            other.set_device(slots[:2], positions=_d(pos[10:12])); other.set_device(slots[2:4], descriptors=_d(desc[20:22]))
            other.erase([150])
            other.set_device(s2, _d(pos[30:35]), _d(desc[30:35]))
            assert _same(other.download(), mp.download()) and other.info() == mp.info()
        finally:
            other.close()
    finally:
        mp.close()


def test_refusals_change_nothing(gpu_handle, pkg, rows):
    import torch
    pos, desc = rows
    mp = pkg.MapPointStore(gpu_handle, 64)
    kf = pkg.KeyFrame(gpu_handle, torch.zeros((4, 7), dtype=torch.float32, device="cuda"), torch.zeros((4, 32), dtype=torch.uint8, device="cuda"), 4)
    try:
        mp.set([3, 4], pos[:2], desc[:2])
        before = mp.download()
        bad = [lambda: mp.set([5, 64], pos[:2], desc[:2]), lambda: mp.set([-1], pos[:1], desc[:1]),            # outside [0, capacity)
               lambda: mp.set([5, 6, 5], pos[:3], desc[:3]), lambda: mp.set([3, 3], positions=pos[:2]),        # a slot twice
               lambda: mp.set([3, 9], positions=pos[:2]), lambda: mp.set([9], descriptors=desc[:1]),           # a first set with a field missing
               lambda: mp.set_device([5, 64], _d(pos[:2]), _d(desc[:2])), lambda: mp.set_device([7, 7], _d(pos[:2]), _d(desc[:2])),
               lambda: mp.set_device([9], positions=_d(pos[:1])), lambda: mp.erase([64]), lambda: mp.erase([-1]), lambda: mp.download([64]),
               lambda: kf.set_map_point_slots(mp, [0, 1, 64, 2]), lambda: kf.set_map_point_slots(mp, [0, -2, 1, 2])]
        for f in bad:
            with pytest.raises(pkg.OrbxError) as e:
                f()
            assert e.value.code == -1
        assert _same(mp.download(), before) and mp.info()["n_live"] == 2
        with pytest.raises(pkg.OrbxError):
            pkg.MapPointStore(gpu_handle, 0)
        # a list_cap below the bound, an unknown source, no frames
        kf.set_map_point_slots(mp, [3, 4, -1, 3])
        L = gpu_handle._L
        import ctypes as C
        arr = (C.c_void_p * 1)(kf._p)
        ko = np.array([0, 1], np.int32)
        out = [torch.zeros(16, dtype=torch.int32, device="cuda"), torch.zeros(16, dtype=torch.int32, device="cuda"), torch.zeros((16, 3), dtype=torch.float64, device="cuda"),
               torch.zeros((16, 32), dtype=torch.uint8, device="cuda")]
        ptr = [C.c_void_p(t.data_ptr()) for t in out]
        call = lambda src, B, cap: L.orbx_map_select_points_device(gpu_handle._h, mp._p, C.c_int(src), C.c_int(B), arr, ko.ctypes.data_as(C.c_void_p), None, None,
                                                                   C.c_int(cap), *ptr)
        assert call(0, 1, 3) == -1 and call(2, 1, 16) == -1 and call(0, 0, 16) == -1 and call(0, 1, 4) == 0
        gpu_handle.synchronize()
        assert out[0][:2].tolist() == [0, 2] and out[1][:2].tolist() == [3, 4]
        # a keyframe whose table belongs to another store
        other = pkg.MapPointStore(gpu_handle, 64)
        try:
            with pytest.raises(pkg.OrbxError) as e:
                gpu_handle.map_select_points_device(other, keyframes=[[kf]])
            assert e.value.code == -1 and "another store" in str(e.value)
        finally:
            other.close()
    finally:
        gpu_handle.synchronize()
        kf.close(); mp.close()


# ---- the selection -------------------------------------------------------------------------------------------------------

def test_known_answers(gpu_handle, pkg):
    import torch
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "map_store_known_answers.json")))
    pos = np.array(k["positions"]); desc = np.arange(12 * 32, dtype=np.uint32).astype(np.uint8).reshape(12, 32)
    w = _World(gpu_handle, pkg, pos, desc, k["live"], capacity=k["capacity"])
    try:
        kfs = [w.keyframe(np.array(t, np.int32)) for t in k["tables"]]
        off, ls, p, d = _select(gpu_handle, w.mp, keyframes=[kfs])
        assert off.tolist() == [0, 5] and ls.tolist() == k["select_keyframes"] and _same((p, d), S.gathered(ls, pos, desc))
        off, ls, p, d = _select(gpu_handle, w.mp, src_slots=_d(np.array(k["src"], np.int32)), src_offsets=[0, len(k["src"])])
        assert off.tolist() == [0, 5] and ls.tolist() == k["select_slots"] and _same((p, d), S.gathered(ls, pos, desc))
    finally:
        w.close()


@pytest.mark.parametrize("total", TOTALS)
def test_candidate_totals_at_the_chunk_edges(gpu_handle, pkg, rows, total):
    """exactly `total` candidates over three keyframes: a slot first seen as candidate 0 and again next to the end (the first
    and the last chunk), a slot first seen as the very last candidate; then a second frame beside it, and the call repeated"""
    tables, live = M.tables_with_total(7 + total, total)
    w = _World(gpu_handle, pkg, rows[0], rows[1], live)
    try:
        kfs = [w.keyframe(t) for t in tables]
        want = _expected_lists([tables], live, *rows)
        got = _select(gpu_handle, w.mp, keyframes=[kfs])
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and _same(got, want)
        assert _same(_select(gpu_handle, w.mp, keyframes=[kfs]), want)                                  # the tables were put back
        want2 = _expected_lists([tables[::-1], tables, tables[1:]], live, *rows)
        assert _same(_select(gpu_handle, w.mp, keyframes=[kfs[::-1], kfs, kfs[1:]]), want2)
        # the same candidates as a slot source: no de-duplication
        src = np.concatenate(tables + [np.zeros(0, np.int32)]).astype(np.int32)
        ls = S.select_slots(src, live)
        got = _select(gpu_handle, w.mp, src_slots=_d(np.concatenate([src, [0]]).astype(np.int32)), src_offsets=[0, total])
        assert got[0].tolist() == [0, len(ls)] and _same(got[1:], (ls,) + S.gathered(ls, *rows))
    finally:
        w.close()


def test_degenerate_sources(gpu_handle, pkg, rows):
    live = np.zeros(M.CAPACITY, np.uint8); live[[5, 6, 4000]] = 1
    w = _World(gpu_handle, pkg, rows[0], rows[1], live)
    try:
        same = w.keyframe(np.full(1500, 4000, np.int32)); none = w.keyframe(np.full(70, -1, np.int32)); dead = w.keyframe(np.arange(100, 1300, dtype=np.int32))
        empty = w.keyframe(np.zeros(0, np.int32)); bare = w.keyframe(None, n=40); some = w.keyframe(np.array([6, -1, 5, 6], np.int32))
        frames = [[same], [none], [dead], [empty], [], [bare], [bare, empty, some, same], [some]]
        tabs = {same: np.full(1500, 4000), none: [-1] * 70, dead: np.arange(100, 1300), empty: [], bare: None, some: [6, -1, 5, 6]}
        want = _expected_lists([[tabs[k] for k in f] for f in frames], live, *rows)
        assert want[0].tolist() == [0, 1, 1, 1, 1, 1, 1, 4, 6] and want[1].tolist() == [4000, 6, 5, 4000, 6, 5]
        got = _select(gpu_handle, w.mp, keyframes=frames)
        assert got[0].tolist() == want[0].tolist() and _same(got, want)
        for b, f in enumerate(frames):                                        # every frame alone gives its own bytes
            one = _select(gpu_handle, w.mp, keyframes=[f])
            s = slice(want[0][b], want[0][b + 1])
            assert one[0].tolist() == [0, s.stop - s.start] and _same(one[1:], [x[s] for x in want[1:]])
        some.set_map_point_slots(w.mp, None)                                   # cleared: all -1 again
        assert _select(gpu_handle, w.mp, keyframes=[[some]])[0].tolist() == [0, 0]
        # slot sources: repeats kept twice, -1 and dead slots dropped, an empty frame in the middle
        src = np.array([5, 5, -1, 77, 6, 5, 4000, 9, 9], np.int32)
        got = _select(gpu_handle, w.mp, src_slots=_d(src), src_offsets=[0, 6, 6, 9])
        assert got[0].tolist() == [0, 4, 4, 5] and got[1].tolist() == [5, 5, 6, 5, 4000] and _same(got[2:], S.gathered(got[1], *rows))
    finally:
        w.close()


def test_erase_removes_exactly_those_entries(gpu_handle, pkg, rows):
    tables, live = M.tables_with_total(3, 1500)
    w = _World(gpu_handle, pkg, rows[0], rows[1], live)
    try:
        kfs = [w.keyframe(t) for t in tables]
        before = _select(gpu_handle, w.mp, keyframes=[kfs])
        gone = before[1][[0, 7, 8, len(before[1]) // 2, len(before[1]) - 1]]
        w.mp.erase(gone)
        live2 = live.copy(); live2[gone] = 0
        after = _select(gpu_handle, w.mp, keyframes=[kfs])
        assert _same(after, _expected_lists([tables], live2, *rows))
        assert after[1].tolist() == [s for s in before[1].tolist() if s not in set(gone.tolist())]       # nothing else moved
        w.mp.set(gone[:2], rows[0][:2], rows[1][:2])                          # back, with other rows
        pos3, desc3 = rows[0].copy(), rows[1].copy(); pos3[gone[:2]] = rows[0][:2]; desc3[gone[:2]] = rows[1][:2]
        live2[gone[:2]] = 1
        assert _same(_select(gpu_handle, w.mp, keyframes=[kfs]), _expected_lists([tables], live2, pos3, desc3))
    finally:
        w.close()


# ---- tracking from the store ---------------------------------------------------------------------------------------------

def _frame_tensors(frames):
    """frames [(kp, desc, search, prior)] -> the feature arguments of the device forms"""
    cat = lambda parts, empty: np.concatenate(parts) if sum(len(p) for p in parts) else empty
    kp = cat([f[0] for f in frames], np.zeros(1, G.KEYPOINT)).view(np.float32).reshape(-1, 7).copy()
    desc = cat([f[1] for f in frames], np.zeros((1, 32), np.uint8))
    fc = np.array([len(f[0]) for f in frames], np.int32)
    fs = (np.cumsum(fc) - fc).astype(np.int32)
    return dict(kp=_d(kp), desc=_d(desc), feat_start=_d(fs), feat_count=_d(fc), max_feat=int(fc.max()), search_poses_wc=_d(np.stack([f[2] for f in frames])),
                priors_wc=_d(np.stack([f[3] for f in frames])))


def _np(pkg, o):
    import torch
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in o.items()}
    r["pnp_results"] = r["pnp_results"].view(pkg.PNP_RESULT).reshape(-1)
    r["results"] = r["results"].view(pkg.TRACK_RESULT).reshape(-1)
    return r


def _check_against_track_frames_device(h, pkg, cam, w, frames, r, lists, mode):
    """r: map_track_frames_device's outputs; lists: the spec's list per frame.  Everything equals track_frames_device on the
    spec's gathered rows, and matched_slot the spec's mapping."""
    off = np.zeros(len(lists) + 1, np.int32); off[1:] = np.cumsum([len(x) for x in lists])
    cat = np.concatenate(lists + [np.zeros(0, np.int32)]).astype(np.int32)
    n = int(off[-1])
    assert r["list_offsets"].tolist() == off.tolist() and r["list_slot"][:n].tolist() == cat.tolist()
    pos, de = S.gathered(cat, w.positions, w.desc)
    assert r["positions"][:n].tobytes() == pos.tobytes() and r["mp_desc"][:n].tobytes() == de.tobytes()
    a = _frame_tensors(frames)
    ref = _np(pkg, h.track_frames_device(cam, positions=_d(np.concatenate([pos, np.zeros((1, 3))])), mp_desc=_d(np.concatenate([de, np.zeros((1, 32), np.uint8)])),
                                         mp_offsets=off, cfg=pkg.TrackConfig.for_mode(mode), **a))
    assert r["offsets"].tolist() == ref["offsets"].tolist()
    for b, f in enumerate(frames):
        nf = len(f[0])
        assert _frame_bytes_device(r, b, nf) == _frame_bytes_device(ref, b, nf), (mode, b)
        assert r["matched_slot"][b].tolist() == S.matched_slot(ref["matched"][b], lists[b]).tolist(), (mode, b)
    return ref


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n_kf", [1, 4, 11])
def test_map_track_frames_device_equals_track_frames_device(gpu_handle, pkg, cam, mode, n_kf):
    """one frame over 1 / 4 / 11 keyframes, beside a frame without keyframes (an empty list: TOO_FEW_CORRESPONDENCES)"""
    sc = M.scene(50 + n_kf, 300, 420, n_kf)
    st = sc["store"]
    w = _World(gpu_handle, pkg, st.positions, st.desc, st.live)
    try:
        kfs = [w.keyframe(t) for t in sc["tables"]]
        f0 = sc["frame"]
        frames = [f0, G.frame(3, 4, 30)[:2] + f0[2:]]
        lists = [S.select_keyframes(sc["tables"], st.live), np.zeros(0, np.int32)]
        r = _np(pkg, gpu_handle.map_track_frames_device(cam, w.mp, keyframes=[kfs, []], cfg=pkg.TrackConfig.for_mode(mode), **_frame_tensors(frames)))
        _check_against_track_frames_device(gpu_handle, pkg, cam, w, frames, r, lists, mode)
        assert r["results"]["status"].tolist() == [pkg.TRACK_OK, pkg.TRACK_TOO_FEW_CORRESPONDENCES] and int(r["results"][0]["n_inliers"]) > 100
        assert (r["matched_slot"][1] == -1).all() and (r["matched_slot"][0] >= 0).sum() > 100
    finally:
        w.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_batch_sharing_keyframes_each_frame_as_alone_and_twice_the_same(gpu_handle, pkg, cam, mode):
    store, scs, frames_kf = M.shared_batch()
    w = _World(gpu_handle, pkg, store.positions, store.desc, store.live)
    try:
        kf = [[w.keyframe(t) for t in sc["tables"]] for sc in scs]
        frames = [scs[0]["frame"], scs[1]["frame"], scs[0]["frame"]]
        kfs = [[kf[s][k] for s, k in fk] for fk in frames_kf]
        lists = [S.select_keyframes([scs[s]["tables"][k] for s, k in fk], store.live) for fk in frames_kf]
        cfg = pkg.TrackConfig.for_mode(mode)
        run = lambda fr, ks: _np(pkg, gpu_handle.map_track_frames_device(cam, w.mp, keyframes=ks, cfg=cfg, **_frame_tensors(fr)))
        r = run(frames, kfs)
        _check_against_track_frames_device(gpu_handle, pkg, cam, w, frames, r, lists, mode)
        assert r["results"]["status"].tolist() == [pkg.TRACK_OK] * 3
        again = run(frames, kfs)
        n = int(r["list_offsets"][-1])                                        # (rows behind the lists' and the correspondences' ends are not written)
        assert again["list_offsets"].tolist() == r["list_offsets"].tolist() and again["offsets"].tolist() == r["offsets"].tolist()
        assert all(again[k][:n].tobytes() == r[k][:n].tobytes() for k in ("list_slot", "positions", "mp_desc")) and again["matched_slot"].tobytes() == r["matched_slot"].tobytes()
        assert all(_frame_bytes_device(again, b, len(f[0])) == _frame_bytes_device(r, b, len(f[0])) for b, f in enumerate(frames))
        for b in range(3):
            one = run(frames[b:b + 1], kfs[b:b + 1])
            s = slice(int(r["list_offsets"][b]), int(r["list_offsets"][b + 1]))
            nf = len(frames[b][0])
            assert _frame_bytes_device(one, 0, nf) == _frame_bytes_device(r, b, nf), b
            assert one["list_slot"][:s.stop - s.start].tolist() == r["list_slot"][s].tolist() and one["matched_slot"][0, :nf].tolist() == r["matched_slot"][b, :nf].tolist()
    finally:
        w.close()


def test_matched_slot_chains_into_the_next_call(gpu_handle, pkg, cam):
    """track_local_map from keyframes, then track_with_motion_model from the slots it matched: the second call's source is the
    first call's matched_slot where it lies"""
    sc = M.scene(71, 260, 380, 5)
    st = sc["store"]
    w = _World(gpu_handle, pkg, st.positions, st.desc, st.live)
    try:
        kfs = [w.keyframe(t) for t in sc["tables"]]
        f = sc["frame"]
        frames = [f, (f[0], f[1], f[2], f[2])]
        a = _frame_tensors(frames)
        first = gpu_handle.map_track_frames_device(cam, w.mp, keyframes=[kfs, kfs[::-1]], cfg=pkg.TrackConfig.for_mode(1), **a)
        mf = a["max_feat"]
        second = gpu_handle.map_track_frames_device(cam, w.mp, src_slots=first["matched_slot"].reshape(-1), src_offsets=np.arange(3) * mf,
                                                    cfg=pkg.TrackConfig.for_mode(0), **a)
        r1, r2 = _np(pkg, first), _np(pkg, second)
        lists1 = [S.select_keyframes(sc["tables"], st.live), S.select_keyframes(sc["tables"][::-1], st.live)]
        ref1 = _check_against_track_frames_device(gpu_handle, pkg, cam, w, frames, r1, lists1, 1)
        lists2 = [S.select_slots(S.matched_slot(ref1["matched"][b], lists1[b]), st.live) for b in range(2)]
        assert all(len(x) > 100 for x in lists2)
        _check_against_track_frames_device(gpu_handle, pkg, cam, w, frames, r2, lists2, 0)
        assert r2["results"]["status"].tolist() == [pkg.TRACK_OK] * 2
    finally:
        w.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_host_form_equals_device_form(gpu_handle, pkg, cam, mode):
    store, scs, frames_kf = M.shared_batch()
    w = _World(gpu_handle, pkg, store.positions, store.desc, store.live)
    try:
        kf = [[w.keyframe(t) for t in sc["tables"]] for sc in scs]
        frames = [scs[0]["frame"], scs[1]["frame"], scs[0]["frame"]]
        kfs = [[kf[s][k] for s, k in fk] for fk in frames_kf]
        cfg = pkg.TrackConfig.for_mode(mode)
        r = _np(pkg, gpu_handle.map_track_frames_device(cam, w.mp, keyframes=kfs, cfg=cfg, **_frame_tensors(frames)))
        host = gpu_handle.map_track_frames(cam, w.mp, frames, keyframes=kfs, cfg=cfg)
        srcs = []
        for b, (t, ls, ms) in enumerate(host):
            nf = len(frames[b][0])
            assert _frame_bytes_host(pkg, t) == _frame_bytes_device(r, b, nf), b
            assert ls.tolist() == r["list_slot"][r["list_offsets"][b]:r["list_offsets"][b + 1]].tolist() and ms.tolist() == r["matched_slot"][b, :nf].tolist()
            srcs.append(ms)
        # the slot source in host memory
        mf = max(len(f[0]) for f in frames)
        src = np.full((3, mf), -1, np.int32)
        for b, ms in enumerate(srcs):
            src[b, :len(ms)] = ms
        r2 = _np(pkg, gpu_handle.map_track_frames_device(cam, w.mp, src_slots=_d(src.reshape(-1)), src_offsets=np.arange(4) * mf, cfg=cfg, **_frame_tensors(frames)))
        for b, (t, ls, ms) in enumerate(gpu_handle.map_track_frames(cam, w.mp, frames, src_slots=srcs, cfg=cfg)):
            nf = len(frames[b][0])
            assert _frame_bytes_host(pkg, t) == _frame_bytes_device(r2, b, nf), b
            assert ls.tolist() == r2["list_slot"][r2["list_offsets"][b]:r2["list_offsets"][b + 1]].tolist() and ms.tolist() == r2["matched_slot"][b, :nf].tolist()
    finally:
        w.close()


def test_map_track_reference_device_equals_keyframe_track_reference(gpu_handle, pkg):
    """the reference-keyframe form: valid and positions made on the device from the slot tables equal the spec's rows, and every
    output equals keyframe_track_reference's on those rows.  Invalid features are -1 or a slot that is not live; frames 0 and 2
    share a keyframe; a keyframe without a table matches but has no correspondences."""
    import torch
    frames = R.batches()["b3_shared_keyframe"] + [R.ref_frame(91, 50, 80)]
    cam = pkg.CameraModel(**R.CAMERA)
    rng = np.random.default_rng(17)
    st = M.Store()
    free = rng.permutation(M.CAPACITY)
    tables, used = {}, 0
    for f in frames[:2]:
        n = len(f[2])
        t = free[used:used + n].astype(np.int32); used += n
        ok = np.asarray(f[4]) != 0
        st.set(t[ok], np.asarray(f[3])[ok], np.zeros((int(ok.sum()), 32), np.uint8))
        t[~ok & (rng.uniform(size=n) < 0.5)] = -1                             # the other invalid ones keep a slot that is not live
        tables[id(f)] = t
    w = _World(gpu_handle, pkg, st.positions, st.desc, st.live)
    try:
        ka, kb = w.keyframe(tables[id(frames[0])], desc=frames[0][2]), w.keyframe(tables[id(frames[1])], desc=frames[1][2])
        kc = w.keyframe(None, n=len(frames[3][2]), desc=frames[3][2])
        kfs = [ka, kb, ka, kc]
        tabs = [tables[id(frames[0])], tables[id(frames[1])], tables[id(frames[0])], np.full(len(frames[3][2]), -1, np.int32)]
        rows = [S.reference_rows(t, st.live, st.positions) for t in tabs]
        for f, (p, v) in list(zip(frames, rows))[:3]:
            assert v.tolist() == np.asarray(f[4]).tolist() and p[v == 1].tobytes() == np.asarray(f[3])[v == 1].tobytes()
        kp = np.concatenate([f[0] for f in frames]).view(np.float32).reshape(-1, 7).copy()
        fc = np.array([len(f[0]) for f in frames], np.int32)
        a = dict(kp=_d(kp), desc=_d(np.concatenate([f[1] for f in frames])), feat_start=_d((np.cumsum(fc) - fc).astype(np.int32)), feat_count=_d(fc),
                 max_feat=int(fc.max()), priors_wc=_d(np.stack([f[5] for f in frames])))
        got = gpu_handle.map_track_reference_device(cam, w.mp, kfs, **a)
        want = gpu_handle.keyframe_track_reference(cam, kfs, a["kp"], a["desc"], a["feat_start"], a["feat_count"], a["max_feat"], [r[0] for r in rows],
                                                   [r[1] for r in rows], a["priors_wc"])
        torch.cuda.synchronize()
        g = {k: v.cpu().numpy() for k, v in got.items()}; x = {k: v.cpu().numpy() for k, v in want.items()}
        assert g["kf_positions"].tobytes() == np.concatenate([r[0] for r in rows]).tobytes() and g["kf_valid"].tobytes() == np.concatenate([r[1] for r in rows]).tobytes()
        n = int(x["offsets"][-1])
        assert g["offsets"].tolist() == x["offsets"].tolist() and n > 30
        for k in ("points3d", "points2d", "kf_idx", "feat_idx", "inlier", "err"):
            assert g[k][:n].tobytes() == x[k][:n].tobytes(), k
        for k in ("poses", "pnp_results", "results"):
            assert g[k].tobytes() == x[k].tobytes(), k
        res = x["results"].view(pkg.TRACK_REF_RESULT).reshape(-1)
        ko = np.cumsum([0] + [k.n for k in kfs])
        for b in range(4):
            nm = int(res[b]["n_matches"])
            assert g["matches"][ko[b]:ko[b] + nm].tobytes() == x["matches"][ko[b]:ko[b] + nm].tobytes()
        assert int(res[3]["n_matches"]) > 0 and int(res[3]["n_correspondences"]) == 0 and int(res[0]["n_correspondences"]) >= 4
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.map_track_reference_device(cam, w.mp, kfs, min_correspondences=3, **a)
        assert e.value.code == -1 and "orbx_map_track_reference_device" in str(e.value)
    finally:
        w.close()


def test_track_configurations_are_refused_before_anything_runs(gpu_handle, pkg, cam):
    sc = M.scene(52, 60, 90, 2)
    st = sc["store"]
    w = _World(gpu_handle, pkg, st.positions, st.desc, st.live)
    try:
        kfs = [w.keyframe(t) for t in sc["tables"]]
        a = _frame_tensors([sc["frame"]])
        for kw in (dict(cfg=pkg.TrackConfig(mode=2)), dict(cfg=pkg.TrackConfig(min_correspondences=3)), dict(pnp_cfg=pkg.PnPConfig(model_points=3))):
            with pytest.raises(pkg.OrbxError) as e:
                gpu_handle.map_track_frames_device(cam, w.mp, keyframes=[kfs], **kw, **a)
            assert e.value.code == -1 and "orbx_map_track_frames_device" in str(e.value)
            with pytest.raises(pkg.OrbxError):
                gpu_handle.map_track_frames(cam, w.mp, [sc["frame"]], keyframes=[kfs], **kw)
        with pytest.raises(pkg.OrbxError):
            gpu_handle.map_track_frames(cam, w.mp, [], keyframes=[])
    finally:
        w.close()
