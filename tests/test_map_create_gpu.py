"""Point creation and removal on the resident map on the GPU against tests/map_create_spec.py.

The neighbour phase alone equals KeyFrame.triangulate_from_neighbors byte for byte on keyframes whose set_map_points flags are the
derived flags (composition: that call is already held to the numpy specification).  With both phases the lists, counts and tables
equal the specification's; a pair within 1e-9 of a gate may fall on either side (tests/test_triangulation_gpu.py's rule, at most
1 % of a scene's pairs: tests/test_map_create_cpu.py), and the tables are then held to the sequential replay of the list the call
gave.  Positions: 1e-9 relative to numpy f64 — that file's tolerance; the stereo phase is the same rotate-and-translate arithmetic.
"""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import covisibility_scenes as V
import covisibility_spec as CS
import map_create_scenes as W
import map_create_spec as S
import map_observations_scenes as OS
import map_store_scenes as M
import map_store_spec as MS
import triangulation_scenes as G
from test_map_create_cpu import build_driver
from test_map_observations_gpu import _world as _obs_world
from test_map_store_gpu import _d, _select
from test_triangulation_gpu import _keyframe

pytestmark = pytest.mark.gpu

POS_TOL = 1e-9
MARGIN = 1e-9


@pytest.fixture(scope="module")
def handle(pkg):
    h = pkg.Handle(pkg.CameraModel(**G.CAMERA), 1000, device=0, max_w=752, max_h=480, max_batch=1)
    yield h
    h.close()


class _CWorld:
    """a store and the keyframes of a creation scene: features, nodes, tables, and set_map_points flags equal to the derived flags"""

    def __init__(self, h, pkg, name):
        self.h, self.pkg, self.w = h, pkg, W.world(name)
        w, sc = self.w, self.w["scene"]
        self.cam = pkg.CameraModel(**sc["camera"])
        self.mp = pkg.MapPointStore(h, W.CAPACITY)
        ls = np.flatnonzero(w["live"]).astype(np.int32)
        self.mp.set(ls, w["positions"][ls], w["desc"][ls])
        self.kfs = []
        for k, (kf, table) in enumerate(zip([sc["current"]] + list(sc["neighbours"]), w["tables"])):
            x = _keyframe(pkg, h, kf, k)
            if len(kf["kp"]):
                x.set_map_points([7 if f else None for f in S.flags(table, w["live"], len(kf["kp"]))])
            if table is not None:
                x.set_map_point_slots(self.mp, table)
            self.kfs.append(x)
        self.cur, self.nbs = self.kfs[0], self.kfs[1:]

    def tables(self):
        return [k.get_map_point_slots() for k in self.kfs]

    def weights(self):
        return self.h.map_covisibility(self.mp, self.kfs, list(range(len(self.kfs))))[0]

    def close(self):
        self.h.synchronize()
        for k in self.kfs:
            k.close()
        self.mp.close()


@pytest.fixture
def world(pkg, handle):
    made = []

    def get(name):
        made.append(_CWorld(handle, pkg, name))
        return made[-1]
    yield get
    for w in made:
        w.close()


def _same_tables(got, want):
    return all(np.asarray(g).tobytes() == np.asarray(w, np.int32).tobytes() for g, w in zip(got, want))


# ---- the table from a device array ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 1024, 1025])
def test_device_table_form_equals_host_form(gpu_handle, pkg, n):
    import torch
    h = gpu_handle
    rng = np.random.default_rng(700 + n)
    cap = 512
    mp = pkg.MapPointStore(h, cap)
    live = np.flatnonzero(rng.random(cap) < 0.7).astype(np.int32)
    mp.set(live, rng.normal(size=(len(live), 3)), rng.integers(0, 256, (len(live), 32), dtype=np.uint8))
    mk = lambda m: pkg.KeyFrame(h, torch.zeros((max(m, 1), 7), dtype=torch.float32, device="cuda"), torch.zeros((max(m, 1), 32), dtype=torch.uint8, device="cuda"), m)
    a, b, other = mk(n), mk(n), mk(300)
    try:
        table = rng.integers(-1, cap, n).astype(np.int32)                  # repeats, -1 and dead slots among them
        if n >= 1024:
            table[1023] = table[3]; table[n - 1] = table[1000]             # a repeat across the 256-feature blocks of the uniq pass
        other.set_map_point_slots(mp, rng.integers(0, cap, 300).astype(np.int32))
        a.set_map_point_slots(mp, table)
        b.set_map_point_slots(mp, _d(table))
        assert b.get_map_point_slots().tobytes() == a.get_map_point_slots().tobytes() == table.tobytes()
        wa = h.map_covisibility(mp, [a, other], [0, 1])[0]
        wb = h.map_covisibility(mp, [b, other], [0, 1])[0]
        assert wa.tobytes() == wb.tobytes() and (n < 1024 or wa[0, 1] > 0)
        wild = table.astype(np.int64)
        if n:
            wild[::3] = rng.choice(np.array([-2, -2 ** 31, cap, cap + 1, 2 ** 31 - 1]), len(wild[::3]))
        b.set_map_point_slots(mp, _d(wild.astype(np.int32)))
        want = np.where((wild >= 0) & (wild < cap), wild, -1).astype(np.int32)
        assert b.get_map_point_slots().tobytes() == want.tobytes()
        a.set_map_point_slots(mp, want)
        assert h.map_covisibility(mp, [a, other], [0, 1])[0].tobytes() == h.map_covisibility(mp, [b, other], [0, 1])[0].tobytes()
    finally:
        h.synchronize()
        for k in (a, b, other):
            k.close()
        mp.close()


# ---- creation ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(W.CASES))
def test_neighbour_phase_alone_equals_the_existing_call(handle, pkg, world, name):
    x = world(name)
    nb, i1, i2, pts, res = x.cur.triangulate_from_neighbors(x.cam, x.nbs)
    before = x.mp.info()["n_live"]
    r = handle.map_create_points(x.cam, x.mp, x.cur, x.nbs, x.w["free_slots"], phases=pkg.MAP_CREATE_NEIGHBOURS)
    assert r["counts"].tolist() == [0, len(nb), len(nb), 0] and len(nb) > 40
    assert r["new_neighbour"].tobytes() == nb.tobytes() and r["new_idx1"].tobytes() == i1.tobytes() and r["new_idx2"].tobytes() == i2.tobytes()
    assert r["new_points"].tobytes() == pts.tobytes() and r["stats"].tobytes() == np.ascontiguousarray(res.per_neighbour, np.int32).tobytes()
    assert r["new_slot"].tobytes() == x.w["free_slots"][:len(nb)].tobytes() and x.mp.info()["n_live"] == before + len(nb)


def _check_both_phases(x, r, spec, what):
    """the host form's dict (nothing truncated) against the specification; returns (the tables read back, the live bytes afterwards)"""
    w, sc = x.w, x.w["scene"]
    near = {(e[0], e[1], e[2]) for e in spec["evaluated"] if e[6] <= MARGIN}
    created, ns = int(r["counts"][2]), int(spec["counts"][0])
    key = lambda d: [(int(t), int(a), int(b)) for t, a, b in zip(d["new_neighbour"], d["new_idx1"], d["new_idx2"])]
    got, want = key(r), key(spec)
    assert r["counts"][0] == ns and r["counts"][3] == 0 and got[:ns] == want[:ns] and all(g[0] == -1 and g[2] == -1 for g in got[:ns])
    assert r["new_slot"].tobytes() == w["free_slots"][:created].tobytes()
    tables = x.tables()
    live = np.array(w["live"], np.uint8, copy=True); live[r["new_slot"]] = 1
    if not near:
        assert r["counts"].tolist() == spec["counts"].tolist() and got == want and r["stats"].tolist() == spec["stats"].tolist()
        assert _same_tables(tables, spec["tables"])
    else:
        # a pair within 1e-9 of a gate may fall on either side: every other pair is the specification's, in its order, and the tables
        # are the sequential replay of the list the call gave
        assert [g for g in got if g not in near] == [g for g in want if g not in near] and abs(len(got) - len(want)) <= len(near)
        replay = S.create_replay(sc["current"], sc["neighbours"], w["tables"], w["live"], w["free_slots"], [g + (None,) for g in got[ns:]])
        assert replay == S.tables_as_points(tables, live)
    by_key = dict(zip(want, spec["new_points"]))
    worst = [0.0, 0.0]
    for i, g in enumerate(got):
        if g in near:
            continue
        e = float(np.linalg.norm(r["new_points"][i] - by_key[g]) / np.linalg.norm(by_key[g]))
        worst[i >= ns] = max(worst[i >= ns], e)
    print("%s: %d stereo + %d pair points, largest position error %.3e (stereo) %.3e (pairs) relative" % (what, ns, created - ns, worst[0], worst[1]))
    assert max(worst) <= POS_TOL
    return tables, live


@pytest.mark.parametrize("name", list(W.CASES))
def test_both_phases_against_spec(handle, pkg, oracle, world, name):
    x = world(name)
    spec = W.expected(oracle, name)
    before = x.mp.info()["n_live"]
    r = handle.map_create_points(x.cam, x.mp, x.cur, x.nbs, x.w["free_slots"])
    tables, live = _check_both_phases(x, r, spec, name)
    created = int(r["counts"][2])
    assert created > 200 and x.mp.info()["n_live"] == before + created
    pos, desc, lv = x.mp.download(r["new_slot"])
    want_desc = x.w["scene"]["current"]["desc"][r["new_idx1"]]
    assert pos.tobytes() == r["new_points"].tobytes() and desc.tobytes() == want_desc.tobytes() and lv.all()
    assert x.weights().tobytes() == CS.weights(tables, live, list(range(len(tables)))).tobytes()      # d_mp_uniq was made again
    y = world(name)                                                        # the same call on a rebuilt world: the same bytes
    r2 = handle.map_create_points(y.cam, y.mp, y.cur, y.nbs, y.w["free_slots"])
    assert all(r[k].tobytes() == r2[k].tobytes() for k in r) and _same_tables(y.tables(), tables)


def test_truncation_at_every_edge(handle, pkg, oracle, world):
    name = "t3_nodes"
    full = W.expected(oracle, name)
    S_, N = int(full["counts"][0]), int(full["counts"][1])
    assert not [e for e in full["evaluated"] if e[6] <= MARGIN]
    for n_free in (0, 1, S_ - 1, S_, S_ + 1, S_ + N - 1, S_ + N, S_ + N + 5):
        x = world(name)
        spec = W.expected(oracle, name, n_free=n_free)
        free = x.w["free_slots"][:n_free]
        before = x.mp.info()["n_live"]
        # through the C ABI, the lists filled with a sentinel: rows past `created` are not written
        counts = np.full(4, -7, np.int32); stats = np.full((3, 4), -7, np.int32)
        li = [np.full(max(n_free, 1) + 2, -7, np.int32) for _ in range(4)]
        pts = np.full((max(n_free, 1) + 2, 3), -7.0)
        cam = x.cam._c(); cfg = pkg.TriangulationConfig()._c()
        rc = handle._L.orbx_map_create_points(handle._h, C.byref(cam), C.byref(cfg), 0, x.mp._p, x.cur._p, handle._kf_array(x.nbs), 3, 3,
                                              free.ctypes.data_as(C.c_void_p) if n_free else None, n_free, counts.ctypes.data_as(C.c_void_p),
                                              *[a.ctypes.data_as(C.c_void_p) for a in li], pts.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(C.c_void_p))
        assert rc == 0
        m = int(counts[2])
        # (a dropped stereo candidate stays unflagged, so below S free slots the neighbour phase finds more pairs: N is the call's own)
        Ni = int(counts[1])
        assert counts.tolist() == spec["counts"].tolist() == [S_, Ni, min(S_ + Ni, n_free), S_ + Ni - min(S_ + Ni, n_free)] and (Ni == N if n_free >= S_ else Ni >= N)
        assert stats.tolist() == spec["stats"].tolist()
        for a, key in zip(li, ("new_slot", "new_neighbour", "new_idx1", "new_idx2")):
            assert a[:m].tobytes() == spec[key].tobytes() and (a[m:] == -7).all(), (n_free, key)
        assert (pts[m:] == -7.0).all() and _same_tables(x.tables(), spec["tables"])
        assert x.mp.info()["n_live"] == before + m and not x.mp.download(x.w["free_slots"][m:])[2].any()        # free slots past `created` stay free


def test_device_form_leaves_the_store_to_the_caller(handle, pkg, oracle, world):
    import torch
    name = "t3_nodes"
    spec = W.expected(oracle, name)
    x, y = world(name), world(name)
    host = handle.map_create_points(y.cam, y.mp, y.cur, y.nbs, y.w["free_slots"])
    before_rows = x.mp.download()
    before = x.mp.info()["n_live"]
    o = handle.map_create_points_device(x.cam, x.mp, x.cur, x.nbs, x.w["free_slots"])
    sel = _select(handle, x.mp, keyframes=[x.kfs])                         # (synchronises)
    assert x.mp.info()["n_live"] == before and all(a.tobytes() == b.tobytes() for a, b in zip(x.mp.download(), before_rows))
    assert _same_tables(x.tables(), spec["tables"])
    assert sel[1].tobytes() == MS.select_keyframes(spec["tables"], x.w["live"]).astype(np.int32).tobytes()      # the new entries are skipped: not live yet
    counts = o["counts"].cpu().numpy()
    m = int(counts[2])
    assert counts.tolist() == host["counts"].tolist() and o["stats"].cpu().numpy().tobytes() == host["stats"].tobytes()
    for k in ("new_slot", "new_neighbour", "new_idx1", "new_idx2", "new_points"):
        assert o[k][:m].cpu().numpy().tobytes() == host[k].tobytes(), k
    x.mp.set_device(x.w["free_slots"][:m], o["new_points"][:m].contiguous(), o["new_desc"][:m].contiguous())
    assert x.mp.info()["n_live"] == before + m and all(a.tobytes() == b.tobytes() for a, b in zip(x.mp.download(), y.mp.download()))
    assert x.weights().tobytes() == y.weights().tobytes()


# ---- removal and culling ------------------------------------------------------------------------------------------------------

def _obs_tables(w):
    return [k.get_map_point_slots() if t is not None else None for k, t in zip(w.kfs, w.tables_in)]


@pytest.mark.parametrize("n_kfs", [3, 11])
def test_remove_and_cull_on_observation_worlds(gpu_handle, pkg, n_kfs):
    h = gpu_handle
    rows = M.random_rows(9)
    seed = 900 + n_kfs
    tables, counts, live = V.world(seed, n_kfs)
    live, lonely = OS.with_unobserved(tables, live)
    rng = np.random.default_rng(seed)
    for which in ("remove", "cull"):
        w = _obs_world(h, pkg, rows, tables, counts, live, seed)
        w.tables_in = tables
        try:
            inside = list(range(n_kfs - 1))                                # the last keyframe is outside kfs[]: it keeps its entries
            t_in = [tables[k] for k in inside]
            ls = rng.permutation(np.flatnonzero(live)).astype(np.int32)
            if which == "remove":
                slots = np.concatenate([ls[:40], ls[:3], np.flatnonzero(live == 0)[:5].astype(np.int32)])      # repeats, and slots that are not live
                want_t, want_live, want_n = S.remove_points(t_in, live, slots)
                got_n = h.map_remove_points(w.mp, [w.kfs[k] for k in inside], slots)
                assert h.map_remove_points(w.mp, [w.kfs[k] for k in inside], slots[:2], count=False) is None     # again: nothing left to clear
            else:
                cand = np.unique(np.concatenate([ls[:len(ls) // 2], [lonely]]))[::-1].astype(np.int32)      # (descending: the order is the candidates')
                min_obs = 2 if n_kfs == 3 else 3                        # (two keyframes inside: nothing has three observers)
                want_c, want_t, want_live, want_n = S.cull_points(t_in, live, cand, min_obs)
                got_c = h.map_cull_points(w.mp, [w.kfs[k] for k in inside], cand, min_obs)
                assert got_c.tobytes() == want_c.tobytes() and 0 < len(want_c) < len(cand) and lonely in want_c.tolist()
                got_n = want_n
            assert got_n == want_n > 0
            got_t = _obs_tables(w)
            for k in inside:
                assert (got_t[k] is None and want_t[k] is None) or got_t[k].tobytes() == want_t[k].tobytes(), k
            last = n_kfs - 1
            assert tables[last] is None or got_t[last].tobytes() == np.asarray(tables[last], np.int32).tobytes()
            assert w.mp.info()["n_live"] == int(want_live.sum()) and w.mp.download()[2].tobytes() == want_live.tobytes()
            full = want_t + [tables[last]]
            q = list(range(n_kfs))
            assert h.map_covisibility(w.mp, w.kfs, q)[0].tobytes() == CS.weights(full, want_live, q).tobytes()  # d_mp_uniq cleared in place; the marks are 0 again
            assert h.map_covisibility(w.mp, w.kfs, q)[0].tobytes() == CS.weights(full, want_live, q).tobytes()
        finally:
            w.close()


def test_cull_after_creation_and_a_removed_slot_handed_back(handle, pkg, oracle, world):
    name = "t3_nodes"
    x = world(name)
    r = handle.map_create_points(x.cam, x.mp, x.cur, x.nbs, x.w["free_slots"])
    tables = x.tables()
    live = np.array(x.w["live"], np.uint8, copy=True); live[r["new_slot"]] = 1
    cand = r["new_slot"][::-1].copy()
    want_c, want_t, want_live, want_n = S.cull_points(tables, live, cand, 2)
    got = handle.map_cull_points(x.mp, x.kfs, cand, 2)
    assert got.tobytes() == want_c.tobytes() and 0 < len(got) < len(cand)
    assert _same_tables(x.tables(), want_t) and x.mp.download()[2].tobytes() == want_live.tobytes()
    assert x.weights().tobytes() == CS.weights(want_t, want_live, list(range(len(want_t)))).tobytes()
    # the culled slots are free again: hand them back (the stereo points had one observer and were culled: they are candidates again)
    again = handle.map_create_points(x.cam, x.mp, x.cur, x.nbs, got)
    m = int(again["counts"][2])
    assert again["counts"][0] == r["counts"][0] and 0 < m == min(int(again["counts"][0] + again["counts"][1]), len(got))
    assert again["new_slot"].tobytes() == got[:m].tobytes()
    t2 = x.tables()
    assert not any(np.isin(t, got[m:]).any() for t in t2)                 # a slot that was not taken again is named by nobody
    for s, nb, a, b in zip(again["new_slot"], again["new_neighbour"], again["new_idx1"], again["new_idx2"]):
        named = {(k, int(i)) for k, t in enumerate(t2) for i in np.flatnonzero(t == s)}
        assert named <= ({(0, int(a))} | ({(1 + int(nb), int(b))} if nb >= 0 else set())) and named, (s, named)


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(handle, pkg, world):
    x = world("t3_nodes")
    free = x.w["free_slots"]
    other_store = pkg.MapPointStore(handle, 64)
    other = pkg.Handle(x.cam, 500, device=0, max_w=752, max_h=480, max_batch=1)
    foreign = _keyframe(pkg, other, x.w["scene"]["neighbours"][0], 99)
    bound = _keyframe(pkg, handle, x.w["scene"]["neighbours"][0], 98)
    bound.set_map_point_slots(other_store, np.full(bound.n, -1, np.int32))
    foreign_store = pkg.MapPointStore(other, 64)
    import torch
    one = lambda: pkg.KeyFrame(handle, torch.zeros((1, 7), dtype=torch.float32, device="cuda"), torch.zeros((1, 32), dtype=torch.uint8, device="cuda"), 1)
    many = [one() for _ in range(257)]                                     # distinct: only the bound on T refuses them
    try:
        before_t, before_s, before_n = x.tables(), x.mp.download(), x.mp.info()["n_live"]
        live_slot = int(np.flatnonzero(x.w["live"])[0])
        far = pkg.TriangulationConfig(); far.max_descriptor_dist = 257
        create = lambda **kw: handle.map_create_points(x.cam, x.mp, kw.get("cur", x.cur), kw.get("nbs", x.nbs), kw.get("free", free), phases=kw.get("phases", 3),
                                                      config=kw.get("config"))
        bad = [lambda: create(nbs=many), lambda: create(config=far), lambda: create(nbs=[x.nbs[0], x.cur]), lambda: create(nbs=[x.nbs[0], x.nbs[0]]),
               lambda: create(nbs=[x.nbs[0], bound]), lambda: create(nbs=[x.nbs[0], foreign]), lambda: create(phases=0), lambda: create(phases=4),
               lambda: create(free=[W.CAPACITY]), lambda: create(free=[-1]), lambda: create(free=[int(free[0]), int(free[1]), int(free[0])]),
               lambda: create(free=[int(free[0]), live_slot]),
               lambda: handle.map_create_points_device(x.cam, x.mp, x.cur, [x.nbs[0], x.cur], free),
               lambda: handle.map_remove_points(x.mp, x.kfs, [W.CAPACITY]), lambda: handle.map_remove_points(x.mp, x.kfs, [-1]),
               lambda: handle.map_remove_points(x.mp, [x.cur, x.cur], [live_slot]), lambda: handle.map_remove_points(x.mp, [x.cur, bound], [live_slot]),
               lambda: handle.map_cull_points(x.mp, x.kfs, [live_slot, live_slot], 3), lambda: handle.map_cull_points(x.mp, x.kfs, [int(free[0])], 3),
               lambda: handle.map_cull_points(x.mp, x.kfs, [W.CAPACITY], 3), lambda: handle.map_cull_points(x.mp, [x.cur, foreign], [live_slot], 3)]
        for i, f in enumerate(bad):
            with pytest.raises(pkg.OrbxError) as e:
                f()
            assert e.value.code == -1, i
        cam = x.cam._c(); cfg = pkg.TriangulationConfig()._c()
        v = np.zeros(8, np.int32).ctypes.data_as(C.c_void_p)
        assert handle._L.orbx_map_create_points(handle._h, C.byref(cam), C.byref(cfg), 0, x.mp._p, x.cur._p, handle._kf_array(x.nbs), 3, 3, v, -1,
                                                v, v, v, v, v, v, v) == -1                                   # n_free < 0
        # the table from a device array: no array, an array that is not 4-byte aligned, a store of another handle
        row = torch.full((x.cur.n + 1,), 5, dtype=torch.int32, device="cuda")
        set_dev = handle._L.orbx_keyframe_set_map_point_slots_device
        assert set_dev(x.cur._p, x.mp._p, None) == -1 and set_dev(x.cur._p, x.mp._p, C.c_void_p(row.data_ptr() + 1)) == -1
        assert set_dev(x.cur._p, foreign_store._p, C.c_void_p(row.data_ptr())) == -1 and set_dev(x.cur._p, None, C.c_void_p(row.data_ptr())) == -1
        assert _same_tables(x.tables(), before_t) and x.mp.info()["n_live"] == before_n
        assert all(a.tobytes() == b.tobytes() for a, b in zip(x.mp.download(), before_s))
        ok = handle.map_create_points(x.cam, x.mp, x.cur, x.nbs, [])       # n_free = 0 is accepted: counts and stats, nothing else
        assert ok["counts"][2] == 0 and ok["counts"][3] == ok["counts"][0] + ok["counts"][1] > 0 and x.mp.info()["n_live"] == before_n
        assert handle.map_remove_points(x.mp, x.kfs, []) == 0 and len(handle.map_cull_points(x.mp, x.kfs, [], 3)) == 0
    finally:
        handle.synchronize(); other.synchronize()
        for k in many:
            k.close()
        foreign.close(); bound.close(); foreign_store.close(); other.close(); other_store.close()


# ---- the C++ mirror -------------------------------------------------------------------------------------------------------------

def test_cpp_driver_equals_the_python_call(handle, pkg, world, tmp_path):
    name = "t3_nodes"
    x = world(name)
    w, sc = x.w, x.w["scene"]
    ls = np.flatnonzero(w["live"]).astype(np.int32)
    with open(tmp_path / "map_create_in.bin", "wb") as f:
        f.write(struct.pack("<4i", W.CAPACITY, len(ls), len(x.kfs), len(w["free_slots"])))
        f.write(ls.tobytes()); f.write(w["positions"][ls].tobytes()); f.write(w["desc"][ls].tobytes()); f.write(w["free_slots"].tobytes())
        for kf, table in zip([sc["current"]] + list(sc["neighbours"]), w["tables"]):
            n = len(kf["kp"])
            node = kf.get("node")
            f.write(struct.pack("<3i", n, int(table is not None), int(node is not None)))
            f.write(np.asarray(kf["pose"], np.float64).tobytes())
            f.write((np.full(n, -1, np.int32) if table is None else table).tobytes())
            f.write(np.ascontiguousarray(kf["kp"]).tobytes()); f.write(np.ascontiguousarray(kf["desc"]).tobytes())
            f.write(np.ascontiguousarray(kf["pts"], np.float64).tobytes()); f.write(np.ascontiguousarray(kf["has"], np.uint8).tobytes())
            f.write((np.zeros(n, np.uint32) if node is None else np.asarray(node, np.uint32)).tobytes())
    exe = build_driver(str(tmp_path))
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "MAP_CREATE_DRIVER_OK" in p.stdout, p.stdout + p.stderr
    blob = open(tmp_path / "map_create_out.bin", "rb").read()
    off = [0]

    def rd(dt, per=1):
        n = struct.unpack_from("<Q", blob, off[0])[0] * per                # (the driver counts rows)
        a = np.frombuffer(blob, dt, n, off[0] + 8)
        off[0] += 8 + n * np.dtype(dt).itemsize
        return a
    r = handle.map_create_points(x.cam, x.mp, x.cur, x.nbs, w["free_slots"])
    assert rd(np.int32).tolist() == [int(r["counts"][0]), int(r["counts"][1]), int(r["counts"][2]), int(r["counts"][3])]
    for key in ("new_slot", "new_neighbour", "new_idx1", "new_idx2"):
        assert rd(np.int32).tobytes() == r[key].tobytes(), key
    assert rd(np.float64, 3).tobytes() == r["new_points"].tobytes() and rd(np.int32).tobytes() == r["stats"].tobytes()
    assert all(rd(np.int32).tobytes() == t.tobytes() for t in x.tables())
    culled = handle.map_cull_points(x.mp, x.kfs, r["new_slot"], 2)
    assert rd(np.int32).tobytes() == culled.tobytes() and len(culled) > 0
    assert all(rd(np.int32).tobytes() == t.tobytes() for t in x.tables())
    pos, desc, live = x.mp.download()
    assert rd(np.uint8).tobytes() == live.tobytes() and rd(np.float64, 3).tobytes() == pos.tobytes() and rd(np.uint8).tobytes() == desc.tobytes()
    assert off[0] == len(blob)
