"""Whole local-mapping sessions on the resident map on the GPU against tests/map_session_spec.py's model: the calls of
process_keyframe in the order a mapper makes them, on one store and one handle, for nine keyframes.

Discrete outputs are equal.  Float outputs are held to the tolerance the existing test of that call uses (new points: POS_TOL and
the near-gate rule of tests/test_map_create_gpu.py; BA: assert_ba_close at 1e-6; the refresh: tests/test_map_point_refresh_gpu.py's
compare; the tracker's PnP: tests/test_pnp_gpu.py's assert_matches_spec); after one passed the model adopts the device's bytes, so
that every later discrete decision is computed from identical inputs on both sides.

host_run(seed) drives a session with the synchronous forms beside the live model, once per seed, and records what the other tests
replay: the device forms chained (byte-equal to the host forms, floats included), BA as a composition on a twin store, a fresh twin
against the session's own store through a read-only panel, refusals in mid-session, two maps alternating on one handle, and a
session on a handle that has made no map call before."""
import types

import numpy as np
import pytest

import map_session_scenes as W
import map_session_spec as S
from conftest import assert_ba_close
from test_ba_collect_gpu import _solve_bytes, _window_arrays
from test_map_create_gpu import MARGIN, POS_TOL
from test_map_point_refresh_gpu import compare as compare_refresh
from test_map_store_gpu import _d, _frame_tensors, _select
from test_pnp_gpu import assert_matches_spec
from test_tracking_gpu import _frame_bytes_host
from test_triangulation_gpu import _keyframe

pytestmark = pytest.mark.gpu

CHECKPOINTS = (1, 4, W.N_KF - 1)
_host = {}


def _new_handle(pkg):
    return pkg.Handle(pkg.CameraModel(**W.CAMERA), 2000, device=0, max_w=752, max_h=480, max_batch=1)


@pytest.fixture(scope="module")
def handle(pkg):
    h = _new_handle(pkg)
    yield h
    h.close()


def _b(x):
    return x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()


class _Device:
    """a store and the session's keyframes on the device; a keyframe has no table until its step"""

    def __init__(self, h, pkg, seed, poses=None):
        self.h, self.pkg, self.sess = h, pkg, W.session(seed)
        self.cam = pkg.CameraModel(**W.CAMERA)
        self.mp = pkg.MapPointStore(h, W.CAPACITY)
        self.kf = [_keyframe(pkg, h, kf if poses is None else dict(kf, pose=poses[g]), 100 + g) for g, kf in enumerate(self.sess["keyframes"])]
        self.track_cfg = pkg.TrackConfig.for_mode(1)
        self.ba_cfg = pkg.LocalBAConfigLM(max_covisible_keyframes=W.BA_COVISIBLE)

    def kfs(self, listed):
        return [self.kf[g] for g in listed]

    def state(self):
        """(every keyframe's table, the store's rows, n_live, every keyframe's pose) as bytes"""
        self.h.synchronize()
        pos, desc, live = self.mp.download()
        return (tuple(_b(k.get_map_point_slots()) for k in self.kf), _b(pos), _b(desc), _b(live), self.mp.info()["n_live"], tuple(_b(k.info()["pose_wc"]) for k in self.kf))

    def twin(self, with_table):
        """a new store and new keyframes from the downloaded state: their scratch has never been used"""
        t = _Device(self.h, self.pkg, self.sess["seed"], poses=[k.info()["pose_wc"] for k in self.kf])
        pos, desc, live = self.mp.download()
        ls = np.flatnonzero(live).astype(np.int32)
        t.mp.set(ls, pos[ls], desc[ls])
        for g in with_table:
            t.kf[g].set_map_point_slots(t.mp, self.kf[g].get_map_point_slots())
        return t

    def panel(self, listed, cur, frame):
        """read-only calls of every kind, as bytes"""
        h, kfs = self.h, self.kfs(listed)
        out = list(_select(h, self.mp, keyframes=[kfs]))
        out += list(h.map_covisibility(self.mp, kfs, range(len(kfs)), 3))
        out += list(h.map_observations(self.mp, kfs, np.flatnonzero(self.mp.download()[2]).astype(np.int32)))
        out += list(h.map_keyframe_redundancy(self.mp, kfs, range(len(kfs)), W.KF_MIN_OBS, W.KF_THRESHOLD))
        c = h.map_collect_ba_window(self.mp, kfs, cur, W.BA_COVISIBLE)
        out += [b"empty"] if c is None else [c[k] for k in ("counts", "local_kf", "fixed_kf", "list_slot", "positions", "obs32")]
        t, ls, ms, lk = h.map_track_local(self.cam, self.mp, [frame], kfs, [cur], W.TRACK_NBEST, cfg=self.track_cfg)[0]
        out += list(_frame_bytes_host(self.pkg, t)) + [ls, ms, lk]
        return [_b(x) for x in out]

    def close(self):
        self.h.synchronize()
        for k in self.kf:
            k.close()
        self.mp.close()


def _frame(sess, g):
    kf = sess["keyframes"][g]
    return (kf["kp"], kf["desc"], sess["priors"][g], sess["priors"][g])


# ---- the host forms beside the live model ------------------------------------------------------------------------------------

class _HostForms:
    """map_session_spec.Model.step's `dev`: makes every call with its synchronous form, compares, and returns the floats to adopt"""

    def __init__(self, dev, oracle):
        self.d, self.oracle = dev, oracle
        self.g = -1
        self.rec = dict(states={}, normals={}, ba={}, panels={}, calls=0)

    def _kfs(self, m):
        return self.d.kfs(m.listed)

    def track(self, m, want):
        d = self.d
        t, ls, ms, lk = d.h.map_track_local(d.cam, d.mp, [want["frame"]], self._kfs(m), [want["ref"]], W.TRACK_NBEST, cfg=d.track_cfg)[0]
        assert lk.tobytes() == want["local_kf"].tobytes() and ls.tobytes() == want["list_slot"].tobytes()
        ga = want["gathered"]
        assert t.mp_idx.tobytes() == ga["mp_idx"].tobytes() and t.feat_idx.tobytes() == ga["feat_idx"].tobytes()
        assert t.points3d.tobytes() == ga["points3d"].tobytes() and t.points2d.tobytes() == ga["points2d"].tobytes()
        assert dict(status=t.status, n_in_front=t.n_in_front, n_correspondences=len(t.mp_idx), n_inliers=t.n_inliers) == want["record"]
        if len(t.mp_idx) >= 4:
            assert_matches_spec(types.SimpleNamespace(stats=t.pnp_stats, inlier_mask=t.inlier_mask, reproj_errors=t.reproj_errors, pose=t.pose), want["pnp"])
        else:
            assert t.pose.tobytes() == want["pose"].tobytes()
        assert t.matched.tobytes() == want["matched"].tobytes() and ms.tobytes() == want["matched_slot"].tobytes()

    def table(self, m, want):
        self.g = want["g"]
        self.d.kf[self.g].set_map_point_slots(self.d.mp, _d(want["table"]) if self.g % 2 and len(want["table"]) else want["table"])      # both forms of the table

    def neighbours(self, m, want):
        w, best, cnt = self.d.h.map_covisibility(self.d.mp, self._kfs(m), [want["cur"]], W.N_NEIGHBOURS)
        assert w[0].tobytes() == want["weights"].tobytes() and best[0].tobytes() == want["best"].tobytes() and int(cnt[0]) == want["n_best"]

    def create(self, m, want):
        d, order = self.d, want["order"]
        kfs = self._kfs(m)
        r = d.h.map_create_points(d.cam, d.mp, kfs[order[0]], [kfs[i] for i in order[1:]], want["free_slots"], is_inertial=want["is_inertial"])
        near = {(e[0], e[1], e[2]) for e in want["evaluated"] if e[6] <= MARGIN}
        key = lambda x: [(int(t), int(a), int(b)) for t, a, b in zip(x["new_neighbour"], x["new_idx1"], x["new_idx2"])]
        got, exp = key(r), key(want)
        ns, created = int(want["counts"][0]), int(r["counts"][2])
        assert r["counts"][0] == ns and got[:min(ns, created)] == exp[:min(ns, created)] and r["new_slot"].tobytes() == want["free_slots"][:created].tobytes()
        if not near:
            assert r["counts"].tolist() == want["counts"].tolist() and got == exp and r["stats"].tolist() == want["stats"].tolist()
        else:
            assert [x for x in got if x not in near] == [x for x in exp if x not in near] and abs(len(got) - len(exp)) <= len(near)
        by_key = dict(zip(exp, want["new_points"]))
        worst = max([float(np.linalg.norm(r["new_points"][i] - by_key[x]) / np.linalg.norm(by_key[x])) for i, x in enumerate(got) if x not in near] + [0.0])
        print("step %d: %d stereo + %d pair points of %d evaluated (%d near a gate), dropped %d, largest position error %.3e relative" % (
            self.g, min(ns, created), created - min(ns, created), len(want["evaluated"]), len(near), int(r["counts"][3]), worst))
        assert worst <= POS_TOL
        return r

    def cull(self, m, want):
        got = self.d.h.map_cull_points(self.d.mp, self._kfs(m), want["cand"], W.CULL_MIN_OBS)
        assert got.tobytes() == want["culled"].tobytes()

    def fuse(self, m, want):
        d = self.d
        got = d.h.map_search_in_neighbors(d.cam, d.mp, self._kfs(m), want["cur"], want["nb"], W.RADIUS_SCALE, W.SCALE_RANGE, slot_normals=want["normals_before"])
        assert got["counts"].tobytes() == np.stack([want["a"]["counts"], want["b"]["counts"]]).tobytes()
        for p in "ab":
            assert got["goner_" + p].tobytes() == want[p]["goner"].tobytes() and got["keeper_" + p].tobytes() == want[p]["keeper"].tobytes()
        assert got["affected"].tobytes() == want["affected"].tobytes()
        compare_refresh("step %d refresh" % self.g, got["refresh"], want["refresh"])
        self.rec["normals"][self.g] = _b(got["refresh"].normals)
        return got["refresh"].normals

    def ba(self, m, want):
        d, b, cur = self.d, want["ba"], want["cur"]
        kfs = self._kfs(m)
        tw = d.twin([g for g in range(W.N_KF) if m.tables[g] is not None])
        try:                                                               # the composition on a twin store, before the session's own call
            tk = tw.kfs(m.listed)
            c = d.h.map_collect_ba_window(tw.mp, tk, cur, W.BA_COVISIBLE)
            comp = None
            if c is not None:
                poses_cw, fixed_cw = _window_arrays(d.pkg, dict(poses_wc=[k.info()["pose_wc"] for k in tk]), c)
                comp = _solve_bytes(d.h.ba_solve_visual(d.cam, d.ba_cfg, poses_cw, fixed_cw, c["positions"], c["obs32"]))
        finally:
            tw.close()
        r = d.h.map_local_ba(d.cam, d.mp, kfs, cur, d.ba_cfg)
        if b is None:
            assert r is None and comp is None
            self.rec["ba"][self.g] = None
            return None
        assert r.counts.tobytes() == b["counts"].tobytes() and r.local_kf.tobytes() == b["local_kf"].tobytes() and r.list_slot.tobytes() == b["list_slot"].tobytes()
        assert list(r.optimized_poses) == b["optimised"]
        got = dict(poses_wc=np.array([r.optimized_poses[k] for k in b["optimised"]]).reshape(-1, 7), points=r.points, iterations=r.iterations,
                   initial_error=r.initial_error, final_error=r.final_error)
        self.rec["ba"][self.g] = (_solve_bytes(got), comp, got, b["solve"])
        assert_ba_close(got, b["solve"], 1e-6)
        assert d.mp.download(b["list_slot"])[0].tobytes() == r.points.tobytes()
        for p, pose in r.optimized_poses.items():
            kfs[p].set_pose(pose)
        return got["poses_wc"], got["points"]

    def remove(self, m, want):
        assert self.d.h.map_remove_points(self.d.mp, self._kfs(m), want["slots"]) == want["n_cleared"]

    def redundancy(self, m, want):
        got = self.d.h.map_keyframe_redundancy(self.d.mp, self._kfs(m), want["cand"], W.KF_MIN_OBS, W.KF_THRESHOLD)
        assert all(a.tobytes() == np.asarray(b).tobytes() for a, b in zip(got, (want["total"], want["redundant"], want["cull"])))

    def state(self, m, after):
        """after every call: the tables, the live rows and the count equal the model's"""
        d = self.d
        self.rec["calls"] += 1
        for g, (k, t) in enumerate(zip(d.kf, S.as_arrays(m.tables, m.counts))):
            assert k.get_map_point_slots().tobytes() == t.tobytes(), (after, self.g, g)
        pos, desc, live = d.mp.download()
        on = m.live == 1
        assert live.tobytes() == m.live.tobytes() and d.mp.info() == dict(capacity=W.CAPACITY, n_live=int(on.sum())), (after, self.g)
        assert desc[on].tobytes() == m.desc[on].tobytes() and pos[on].tobytes() == m.positions[on].tobytes(), (after, self.g)


def host_run(h, pkg, oracle, seed):
    """the session of `seed` driven with the host forms against the live model, once -> (model, what it recorded)"""
    if seed not in _host:
        sess = W.session(seed)
        d = _Device(h, pkg, seed)
        try:
            dev = _HostForms(d, oracle)
            m = S.Model(sess, oracle)
            for g in range(W.N_KF):
                m.step(g, dev)
                dev.rec["states"][g] = d.state()
                assert all(d.kf[k].info()["pose_wc"].tobytes() == m.poses_wc[k].tobytes() for k in range(W.N_KF))
                if g in CHECKPOINTS:                                        # a fresh twin against the session's own store
                    tw = d.twin([k for k in range(W.N_KF) if m.tables[k] is not None])
                    try:
                        frame = _frame(sess, (g + 1) % W.N_KF)
                        dev.rec["panels"][g] = (tw.panel(m.listed, len(m.listed) - 1, frame), d.panel(m.listed, len(m.listed) - 1, frame))
                    finally:
                        tw.close()
                    assert d.state() == dev.rec["states"][g]               # the panel changed nothing
            _host[seed] = (m, dev.rec)
        finally:
            d.close()
    return _host[seed]


# ---- the device forms, replayed from a host run's trace ----------------------------------------------------------------------

def replay(d, m, steps=None, wait=True, between=None):
    """a generator: per step every call of the session enqueued back to back in its device form, its arguments taken from the trace
    of the host run's model `m`; one synchronize at the end of the step (none with wait=False), then the step's number is yielded"""
    import torch
    h, cam, mp = d.h, d.cam, d.mp
    for g in range(W.N_KF if steps is None else steps):
        tr = m.trace[g]
        if between is not None:
            between(g, d, tr)
        if "track" in tr:
            a = _frame_tensors([tr["track"]["frame"]])
            o = h.map_track_local_device(cam, mp, d.kfs(tr["listed_before"]), [tr["track"]["ref"]], W.TRACK_NBEST, cfg=d.track_cfg, **a)
            d.kf[g].set_map_point_slots(mp, o["matched_slot"][0].contiguous() if d.kf[g].n else torch.zeros(1, dtype=torch.int32, device="cuda"))
        else:
            d.kf[g].set_map_point_slots(mp, tr["table"])
        kfs, cur, nb = d.kfs(tr["listed"]), tr["cur"], tr["neighbours"]
        out = dict(cov=h.map_covisibility_device(mp, kfs, [cur], W.N_NEIGHBOURS))
        c = tr["create"]
        o = h.map_create_points_device(cam, mp, kfs[cur], [kfs[i] for i in nb], c["free_slots"])
        n = c["created"]
        mp.set_device(c["free_slots"][:n], o["new_points"][:n].contiguous(), o["new_desc"][:n].contiguous())
        out["create"] = o
        if g > 0:
            h.map_remove_points(mp, kfs, tr["cull"]["culled"], count=False)
            f = tr["fuse"]
            out["fuse"] = [h.map_fuse_device(cam, mp, kfs, [cur], nb, W.RADIUS_SCALE), h.map_fuse_device(cam, mp, kfs, nb, [cur], W.RADIUS_SCALE)]
            mp.erase(np.concatenate([f["goner_a"], f["goner_b"]]).astype(np.int32))
            normals = _d(np.ascontiguousarray(f["normals_before"][f["affected"]]))
            out["refresh"] = h.map_refresh_points_device(mp, kfs, f["affected"], W.SCALE_RANGE, normals)
            out["normals"] = normals
            r = h.map_local_ba(cam, mp, kfs, cur, d.ba_cfg, read_points=False)
            assert (r is None) == (tr["ba"] is None)
            if r is not None:
                for p, pose in r.optimized_poses.items():
                    kfs[p].set_pose(pose)
            h.map_remove_points(mp, kfs, tr["outliers"], count=False)
            out["redundancy"] = h.map_keyframe_redundancy_device(mp, kfs, tr["redundancy"]["cand"], W.KF_MIN_OBS, W.KF_THRESHOLD)
        if wait:
            h.synchronize()
        d.last = out
        yield g


@pytest.mark.parametrize("seed", W.SEEDS)
def test_host_forms_step_by_step(handle, pkg, oracle, seed):
    m, rec = host_run(handle, pkg, oracle, seed)
    assert rec["calls"] == 2 + 7 * (W.N_KF - 1) and len(rec["states"]) == W.N_KF
    assert sum(1 for g in range(W.N_KF) if m.stats[g]["dropped"] > 0) >= 1 and sum(m.stats[g]["reused"] for g in range(W.N_KF)) > 100
    assert len(m.unlisted) == W.MAX_UNLISTED and sum(1 for v in rec["ba"].values() if v is not None and v[2]["iterations"] > 0) >= 3


@pytest.mark.parametrize("seed", W.SEEDS)
def test_device_forms_chained_equal_the_host_forms(handle, pkg, oracle, seed):
    m, rec = host_run(handle, pkg, oracle, seed)
    d = _Device(handle, pkg, seed)
    try:
        for g in replay(d, m):
            got, want = d.state(), rec["states"][g]
            for name, a, b in zip(("tables", "positions", "descriptors", "live", "n_live", "poses"), got, want):
                assert a == b, (g, name)
            o = d.last
            assert int(o["create"]["counts"][2]) == m.trace[g]["create"]["created"]
            c = m.trace[g]["cov"]
            assert _b(o["cov"]["weights"][0].cpu().numpy()) == _b(c["weights"]) and _b(o["cov"]["best"][0].cpu().numpy()) == _b(c["best"]), g
            assert int(o["cov"]["n_best"][0]) == c["n_best"], g
            if g > 0:
                f = m.trace[g]["fuse"]
                assert o["fuse"][0]["goner"][:len(f["goner_a"])].cpu().numpy().tobytes() == f["goner_a"].tobytes() and int(o["fuse"][0]["counts"][3]) == len(f["goner_a"])
                assert o["fuse"][1]["goner"][:len(f["goner_b"])].cpu().numpy().tobytes() == f["goner_b"].tobytes() and int(o["fuse"][1]["counts"][3]) == len(f["goner_b"])
                assert _b(o["normals"].cpu().numpy()) == rec["normals"][g], g
                assert all(_b(o["redundancy"][k].cpu().numpy()) == _b(m.trace[g]["redundancy"][k]) for k in ("total", "redundant", "cull")), g
    finally:
        d.close()


@pytest.mark.parametrize("seed", W.SEEDS)
def test_local_ba_is_the_composition_on_a_twin_and_close_to_the_oracle(handle, pkg, oracle, seed):
    m, rec = host_run(handle, pkg, oracle, seed)
    solved = 0
    for g in range(1, W.N_KF):
        if rec["ba"][g] is None:
            assert m.trace[g]["ba"] is None
            continue
        own, comp, got, want = rec["ba"][g]
        assert own == comp, g                                              # bit for bit: collect + ba_solve_visual on a host copy, on a store that never ran a session
        assert_ba_close(got, want, 1e-6)
        solved += got["iterations"] > 0
    assert solved >= 3


@pytest.mark.parametrize("seed", W.SEEDS)
def test_a_fresh_twin_sees_the_same_map(handle, pkg, oracle, seed):
    m, rec = host_run(handle, pkg, oracle, seed)
    assert sorted(rec["panels"]) == list(CHECKPOINTS)
    for g, (twin, own) in rec["panels"].items():
        assert len(twin) == len(own) > 20
        for i, (a, b) in enumerate(zip(twin, own)):
            assert a == b, (g, i)


def _refusals(pkg, other_store):
    def between(g, d, tr):
        """before step 5: one refused call of each kind; every one returns -1"""
        if g != 5:
            return
        h, cam, mp = d.h, d.cam, d.mp
        kfs = d.kfs(tr["listed_before"])
        free = tr["create"]["free_slots"]
        live = np.flatnonzero(mp.download()[2]).astype(np.int32)
        stranger = _keyframe(pkg, h, d.sess["keyframes"][0], 999)
        stranger.set_map_point_slots(other_store, np.full(stranger.n, -1, np.int32))
        K = len(kfs)
        nr = np.zeros((2, 3))
        try:
            bad = [lambda: h.map_create_points(cam, mp, kfs[-1], kfs[:-1], [int(free[0]), int(free[1]), int(free[0])]),
                   lambda: h.map_create_points(cam, mp, kfs[-1], kfs[:-1], [int(free[0]), int(live[0])]),
                   lambda: h.map_create_points_device(cam, mp, kfs[-1], [kfs[0], kfs[-1]], free),
                   lambda: h.map_cull_points(mp, kfs, [int(live[0]), int(live[0])], W.CULL_MIN_OBS), lambda: h.map_cull_points(mp, kfs, [int(free[0])], W.CULL_MIN_OBS),
                   lambda: h.map_remove_points(mp, kfs, [W.CAPACITY]), lambda: h.map_remove_points(mp, kfs + [stranger], [int(live[0])]),
                   lambda: h.map_fuse(cam, mp, kfs, [K], [0], W.RADIUS_SCALE), lambda: h.map_fuse_device(cam, mp, kfs, [0], [1, 1], W.RADIUS_SCALE),
                   lambda: h.map_search_in_neighbors(cam, mp, kfs, K, [0], W.RADIUS_SCALE, W.SCALE_RANGE),
                   lambda: h.map_search_in_neighbors(cam, mp, kfs + [stranger], 0, [1], W.RADIUS_SCALE, W.SCALE_RANGE),
                   lambda: h.map_observations(mp, kfs, [int(live[0]), int(live[0])]), lambda: h.map_observations(mp, kfs, [int(free[0])]),
                   lambda: h.map_refresh_points(mp, kfs, [int(live[0]), int(free[0])], W.SCALE_RANGE, nr),
                   lambda: h.map_keyframe_redundancy(mp, kfs, [K], W.KF_MIN_OBS, W.KF_THRESHOLD), lambda: h.map_keyframe_redundancy(mp, kfs + [stranger], [0], W.KF_MIN_OBS, W.KF_THRESHOLD),
                   lambda: h.map_covisibility(mp, kfs, [K], 2), lambda: h.map_covisibility(mp, kfs + [stranger], [0], 2),
                   lambda: h.map_collect_ba_window(mp, kfs, K, W.BA_COVISIBLE), lambda: h.map_local_ba(cam, mp, kfs + [stranger], 0, d.ba_cfg),
                   lambda: h.map_local_ba(cam, mp, kfs, K, d.ba_cfg),
                   lambda: h.map_track_local(cam, mp, [_frame(d.sess, 5)], kfs, [K], W.TRACK_NBEST, cfg=d.track_cfg),
                   lambda: h.map_track_local(cam, mp, [_frame(d.sess, 5)], kfs + [stranger], [0], W.TRACK_NBEST, cfg=d.track_cfg)]
            for i, f in enumerate(bad):
                with pytest.raises(pkg.OrbxError) as e:
                    f()
                assert e.value.code == -1, i
        finally:
            h.synchronize()
            stranger.close()
    return between


def test_refusals_in_mid_session_leave_no_trace(handle, pkg, oracle):
    seed = W.SEEDS[0]
    m, rec = host_run(handle, pkg, oracle, seed)
    d = _Device(handle, pkg, seed)
    other = pkg.MapPointStore(handle, 64)
    try:
        for g in replay(d, m, between=_refusals(pkg, other)):
            if g >= 4:
                assert d.state() == rec["states"][g], g                    # before the refusals, the step after them, and every later one
        tw = d.twin([k for k in range(W.N_KF) if m.tables[k] is not None])
        try:
            frame = _frame(d.sess, 0)
            own = d.panel(m.listed, len(m.listed) - 1, frame)
            assert tw.panel(m.listed, len(m.listed) - 1, frame) == own == rec["panels"][W.N_KF - 1][1]
        finally:
            tw.close()
    finally:
        handle.synchronize()
        other.close()
        d.close()


def test_two_maps_alternate_on_one_handle(handle, pkg, oracle):
    runs = [host_run(handle, pkg, oracle, seed) for seed in W.SEEDS]
    ds = [_Device(handle, pkg, seed) for seed in W.SEEDS]
    try:
        gens = [replay(d, m, wait=False) for d, (m, _) in zip(ds, runs)]
        for g in range(W.N_KF):
            for gen in gens:                                               # the other map's step is enqueued behind this one's without a wait
                assert next(gen) == g
        for d, (m, rec) in zip(ds, runs):
            assert d.state() == rec["states"][W.N_KF - 1]
    finally:
        for d in ds:
            d.close()


def test_a_session_that_grows_every_workspace(pkg, oracle, handle):
    seed = W.SEEDS[1]
    m, rec = host_run(handle, pkg, oracle, seed)
    h = _new_handle(pkg)                                                   # no map call before: every workspace and pinned slot is allocated and regrown on the way
    try:
        d = _Device(h, pkg, seed)
        try:
            listed, n_live = [], []
            for g in replay(d, m):
                listed.append(len(m.trace[g]["listed"])); n_live.append(d.mp.info()["n_live"])
                assert d.state() == rec["states"][g], g
            assert listed[1] == 2 and max(listed) >= 8 and listed[0] == 1 and sum(k.n for k in d.kf) > 3000
            assert n_live == [rec["states"][g][4] for g in range(W.N_KF)] and max(n_live) > 3 * n_live[0] // 2 and d.mp.info()["capacity"] == W.CAPACITY
        finally:
            d.close()
    finally:
        h.close()
