"""Whole local-mapping sessions on the resident map that switch to the inertial local BA in mid-session, on the GPU against
tests/map_inertial_session_spec.py's model: tests/test_map_session_gpu.py's session with the caller's inertial state beside it.  Steps
1 and 2 run orbx_map_local_ba, every step from IMU_INIT on orbx_map_local_inertial_ba, on the same store and the same handle, whose
BA-window workspaces the visual windows shaped.

Every call of every step is held to the model as the visual session holds it.  The inertial BA's discrete outputs (counts, fixed_kf,
and list_slot and obs32 as orbx_map_collect_inertial_window gives them on the session's store) are byte-equal to the model, its solve
is held to the oracle at tests/test_inertial_ba.py's tolerances (map_inertial_session_spec.assert_solve_close), and it is bit for bit
the composition of the collection and orbx_ba_solve_inertial_obs32 on a twin store that never saw a visual window.  The velocities
and biases a solve returns go to the caller's arrays (the device object's, not the model's) and are the next step's inputs.

host_run(seed) drives a session with the synchronous forms beside the live model, once per seed, and records what the other tests
replay: the device forms chained, visual and inertial windows interleaved on one handle, refusals in mid-session, and a handle whose
first BA is an inertial one."""
import numpy as np
import pytest

import ba_collect_spec as BAS
import inertial_collect_spec as ICS
import map_inertial_session_scenes as I
import map_inertial_session_spec as M
import map_session_scenes as W
from test_inertial_collect_gpu import _solve_bytes as _inertial_bytes
from test_map_session_gpu import _b, _Device, _HostForms, _new_handle
from test_map_store_gpu import _d, _frame_tensors

pytestmark = pytest.mark.gpu

_host = {}
STATE = ("tables", "positions", "descriptors", "live", "n_live", "poses", "velocities", "biases")


@pytest.fixture(scope="module")
def handle(pkg):
    h = _new_handle(pkg)
    yield h
    h.close()


class _IDevice(_Device):
    """the session's store and keyframes, and the caller's inertial state: velocities and biases per keyframe"""

    def __init__(self, h, pkg, seed, poses=None, velocities=None, biases=None):
        super().__init__(h, pkg, seed, poses)
        self.imu = I.inertial(seed)
        self.icfg = pkg.LocalInertialBAConfig(max_iterations=I.INERTIAL_ITERATIONS)
        self.velocities = np.array(self.imu["velocities"] if velocities is None else velocities, copy=True)
        self.biases = np.array(self.imu["biases"] if biases is None else biases, copy=True)

    def state(self):
        return super().state() + (_b(self.velocities), _b(self.biases))

    def twin_on(self, h, with_table):
        """_Device.twin on the handle `h`: a new store and new keyframes from the downloaded state, the caller's arrays copied"""
        t = _IDevice(h, self.pkg, self.sess["seed"], poses=[k.info()["pose_wc"] for k in self.kf], velocities=self.velocities, biases=self.biases)
        pos, desc, live = self.mp.download()
        ls = np.flatnonzero(live).astype(np.int32)
        t.mp.set(ls, pos[ls], desc[ls])
        for g in with_table:
            t.kf[g].set_map_point_slots(t.mp, self.kf[g].get_map_point_slots())
        return t

    def window(self, listed):
        """the inertial window's arguments for the list `listed`: kfs, chain, its keyframes, velocities, biases, edge_kf, preint"""
        chain = I.chain(listed)
        members = [listed[p] for p in chain]
        edge_kf, preint, _ = I.edges(self.imu, members)
        return self.kfs(listed), chain, members, self.velocities[members].copy(), self.biases[members].copy(), edge_kf, preint

    def inertial_ba(self, listed):
        """orbx_map_local_inertial_ba as the mapper calls it: the poses go in with set_pose, velocities and biases to the caller's arrays"""
        kfs, chain, members, vel, bias, edge_kf, preint = self.window(listed)
        r = self.h.map_local_inertial_ba(self.cam, self.mp, kfs, chain, vel, bias, edge_kf, preint, self.icfg)
        if r is not None:
            for p, pose in zip(chain, r["poses_wc"]):
                kfs[p].set_pose(pose)
            self.velocities[members] = r["velocities"]; self.biases[members] = r["biases"]
        return r


def _tabled(m):
    return [g for g in range(W.N_KF) if m.tables[g] is not None]


def _composition(d, tw, listed):
    """orbx_map_collect_inertial_window + orbx_ba_solve_inertial_obs32 on the store `tw` -> (the collection or None, the solve or None)"""
    kfs, chain, members, vel, bias, edge_kf, preint = tw.window(listed)
    c = tw.h.map_collect_inertial_window(tw.mp, kfs, chain)
    if c is None:
        return None, None
    poses_wc = np.array([kfs[p].info()["pose_wc"] for p in chain]).reshape(-1, 7)
    fixed_cw = np.array([d.pkg.se3_inverse(kfs[k].info()["pose_wc"]) for k in [chain[0]] + c["fixed_kf"].tolist()]).reshape(-1, 7)
    return c, tw.h.ba_solve_inertial_obs32(tw.cam, d.icfg, poses_wc, vel, bias, fixed_cw, c["positions"], c["obs32"], edge_kf, preint)


class _InertialHostForms(_HostForms):
    """_HostForms whose BA step is the inertial one from IMU_INIT on; keeps every float the model adopts and the inertial windows'
    discrete outputs (rec["device"][step][call][field]).  tests/golden/map_inertial_session_device_seed2.npz is seed 2's, saved with
    numpy.savez_compressed under the keys "<step>.<call>.<field>", for tests/test_map_inertial_session_cpu.py."""

    def __init__(self, dev, oracle):
        super().__init__(dev, oracle)
        self.rec.update(device={}, inertial={})

    def _keep(self, name, **arrays):
        self.rec["device"].setdefault(self.g, {})[name] = {k: np.array(v, copy=True) for k, v in arrays.items()}

    def create(self, m, want):
        r = super().create(m, want)
        self._keep("create", **{k: r[k] for k in ("counts", "new_slot", "new_neighbour", "new_idx1", "new_idx2", "new_points")})
        return r

    def fuse(self, m, want):
        normals = super().fuse(m, want)
        self._keep("fuse", normals=normals)
        return normals

    def ba(self, m, want):
        if not m.imu_initialized(self.g):
            got = super().ba(m, want)
            if got is not None:
                self._keep("ba", poses_wc=got[0], points=got[1])
            return got
        d, b = self.d, want["ba"]
        tw = d.twin_on(d.h, _tabled(m))                                     # the composition on a twin store, before the session's own call
        try:
            c, comp = _composition(d, tw, m.listed)
        finally:
            tw.close()
        own = d.h.map_collect_inertial_window(d.mp, d.kfs(m.listed), I.chain(m.listed))
        before = d.mp.download()
        r = d.inertial_ba(m.listed)
        if b is None:
            assert r is None and c is None and own is None
            self.rec["inertial"][self.g] = None
            return None
        assert b["chain"] == I.chain(m.listed) and m.trace[self.g]["inertial"]["preint"].tobytes() == d.window(m.listed)[6].tobytes()
        for k in ("counts", "fixed_kf"):
            assert r[k].tobytes() == b[k].tobytes() == c[k].tobytes() == own[k].tobytes(), (self.g, k)
        for k in ("list_slot", "obs32"):
            assert own[k].tobytes() == b[k].tobytes() == c[k].tobytes(), (self.g, k)
        pos, desc, live = d.mp.download()
        P = b["list_slot"]
        got = dict(r, points=pos[P])
        rest = np.setdiff1d(np.arange(W.CAPACITY), P)
        assert pos[rest].tobytes() == before[0][rest].tobytes() and desc.tobytes() == before[1].tobytes() and live.tobytes() == before[2].tobytes(), self.g
        self.rec["inertial"][self.g] = (_inertial_bytes(got), _inertial_bytes(comp), got, b["solve"])
        M.assert_solve_close(got, b["solve"], "seed %d step %d" % (d.sess["seed"], self.g))
        self._keep("ba", counts=r["counts"], fixed_kf=r["fixed_kf"], list_slot=own["list_slot"], obs32=own["obs32"].view(np.uint8), iterations=r["iterations"],
                   errors=[r["initial_error"], r["final_error"]], **{k: got[k] for k in M.E.OUTPUTS})
        b["imu"] = dict(velocities=r["velocities"], biases=r["biases"])     # the model adopts them with the poses
        return r["poses_wc"], got["points"]


def host_run(h, pkg, oracle, seed):
    """the session of `seed` driven with the host forms against the live model, once -> (model, what it recorded)"""
    if seed not in _host:
        d = _IDevice(h, pkg, seed)
        try:
            dev = _InertialHostForms(d, oracle)
            m = M.Model(W.session(seed), oracle)
            for g in range(W.N_KF):
                m.step(g, dev)
                dev.rec["states"][g] = d.state()
                assert all(d.kf[k].info()["pose_wc"].tobytes() == m.poses_wc[k].tobytes() for k in range(W.N_KF)), g
                assert d.velocities.tobytes() == m.velocities.tobytes() and d.biases.tobytes() == m.biases.tobytes(), g
            _host[seed] = (m, dev.rec)
        finally:
            d.close()
    return _host[seed]


# ---- the device forms, replayed from a host run's trace ----------------------------------------------------------------------

def replay(d, m, start=0, steps=None, between=None):
    """test_map_session_gpu.replay with the session's switch: per step every call enqueued back to back in its device form, its
    arguments from the trace of the host run's model `m`, the BA the inertial one from IMU_INIT on; one synchronize per step, then
    the step's number is yielded.  between(g, d, tr) runs before step g's calls."""
    import torch
    h, cam, mp = d.h, d.cam, d.mp
    for g in range(start, W.N_KF if steps is None else steps):
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
        h.map_covisibility_device(mp, kfs, [cur], W.N_NEIGHBOURS)
        c = tr["create"]
        o = h.map_create_points_device(cam, mp, kfs[cur], [kfs[i] for i in nb], c["free_slots"], is_inertial=m.imu_initialized(g))
        n = c["created"]
        mp.set_device(c["free_slots"][:n], o["new_points"][:n].contiguous(), o["new_desc"][:n].contiguous())
        if g > 0:
            h.map_remove_points(mp, kfs, tr["cull"]["culled"], count=False)
            f = tr["fuse"]
            h.map_fuse_device(cam, mp, kfs, [cur], nb, W.RADIUS_SCALE); h.map_fuse_device(cam, mp, kfs, nb, [cur], W.RADIUS_SCALE)
            mp.erase(np.concatenate([f["goner_a"], f["goner_b"]]).astype(np.int32))
            h.map_refresh_points_device(mp, kfs, f["affected"], W.SCALE_RANGE, _d(np.ascontiguousarray(f["normals_before"][f["affected"]])))
            if m.imu_initialized(g):
                r = d.inertial_ba(tr["listed"])
                assert (r is None) == (tr["ba"] is None) and (r is None or r["counts"].tobytes() == tr["ba"]["counts"].tobytes())
            else:
                r = h.map_local_ba(cam, mp, kfs, cur, d.ba_cfg, read_points=False)
                assert (r is None) == (tr["ba"] is None)
                for p, pose in ({} if r is None else r.optimized_poses).items():
                    kfs[p].set_pose(pose)
            h.map_remove_points(mp, kfs, tr["outliers"], count=False)
            h.map_keyframe_redundancy_device(mp, kfs, tr["redundancy"]["cand"], W.KF_MIN_OBS, W.KF_THRESHOLD)
        h.synchronize()
        yield g


def _assert_state(got, want, g, live_only=False):
    """live_only: a twin's store holds the live rows alone, the session's keeps what an erased point left behind"""
    for name, a, b in zip(STATE, got, want):
        if live_only and name in ("positions", "descriptors"):
            on = np.frombuffer(want[STATE.index("live")], np.uint8) == 1
            a, b = (np.frombuffer(x, np.uint8).reshape(W.CAPACITY, -1)[on].tobytes() for x in (a, b))
        assert a == b, (g, name)


@pytest.mark.parametrize("seed", I.SEEDS)
def test_host_forms_step_by_step(handle, pkg, oracle, seed):
    m, rec = host_run(handle, pkg, oracle, seed)
    assert rec["calls"] == 2 + 7 * (W.N_KF - 1) and len(rec["states"]) == W.N_KF and len(m.unlisted) == W.MAX_UNLISTED
    assert sorted(rec["ba"]) == list(range(1, I.IMU_INIT)) and sorted(rec["inertial"]) == list(range(I.IMU_INIT, W.N_KF))
    assert all(rec["ba"][g][2]["iterations"] > 0 for g in rec["ba"])
    st = [m.stats[g]["inertial"] for g in rec["inertial"]]
    assert sum(1 for g in rec["inertial"] if rec["inertial"][g][2]["iterations"] > 0) >= 4
    assert any(s["skip"] for s in st) and any(s["blind"] for s in st) and any(s["F"] == 1 for s in st) and any(s["F"] >= 3 for s in st)
    assert all(0.0 < s["stereo"] < 1.0 for s in st) and max(s["third"] for s in st) >= 1


@pytest.mark.parametrize("seed", I.SEEDS)
def test_inertial_ba_is_the_composition_on_a_twin_that_saw_no_visual_window(handle, pkg, oracle, seed):
    m, rec = host_run(handle, pkg, oracle, seed)
    for g in range(I.IMU_INIT, W.N_KF):
        own, comp, got, want = rec["inertial"][g]
        assert own == comp, g                                              # outputs, iterations and both errors, bit for bit
        M.assert_solve_close(got, want, "seed %d step %d" % (seed, g))


@pytest.mark.parametrize("seed", I.SEEDS)
def test_device_forms_chained_equal_the_host_forms(handle, pkg, oracle, seed):
    m, rec = host_run(handle, pkg, oracle, seed)
    d = _IDevice(handle, pkg, seed)
    try:
        done = []
        for g in replay(d, m):
            _assert_state(d.state(), rec["states"][g], g)
            done.append(g)
        assert done == list(range(W.N_KF)) and rec["states"][W.N_KF - 1][6] != rec["states"][I.IMU_INIT - 1][6]     # (the velocities moved)
    finally:
        d.close()


def _visual(d, listed):
    r = d.h.map_local_ba(d.cam, d.mp, d.kfs(listed), len(listed) - 1, d.ba_cfg)
    return None if r is None else (r.counts.tobytes(), r.local_kf.tobytes(), r.list_slot.tobytes(), sorted((p, v.tobytes()) for p, v in r.optimized_poses.items()),
                                   r.points.tobytes(), r.iterations, r.initial_error, r.final_error)


def _inertial(d, listed):
    r = d.inertial_ba(listed)
    return None if r is None else tuple(_b(r[k]) for k in ("counts", "fixed_kf", "poses_wc", "velocities", "biases")) + (
        r["iterations"], r["initial_error"], r["final_error"], _b(d.mp.download()[0]))


def test_visual_and_inertial_windows_interleaved_on_one_handle(handle, pkg, oracle):
    seed, at = I.SEEDS[1], I.IMU_INIT + 2
    m, rec = host_run(handle, pkg, oracle, seed)
    snap = m.snap[at]
    listed, tabled = snap["listed"], [g for g in range(W.N_KF) if snap["tables"][g] is not None]
    tables = [snap["tables"][g] for g in listed]
    xy, has = [m.xy[g] for g in listed], [m.kf[g]["has"] for g in listed]
    cur, chain = len(listed) - 1, I.chain(listed)
    want_v = BAS.collect(BAS_tables(tables, [m.counts[g] for g in listed]), xy, snap["live"], cur, W.BA_COVISIBLE)
    want_i = ICS.collect(tables, xy, has, snap["live"], chain)
    alone = []
    d = _IDevice(handle, pkg, seed)
    twins = []
    try:
        assert [g for g in replay(d, m, steps=at + 1)] == list(range(at + 1))
        _assert_state(d.state(), rec["states"][at], at)
        for call in (_visual, _inertial):                                   # each call alone, on a handle that makes no other
            h2 = _new_handle(pkg)
            try:
                t = d.twin_on(h2, tabled)
                try:
                    alone.append(call(t, listed))
                finally:
                    t.close()
            finally:
                h2.close()
        got = []
        for call in (_visual, _inertial, _visual, _inertial):               # one handle, identical inputs: a twin each
            t = d.twin_on(handle, tabled); twins.append(t)
            cv = handle.map_collect_ba_window(t.mp, t.kfs(listed), cur, W.BA_COVISIBLE)
            ci = handle.map_collect_inertial_window(t.mp, t.kfs(listed), chain)
            for k in ("counts", "local_kf", "fixed_kf", "list_slot", "obs32"):
                assert cv[k].tobytes() == want_v[k].tobytes(), (len(got), k)
            for k in ("counts", "fixed_kf", "list_slot", "obs32"):
                assert ci[k].tobytes() == want_i[k].tobytes(), (len(got), k)
            got.append(call(t, listed))
        assert alone[0] is not None and alone[1] is not None and alone[0][5] > 0 and alone[1][5] > 0
        assert got[0] == alone[0] and got[2] == alone[0], "the visual window either side of an inertial one"
        assert got[1] == alone[1] and got[3] == alone[1], "the inertial window either side of a visual one"
        _assert_state(d.state(), rec["states"][at], at)
    finally:
        handle.synchronize()
        for t in twins:
            t.close()
        d.close()


def BAS_tables(tables, counts):
    import map_fuse_spec as FS
    return FS.Tables(tables, counts)


def _refusals(pkg, at, seen):
    def between(g, d, tr):
        """before step `at`: every refused inertial call raises ORBX_ERR_INVALID, the two empty chains return None; nothing changes"""
        if g != at:
            return
        listed = tr["listed_before"]
        kfs, chain, members, vel, bias, edge_kf, preint = d.window(listed)
        K, n = len(kfs), len(chain)
        assert n >= 3 and d.kf[g].get_map_point_slots().max() < 0 and d.kf[g + 1].get_map_point_slots().max() < 0
        call = lambda kfs, chain, ek: d.h.map_local_inertial_ba(d.cam, d.mp, kfs, chain, vel[:len(chain)], bias[:len(chain)], np.array(ek, np.int32).reshape(-1, 2),
                                                                 preint[:len(ek)], d.icfg)
        chained = [(i, i + 1) for i in range(n - 1)]
        before = d.state()
        bad = [lambda: call(kfs, chain[:-1] + [K], chained), lambda: call(kfs, chain[:-1] + [chain[0]], chained), lambda: call(kfs, chain, chained[:-1] + [(0, n)]),
               lambda: call(kfs, chain, chained[:-1] + [(n - 1, n - 1)])]
        for i, f in enumerate(bad):
            with pytest.raises(pkg.OrbxError) as e:
                f()
            assert e.value.code == -1, i                                    # ORBX_ERR_INVALID
            assert d.state() == before, i
        assert call(kfs, chain[-1:], []) is None and d.state() == before                                        # a chain of one keyframe
        assert call(kfs + [d.kf[g], d.kf[g + 1]], [K, K + 1], [(0, 1)]) is None and d.state() == before          # no live point in the chain's tables
        seen.append(g)
    return between


def test_refusals_in_mid_session_leave_no_trace(handle, pkg, oracle):
    seed, at = I.SEEDS[0], I.IMU_INIT + 4
    m, rec = host_run(handle, pkg, oracle, seed)
    d = _IDevice(handle, pkg, seed)
    seen = []
    try:
        for g in replay(d, m, between=_refusals(pkg, at, seen)):
            if g >= at - 1:
                _assert_state(d.state(), rec["states"][g], g)              # before the refusals, the step after them and the last one
        assert seen == [at]
    finally:
        handle.synchronize()
        d.close()


def test_a_handle_whose_first_ba_is_an_inertial_one(handle, pkg, oracle):
    seed = I.SEEDS[0]
    m, rec = host_run(handle, pkg, oracle, seed)
    d = _IDevice(handle, pkg, seed)
    try:
        assert [g for g in replay(d, m, steps=I.IMU_INIT)] == list(range(I.IMU_INIT))
        h2 = _new_handle(pkg)                                              # no map call before: the state of step IMU_INIT - 1 is uploaded, not computed
        try:
            t = d.twin_on(h2, _tabled_at(m, I.IMU_INIT - 1))
            try:
                done = []
                for g in replay(t, m, start=I.IMU_INIT, steps=I.IMU_INIT + 2):
                    _assert_state(t.state(), rec["states"][g], g, live_only=True)
                    done.append(g)
                assert done == [I.IMU_INIT, I.IMU_INIT + 1] and m.trace[I.IMU_INIT]["ba"] is not None
            finally:
                t.close()
        finally:
            h2.close()
    finally:
        handle.synchronize()
        d.close()


def _tabled_at(m, g):
    return [k for k in range(W.N_KF) if m.snap[g]["tables"][k] is not None]
