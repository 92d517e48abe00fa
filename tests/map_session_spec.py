"""The host model of a local-mapping session on the resident map: the existing specifications composed over one state, in the order
process_keyframe makes the calls ("Creating and culling map points on the resident map", "Observations from the
resident map", "Local BA from the resident map").  It adds no rule of its own: every method is a thin composition that returns what
the device call must return and applies it to the state.

state   tables (map_fuse_spec.Tables over all keyframes of the session, None = no table yet), live, positions, desc, poses_wc,
        normals, free (a list in the shim's push / pop order: pop() hands out, a removed slot is pushed), recent ({slot: the step
        at which it was created}, live points not yet seen by culling), listed (the keyframes passed as kfs[], in order)
step    track -> set_table -> neighbours -> create -> cull -> fuse -> ba -> outliers -> redundancy
adopt   after a float output of the device passed its tolerance the model takes the device's bytes, so that the next discrete
        decision is computed from identical inputs on both sides

A `dev` object passed to step() is shown every call's expectation before it is applied (dev.<call>(model, want) -> the floats to
adopt, or None); without one the model adopts its own.  step() records everything a replay of the session needs in model.trace.
"""
import numpy as np

import ba_collect_spec as BAS
import covisibility_spec as CS
import map_create_spec as MC
import map_fuse_spec as FS
import map_observations_spec as OSP
import map_session_scenes as W
import map_store_spec as MS
import pnp_spec as P
import tracking_spec as TS
import triangulation_spec as XS

NEAR = 1e-9                     # tests/test_map_create_cpu.py's MARGIN: a pair this close to a gate may fall on either side


def as_arrays(tables, counts):
    return [np.full(n, -1, np.int32) if t is None else np.asarray(t, np.int32) for t, n in zip(tables, counts)]


class Model:
    forgetful = False

    def __init__(self, sess, oracle, capacity=W.CAPACITY):
        self.sess, self.oracle, self.capacity = sess, oracle, capacity
        self.kf = sess["keyframes"]
        self.counts = [len(k["kp"]) for k in self.kf]
        self.tables = FS.Tables([None] * len(self.kf), self.counts)
        self.live = np.zeros(capacity, np.uint8)
        self.positions = np.zeros((capacity, 3)); self.desc = np.zeros((capacity, 32), np.uint8); self.normals = np.zeros((capacity, 3))
        self.poses_wc = np.array(sess["poses"], np.float64, copy=True)
        self.free = list(range(capacity - 1, -1, -1))                       # pop() hands out 0, 1, 2, ...
        self.recent = {}
        self.listed, self.unlisted = [], []
        self.n_created = self.n_removed = 0
        self.used = set()                                                   # slots that have held a point
        self.gone_by = {}                                                   # slot -> "cull" / "fuse" / "outlier": how it was last freed
        self.trace, self.stats, self.snap = {}, {}, {}
        self.xy = [np.stack([k["kp"]["x"], k["kp"]["y"]], 1).astype(np.float32).reshape(-1, 2) for k in self.kf]

    # ---- views of the state in kfs[] order ---------------------------------------------------------------------------------
    def T(self):
        return FS.Tables([self.tables[g] for g in self.listed], [self.counts[g] for g in self.listed])

    def _put(self, tabs, where=None):
        for p, t in zip(range(len(self.listed)) if where is None else where, tabs):
            self.tables[self.listed[p]] = None if t is None else np.array(t, np.int32, copy=True)

    def _purged(self, before, after):
        """the tables a removal leaves: the forgetful variant keeps the entries that name the removed slots"""
        return before if self.forgetful else after

    def _keyframe(self, g):
        return dict(self.kf[g], pose=self.poses_wc[g].copy())

    def _freed(self, slots, how):
        for s in (int(x) for x in slots):
            self.free.append(s); self.recent.pop(s, None); self.gone_by[s] = how
        self.n_removed += len(slots)

    def search(self):
        """map_fuse_spec's search: the oracle's fuse_search against the listed keyframes at their present poses"""
        o, L = self.oracle, list(self.listed)
        poses = self.poses_wc.copy()

        def search(positions, desc, tgt):
            off = np.zeros(len(tgt) + 1, np.int32); off[1:] = np.cumsum([self.counts[L[t]] for t in tgt])
            idx, _ = o.fuse_search(o.Camera(**W.CAMERA), positions, desc, poses[[L[t] for t in tgt]].reshape(-1, 7), off,
                                   np.concatenate([self.kf[L[t]]["kp"].astype(o.KEYPOINT) for t in tgt] + [np.zeros(0, o.KEYPOINT)]),
                                   np.concatenate([self.kf[L[t]]["desc"] for t in tgt] + [np.zeros((0, 32), np.uint8)]), W.RADIUS_SCALE, 50)
            return idx
        return search

    # ---- the calls -----------------------------------------------------------------------------------------------------------
    def track(self, g):
        """map_track_local for keyframe g's features against the listed keyframes: reference = the last listed, mode 1"""
        kf, T = self.kf[g], self.T()
        ref = len(self.listed) - 1
        local, row = CS.local_keyframes(T, self.live, ref, W.TRACK_NBEST)
        list_slot = MS.select_keyframes([T[k] for k in local], self.live)
        pos, md = MS.gathered(list_slot, self.positions, self.desc)
        cfg = TS.default_config(TS.LOCAL_MAP)
        prior = np.array(self.sess["priors"][g], np.float64, copy=True)
        match = TS.search(self.oracle, W.CAMERA, cfg, kf["kp"], kf["desc"], pos, md, prior)
        ga = TS.gather(kf["kp"], pos, match)
        pnp = P.solve(W.CAMERA, ga["points3d"], ga["points2d"], prior)
        rec, pose, matched = TS.finish(cfg, len(kf["kp"]), match, ga, prior, pnp["pose"], pnp["inlier_mask"], pnp["status"], pnp["n_inliers"])
        return dict(local_kf=row.astype(np.int32), list_slot=list_slot.astype(np.int32), gathered=ga, pnp=pnp, record=rec, pose=pose, matched=matched,
                    matched_slot=MS.matched_slot(matched, list_slot), ref=ref, frame=(kf["kp"], kf["desc"], prior, prior))

    def set_table(self, g, matched_slot):
        self.tables[g] = np.array(matched_slot, np.int32, copy=True)
        self.listed.append(g)

    def neighbours(self, cur):
        """the N_NEIGHBOURS best covisibles of kfs[cur]; a keyframe that shares with fewer than two takes the ones listed just before
        it as well (the tracker was lost: the map is joined again by fuse)"""
        w = CS.weights(self.T(), self.live, [cur])[0]
        b, n = CS.best(w, W.N_NEIGHBOURS)
        nb = b[:n].tolist()
        for k in range(cur - 1, -1, -1):
            if len(nb) < min(2, cur) and k not in nb:
                nb.append(k)
        return dict(weights=w, best=b, n_best=n, neighbours=nb)

    def create(self, cur, nb, is_inertial=0):
        n_free = min(len(self.free), W.MAX_FREE)
        free_slots = np.array([self.free.pop() for _ in range(n_free)], np.int32)
        T = self.T()
        order = [cur] + list(nb)
        spec = MC.create_points(self.oracle, W.CAMERA, XS.default_config(), is_inertial, self._keyframe(self.listed[cur]), [self._keyframe(self.listed[i]) for i in nb],
                                [T[i] for i in order], self.live, free_slots)
        spec.update(free_slots=free_slots, order=order, is_inertial=is_inertial, tables_before=[T[i] for i in order], near=sum(1 for e in spec["evaluated"] if e[6] <= NEAR))
        return spec

    def take_created(self, spec, got):
        """the device's lists in place of the specification's where they differ in near-gate pairs only: the tables are then the
        sequential replay of the list the call gave (tests/test_map_create_gpu.py's rule)"""
        ns = int(spec["counts"][0])
        key = lambda d: [(int(t), int(a), int(b)) for t, a, b in zip(d["new_neighbour"], d["new_idx1"], d["new_idx2"])]
        pairs = key(got)
        cur, nbs = self._keyframe(self.listed[spec["order"][0]]), [self._keyframe(self.listed[i]) for i in spec["order"][1:]]
        kp = MC.create_replay(cur, nbs, spec["tables_before"], self.live, spec["free_slots"], [p + (None,) for p in pairs[ns:]])
        tabs = as_arrays(spec["tables_before"], [self.counts[self.listed[i]] for i in spec["order"]])
        tabs = [t.copy() for t in tabs]
        for t, d in zip(tabs, kp):
            for i, s in d.items():
                t[i] = s
        out = dict(spec, tables=tabs, new_desc=cur["desc"][got["new_idx1"]])
        for k in ("new_slot", "new_neighbour", "new_idx1", "new_idx2", "new_points"):
            out[k] = np.array(got[k], copy=True)
        c = len(pairs)
        out["counts"] = np.array([ns, int(got["counts"][1]), c, int(got["counts"][3])], np.int32)
        return out

    def apply_create(self, spec, step):
        m = int(spec["counts"][2])
        self._put(spec["tables"], spec["order"])
        slots = spec["new_slot"]
        self.live[slots] = 1; self.positions[slots] = spec["new_points"]; self.desc[slots] = spec["new_desc"]; self.normals[slots] = 0.0
        for s in reversed(spec["free_slots"][m:].tolist()):                 # the unused slots go back as they came
            self.free.append(s)
        reused = [int(s) for s in slots if int(s) in self.used]
        for s in slots.tolist():
            self.recent[s] = step; self.used.add(s)
        self.n_created += m
        return reused

    def cull(self, step):
        cand = np.array([s for s, st in self.recent.items() if st <= step - W.GRACE], np.int32)
        T = self.T()
        culled, tabs, live, n = MC.cull_points(T, self.live, cand, W.CULL_MIN_OBS)
        return dict(cand=cand, culled=culled, tables=self._purged(T, tabs), live=live, n_cleared=n)

    def apply_cull(self, r):
        self._put(r["tables"]); self.live = r["live"]
        for s in r["cand"].tolist():
            self.recent.pop(s, None)
        self._freed(r["culled"], "cull")

    def fuse(self, cur, nb):
        T = self.T()
        r = FS.search_in_neighbors(T, self.live, self.positions, self.desc, cur, nb, self.search())
        L = self.listed
        ref, scene = OSP.refresh(r["tables"], r["live"], r["affected"], self.positions, self.desc, self.poses_wc[L], [self.kf[g]["desc"] for g in L], W.SCALE_RANGE,
                                 self.normals[r["affected"]])
        return dict(r, refresh=ref, refresh_scene=scene, tables_before=T, normals_before=self.normals.copy(), cur=cur, nb=list(nb))

    def apply_fuse(self, r):
        self._put(r["tables"]); self.live = r["live"]
        aff = r["affected"]
        self.desc[aff] = r["refresh"]["mp_desc"]; self.normals[aff] = r["refresh"]["normals"]
        self._freed(r["a"]["goner"], "fuse"); self._freed(r["b"]["goner"], "fuse")

    def ba(self, cur):
        """the window by ba_collect_spec, solved by the oracle's dense solver; None: the window is empty"""
        o, L = self.oracle, self.listed
        w = BAS.collect(self.T(), [self.xy[g] for g in L], self.live, cur, W.BA_COVISIBLE)
        if w["empty"]:
            return None
        K, F = int(w["counts"][0]), int(w["counts"][1])
        poses_cw = np.array([o.se3_inverse(self.poses_wc[L[k]]) for k in w["local_kf"][1:1 + K]]).reshape(-1, 7)
        fixed_cw = np.array([o.se3_inverse(self.poses_wc[L[k]]) for k in [w["local_kf"][0]] + w["fixed_kf"].tolist()]).reshape(-1, 7)
        obs = np.zeros(len(w["obs32"]), o.BA_OBS)
        k = w["obs32"]["kf_idx"]
        obs["kf_idx"] = np.where(k >= 0, k, -1); obs["fixed_idx"] = np.where(k >= 0, -1, -1 - k); obs["mp_idx"] = w["obs32"]["mp_idx"]
        obs["u"] = w["obs32"]["u"]; obs["v"] = w["obs32"]["v"]
        pts = np.ascontiguousarray(self.positions[w["list_slot"]])
        cfg = o.ba_config(); cfg.max_covisible_keyframes = W.BA_COVISIBLE
        solve = o.ba_solve_dense(o.Camera(**W.CAMERA), cfg, poses_cw, fixed_cw, pts, obs)
        return dict(w, solve=solve, poses_cw=poses_cw, fixed_cw=fixed_cw, points=pts, obs=obs, optimised=[int(x) for x in w["local_kf"][1:1 + K]])

    def adopt(self, positions=None, poses=None, normals=None):
        """positions / normals: (slots, rows); poses: {position in kfs[]: pose_wc}"""
        if positions is not None:
            self.positions[np.asarray(positions[0], np.int64)] = positions[1]
        if normals is not None:
            self.normals[np.asarray(normals[0], np.int64)] = normals[1]
        for p, pose in (poses or {}).items():
            self.poses_wc[self.listed[int(p)]] = pose

    def outliers(self, ba):
        """the points of the N_OUTLIERS worst-reprojecting observations of the window, by the model's present poses and positions
        (the device's bytes once adopted), worst first"""
        if ba is None:
            return np.zeros(0, np.int32)
        L = self.listed
        order = [int(x) for x in ba["local_kf"][:1 + int(ba["counts"][0])]] + ba["fixed_kf"].tolist()
        err = np.zeros(len(ba["obs32"]))
        code = ba["obs32"]["kf_idx"]
        place = np.where(code >= -1, code + 1, len(order) - int(ba["counts"][1]) + 1 + (-2 - code))
        for j, k in enumerate(order):
            sel = np.flatnonzero(place == j)
            if len(sel):
                z, u, v = TS.project(W.CAMERA, self.poses_wc[L[k]], self.positions[ba["list_slot"][ba["obs32"]["mp_idx"][sel]]])
                err[sel] = (u - ba["obs32"]["u"][sel]) ** 2 + (v - ba["obs32"]["v"][sel]) ** 2
        worst = np.argsort(-err, kind="stable")[:W.N_OUTLIERS]
        out = []
        for s in ba["list_slot"][ba["obs32"]["mp_idx"][worst]].tolist():
            if s not in out:
                out.append(s)
        return np.array(out, np.int32)

    def remove(self, slots):
        T = self.T()
        tabs, live, n = MC.remove_points(T, self.live, slots)
        return dict(slots=np.asarray(slots, np.int32), tables=self._purged(T, tabs), live=live, n_cleared=n)

    def apply_remove(self, r):
        self._put(r["tables"]); self.live = r["live"]
        self._freed(r["slots"], "outlier")

    def redundancy(self, cur):
        cand = np.array([p for p in range(1, len(self.listed)) if p != cur], np.int32)
        total, red, cull = OSP.redundancy(self.T(), self.live, cand, W.KF_MIN_OBS, W.KF_THRESHOLD)
        drop = [int(c) for c, f in zip(cand, cull) if f][:max(W.MAX_UNLISTED - len(self.unlisted), 0)]
        return dict(cand=cand, total=total, redundant=red, cull=cull, drop=drop)

    def apply_redundancy(self, r):
        for g in [self.listed[p] for p in r["drop"]]:                       # its table stays where it is, unlisted from now on
            self.listed.remove(g); self.unlisted.append(g)

    # ---- one step ------------------------------------------------------------------------------------------------------------
    def step(self, g, dev=None):
        """keyframe g joins the map.  Step 0 creates keyframe 0's stereo points and nothing else."""
        self._step(g, dev)
        self.snap[g] = dict(tables=[None if t is None else t.copy() for t in self.tables], live=self.live.copy(), free=list(self.free), listed=list(self.listed),
                            positions=self.positions.copy(), desc=self.desc.copy(), poses_wc=self.poses_wc.copy())

    def _step(self, g, dev):
        tr = self.trace[g] = dict(listed_before=list(self.listed))
        st = self.stats[g] = dict(created=0, dropped=0, culled=0, goners=0, reused=0, near=0, evaluated=0, ba_iterations=0, fuse_counts=None)
        call = lambda name, want: getattr(dev, name)(self, want) if dev is not None else None
        if self.listed:
            t = self.track(g)
            call("track", t)
            tr["track"] = t
            self.set_table(g, t["matched_slot"])
        else:
            self.set_table(g, np.full(self.counts[g], -1, np.int32))
        tr["table"] = self.tables[g].copy()
        call("table", dict(g=g, table=tr["table"]))
        call("state", "table")
        cur = len(self.listed) - 1
        tr.update(listed=list(self.listed), cur=cur)
        nb = self.neighbours(cur)
        call("neighbours", dict(nb, cur=cur))
        tr["cov"] = dict(weights=nb["weights"], best=nb["best"], n_best=nb["n_best"])
        nb = tr["neighbours"] = nb["neighbours"]
        c = self.create(cur, nb)
        got = call("create", c)
        if got is not None:
            c = self.take_created(c, got)
        reused = self.apply_create(c, g)
        tr["create"] = dict(free_slots=c["free_slots"], created=int(c["counts"][2]), new_slot=c["new_slot"].copy())
        st.update(created=int(c["counts"][2]), dropped=int(c["counts"][3]), reused=len(reused), near=c["near"], evaluated=len(c["evaluated"]),
                  reused_after={how: sum(1 for s in reused if self.gone_by.get(s) == how) for how in ("cull", "fuse", "outlier")})
        call("state", "create")
        if g == 0:
            return
        r = self.cull(g)
        call("cull", r)
        self.apply_cull(r)
        tr["cull"] = dict(cand=r["cand"], culled=r["culled"])
        st["culled"] = len(r["culled"])
        call("state", "cull")
        f = self.fuse(cur, nb)
        got = call("fuse", f)
        self.apply_fuse(f)
        if got is not None:
            self.adopt(normals=(f["affected"], got))
        tr["fuse"] = dict(goner_a=f["a"]["goner"], goner_b=f["b"]["goner"], affected=f["affected"], normals_before=f["normals_before"],
                          agree=[agrees(f["a"], len(nb)), agrees(f["b"], 1)])
        st.update(goners=len(f["a"]["goner"]) + len(f["b"]["goner"]), fuse_counts=[f["a"]["counts"].tolist(), f["b"]["counts"].tolist()])
        call("state", "fuse")
        b = self.ba(cur)
        got = call("ba", dict(ba=b, cur=cur))
        if b is not None:
            poses, points = got if got is not None else (b["solve"]["poses_wc"], b["solve"]["points"])
            self.adopt(positions=(b["list_slot"], points), poses=dict(zip(b["optimised"], poses)))
            st["ba_iterations"] = int(b["solve"]["iterations"])
        tr["ba"] = None if b is None else dict(optimised=b["optimised"], counts=b["counts"], list_slot=b["list_slot"])
        call("state", "ba")
        out = self.remove(self.outliers(b))
        call("remove", out)
        self.apply_remove(out)
        tr["outliers"] = out["slots"]
        call("state", "remove")
        red = self.redundancy(cur)
        call("redundancy", red)
        call("state", "redundancy")
        self.apply_redundancy(red)
        tr["redundancy"] = dict(cand=red["cand"], drop=red["drop"], total=red["total"], redundant=red["redundant"], cull=red["cull"])
        tr["poses_after"] = self.poses_wc.copy()


class ForgetfulModel(Model):
    """a model that frees removed slots without purging them from the tables: what recycling turns into a wrong map"""
    forgetful = True


def agrees(r, n_tgt):
    """map_fuse_spec.reference_replay's agreement conditions on one pass (tests/test_map_fuse_cpu.py states them): classes of at most
    two, no feature matched twice, every merge kept by the projected point, counts of a merged pair more than n_tgt apart"""
    st = r["stats"]
    flat = [(t, int(f)) for row in r["match"] for t, f in enumerate(row) if f >= 0]
    return (max([len(m) for m in st["members"].values()] + [0]) <= 2 and all(len(j) == 1 for j in st["claims"].values()) and len(flat) == len(set(flat))
            and all(int(k) in st["place"] and int(g) not in st["place"] for g, k in zip(r["goner"], r["keeper"]))
            and all(abs(int(st["nobs"][g]) - int(st["nobs"][k])) > n_tgt for g, k in zip(r["goner"], r["keeper"])))


def run(sess, oracle, cls=Model, dev=None, steps=None):
    m = cls(sess, oracle)
    for g in range(len(sess["keyframes"]) if steps is None else steps):
        m.step(g, dev)
    return m
