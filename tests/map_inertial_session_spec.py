"""The host model of a local-mapping session on the resident map that switches to the inertial local BA once the IMU is initialised
(local_mapper.rs:334-375): tests/map_session_spec.py's model with the caller's inertial state of tests/map_inertial_session_scenes.py
beside it.  Like its parent it adds no rule of its own.

state   the parent's, and velocities [9,3], biases [9,6]: the scenes' initial state until a solve returns a keyframe's
create  from IMU_INIT on the triangulation takes the parallax gate of an inertial map (is_inertial = 1)
ba      from IMU_INIT on: inertial_collect_spec.collect over the chain (map_inertial_session_scenes.chain) with the keyframes' own
        has_point bytes, widen, the oracle's inertial solve from the model's present poses, velocities and biases and the store's
        positions.  Returns what the device must return: counts, fixed_kf, list_slot, obs32 and the solve.
adopt   extends to velocities and biases: they are the next step's inputs.  The floats of an inertial solve travel in the
        expectation itself: ba()'s dict carries `imu` (velocities, biases: the oracle's), which a device that passed its tolerances
        replaces by its own bytes before the model adopts them with the poses.

Four deliberately wrong variants (WRONG) are what tests/test_map_inertial_session_cpu.py holds the scenes' reach against.
"""
import numpy as np

import inertial_collect_spec as ICS
import inertial_edge_windows as E
import map_inertial_session_scenes as I
import map_session_scenes as W
import map_session_spec as S
import orientation_cases as C


class Model(S.Model):
    all_mono = False            # (a) every observation taken as mono: no stereo bit in obs32
    mono_in_solver = False      # (a) inside the solver alone: obs32 as it should be, the bit ignored where the Huber threshold is chosen
    has_by_creation = False     # (b) has_point from how the feature's point was created, not from the keyframe's byte
    carry = True                # (c) False: velocities and biases are not carried from one step to the next
    merged = True               # (d) False: the last interval's preintegration in place of the merged two-interval edge

    def __init__(self, sess, oracle, capacity=W.CAPACITY):
        super().__init__(sess, oracle, capacity)
        self.imu = I.inertial(sess["seed"])
        self.velocities = self.imu["velocities"].copy()
        self.biases = self.imu["biases"].copy()
        self.g = -1
        self.points_held = np.zeros(capacity, np.int32)                     # how many points a slot has held, the present one included
        self.stereo_made = np.zeros(capacity, np.uint8)                     # the slot's point came from the stereo phase
        self._window = None

    def imu_initialized(self, step):
        return step >= I.IMU_INIT

    def _step(self, g, dev):
        self.g = g
        super()._step(g, dev)

    def create(self, cur, nb):
        return super().create(cur, nb, is_inertial=int(self.imu_initialized(self.g)))

    def apply_create(self, spec, step):
        reused = super().apply_create(spec, step)
        slots = np.asarray(spec["new_slot"], np.int64)
        self.points_held[slots] += 1
        self.stereo_made[slots] = 0; self.stereo_made[slots[:int(spec["counts"][0])]] = 1
        return reused

    def has_point(self, g):
        if not self.has_by_creation:
            return self.kf[g]["has"]
        t = self.tables[g]
        return np.where(t >= 0, self.stereo_made[np.maximum(t, 0)], 0).astype(np.uint8)

    def ba(self, cur):
        """None: fewer than two keyframes in the chain, or no live point in its tables"""
        self._window = None
        if not self.imu_initialized(self.g):
            return super().ba(cur)
        o, L = self.oracle, self.listed
        chain = I.chain(L)
        c = ICS.collect(self.T(), [self.xy[g] for g in L], [self.has_point(g) for g in L], self.live, chain)
        if c is None or c["empty"]:
            return None
        members = [L[p] for p in chain]
        K, F, M, N = (int(x) for x in c["counts"])
        edge_kf, preint, skips = I.edges(self.imu, members, self.merged)
        fixed_cw = np.array([o.se3_inverse(self.poses_wc[L[k]]) for k in [chain[0]] + c["fixed_kf"].tolist()]).reshape(-1, 7)
        if self.all_mono:
            c["obs32"]["mp_idx"] &= ~ICS.STEREO
        obs = ICS.widen(c["obs32"], F)
        if self.mono_in_solver:
            obs["_pad"] = 0
        args = dict(poses_wc=self.poses_wc[members].copy(), velocities=self.velocities[members].copy(), biases=self.biases[members].copy(), fixed_cw=fixed_cw,
                    points=np.ascontiguousarray(self.positions[c["list_slot"]]), obs=obs, edge_kf=edge_kf, preint=preint)
        cfg = o.inertial_ba_config(); cfg.max_iterations = I.INERTIAL_ITERATIONS
        solve = o.inertial_ba_solve(o.Camera(**W.CAMERA), cfg, args["poses_wc"], args["velocities"], args["biases"], fixed_cw, args["points"], obs,
                                    edge_kf, preint)
        stereo = (c["obs32"]["mp_idx"] & ICS.STEREO) != 0
        held = self.points_held[c["list_slot"]]
        self.stats[self.g]["inertial"] = dict(K=K, F=F, M=M, N=N, stereo=float(stereo.mean()), E=len(edge_kf), skip=skips > 0, blind=W.EMPTY in members,
                                              reused=int((held >= 2).sum()), third=int((held >= 3).sum()), iterations=int(solve["iterations"]),
                                              margin=C.lm_margin(solve["trace"]))
        self.trace[self.g]["inertial"] = dict(chain=chain, edge_kf=edge_kf, preint=preint, fixed_kf=c["fixed_kf"])
        self._window = dict(c, chain=chain, optimised=chain, solve=solve, args=args, imu=dict(velocities=solve["velocities"], biases=solve["biases"]))
        return self._window

    def adopt(self, positions=None, poses=None, normals=None, velocities=None, biases=None):
        """velocities / biases: {position in kfs[]: row}.  The poses of an inertial window bring the window's velocities and biases."""
        super().adopt(positions, poses, normals)
        if poses is not None and self._window is not None and self.carry:
            w = self._window
            velocities, biases = dict(zip(w["chain"], w["imu"]["velocities"])), dict(zip(w["chain"], w["imu"]["biases"]))
        for p, row in (velocities or {}).items():
            self.velocities[self.listed[int(p)]] = row
        for p, row in (biases or {}).items():
            self.biases[self.listed[int(p)]] = row

    def outliers(self, ba):
        """the parent's rule on the inertial window's observations: the chain takes the place of the local keyframes (the anchor that
        of the current one: it is the observer coded -1), the stereo bit is taken off the point index"""
        if ba is None or "chain" not in ba:
            return super().outliers(ba)
        obs = ba["obs32"].copy()
        obs["mp_idx"] &= ~ICS.STEREO
        obs["kf_idx"] = np.where(obs["kf_idx"] >= 1, obs["kf_idx"] - 1, obs["kf_idx"])
        counts = ba["counts"].copy(); counts[0] -= 1
        return super().outliers(dict(local_kf=np.array(ba["chain"], np.int32), counts=counts, fixed_kf=ba["fixed_kf"], obs32=obs, list_slot=ba["list_slot"]))

    def step(self, g, dev=None):
        super().step(g, dev)
        w = self._window
        self.snap[g].update(velocities=self.velocities.copy(), biases=self.biases.copy(), solve=None if w is None else {k: w["solve"][k].copy() for k in E.OUTPUTS},
                            window=None if w is None else tuple(w[k].tobytes() for k in ("counts", "fixed_kf", "list_slot", "obs32")))


def assert_solve_close(got, want, label):
    """an inertial solve against the oracle's at tests/test_inertial_ba.py's tolerances, unchanged: iterations equal, initial error 1e-10
    relative, final error 1e-7 relative, poses / velocities / biases / points 1e-6 by inertial_edge_windows.rel"""
    e0 = abs(got["initial_error"] - want["initial_error"]) / want["initial_error"]
    e1 = abs(got["final_error"] - want["final_error"]) / want["final_error"]
    out = {k: E.rel(got[k], want[k]) for k in E.OUTPUTS}
    print("%s: iterations %d / %d, initial %.3e, final %.3e, %s" % (label, got["iterations"], want["iterations"], e0, e1, " ".join("%s %.2e" % kv for kv in out.items())))
    assert got["iterations"] == want["iterations"], label
    assert e0 < 1e-10 and e1 < 1e-7, (label, e0, e1)
    for k, v in out.items():
        assert v < 1e-6, (label, k, v)


def variant(**flags):
    return type("Wrong" + "".join(sorted(flags)), (Model,), flags)


MONO_IN_SOLVER = variant(mono_in_solver=True)
WRONG = dict(a=variant(all_mono=True), b=variant(has_by_creation=True), c=variant(carry=False), d=variant(merged=False))


def run(sess, oracle, cls=Model, dev=None, steps=None):
    return S.run(sess, oracle, cls=cls, dev=dev, steps=steps)
