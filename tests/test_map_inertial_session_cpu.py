"""The inertial session model (tests/map_inertial_session_spec.py) over its scenes (tests/map_inertial_session_scenes.py), without a GPU:
the model and the oracle alone.  Prints and asserts the per-step table the scenes' docstring quotes, the margin rule that chose the
seeds, and the reach of the scenes: four deliberately wrong models must move the session by at least 100 times the GPU tolerance or
change a discrete output.  The host map of tests/test_map_session_cpu.py runs beside the model and checks its invariants after every
call, as in the visual session.

The last test runs the model beside a recorded run of the device (tests/golden/map_inertial_session_device_seed2.npz: the floats the
model adopted in tests/test_map_inertial_session_gpu.py's host run of seed 2 on an MI355X, and the inertial windows' discrete outputs)
with that test's comparisons: the model passes every step, each wrong model fails at a named one.

Wall time of this module: 41 s where tests/test_map_session_cpu.py takes 33 s on the same host (one session of the model with the
host map beside it: 7 s); the wrong models go on from a copy of the model taken before IMU_INIT."""
import copy
import os

import numpy as np
import pytest

import inertial_edge_windows as E
import map_inertial_session_scenes as I
import map_inertial_session_spec as M
import map_session_scenes as W
from conftest import assert_ba_close
from test_map_session_cpu import HostMap

REACH = 100 * 1e-6                      # 100 times the GPU tolerance on poses, velocities, biases and points (tests/test_inertial_ba.py's TOL)
_runs, _before = {}, {}


def model_run(seed, oracle):
    if seed not in _runs:
        h = HostMap(W.N_KF)
        _runs[seed] = (M.run(W.session(seed), oracle, dev=h), h)
    return _runs[seed]


def inertial_steps(m):
    return [(g, m.stats[g]["inertial"]) for g in range(W.N_KF) if "inertial" in m.stats[g]]


def _line(seed, g, s):
    return "seed %d  %d: %d/%d/%d/%d/%.3f/%d/%s/%s/%d(%d)/%d  %.2e" % (seed, g, s["K"], s["F"], s["M"], s["N"], s["stereo"], s["E"], "skip" if s["skip"] else "-",
                                                                    "blind" if s["blind"] else "-", s["reused"], s["third"], s["iterations"], s["margin"])


def test_the_sessions_reach_what_the_one_piece_scenes_do_not(oracle):
    steps = []
    for seed in I.SEEDS:
        m, h = model_run(seed, oracle)
        for g, s in inertial_steps(m):
            print(_line(seed, g, s))
            steps.append(s)
            assert 0.0 < s["stereo"] < 1.0 and s["E"] == s["K"] - 1 and s["K"] <= I.INERTIAL_WINDOW
        assert [g for g, _ in inertial_steps(m)] == list(range(I.IMU_INIT, W.N_KF))                       # no inertial window is empty, keyframe EMPTY's included
        assert all(m.stats[g]["ba_iterations"] > 0 for g in range(1, I.IMU_INIT))                         # the visual windows before the switch
        assert h.calls == 2 + 7 * (W.N_KF - 1) and len(m.unlisted) == W.MAX_UNLISTED
        assert any(s["skip"] for _, s in inertial_steps(m)) and any(s["blind"] for _, s in inertial_steps(m))    # in either seed
    assert sum(1 for s in steps if s["iterations"] > 0) >= 4
    assert any(s["F"] == 1 for s in steps) and any(s["F"] >= 3 for s in steps)
    assert max(s["reused"] for s in steps) >= 100 and max(s["third"] for s in steps) >= 1
    assert all(s["iterations"] == I.INERTIAL_ITERATIONS for s in steps)


def test_the_seeds_are_the_first_two_that_keep_their_margins(oracle):
    chosen = []
    for seed in I.CANDIDATES:
        m, _ = model_run(seed, oracle)
        margin = min(s["margin"] for _, s in inertial_steps(m))
        print("seed %d: smallest LM margin over the inertial steps %.3e" % (seed, margin))
        if margin >= E.MARGIN:
            chosen.append(seed)
        if len(chosen) == len(I.SEEDS):
            break
    assert tuple(chosen) == I.SEEDS


def _difference(a, b):
    """two snapshots of a step -> "discrete" where the tables, the live bytes, the list or the window's counts, fixed_kf, list_slot or
    obs32 differ, else the largest difference by inertial_edge_windows.rel over the live positions, the poses and what the step's
    inertial solve returned (poses, velocities, biases, points): every float the GPU test holds to the model at 1e-6"""
    same = a["live"].tobytes() == b["live"].tobytes() and a["listed"] == b["listed"] and a["window"] == b["window"] and all(
        (x is None and y is None) or (x is not None and y is not None and x.tobytes() == y.tobytes()) for x, y in zip(a["tables"], b["tables"]))
    d = {}
    if a["solve"] is not None and b["solve"] is not None and a["window"][:3] == b["window"][:3]:
        d.update({k: E.rel(a["solve"][k], b["solve"][k]) for k in E.OUTPUTS})
    if not same:
        return "discrete", d
    on = a["live"] == 1
    d.update(map_positions=E.rel(a["positions"][on], b["positions"][on]), map_poses=E.rel(a["poses_wc"], b["poses_wc"]))
    return max(d.values()), d


def _fork(m, cls):
    """a copy of the model `m` that goes on as a `cls`: the wrong models differ from the model from IMU_INIT on only"""
    c = copy.deepcopy(m, {id(x): x for x in (m.sess, m.oracle, m.kf, m.imu)})
    c.__class__ = cls
    return c


def reach(seed, oracle, cls):
    """the first step at which the wrong model `cls` is REACH away from the model or differs in a discrete output, else its largest
    difference -> (step, "discrete" or the figure, the figure per output)"""
    base, _ = model_run(seed, oracle)
    if seed not in _before:
        _before[seed] = M.run(W.session(seed), oracle, steps=I.IMU_INIT)
    v = _fork(_before[seed], cls)
    worst = (None, 0.0, {})
    for g in range(I.IMU_INIT, W.N_KF):
        v.step(g)
        d, per = _difference(v.snap[g], base.snap[g])
        if d == "discrete" or d >= REACH:
            return g, d, per
        worst = max(worst, (g, d, per), key=lambda x: x[1])
    return worst


FIRST = dict(a=I.IMU_INIT, b=I.IMU_INIT, c=I.IMU_INIT + 1, d=I.IMU_INIT + 1)    # seed SEEDS[1]: the first inertial window; the first with carried states; the first skip edge


@pytest.mark.parametrize("name", sorted(M.WRONG))
def test_a_wrong_model_moves_the_session(oracle, name):
    """(a) every observation mono, (b) has_point by the creation method, (c) velocities and biases not carried, (d) the one-interval
    preintegration on the skip edge.  (a) and (b) change obs32, a discrete output.  (c) reaches the returned biases
    and nothing else: the biases enter the cost through the random walk alone and the velocities are found again from the
    preintegrations, so poses and positions move by 1e-9 whatever the scene; they are outputs held at the same 1e-6.  (a) inside the
    solver alone, with obs32 as it should be, stays below the GPU tolerance: the stereo bit chooses the Huber threshold (2.45 or 2.80
    px) and no observation of these sessions, whose features lie within 0.4 px of their projections, falls between the two.  That
    the solver reads the bit is held by tests/test_inertial_ba.py and tests/test_inertial_collect_gpu.py on 1 px noise."""
    seed = I.SEEDS[1]
    g, d, per = reach(seed, oracle, M.WRONG[name])
    print("variant (%s), seed %d: step %d, %s %s" % (name, seed, g, d if d == "discrete" else "%.3e" % d, " ".join("%s %.2e" % kv for kv in per.items())))
    assert g == FIRST[name] and (d == "discrete" or d >= REACH)
    if name == "a":
        g, d, per = reach(seed, oracle, M.MONO_IN_SOLVER)
        print("variant (a) inside the solver alone, seed %d: largest difference %.3e at step %d" % (seed, d, g))
        assert d != "discrete" and d < REACH


# ---- against a recorded run of the device ------------------------------------------------------------------------------------

class Recorded:
    """map_session_spec.Model.step's `dev` from tests/golden/map_inertial_session_device_seed2.npz: every float the model adopted from
    the MI355X in tests/test_map_inertial_session_gpu.py's host run of seed 2, and the inertial windows' discrete outputs.  Its ba
    holds them to the model as that test's does; a failure names the step."""

    def __init__(self):
        self.z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_inertial_session_device_seed2.npz"))
        self.g = -1

    def _get(self, call, key):
        return self.z["%d.%s.%s" % (self.g, call, key)]

    def table(self, m, want):
        self.g = want["g"]

    def create(self, m, want):
        return {k: self._get("create", k) for k in ("counts", "new_slot", "new_neighbour", "new_idx1", "new_idx2", "new_points")}

    def fuse(self, m, want):
        return self._get("fuse", "normals")

    def ba(self, m, want):
        b, step = want["ba"], "step %d" % self.g
        assert b is not None, step
        if not m.imu_initialized(self.g):
            got = dict(poses_wc=self._get("ba", "poses_wc"), points=self._get("ba", "points"))
            assert_ba_close(got, b["solve"], 1e-6)
            return got["poses_wc"], got["points"]
        for k in ("counts", "fixed_kf", "list_slot"):
            assert self._get("ba", k).tobytes() == b[k].tobytes(), (step, k)
        assert self._get("ba", "obs32").tobytes() == b["obs32"].tobytes(), (step, "obs32")
        e = self._get("ba", "errors")
        got = dict({k: self._get("ba", k) for k in E.OUTPUTS}, iterations=int(self._get("ba", "iterations")), initial_error=float(e[0]), final_error=float(e[1]))
        M.assert_solve_close(got, b["solve"], step)
        b["imu"] = dict(velocities=got["velocities"], biases=got["biases"])
        return got["poses_wc"], got["points"]

    track = neighbours = cull = remove = redundancy = state = lambda self, m, want: None


def test_the_model_passes_a_recorded_device_run_and_no_wrong_model_does(oracle):
    before = M.run(W.session(2), oracle, dev=Recorded(), steps=I.IMU_INIT)

    def go_on(cls):
        m, dev = _fork(before, cls), Recorded()
        for g in range(I.IMU_INIT, W.N_KF):
            m.step(g, dev)
        return m

    m = go_on(M.Model)
    assert [g for g, _ in inertial_steps(m)] == list(range(I.IMU_INIT, W.N_KF))
    for name, cls in sorted(M.WRONG.items()):
        with pytest.raises(AssertionError) as e:
            go_on(cls)
        print("variant (%s) against the recorded run: %s" % (name, str(e.value).splitlines()[0][:160]))
        assert "step %d" % FIRST[name] in str(e.value), name
