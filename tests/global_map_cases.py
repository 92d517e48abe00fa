"""Whole maps for the global BA of more than 128 optimised keyframes (orbx_ba_solve_global_map): 129 to 257 optimised keyframes against
the CPU oracle's global_ba_solve_schur, which has no size limit, and a map of 1025 without an oracle.  Test infrastructure only
(tests/test_global_map_cpu.py proves the conditions on the cases; tests/test_global_map_gpu.py runs them).

The coupled cases are large_ba_windows._covis_with_common_points: covis_window's corridor plus a dozen far points that every camera
sees, so that no tile of the reduced system is an exact zero; the banded case is covis_window alone, whose reduced system has true zero
tiles far from the diagonal.  Some points start behind the cameras that observe them, placed as large_ba_windows.global_map places them:
their observations keep the 100-px penalty and get no Jacobian rows, so the solver must hand them back untouched.

n = 6 K: 774 (the first size the window solver refuses), 960 (a multiple of 16 and of 64: no short last panel), 1026 (the first past
1024), 1542 (K past 256), 1200 banded.
"""
import numpy as np

import orb_slam3_rust_amd as P
import covis_windows as W
import large_ba_windows as L

# name -> (banded, arguments of covis_window, points behind the cameras)
CASES = {
    "k129": (False, dict(seed=1, K=129, F=1, M=2600, step=1.0, keep=0.35, depth=(2, 6)), 20),
    "k160": (False, dict(seed=2, K=160, F=1, M=3200, step=1.0, keep=0.35, depth=(2, 6)), 24),
    "k171": (False, dict(seed=1, K=171, F=1, M=3400, step=1.0, keep=0.35, depth=(2, 6)), 24),
    "k257": (False, dict(seed=1, K=257, F=1, M=3900, step=1.0, keep=0.35, depth=(2, 6)), 30),
    "k200_banded": (True, dict(seed=1, K=200, F=1, M=4000, step=1.0, keep=0.35, depth=(2, 6)), 24),
}
BIG = dict(seed=1, K=1025, F=1, M=20000, step=1.0, keep=0.35, depth=(2, 6))      # n = 6150, banded, no oracle
BIG_BEHIND = 40
_cache = {}
_oracle_cache = {}


def _with_points_behind(w, seed, M, n_behind):
    j = np.random.default_rng([0xC4, seed]).permutation(M)[:n_behind]            # large_ba_windows.global_map
    w["points"] = w["points"].copy()
    w["points"][j, 2] = -w["points"][j, 2] - 5.0                                 # the cameras look along +z from z ~ 0
    w["behind"] = j
    return w


def behind_depths(w):
    """depth, at the initial poses, of every observation of a point in w["behind"] in the camera that makes it"""
    ob = w["obs"][np.isin(w["obs"]["mp_idx"], w["behind"])]
    pose = np.where((ob["kf_idx"] >= 0)[:, None], w["poses_cw"][np.maximum(ob["kf_idx"], 0)], w["fixed_cw"][np.maximum(ob["fixed_idx"], 0)])
    X = w["points"][ob["mp_idx"]]
    return np.array([(P.synth._quat_rot(p[:4], x[None])[0] + p[4:])[2] for p, x in zip(pose, X)])


def _big():
    """The corridor of 1026 cameras is 1 km long: a pose's rotation noise of a few hundredths of a radian turns a world point 700 m from
    the origin by metres, so a point mirrored to z ~ -8 is not behind EVERY noisy camera that observes it.  The candidates are taken in
    the order large_ba_windows.global_map takes them, and those with an observation nearer than 1 m behind its camera are passed over."""
    w = W.covis_window(order="shuffled", **BIG)
    cand = np.random.default_rng([0xC4, BIG["seed"]]).permutation(BIG["M"])
    pts = w["points"].copy()
    keep = []
    for j in cand:
        if len(keep) == BIG_BEHIND:
            break
        x = pts[j].copy(); x[2] = -x[2] - 5.0
        ob = w["obs"][w["obs"]["mp_idx"] == j]
        pose = np.where((ob["kf_idx"] >= 0)[:, None], w["poses_cw"][np.maximum(ob["kf_idx"], 0)], w["fixed_cw"][np.maximum(ob["fixed_idx"], 0)])
        if len(ob) and all((P.synth._quat_rot(p[:4], x[None])[0] + p[4:])[2] < -1.0 for p in pose):
            keep.append(j); pts[j] = x
    w["points"] = pts
    w["behind"] = np.array(keep)
    return w


def case(name):
    """the case's map (made once per process; read-only)"""
    if name not in _cache:
        if name == "big":
            w = _big()
        else:
            banded, kw, n_behind = CASES[name]
            w = W.covis_window(order="shuffled", **kw) if banded else L._covis_with_common_points("shuffled", **kw)
            w = _with_points_behind(w, kw["seed"], kw["M"], n_behind)
        _cache[name] = w
    return _cache[name]


def oracle_answer(oracle, name):
    """global_ba_solve_schur on the case, once per process"""
    if name not in _oracle_cache:
        w = case(name)
        _oracle_cache[name] = oracle.global_ba_solve_schur(oracle.Camera(**w["camera"]), L._gcfg(oracle), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    return _oracle_cache[name]


def camera(w):
    return P.CameraModel(**w["camera"])
