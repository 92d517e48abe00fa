"""Small maps for the whole-map global BA (orbx_ba_solve_global_map) that reach what the maps of tests/global_map_cases.py do not: keyframe
lists of several hundred observations, optimised keyframes without or with one or two observations, observations by the identity pose,
(keyframe, point) pairs observed two and three times, a reduced system with a few blocks far from its band, and LM runs that a stop rule
ends.  Test infrastructure only (tests/test_global_map_edges_cpu.py proves the conditions on the cases, on the reference alone;
tests/test_global_map_edges_gpu.py runs them).  Every map is covis_windows.covis_window's with one fixed keyframe.

- dense     12 keyframes 0.1 m apart that each see nine tenths of 1200 points: lists of 575 to 649 observations, so that
            gba_kforder_kernel's 256-stride loop takes three trips and gba_kf_schur_kernel's 64-entry chunk loop nine to eleven.
- edges     40 keyframes (n = 240: three full panels and a short one of 48 columns); keyframes 0, 17 and 39 have no observation, keyframe 5
            one and keyframe 6 two; 30 observations by the identity pose; 60 duplicated pairs, 8 of them observed three times; 12 points
            start behind the cameras that observe them.
- loop      tests/global_map_cases.py's banded generator at 40 keyframes plus 20 far points that keyframes 0..3 and 36..39 alone
            observe: the reduced system is a band and one far corner.
- converged global_k20 with 600 points and no pixel noise, started at the ground truth: the gradient rule ends it in iteration 1.
- natural_stop   the dense map with a hundredth of a pixel of noise: the parameter rule ends it in iteration 5 at the default tolerances;
  gtol_stop, ptol_stop   the same map with the tolerance of one rule raised until that rule ends the run in iteration 4.

Each case has the largest iteration limit, at most 10, up to which every accept / reject decision of the reference is at least 1e-3
(relative) from a tie (orientation_cases.lm_margin): near convergence a trial error equals the current one to six or seven digits, and
equal iteration counts could not be demanded there.  tests/test_global_map_edges_cpu.py holds the measured traces.
"""
import numpy as np

import orb_slam3_rust_amd as P
import covis_windows as W
import global_map_cases as G

synth = P.synth
HUBER = float(np.sqrt(5.991))

# name -> (arguments of covis_window, points behind the cameras, max_iterations, param_tolerance, gradient_tolerance)
_STOP_MAP = dict(seed=6, K=12, F=1, M=1200, step=0.1, keep=0.9, depth=(2, 6), noise_px=0.01)      # see STOP below
_EDGES = dict(seed=6, K=40, F=1, M=1500, step=0.5, keep=0.5, depth=(2, 6), identity_observer=30, empty_kf=[0, 17, 39], thin_kf={5: 1, 6: 2}, duplicates=60)
CASES = {
    "dense": (dict(seed=8, K=12, F=1, M=1200, step=0.1, keep=0.9, depth=(2, 6)), 0, 3, 1e-6, 1e-6),
    "edges": (_EDGES, 12, 6, 1e-6, 1e-6),
    "edges_plain": (_EDGES, 0, 6, 1e-6, 1e-6),            # edges with every point in front: the local solver's F = 2 form agrees on it
    "loop": (dict(seed=2, K=40, F=1, M=800, step=1.0, keep=0.35, depth=(2, 6)), 6, 10, 1e-6, 1e-6),
    "converged": (dict(W.GLOBAL_CASES["global_k20"], noise_px=0.0, M=600), 0, 10, 1e-6, 1e-6),   # (M = 2000: |g| = 1.4e-8, not a hundredth of the tolerance)
    "gtol_stop": (_STOP_MAP, 0, 10, 1e-6, 2.3e3),
    "ptol_stop": (_STOP_MAP, 0, 10, 1e-4, 1e-6),
    "natural_stop": (_STOP_MAP, 0, 10, 1e-6, 1e-6),
}
# The stop-rule cases.  global_k20 cannot be pinned.  As it is, |g| stays between 1.6e5 and 4.7e5 over its 10 iterations and |delta|
# falls by less than a factor of 2 from one iteration to the next, and a stop that survives the tolerance halved AND doubled needs a
# factor of 4 between the iteration that stops and every one before it.  With less pixel noise (and other seeds) it does converge in
# mid-course, but its corridor is so loosely coupled that after five accepted steps the reference's own answer moves by 3e-6 (poses) with
# the order of the observation array, and by 3e-5 after six: the reference does not pin the answer to the project's 1e-6.  The dense
# map does (1e-13), and with a hundredth of a pixel of noise it converges 10- to 80-fold per iteration with every decision 1e-2 or more
# from a tie: the parameter rule ends it in iteration 5 at the default tolerances (natural_stop), and either rule in iteration 4 with its
# tolerance raised.  The dense case itself (one pixel of noise) cannot serve as the natural stop: from iteration 4 on its decisions are
# within 2e-5 of a tie.
# name -> (rule, the iteration the reference stops in)
STOP = {"converged": ("gradient", 1), "gtol_stop": ("gradient", 4), "ptol_stop": ("param", 4), "natural_stop": ("param", 5)}
LOOP_POINTS = 20
LOOP_KEYFRAMES = (0, 1, 2, 3, 36, 37, 38, 39)
EDGE_ORDERS = ("shuffled", "kf_major", "reversed")
_cache = {}
_oracle_cache = {}


def _with_loop_points(w, kw):
    """LOOP_POINTS points far behind the middle of the corridor (large_ba_windows._covis_with_common_points says why every camera sees
    them there) that the keyframes LOOP_KEYFRAMES alone observe; they are the last points of the map"""
    cam = w["camera"]; n = LOOP_POINTS; M = len(w["points"])
    rng = np.random.default_rng([0xC6, kw["seed"]])
    span = kw["step"] * (kw["K"] + kw["F"])
    z0 = 2.0 * (span / 2 + 1.0) * cam["fx"] / cam["cx"]
    X = np.stack([span / 2 + rng.uniform(-1, 1, n), rng.uniform(-1.5, 1.5, n), rng.uniform(z0, z0 + 4.0, n)], 1)
    parts = [w["obs"]]
    for k in LOOP_KEYFRAMES:
        pose = w["gt_poses_cw"][k]
        pc = synth._quat_rot(pose[:4], X) + pose[4:]
        u = cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"]; v = cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]
        assert np.all((pc[:, 2] > 0.1) & (u >= 0) & (u < 752) & (v >= 0) & (v < 480)), "keyframe %d does not see a loop point" % k
        o = np.zeros(n, P.BA_OBS)
        o["kf_idx"] = k; o["fixed_idx"] = -1; o["mp_idx"] = M + np.arange(n); o["u"] = u + rng.normal(0, 1.0, n); o["v"] = v + rng.normal(0, 1.0, n)
        parts.append(o)
    w["obs"] = np.concatenate(parts)
    w["points"] = np.concatenate([w["points"], X + rng.normal(0, 0.03, X.shape)])
    w["gt_points"] = np.concatenate([w["gt_points"], X])
    w["loop_points"] = M + np.arange(n)
    return w


def case(name, order="shuffled"):
    """the case's map (made once per order and process; read-only).  Orders other than "shuffled" are for edges."""
    if (name, order) not in _cache:
        kw, n_behind, _, _, _ = CASES[name]
        if name == "loop":
            w = _with_loop_points(W.covis_window(order="kf_major", **kw), kw)
            w["obs"] = W.reorder(w["obs"], order, kw["seed"])
        else:
            w = W.covis_window(order=order, **kw)
        if name == "converged":
            w["poses_cw"] = w["gt_poses_cw"].copy(); w["points"] = w["gt_points"].copy()
        w["behind"] = np.zeros(0, np.int64)
        if n_behind:
            w = G._with_points_behind(w, kw["seed"], kw["M"], n_behind)
        w["unobserved"] = np.flatnonzero(np.bincount(w["obs"]["mp_idx"], minlength=len(w["points"])) == 0)
        _cache[(name, order)] = w
    return _cache[(name, order)]


def config(name, **override):
    """the keyword arguments of GlobalBAConfig for the case"""
    _, _, it, ptol, gtol = CASES[name]
    return dict(dict(max_iterations=it, param_tolerance=ptol, gradient_tolerance=gtol), **override)


def oracle_answer(oracle, name, order="shuffled", stop_after=-1, **override):
    """global_ba_solve_schur on the case with the case's configuration (`override` replaces fields of it), once per process"""
    c = config(name, **override)
    key = (name, order, stop_after, c["max_iterations"], c["param_tolerance"], c["gradient_tolerance"])
    if key not in _oracle_cache:
        w = case(name, order)
        cfg = oracle.BaConfig(c["max_iterations"], c["param_tolerance"], c["gradient_tolerance"], HUBER, 0)
        _oracle_cache[key] = oracle.global_ba_solve_schur(oracle.Camera(**w["camera"]), cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"], stop_after=stop_after)
    return _oracle_cache[key]


def is_identity(obs):
    return (obs["kf_idx"] < 0) & (obs["fixed_idx"] < 0)


def behind_depths(w):
    """depth, at the initial poses, of every observation of a point in w["behind"] in the camera that makes it (the identity pose included)"""
    ob = w["obs"][np.isin(w["obs"]["mp_idx"], w["behind"])]
    ident = np.array([1.0, 0, 0, 0, 0, 0, 0])
    d = []
    for o in ob:
        p = w["poses_cw"][o["kf_idx"]] if o["kf_idx"] >= 0 else (w["fixed_cw"][o["fixed_idx"]] if o["fixed_idx"] >= 0 else ident)
        d.append((synth._quat_rot(p[:4], w["points"][o["mp_idx"]][None])[0] + p[4:])[2])
    return np.array(d)


def identity_as_second_fixed(w):
    """the map with its identity observations rewritten as observations of a second fixed keyframe that IS the identity pose"""
    w2 = dict(w)
    w2["fixed_cw"] = np.concatenate([w["fixed_cw"], [[1.0, 0, 0, 0, 0, 0, 0]]])
    o = w["obs"].copy(); o["fixed_idx"][is_identity(o)] = len(w["fixed_cw"])
    w2["obs"] = o
    return w2


def poses_wc(poses_cw):
    """[K,7] world-to-camera -> camera-to-world"""
    p = np.asarray(poses_cw, np.float64)
    qi = p[:, :4] * np.array([1.0, -1.0, -1.0, -1.0])
    return np.concatenate([qi, -np.stack([synth._quat_rot(q, t[None])[0] for q, t in zip(qi, p[:, 4:])])], 1)


def shared_point_pairs(w):
    """[K,K] bool: the pairs of optimised keyframes that share a point, i.e. the non-zero blocks of the reduced system"""
    K = len(w["poses_cw"]); o = w["obs"][w["obs"]["kf_idx"] >= 0]
    A = np.zeros((len(w["points"]), K), np.int64); A[o["mp_idx"], o["kf_idx"]] = 1
    return (A.T @ A) > 0
