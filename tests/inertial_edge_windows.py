"""Inertial-BA windows whose IMU edge graph is not an ascending chain (tests/test_inertial_edges_cpu.py, tests/test_inertial_edges_gpu.py).

Test infrastructure only; no GPU import.  synth.inertial_window lists its IMU edges as (k, k + 1) for k = 0 .. K - 2: always older -> newer
with ki < kj, in ascending order, one dt, an edge on both sides of every interior keyframe and every keyframe seen by dozens of points.  The
15K x 15K assembly of the solver (csrc/ba_kernels.hip: the tiled form in LDS up to 11 keyframes, the global form beyond) takes the edges as
an arbitrary list of index pairs, and its branches (which half of an 18 x 18 edge record lands in the lower triangle, max / min of the two
bias rows of the random walk, the E == 0 guards, rows that carry only the damping) see one side only from such a window.  The helpers here
turn a synth.inertial_window dict into a window of the same keys with another edge graph:

- relabel: the same physical window with its keyframes listed in another order — edge (i, j) is still the edge from the older to the newer
  keyframe, so the answer is the chain's answer under the permutation;
- reorder_edges, drop_edges, skip_edge (a preintegration over two keyframe intervals from the ground truth, dt = 0.5), blind, pad.

NAMES / build() are the named cases, case() picks the seed by the rule of tests/test_orientation_gpu.py's _inertial_scene: the first seed
of 31 + 7919 s whose oracle trace keeps every LM accept / reject decision MARGIN (relative) away from a tie.
"""
import numpy as np

import orb_slam3_rust_amd as P
from oracle import oracle as O
import orientation_cases as C

synth = P.synth
MARGIN = 1e-7                       # tests/test_orientation_gpu.py's constant
DT = 0.25                           # synth.inertial_window's default keyframe spacing
GRAVITY = np.array([0.0, 0.0, -9.81])
NAMES = ("descending", "shuffled", "gap", "no_edges", "skip", "duplicate", "blind", "descending_skip_gap")
# the smallest windows that reach each solve path (n_fixed = 1): K = 5 and K = 11 the tiled LDS solve (K = 11: its largest system, 66 tiles),
# K = 13 the one-launch global factorisation, K = 22 one launch per panel (15 K = 330)
POINTS = {5: 60, 11: 250, 13: 250, 22: 150}
CASES = [(n, K) for K in (5, 11) for n in NAMES] + [(n, 13) for n in ("descending", "shuffled", "gap", "skip", "no_edges")] + \
        [(n, 22) for n in ("descending", "descending_skip_gap")]
OUTPUTS = ("poses_wc", "velocities", "biases", "points")
_PER_KF = ("poses_wc", "velocities", "biases", "gt_poses_wc", "gt_velocities")


def rel(a, b):
    """tests/test_inertial_ba.py's _rel"""
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


def oracle(w, **kw):
    return O.inertial_ba_solve(O.Camera(**w["camera"]), O.inertial_ba_config(), w["poses_wc"], w["velocities"], w["biases"], w["fixed_cw"],
                               w["points"], w["obs"], w["edge_kf"], w["preint"], **kw)


def _copy(w):
    return {k: (v.copy() if isinstance(v, np.ndarray) else dict(v)) for k, v in w.items()}


def relabel(w, perm):
    """Keyframe perm[i] of `w` becomes keyframe i: the per-keyframe arrays are reordered by `perm`, edge_kf and obs["kf_idx"] (where >= 0)
    go through its inverse.  The preintegrations are untouched: edge (i, j) still runs from the older keyframe to the newer one."""
    perm = np.asarray(perm, np.int64)
    K = len(w["poses_wc"])
    assert sorted(perm.tolist()) == list(range(K))
    inv = np.empty(K, np.int64); inv[perm] = np.arange(K)
    r = _copy(w)
    for key in _PER_KF:
        r[key] = w[key][perm].copy()
    r["edge_kf"] = inv[w["edge_kf"].astype(np.int64)].astype(np.int32).reshape(-1, 2)
    kf = w["obs"]["kf_idx"]
    r["obs"]["kf_idx"] = np.where(kf >= 0, inv[np.maximum(kf, 0)], kf).astype(kf.dtype)
    return r


def reorder_edges(w, order):
    """the rows of edge_kf and preint in the order `order` (a permutation of the edges)"""
    order = np.asarray(order, np.int64)
    assert sorted(order.tolist()) == list(range(len(w["edge_kf"])))
    r = _copy(w)
    r["edge_kf"] = w["edge_kf"][order].copy(); r["preint"] = w["preint"][order].copy()
    return r


def drop_edges(w, which):
    keep = np.array([e for e in range(len(w["edge_kf"])) if e not in set(int(x) for x in which)], np.int64)
    r = _copy(w)
    r["edge_kf"] = w["edge_kf"][keep].reshape(-1, 2).copy(); r["preint"] = w["preint"][keep].reshape(-1, 11).copy()
    return r


def preintegration(w, i, j, dt):
    """the exact deltas between keyframes i and j of the ground truth (synth.inertial_window's docstring): dR = Ri^-1 Rj,
    dv = Ri^-1 (vj - vi - g dt), dp = Ri^-1 (pj - pi - vi dt - g dt^2 / 2)"""
    gp, gv = w["gt_poses_wc"], w["gt_velocities"]
    qic = C.conj(gp[i, :4])
    dR = C.qmul(qic, gp[j, :4])
    dv = synth._quat_rot(qic, gv[j] - gv[i] - GRAVITY * dt)
    dp = synth._quat_rot(qic, gp[j, 4:] - gp[i, 4:] - gv[i] * dt - 0.5 * GRAVITY * dt * dt)
    return np.concatenate([dR / np.linalg.norm(dR), dv, dp, [dt]])


def skip_edge(w, i, j, rng=None):
    """`w` (keyframes in the generator's order, DT apart) with one more edge (i, j), appended: the preintegration over (j - i) DT from the
    ground truth plus noise of the generator's magnitudes (2e-3 rad, 5e-3 m/s, 2e-3 m); rng=None adds none."""
    pre = preintegration(w, i, j, (j - i) * DT)
    if rng is not None:
        dR = C.qmul(pre[:4], synth._quat_from_axis_angle(rng.normal(0, 1, 3), rng.normal(0, 2e-3)))
        pre[:4] = dR / np.linalg.norm(dR)
        pre[4:7] += rng.normal(0, 5e-3, 3)
        pre[7:10] += rng.normal(0, 2e-3, 3)
    r = _copy(w)
    r["edge_kf"] = np.concatenate([w["edge_kf"], np.array([[i, j]], np.int32)]).astype(np.int32)
    r["preint"] = np.concatenate([w["preint"], pre[None]])
    return r


def blind(w, k):
    """keyframe k loses every visual observation"""
    r = _copy(w)
    r["obs"] = w["obs"][w["obs"]["kf_idx"] != k].copy()
    return r


def pad(w):
    """one more keyframe at the end with no IMU edge and no observation (its states: the last keyframe's): 15 rows that carry only the
    damping and give a zero step"""
    r = _copy(w)
    for key in _PER_KF:
        r[key] = np.concatenate([w[key], w[key][-1:]])
    return r


def permutation(name, K):
    """the keyframe relabelling of the named case (build(name) lists keyframe permutation[i] of the generator's window as keyframe i)"""
    if name in ("descending", "descending_skip_gap"):
        return np.arange(K)[::-1].copy()
    if name == "shuffled":
        return np.random.default_rng([0xED6E, K]).permutation(K)
    return np.arange(K)


def _with_skips(w, seed):
    rng = np.random.default_rng([0x5C1B, seed])
    for k in range(0, len(w["poses_wc"]) - 2, 2):
        w = skip_edge(w, k, k + 2, rng)
    return w


def build(name, seed, K, M):
    """the named case on synth.inertial_window(seed, K, M, n_fixed=1); "chain" is the generator's window itself"""
    w = synth.inertial_window(seed, K, M, P.BA_OBS, n_fixed=1)
    if name == "chain":
        return w
    if name == "descending":
        return relabel(w, permutation(name, K))
    if name == "shuffled":
        r, rng = relabel(w, permutation(name, K)), np.random.default_rng([0xED6F, K])
        while True:                                                        # (a draw that happens to sort the list is drawn again)
            s = reorder_edges(r, rng.permutation(K - 1))
            if s["edge_kf"].tolist() != sorted(s["edge_kf"].tolist()):
                return s
    if name == "gap":
        return drop_edges(w, [K // 2, 0])
    if name == "no_edges":
        return drop_edges(w, range(K - 1))
    if name == "skip":
        return _with_skips(w, seed)
    if name == "duplicate":
        r = _copy(w)
        r["edge_kf"] = np.concatenate([w["edge_kf"], w["edge_kf"][1:2]]); r["preint"] = np.concatenate([w["preint"], w["preint"][1:2]])
        return r
    if name == "blind":
        return blind(w, 2)
    if name == "descending_skip_gap":
        return relabel(drop_edges(_with_skips(w, seed), [K // 2]), permutation(name, K))
    if name == "shuffled_padded":                                          # K counts the padding keyframe
        return pad(build("shuffled", seed, K - 1, M))
    raise KeyError(name)


SEEDS = [31 + 7919 * s for s in range(40)]
_cache = {}


def solved(name, seed, K, M):
    """(window, oracle result) of build(name, seed, K, M), cached per process; the results are shared: do not write to them"""
    key = (name, seed, K, M)
    if key not in _cache:
        w = build(name, seed, K, M)
        _cache[key] = (w, oracle(w))
    return _cache[key]


def case(name, K, M=None):
    """(seed, window, oracle result) of the first seed whose oracle solve has every LM decision at least MARGIN from a tie"""
    M = POINTS[K] if M is None else M
    for seed in SEEDS:
        w, o = solved(name, seed, K, M)
        if C.lm_margin(o["trace"]) >= MARGIN:
            return seed, w, o
    raise AssertionError("no seed of %s at K = %d keeps every LM decision %.0e from a tie" % (name, K, MARGIN))


def map_back(result, perm):
    """the result of a relabelled window in the generator's keyframe order (keyframe i of the relabelled window is keyframe perm[i])"""
    inv = np.empty(len(perm), np.int64); inv[perm] = np.arange(len(perm))
    r = dict(result)
    for key in ("poses_wc", "velocities", "biases"):
        r[key] = result[key][inv]
    return r


def relabel_spread(name, K):
    """The oracle on a relabelled case and on the chain of the same seed, mapped back: the largest difference over the outputs (rel) and
    the errors (relative) — what relabelling costs the oracle itself.  -> seed, spread"""
    seed, _, o = case(name, K)
    _, oc = solved("chain", seed, K, POINTS[K])
    ob = map_back(o, permutation(name, K))
    spread = max([rel(ob[k], oc[k]) for k in OUTPUTS] + [abs(o[k] - oc[k]) / oc[k] for k in ("initial_error", "final_error")])
    return seed, (spread if o["iterations"] == oc["iterations"] else np.inf)


def padded_pair():
    """The shuffled edge graph at K = 11 (tiled assembly) and the same window padded to K = 12 (global assembly): the first seed at which
    BOTH oracle solves keep their margins.  -> seed, (w11, o11), (w12, o12)"""
    for seed in SEEDS:
        a, b = solved("shuffled", seed, 11, POINTS[11]), solved("shuffled_padded", seed, 12, POINTS[11])
        if min(C.lm_margin(a[1]["trace"]), C.lm_margin(b[1]["trace"])) >= MARGIN:
            return seed, a, b
    raise AssertionError("no seed for the padded pair")
