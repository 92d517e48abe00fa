"""The caller's inertial state for the sessions of tests/map_session_scenes.py: what a stereo-inertial mapper holds beside the resident
map once the IMU is initialised, for tests/map_inertial_session_spec.py's model and the device (tests/test_map_inertial_session_cpu.py,
tests/test_map_inertial_session_gpu.py).  map_session_scenes.session(seed) is used unchanged: the same keyframes, landmarks, priors,
CAPACITY and mapper constants.

inertial(seed) -> the ground truth and the initial state of the nine keyframes, DT apart:
  gt_velocities  central differences of the camera centres (one-sided at the two ends), so that they are consistent with them
  gt_bias        one small bias (gyro 1e-3, accelerometer 1e-2) for every keyframe
  preint         {(i, i + 1): [11]} for every consecutive pair and {(i, i + 2): [11]} for every pair one keyframe apart, each built by
                 inertial_edge_windows.skip_edge from the ground truth: the exact deltas over (j - i) DT plus seeded noise of the
                 generator's magnitudes (2e-3 rad, 5e-3 m/s, 2e-3 m).  The second kind is the merged edge a mapper holds after it
                 dropped the keyframe in between.
  velocities, biases   the initial state: the truth perturbed as synth.inertial_window perturbs its own (0.05 m/s; 2e-3 and 2e-2)
The world's gravity is inertial_edge_windows.GRAVITY, along the optical axis of these cameras.

chain(listed) / edges(chain members) state the chain rule: the last INERTIAL_WINDOW listed keyframes, oldest first, one edge per
consecutive pair; two members with an unlisted keyframe between them (the redundancy drop) get the two-interval preintegration.
Keyframe EMPTY stays in the chain with its IMU edges and no observation.

IMU_INIT = 3 is the first step whose BA is inertial: steps 1 and 2 are visual and the switch happens in mid-session.
INERTIAL_WINDOW = 5.  With a chain of four the keyframe that seed 1 unlists (keyframe 1, at step 4) has left the chain before the next
window is collected, so that seed never sees a skip edge, and no window holds 100 points in slots that held a point before (93 at
most); with five both seeds have a skip edge and seed 1's last window holds 101.  The chain is the whole list up to step 4 (seed 2)
or 5 (seed 1): no fixed observer but the anchor, F = 1; from then on older listed keyframes are fixed observers, up to F = 4.
INERTIAL_ITERATIONS = 4 is the mapper's LocalInertialBAConfig::max_iterations.  The reference's default of ten cannot be held to
the margin rule here: the keyframes of these sessions hardly rotate (MAX_ROT), the windows are close to linear, and the solver, which
has no convergence test, goes on to relative decreases of 1e-10 and less from the sixth iteration on and ends where every accept /
reject decision is a tie (smallest margins of 1e-16 and 0 at seeds 1 and 2).  Over seeds 1 to 4 the smallest margin of a session
is 6.6e-6 to 1.1e-4 with four iterations and 4.8e-9 to 8.9e-7 with five; four is the largest count at which seeds 1 and 2, for
which map_session_scenes chose CAPACITY and the mapper's constants, both pass.

SEEDS are the first two of CANDIDATES for which the model alone keeps every LM accept / reject decision of every inertial step at
least inertial_edge_windows.MARGIN (1e-7 relative) from a tie (orientation_cases.lm_margin on the oracle's trace);
tests/test_map_inertial_session_cpu.py recomputes the rule.  The model alone (every BA by the oracle) gives per inertial step
K / F / M / N / stereo share of the observations / E / skip edge / blind keyframe in the chain / window points in slots that held a
point before (in slots on their third point or later) / iterations, and the step's smallest margin:

  seed 1  3: 4/1/333/1047/0.371/3/-/-/28(2)/4  2.68e-04          seed 2  3: 4/1/340/1055/0.420/3/-/-/36(3)/4  2.24e-04
          4: 5/1/348/1364/0.377/4/-/-/46(8)/4  5.73e-04                  4: 4/1/343/1160/0.415/3/skip/-/53(11)/4  3.18e-03
          5: 5/1/344/1329/0.391/4/skip/-/54(13)/4  1.28e-03              5: 5/1/344/1401/0.418/4/skip/-/64(19)/4  1.93e-04
          6: 5/2/331/1283/0.391/4/-/blind/54(13)/4  5.99e-03             6: 5/2/335/1360/0.415/4/skip/blind/62(17)/4  2.42e-03
          7: 5/3/361/1422/0.409/4/-/blind/76(28)/4  1.07e-04             7: 5/3/343/1471/0.417/4/-/blind/72(23)/4  1.81e-04
          8: 5/4/370/1738/0.411/4/-/blind/101(43)/4  1.46e-04            8: 5/4/352/1733/0.423/4/-/blind/91(38)/4  6.63e-06

Smallest margins: 1.071e-04 (seed 1), 6.631e-06 (seed 2).  Keyframe 1 (seed 1, at step 4) and keyframe 2 (seed 2, at step 3) are
unlisted, as in the visual session.  What the scenes can and cannot see (tests/test_map_inertial_session_cpu.py, seed 2): without the
stereo bits, or with has_point by the way a feature's point was created, obs32 differs at step 3; biases not carried move the
returned biases by 9.6e-3 at step 4 and nothing else by more than 1e-9; the one-interval preintegration on the skip edge moves
the poses by 6.9e-2 at step 4 and then the outlier removal.  A solver that ignored the stereo bit would move nothing by more than
9.7e-7: the bit only chooses the Huber threshold and no observation of these sessions lies between the two thresholds.
"""
import numpy as np

import inertial_edge_windows as E
import map_session_scenes as W

DT = E.DT
IMU_INIT = 3
INERTIAL_WINDOW = 5
INERTIAL_ITERATIONS = 4
CANDIDATES = (1, 2, 3, 4, 5, 6)
SEEDS = (1, 2)

_cache = {}


def inertial(seed):
    """-> dict(gt_poses_wc [9,7], gt_velocities [9,3], gt_bias [6], velocities [9,3], biases [9,6], preint {(i, j): [11]}).  Cached: never
    modify it."""
    if seed in _cache:
        return _cache[seed]
    sess = W.session(seed)
    rng = np.random.default_rng([0x1A5E, seed])
    gt = np.array(sess["poses"], np.float64, copy=True)
    c = gt[:, 4:]
    v = np.empty_like(c)
    v[1:-1] = (c[2:] - c[:-2]) / (2 * DT); v[0] = (c[1] - c[0]) / DT; v[-1] = (c[-1] - c[-2]) / DT
    w = dict(gt_poses_wc=gt, gt_velocities=v, edge_kf=np.zeros((0, 2), np.int32), preint=np.zeros((0, 11)))
    for span in (1, 2):
        for i in range(W.N_KF - span):
            w = E.skip_edge(w, i, i + span, rng)
    pre = {(int(i), int(j)): row.copy() for (i, j), row in zip(w["edge_kf"], w["preint"])}
    bias = np.concatenate([rng.normal(0, 1e-3, 3), rng.normal(0, 1e-2, 3)])
    vel0 = v + rng.normal(0, 0.05, (W.N_KF, 3))
    bias0 = bias + np.concatenate([rng.normal(0, 2e-3, (W.N_KF, 3)), rng.normal(0, 2e-2, (W.N_KF, 3))], 1)
    _cache[seed] = dict(gt_poses_wc=gt, gt_velocities=v, gt_bias=bias, velocities=vel0, biases=bias0, preint=pre)
    return _cache[seed]


def chain(listed):
    """the positions in kfs[] of the chain: the last INERTIAL_WINDOW listed keyframes (they are listed in temporal order)"""
    assert list(listed) == sorted(listed)
    return list(range(max(len(listed) - INERTIAL_WINDOW, 0), len(listed)))


def edges(imu, members, merged=True):
    """members: the chain's keyframes, oldest first -> (edge_kf int32 [K - 1, 2] of positions in the chain, preint [K - 1, 11], the
    number of edges that span two intervals).  merged=False is the fault of tests/test_map_inertial_session_cpu.py's variant (d): the
    last interval's preintegration where the merged one belongs."""
    ek, pre, skips = [], [], 0
    for p, (a, b) in enumerate(zip(members[:-1], members[1:])):
        assert 1 <= b - a <= 2
        skips += b - a == 2
        ek.append((p, p + 1)); pre.append(imu["preint"][(a, b) if merged else (b - 1, b)])
    return np.array(ek, np.int32).reshape(-1, 2), np.array(pre, np.float64).reshape(-1, 11), skips
