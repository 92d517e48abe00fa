"""World rotations for the orientation tests (tests/test_orientation_cpu.py, tests/test_orientation_gpu.py).

Test infrastructure only.  Every generator of synth takes a world rotation G (a unit quaternion) that turns its finished scene about
the world origin.  Two kinds of case:

- a plain G: EuRoC's camera orientation with a yaw; uniformly random rotations, half of them with w < 0; rotations of pi - 1e-9,
  exactly pi (w = 0) and pi + 1e-9 (w < 0) about an oblique axis; the identity turned by 1e-12 and 1e-9 rad;
- an anchored G: the G that puts the first solver-input pose of the scene (the first optimised keyframe, the PnP prior, the
  pose-inertial initial pose) exactly on a rotation of 1e-12 or 1e-9 rad (either side of the 1e-10 cut of se3_from_params), of
  pi - 1e-9, pi or pi + 1e-9.  The pose is then set to that quaternion exactly — it differs from G's product by rounding only — so the
  solver's scaled axis starts on the edge itself.  A plain G cannot reach these edges: the generators' first optimised keyframe is
  never near the identity.
"""
import numpy as np

import orb_slam3_rust_amd as P

synth = P.synth
AXIS = np.array([0.3, -0.8, 0.52]) / np.linalg.norm([0.3, -0.8, 0.52])


def _random_rotations(n, seed=5):
    """uniform on SO(3) (normalised 4-d Gaussians); the sign is then chosen so that every odd one has w < 0"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        if (q[0] < 0) != (i % 2 == 1):
            q = -q
        out.append(q)
    return out


PLAIN = [("euroc_yaw2.3", synth.euroc_orientation(2.3)), ("euroc_yaw-1.2", synth.euroc_orientation(-1.2))] + \
        [("random%d" % i, q) for i, q in enumerate(_random_rotations(4))] + \
        [("pi-1e-9", synth.world_rotation(AXIS, np.pi - 1e-9)), ("pi", synth.world_rotation(AXIS, np.pi)),
         ("pi+1e-9", synth.world_rotation(AXIS, np.pi + 1e-9)),
         ("id+1e-12", synth.world_rotation(AXIS, 1e-12)), ("id+1e-9", synth.world_rotation(AXIS, 1e-9))]

ANCHORED = [("at1e-12", synth.world_rotation(AXIS, 1e-12)), ("at1e-9", synth.world_rotation(AXIS, 1e-9)),
            ("atpi-1e-9", synth.world_rotation(AXIS, np.pi - 1e-9)), ("atpi", synth.world_rotation(AXIS, np.pi)),
            ("atpi+1e-9", synth.world_rotation(AXIS, np.pi + 1e-9))]
CUT = ("id+1e-12", "id+1e-9", "at1e-12", "at1e-9")      # the cases at the 1e-10 cut: initial_error is compared within 1e-12 relative
IDS = [n for n, _ in PLAIN] + [n for n, _ in ANCHORED]

# which input pose an anchored case puts on the edge, and in which frame the generator stores it
_ANCHOR = dict(ba_window=("poses_cw", "cw"), inertial_window=("poses_wc", "wc"), pnp_problem=("prior_wc", "wc"),
               pose_inertial_problem=("pose_wc", "wc"))


def qmul(a, b):
    return synth._quat_mul(a, b)


def conj(q):
    return np.asarray(q, np.float64) * np.array([1.0, -1.0, -1.0, -1.0])


def scene(gen, case, *args, **kw):
    """synth.<gen>(*args, G=..., **kw) for the case named `case` ("identity" = G None)"""
    fn = getattr(synth, gen)
    if case == "identity":
        return fn(*args, **kw)
    plain = dict(PLAIN)
    if case in plain:
        return fn(*args, G=plain[case], **kw)
    delta = dict(ANCHORED)[case]
    key, frame = _ANCHOR[gen]
    q = np.asarray(fn(*args, **kw)[key], np.float64).reshape(-1, 7)[0, :4]
    # q_cw -> q_cw G^-1 = delta  <=>  G = delta^-1 q_cw;   q_wc -> G q_wc = delta  <=>  G = delta q_wc^-1
    G = qmul(conj(delta), q) if frame == "cw" else qmul(delta, conj(q))
    s = fn(*args, G=G / np.linalg.norm(G), **kw)
    a = np.array(s[key], np.float64, copy=True)
    a.reshape(-1, 7)[0, :4] = delta
    s[key] = a
    return s


def negate(scene, fields, alternate=False):
    """synth.with_quaternion_signs with -1 on every row of `fields` (every other row from the first when `alternate`) — but +1 on a row
    whose w is +-0: there nalgebra's `!(w >= 0)` test lets neither sign flip, so q = (+0, v) and -q = (-0, -v) give the scaled axes
    +pi v and -pi v (the same rotation, other rounding), and no byte-identical result is predicted"""
    signs = {}
    for f in fields:
        rows = np.asarray(scene[f], np.float64).reshape(-1, np.shape(scene[f])[-1])
        sg = np.where(np.arange(len(rows)) % 2 == 1, 1.0, -1.0) if alternate else np.full(len(rows), -1.0)
        signs[f] = np.where(rows[:, 0] == 0.0, 1.0, sg)
    return synth.with_quaternion_signs(scene, signs, fields)


def lm_margin(trace):
    """the smallest |trial - current| / current over an oracle trace's LM decisions (columns: current |r|^2, |g|, |delta|, trial)"""
    tr = np.asarray(trace).reshape(-1, 4)
    tr = tr[tr[:, 3] > 0]
    return float(np.min(np.abs(tr[:, 3] - tr[:, 0]) / tr[:, 0])) if len(tr) else np.inf
