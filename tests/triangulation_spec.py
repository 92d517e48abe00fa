"""Specification of the pair loop of triangulate_from_neighbors (reference src/local_mapping/triangulation.rs:117-294) with
triangulate_dlt (:715-760) and validate_triangulation (:776-850), restated literally in numpy f64.

triangulate_pair returns (status, method, p_world, margin).  `margin` is the smallest relative distance of any comparison
the evaluation made to that comparison's threshold: |a - b| / max(|a|, |b|), or |a - b| / scale where the threshold is 0 and the
quantity has a natural scale (a depth against the point's distance, a cosine against 1).  A pair whose margin is below 1e-9 may
legitimately come out on the other side of a gate in another f64 implementation; every other pair may not.
"""
import math

import numpy as np

CREATED, SKIPPED, DLT_DEGENERATE, REJ_DEPTH, REJ_REPROJ1, REJ_REPROJ2, REJ_DIST, REJ_SCALE, BAD_INDEX = range(9)
DLT, STEREO_CURRENT, STEREO_NEIGHBOUR = range(3)
STATUS_NAMES = ["CREATED", "SKIPPED", "DLT_DEGENERATE", "REJ_DEPTH", "REJ_REPROJ1", "REJ_REPROJ2", "REJ_DIST", "REJ_SCALE", "BAD_INDEX"]
F64_MAX = float(np.finfo(np.float64).max)


def default_config():
    """TriangulationConfig::default (:39-52); TH_LOW = 50 (stereo.rs:10-12)."""
    return dict(num_neighbors=10, max_descriptor_dist=50, min_baseline_ratio=0.01, min_parallax_inertial=math.acos(0.9996),
                min_parallax_visual=math.acos(0.9998), max_reproj_error_mono=5.991, max_reproj_error_stereo=7.8, scale_ratio_factor=1.5)


def min_parallax_cos(cfg, is_inertial):
    return math.cos(cfg["min_parallax_inertial"]) if is_inertial else math.cos(cfg["min_parallax_visual"])   # :110-114


def rotation_matrix(q):
    """UnitQuaternion::to_rotation_matrix for (w, x, y, z)."""
    w, x, y, z = (float(v) for v in q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (w * y + x * z)],
                     [2 * (w * z + x * y), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (w * x + y * z), w * w - x * x - y * y + z * z]])


def pose_inverse(pose):
    """SE3::inverse of (qw,qx,qy,qz,tx,ty,tz): (q^-1, -(q^-1 t))."""
    pose = np.asarray(pose, np.float64)
    qi = pose[:4] * np.array([1.0, -1.0, -1.0, -1.0])
    return np.concatenate([qi, -(rotation_matrix(qi) @ pose[4:])])


def transform_point(pose, p):
    return rotation_matrix(pose[:4]) @ np.asarray(p, np.float64) + np.asarray(pose[4:], np.float64)


class _Margin:
    def __init__(self):
        self.m = math.inf

    def le(self, a, b, scale=None):
        """a <= b, recording how close the comparison was (a NaN compares false, as in the reference)."""
        self.lt(a, b, scale)
        return a <= b

    def lt(self, a, b, scale=None):
        """a < b, recording how close the comparison was."""
        s = max(abs(a), abs(b)) if scale is None else scale
        if math.isfinite(a) and math.isfinite(b) and b != F64_MAX and a != F64_MAX:
            self.m = min(self.m, abs(a - b) / s if s > 0 else 0.0)
        return a < b


def triangulate_dlt(xn1, xn2, pose1_wc, pose2_wc, mg=None):
    """:715-760.  Returns the point or None (|w| < 1e-10)."""
    mg = mg or _Margin()
    P = []
    for pose in (pose1_wc, pose2_wc):
        cw = pose_inverse(pose)
        P.append(np.concatenate([rotation_matrix(cw[:4]), cw[4:, None]], axis=1))        # projection_matrix (:763-773)
    A = np.zeros((4, 4))
    A[0] = xn1[0] * P[0][2] - P[0][0]; A[1] = xn1[1] * P[0][2] - P[0][1]
    A[2] = xn2[0] * P[1][2] - P[1][0]; A[3] = xn2[1] * P[1][2] - P[1][1]
    v = np.linalg.svd(A)[2][3]                                                            # right singular vector of the smallest singular value
    if mg.lt(abs(v[3]), 1e-10):
        return None
    return v[:3] / v[3]


def triangulate_pair(cam, cfg, is_inertial, kp1, pts1, has1, pose1_wc, kp2, pts2, has2, pose2_wc, idx1, idx2):
    """One (idx1, idx2) of the loop at :184-293.  cam / cfg are dicts; kp KEYPOINT records; pts [n,3] f64; has [n] u8."""
    if not (0 <= idx1 < len(kp1) and 0 <= idx2 < len(kp2)):
        return BAD_INDEX, DLT, np.zeros(3), math.inf
    mg = _Margin()
    pose1_wc = np.asarray(pose1_wc, np.float64); pose2_wc = np.asarray(pose2_wc, np.float64)
    fx, fy, cx, cy, bl = (float(cam[k]) for k in ("fx", "fy", "cx", "cy", "baseline"))
    s1 = np.asarray(pts1[idx1], np.float64) if has1[idx1] else None                      # :186-187
    s2 = np.asarray(pts2[idx2], np.float64) if has2[idx2] else None
    u1, v1 = float(kp1["x"][idx1]), float(kp1["y"][idx1])                                 # f32 widened to f64
    u2, v2 = float(kp2["x"][idx2]), float(kp2["y"][idx2])
    xn1 = np.array([(u1 - cx) / fx, (v1 - cy) / fy, 1.0])                                 # :194-203
    xn2 = np.array([(u2 - cx) / fx, (v2 - cy) / fy, 1.0])
    ray1 = rotation_matrix(pose1_wc[:4]) @ xn1; ray2 = rotation_matrix(pose2_wc[:4]) @ xn2
    cos_par = float(ray1 @ ray2) / (math.sqrt(float(ray1 @ ray1)) * math.sqrt(float(ray2 @ ray2)))   # :208
    stereo_cos = lambda p: math.cos(2.0 * math.atan(bl / 2.0 / float(p[2])))              # :211-218
    with np.errstate(divide="ignore"):
        c1 = stereo_cos(s1) if s1 is not None and s1[2] != 0 else (math.cos(math.pi) if s1 is not None else None)
        c2 = stereo_cos(s2) if s2 is not None and s2[2] != 0 else (math.cos(math.pi) if s2 is not None else None)
    cs = min(c1, c2) if (c1 is not None and c2 is not None) else (c1 if c1 is not None else (c2 if c2 is not None else F64_MAX))
    mpc = min_parallax_cos(cfg, is_inertial)
    use_dlt = mg.lt(cos_par, cs) and mg.lt(0.0, cos_par, 1.0) and (s1 is not None or s2 is not None or mg.lt(cos_par, mpc))   # :227-229
    if use_dlt:
        method = DLT
        p = triangulate_dlt(xn1, xn2, pose1_wc, pose2_wc, mg)
        if p is None:
            return DLT_DEGENERATE, method, np.zeros(3), mg.m
    elif s1 is not None:
        if mg.lt(c1, c2 if c2 is not None else F64_MAX):                                  # :239
            method = STEREO_CURRENT; p = transform_point(pose1_wc, s1)
        elif s2 is not None:
            method = STEREO_NEIGHBOUR; p = transform_point(pose2_wc, s2)
        else:
            return SKIPPED, DLT, np.zeros(3), mg.m                                        # :245
    elif s2 is not None:
        method = STEREO_NEIGHBOUR; p = transform_point(pose2_wc, s2)                      # :247-249
    else:
        return SKIPPED, DLT, np.zeros(3), mg.m                                            # :252
    # validate_triangulation (:776-850)
    pc1 = transform_point(pose_inverse(pose1_wc), p); pc2 = transform_point(pose_inverse(pose2_wc), p)
    n1 = float(np.linalg.norm(pc1)); n2 = float(np.linalg.norm(pc2))
    if mg.le(float(pc1[2]), 0.0, n1) or mg.le(float(pc2[2]), 0.0, n2):                   # :794 (a NaN depth passes, as there)
        return REJ_DEPTH, method, p, mg.m
    for pc, u, v, st, code in ((pc1, u1, v1, s1 is not None, REJ_REPROJ1), (pc2, u2, v2, s2 is not None, REJ_REPROJ2)):
        ex = fx * pc[0] / pc[2] + cx - u; ey = fy * pc[1] / pc[2] + cy - v               # :799-803
        lim = cfg["max_reproj_error_stereo"] if st else cfg["max_reproj_error_mono"]
        if mg.lt(lim, float(ex * ex + ey * ey) / 1.0):                                    # :808, :821
            return code, method, p, mg.m
    d1 = float(np.linalg.norm(p - pose1_wc[4:])); d2 = float(np.linalg.norm(p - pose2_wc[4:]))   # :826-829
    if mg.lt(d1, 1e-6) or mg.lt(d2, 1e-6):
        return REJ_DIST, method, p, mg.m
    ratio_dist = d2 / d1
    ratio_oct = math.pow(1.2, float(kp1["octave"][idx1])) / math.pow(1.2, float(kp2["octave"][idx2]))   # :838-841
    f = cfg["scale_ratio_factor"]
    if mg.lt(ratio_dist * f, ratio_oct) or mg.lt(ratio_oct * f, ratio_dist):             # :843-844
        return REJ_SCALE, method, p, mg.m
    return CREATED, method, p, mg.m


def triangulate_from_neighbors(oracle, cam, cfg, is_inertial, current, neighbours):
    """The neighbour loop (:117-294) on keyframe dicts {kp, desc, mp, pts, has, pose, node (or None)}; `oracle` is the CPU oracle
    module whose searches give the pairs.  Returns (created, stats, result, evaluated): created = [(t, idx1, idx2, p_world)],
    stats [T][4] = searched, matches_found, triangulated, validated; result = the reference's five counters;
    evaluated = [(t, idx1, idx2, status, method, p, margin)] for every pair."""
    ocam = oracle.Camera(**{k: cam[k] for k in ("fx", "fy", "cx", "cy", "baseline")})
    created, evaluated = [], []
    stats = np.zeros((len(neighbours), 4), np.int32)
    res = dict(num_new_points=0, num_pairs_checked=0, num_matches_found=0, num_triangulated=0, num_validated=0)
    c1 = np.asarray(current["pose"], np.float64)[4:]
    for t, nb in enumerate(neighbours):
        res["num_pairs_checked"] += 1                                                     # :118
        if float(np.linalg.norm(np.asarray(nb["pose"], np.float64)[4:] - c1)) < cam["baseline"]:   # :137-141
            continue
        if len(current["kp"]) == 0 or len(nb["kp"]) == 0:
            continue
        a = (current["kp"], current["desc"], current["mp"], current["has"])
        if current.get("node") is not None and nb.get("node") is not None:               # :145
            pairs = oracle.search_for_triangulation_bow(ocam, *a, current["node"], nb["kp"], nb["desc"], nb["mp"], nb["node"],
                                                        current["pose"], nb["pose"], cfg["max_descriptor_dist"])
        else:
            pairs = oracle.search_for_triangulation(ocam, *a, nb["kp"], nb["desc"], nb["mp"], current["pose"], nb["pose"],
                                                    cfg["max_descriptor_dist"])
        stats[t, 0] = 1; stats[t, 1] = len(pairs)
        res["num_matches_found"] += len(pairs)
        for i1, i2 in pairs:
            st, me, p, m = triangulate_pair(cam, cfg, is_inertial, current["kp"], current["pts"], current["has"], current["pose"],
                                            nb["kp"], nb["pts"], nb["has"], nb["pose"], int(i1), int(i2))
            evaluated.append((t, int(i1), int(i2), st, me, p, m))
            if st in (SKIPPED, DLT_DEGENERATE):
                continue
            stats[t, 2] += 1; res["num_triangulated"] += 1                                # :260
            if st != CREATED:
                continue
            stats[t, 3] += 1; res["num_validated"] += 1                                   # :277
            created.append((t, int(i1), int(i2), p))
    res["num_new_points"] = len(created)
    return created, stats, res, evaluated
