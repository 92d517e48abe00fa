"""Seeded scenes for the camera tests: generators that take a case of tests/camera_cases.py and cover its whole image.

two_view()         two keyframes for search_for_triangulation / triangulate_pairs.  synth.two_view_features keeps its points within
                   +-5 m at 4..14 m and moves view 2 by 0.45 m whatever the focal length: at fx >= 1400 the pixel displacement leaves
                   the 100-px window and the bottom-right cells stay empty.  Here view-1 pixels are drawn over the whole image (a
                   chosen share in the bottom-right block), back-projected at a random depth, and the second pose's translation and
                   rotation are scaled by 458.654 / fx, so the displacement in pixels is the same at every camera.
stereo_features()  a left / right feature set whose disparities are drawn from the case's own [min_disp, min(max_disp, ul)].
guided_features()  keypoints and queries for guided_match at the case's image size, with keypoints on and beyond the image's edges and
                   queries whose search window ends exactly on a cell boundary.
fuse_scene()       synth.fuse_scene at the case's camera plus map points that project exactly to u, v in {0, 2c, the f64 below 2c}.
track_frame()      tracking_scenes.frame at the case's camera and image size; track_frames() the three frames the tests run.
pair_case()        pairs for triangulate_pairs from two_view(); with_nodes() adds FeatureVector nodes to it.
fused_scene()      a current keyframe and three neighbours for triangulate_from_neighbors.
"""
import numpy as np

import tracking_scenes as TS

KEYPOINT = TS.KEYPOINT
EUROC_FX = 458.654
CORNER = 260.0                                    # the bottom-right block of two_view(): the last CORNER px of each axis


def _quat(axis, ang):
    return TS._quat(axis, ang)


def _rot(q, v):
    return TS._rot(q, v)


def _conj(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def project(cam, pose_wc, X):
    pc = _rot(_conj(pose_wc[:4]), X - pose_wc[4:])
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"], cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]], 1)
    return uv, pc


def disparity_bounds(cam):
    """(max_disp, min_disp) as stereo.rs:84-90: f64 product and quotient, then f32."""
    return np.float32(cam["fx"] * cam["baseline"] / 0.1), np.float32(cam["fx"] * cam["baseline"] / 40.0)


def tri_grid_dims(cam):
    """(cols, rows) of search_for_triangulation's grid (triangulation.rs:434-438): u32 cast, f32 divide, ceil, min 64."""
    u32 = lambda v: int(min(max(v, 0.0), 4294967295.0))
    f = lambda v: int(min(np.ceil(np.float32(u32(2.0 * v)) / np.float32(32.0)), np.float32(64.0)))
    return f(cam["cx"]), f(cam["cy"])


def two_view(case, seed=3, n_points=3000, n_distractors=300, corner_share=0.3, dup=0.0):
    """The dict of synth.two_view_features (kp1, desc1, mp1, stereo1, kp2, desc2, mp2, pose1_wc, pose2_wc, camera) plus pts1 / has1 /
    pts2 / has2 (camera-frame stereo points of half the features, for triangulate_pairs) and gt [m,2] (the true index pairs)."""
    cam, w, h = dict(case["camera"]), float(case["w"]), float(case["h"])
    rng = np.random.default_rng([0xCA3E, seed])
    s = EUROC_FX / cam["fx"]
    n_c = int(corner_share * n_points)
    u = np.concatenate([rng.uniform(max(w - CORNER, 0.0), w, n_c), rng.uniform(0.0, w, n_points - n_c)])
    v = np.concatenate([rng.uniform(max(h - CORNER, 0.0), h, n_c), rng.uniform(0.0, h, n_points - n_c)])
    z = rng.uniform(5.0, 14.0, n_points)
    # the reference forms R12 as R2^-1 R1^-1 (triangulation.rs:428), the relative rotation only for R1 = I: view 1 barely turned
    pose1 = np.concatenate([_quat([0.0, 1.0, 0.0], 0.0005), [0.0, 0.0, 0.0]])
    pose2 = np.concatenate([_quat([0.1, 1.0, 0.05], -0.03 * s), np.array([0.45, 0.03, 0.05]) * s])
    X = TS.backproject(pose1, np.stack([u, v], 1), z, cam)
    uv1, pc1 = project(cam, pose1, X)
    uv2, pc2 = project(cam, pose2, X)
    ok = (pc2[:, 2] > 0.5) & (uv2[:, 0] > 0) & (uv2[:, 0] < w) & (uv2[:, 1] > 0) & (uv2[:, 1] < h)
    uv1, uv2, pc1, pc2 = uv1[ok], uv2[ok], pc1[ok], pc2[ok]
    m = len(uv1)
    d = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    if dup > 0:
        k = int(dup * m)
        d[rng.permutation(m)[:k]] = d[rng.integers(0, max(m // 20, 1), k)]
    flips = rng.random((m, 256)) < 0.03
    d2 = np.packbits(np.unpackbits(d, axis=1, bitorder="little") ^ flips.astype(np.uint8), axis=1, bitorder="little")
    out, where = {}, {}
    nd = n_distractors
    for name, uv, pc, dd in (("1", uv1, pc1, d), ("2", uv2, pc2, d2)):
        kp = np.zeros(m + nd, KEYPOINT)
        x = np.concatenate([uv[:, 0] + rng.normal(0, 0.4, m), rng.uniform(0, w, nd)])
        y = np.concatenate([uv[:, 1] + rng.normal(0, 0.4, m), rng.uniform(0, h, nd)])
        kp["x"] = np.clip(x, 0.0, np.nextafter(np.float32(w), np.float32(0))).astype(np.float32)
        kp["y"] = np.clip(y, 0.0, np.nextafter(np.float32(h), np.float32(0))).astype(np.float32)
        kp["size"] = 31.0
        kp["octave"] = rng.integers(0, 3, m + nd)
        desc = np.concatenate([dd, rng.integers(0, 256, (nd, 32), dtype=np.uint8)])
        has = (rng.random(m + nd) < 0.5).astype(np.uint8)
        pts = np.concatenate([pc * (1.0 + rng.normal(0, 0.01, m))[:, None], np.stack([np.zeros(nd), np.zeros(nd), rng.uniform(5.0, 14.0, nd)], 1)])
        pts = pts * has[:, None]
        perm = rng.permutation(m + nd)
        inv = np.empty(m + nd, np.int64); inv[perm] = np.arange(m + nd)
        where[name] = inv[:m]
        out["kp" + name] = kp[perm]; out["desc" + name] = desc[perm]
        out["pts" + name] = np.ascontiguousarray(pts[perm]); out["has" + name] = has[perm]
        out["mp" + name] = (rng.random(m + nd) < 0.3).astype(np.uint8)
    out["stereo1"] = out["has1"]
    out["pose1_wc"] = pose1; out["pose2_wc"] = pose2; out["camera"] = cam
    out["gt"] = np.stack([where["1"], where["2"]], 1).astype(np.int32)
    return out


def corner_pairs(s, pairs):
    """the pairs whose partner lies in grid row 63 and whose window reaches column 63: they read cell_start[64 * 64]"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    y2 = s["kp2"]["y"][pairs[:, 1]]
    x1 = s["kp1"]["x"][pairs[:, 0]]
    return pairs[(y2 >= 2016.0) & (np.ceil((x1 + np.float32(100.0)) / np.float32(32.0)) >= 63)]


def stereo_features(case, seed, n_left, n_right):
    """synth.matcher_features over the case's whole image (rows up to h), with the disparities of the corresponding 70 % drawn from
    the camera's own [min_disp, min(max_disp, ul)]."""
    cam, w, h = case["camera"], float(case["w"]), float(case["h"])
    max_d, min_d = (float(x) for x in disparity_bounds(cam))
    rng = np.random.default_rng([0x57E0, seed])
    kpL = np.zeros(n_left, KEYPOINT); kpR = np.zeros(n_right, KEYPOINT)
    top = lambda a: np.nextafter(np.float32(a), np.float32(0))
    kpL["x"] = np.minimum(rng.uniform(0, w, n_left).astype(np.float32), top(w)); kpL["y"] = np.minimum(rng.uniform(0, h, n_left).astype(np.float32), top(h))
    kpR["x"] = np.minimum(rng.uniform(0, w, n_right).astype(np.float32), top(w)); kpR["y"] = np.minimum(rng.uniform(0, h, n_right).astype(np.float32), top(h))
    descL = rng.integers(0, 256, (n_left, 32), dtype=np.uint8)
    descR = rng.integers(0, 256, (n_right, 32), dtype=np.uint8)
    n_corr = min(int(0.7 * n_right), n_left)
    src = rng.permutation(n_left)[:n_corr]
    dst = rng.permutation(n_right)[:n_corr]
    flips = rng.random((n_corr, 256)) < 0.06
    descR[dst] = np.packbits(np.unpackbits(descL[src], axis=1, bitorder="little") ^ flips.astype(np.uint8), axis=1, bitorder="little")
    ul = kpL["x"][src].astype(np.float64)
    hi = np.minimum(max_d, ul)
    disp = min_d + rng.random(n_corr) * np.maximum(hi - min_d, 0.0)
    kpR["y"][dst] = np.clip(kpL["y"][src] + rng.integers(-1, 2, n_corr).astype(np.float32), 0.0, top(h))
    kpR["x"][dst] = np.maximum(ul - disp, 0.0).astype(np.float32)
    for kp in (kpL, kpR):
        kp["size"] = 31.0
        kp["angle"] = rng.uniform(0, 360, len(kp)).astype(np.float32)
        kp["response"] = rng.uniform(0, 1e-3, len(kp)).astype(np.float32)
        kp["class_id"] = -1
    return kpL, descL, kpR, descR


STEREO_SIZES = [(300, 280), (1, 1), (17, 1500), (2100, 2300)]          # the last: more keypoints than the one-launch LDS form holds


def crowded_tall():
    """1500 right keypoints in image rows 4088..4094, 400 left ones around them (tests/test_matcher_gpu.py's crowded rows, at the bottom of a
    4095-row image: the matcher's row range vl -+ 2.01 and its +-3 buckets run into the last bucket)"""
    rng = np.random.default_rng(21)
    nL, nR = 400, 1500
    kpL = np.zeros(nL, KEYPOINT); kpR = np.zeros(nR, KEYPOINT)
    kpL["x"] = rng.uniform(300, 630, nL).astype(np.float32); kpL["y"] = rng.uniform(4087.0, 4094.9, nL).astype(np.float32)
    kpR["x"] = rng.uniform(31, 600, nR).astype(np.float32); kpR["y"] = rng.uniform(4088.0, 4094.999, nR).astype(np.float32)
    dL = rng.integers(0, 256, (nL, 32), dtype=np.uint8)
    dR = dL[rng.integers(0, nL, nR)].copy(); dR[:, :4] ^= rng.integers(0, 256, (nR, 4), dtype=np.uint8)
    return kpL, dL, kpR, dR


def vertical_edges(vl):
    """vr = vl + 2 exactly, the next float above and below, the same at vl - 2, and four rows further in and out: one descriptor per pair (tests/test_matcher_gpu.py's construction)"""
    vl = np.float32(vl)
    up, dn = np.float32(1e9), np.float32(0)
    edge = np.array([vl + np.float32(2.0), np.nextafter(vl + np.float32(2.0), up), np.nextafter(vl + np.float32(2.0), dn),
                     vl - np.float32(2.0), np.nextafter(vl - np.float32(2.0), dn), np.nextafter(vl - np.float32(2.0), up),
                     vl + np.float32(2.25), vl - np.float32(2.75), vl + np.float32(1.9999), vl - np.float32(2.25)], np.float32)
    kl = np.zeros(len(edge), KEYPOINT); kr = np.zeros(len(edge), KEYPOINT)
    kl["x"] = 300.0 + 10.0 * np.arange(len(edge)); kl["y"] = vl
    kr["x"] = kl["x"] - 20.0; kr["y"] = edge
    d = np.random.default_rng(22).integers(0, 256, (len(edge), 32), dtype=np.uint8)      # some 128 bits apart: a left keypoint matches its own partner or nobody
    return kl, d, kr, d


def horizontal_edges(case, ul, n_left, n_right, which):
    """Left keypoint i and right keypoint i share image row 40 + 10 i and a descriptor no other pair has, so who matches is the
    horizontal gates' doing (stereo.rs:100-127): min_u = max(ul - max_disp, 0) <= ur <= max_u = min(ul - min_disp, lim),
    lim = (nR as f32 * ul) / nL as f32, and ul > ur — every value in numpy f32, in the reference's operation order.  `which` names
    the edges; each is placed exactly, one float below and one above."""
    max_d, min_d = disparity_bounds(case["camera"])
    ul = np.float32(ul)
    min_u = max(np.float32(ul - max_d), np.float32(0.0))
    lim = np.float32(np.float32(n_right) * ul) / np.float32(n_left)
    max_u = min(np.float32(ul - min_d), lim)
    val = dict(min_u=min_u, max_u=max_u, ul=ul, lim=lim)
    big, low = np.float32(1e9), np.float32(-1e9)
    ur = []
    for k in which:
        ur += [val[k], np.nextafter(val[k], low), np.nextafter(val[k], big)]
    assert len(ur) <= n_right
    ur = np.array(ur + [float(ul) - 1.5 * float(min_d) - 2.0] * (n_right - len(ur)), np.float32)     # the rest: plainly inside
    kl = np.zeros(n_left, KEYPOINT); kr = np.zeros(n_right, KEYPOINT)
    kl["x"] = ul; kl["y"] = 40.0 + 10.0 * np.arange(n_left)
    kr["x"] = ur; kr["y"] = 40.0 + 10.0 * np.arange(n_right)
    dl = np.random.default_rng(23).integers(0, 256, (n_left, 32), dtype=np.uint8)
    return kl, dl, kr, dl[:n_right].copy(), val


def guided_features(case, seed, n=1500, nq=800, radius=15.0):
    """(kp, desc, q_uv, q_desc): keypoints over the image, eight of them on and beyond its edges (x = w, y = h, beyond, negative);
    queries near keypoints with a noisy copy of the descriptor, every 17th anywhere in [-200, w + 250] x [-200, h + 250] (outside the
    image: the wrap-around quirk), and 24 whose window's end x -+ radius / y -+ radius is k w / 64 (k h / 48) in f64 or one f64 step
    either side."""
    w, h = float(case["w"]), float(case["h"])
    rng = np.random.default_rng([0x601D, seed])
    kp = np.zeros(n, KEYPOINT)
    kp["x"] = rng.uniform(0, w, n).astype(np.float32); kp["y"] = rng.uniform(0, h, n).astype(np.float32)
    edge = np.array([[w, h / 2], [w / 2, h], [w, h], [w + 40.0, h / 3], [w / 3, h + 40.0], [-3.0, h / 2], [w / 2, -3.0], [-5.0, -5.0]], np.float32)
    kp["x"][:8] = edge[:, 0]; kp["y"][:8] = edge[:, 1]
    kp["size"] = 31.0
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    src = rng.integers(0, n, nq)
    src[2:10] = np.arange(8)                                           # the edge keypoints are somebody's target
    uv = np.stack([kp["x"][src].astype(np.float64) + rng.uniform(-0.6, 0.6, nq) * radius, kp["y"][src].astype(np.float64) + rng.uniform(-0.6, 0.6, nq) * radius], 1)
    flips = rng.random((nq, 256)) < 0.05
    qd = np.packbits(np.unpackbits(desc[src], axis=1, bitorder="little") ^ flips.astype(np.uint8), axis=1, bitorder="little")
    far = np.arange(0, nq, 17)
    uv[far] = np.stack([rng.uniform(-200.0, w + 250.0, len(far)), rng.uniform(-200.0, h + 250.0, len(far))], 1)
    # cell boundaries: rows 1, 18, 35, ... of the queries
    j = 1
    for k in (1, 31, 63, 64):
        for cells, size, axis in ((64, w, 0), (48, h, 1)):
            b = min(k, cells) * size / cells
            for sign in (-1.0, 1.0):                                  # x - radius = b and x + radius = b
                for step in (b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf)):
                    if j < nq:
                        uv[j, axis] = step - sign * radius
                        j += 17
    return kp, desc, uv, qd


def _on_ray(f, c, target, depths=(4.0, 8.0, 5.0, 11.0, 7.0, 16.0, 3.0, 13.0)):
    """(x, z) of a camera-frame point with f * x / z + c == target exactly in f64 (the projection's own operation order)"""
    for z in depths:
        x = (target - c) * z / f
        for _ in range(2):
            for cand in (x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)):
                if f * cand / z + c == target:
                    return cand, z
            x = np.nextafter(np.nextafter(x, np.inf), np.inf)
    raise AssertionError("no exact point for %r" % target)


def fuse_scene(P, case, seed, n_points=600, n_kfs=3, n_feat=700):
    """synth.fuse_scene at the case's camera, plus 6 map points in front of keyframe 0 (whose pose is the identity: camera frame =
    world frame, the projection is fx x / z + cx with nothing before it) that project to u = 0.0, 2cx and the f64 just below 2cx at
    v = 0.9 cy, and to v = 0.0, 2cy, just below 2cy at u = 0.9 cx — exactly.  (-0.0 cannot come out of `+ cx`.)  Each carries the
    descriptor of a feature of keyframe 0 placed under it.  edge_rows: their indices; edge_target: (axis, value)."""
    cam = dict(case["camera"])
    s = P.synth.fuse_scene(seed, n_points, n_kfs, n_feat, KEYPOINT, camera=cam, far_fraction=0.2)
    assert np.array_equal(s["kf_poses_wc"][0], [1.0, 0, 0, 0, 0, 0, 0])
    rng = np.random.default_rng([0xF0CE, seed])
    W, H = 2.0 * cam["cx"], 2.0 * cam["cy"]
    X, uv, target = [], [], []
    for val in (0.0, W, np.nextafter(W, 0.0)):
        x, z = _on_ray(cam["fx"], cam["cx"], val)
        v = 0.9 * cam["cy"]
        X.append((x, (v - cam["cy"]) * z / cam["fy"], z)); uv.append((val, v)); target.append((0, val))
    for val in (0.0, H, np.nextafter(H, 0.0)):
        y, z = _on_ray(cam["fy"], cam["cy"], val)
        u = 0.9 * cam["cx"]
        X.append(((u - cam["cx"]) * z / cam["fx"], y, z)); uv.append((u, val)); target.append((1, val))
    X, uv = np.array(X), np.array(uv)
    n0 = int(s["kf_feat_offset"][1])
    slots = rng.permutation(n0)[:len(X)]
    kps = s["kps"].copy(); descs = s["descs"].copy()
    md = rng.integers(0, 256, (len(X), 32), dtype=np.uint8)
    kps["x"][slots] = uv[:, 0].astype(np.float32); kps["y"][slots] = uv[:, 1].astype(np.float32)
    descs[slots] = md
    out = dict(s)
    out["kps"], out["descs"] = kps, descs
    out["edge_rows"] = np.arange(len(s["positions"]), len(s["positions"]) + len(X))
    out["positions"] = np.concatenate([s["positions"], X]); out["mp_desc"] = np.concatenate([s["mp_desc"], md])
    out["edge_target"] = target
    return out


def track_frame(case, seed, n_mp=150, n_feat=400):
    """tracking_scenes.frame at the case's camera, map points over [0, max(w, 2cx)) x [0, max(h, 2cy)): where the image and 2c differ,
    some points lie inside the one and outside the other."""
    cam = case["camera"]
    w, h = float(case["w"]), float(case["h"])
    xr = (2.0, max(w, 2.0 * cam["cx"]) - 2.0)
    yr = (2.0, max(h, 2.0 * cam["cy"]) - 2.0)
    return TS.frame(seed, n_mp, n_feat, x_range=xr, y_range=yr, camera=cam, w=w, h=h)


def track_frames(case):
    """the three frames (150 map points, 400 features) the tracking tests run at this case"""
    import camera_cases as CC
    return [track_frame(case, 900 + 10 * CC.NAMES.index(case["name"]) + k) for k in range(3)]


def with_nodes(s, seed=0):
    """two_view()'s scene plus node1 / node2 for the FeatureVector search: a true pair shares one of 12 nodes, 10 % of the features are in no list"""
    rng = np.random.default_rng([0x20DE, seed])
    out = dict(s)
    n1 = rng.integers(1, 13, len(s["kp1"])).astype(np.uint32); n2 = rng.integers(1, 13, len(s["kp2"])).astype(np.uint32)
    n2[s["gt"][:, 1]] = n1[s["gt"][:, 0]]
    n1[rng.random(len(n1)) < 0.1] = 0xFFFFFFFF; n2[rng.random(len(n2)) < 0.1] = 0xFFFFFFFF
    out["node1"], out["node2"] = n1, n2
    return out


def pair_case(case, n_pairs=300):
    """(scene, pairs [n_pairs,2]) for triangulate_pairs: true pairs of two_view(case), every fourth slot a random pair (wrong
    correspondences: reprojection, depth and scale rejections)."""
    import camera_cases as CC
    s = two_view(case)
    rng = np.random.default_rng([0x9A1C, CC.NAMES.index(case["name"])])
    gt = s["gt"][rng.permutation(len(s["gt"]))]
    pairs = np.zeros((n_pairs, 2), np.int32)
    for i in range(n_pairs):
        pairs[i] = (rng.integers(0, len(s["kp1"])), rng.integers(0, len(s["kp2"]))) if i % 4 == 3 else gt[i % len(gt)]
    return s, pairs


def fused_scene(case, seed=4, T=3, n_points=1500, n_distractors=150, corner_share=0.3):
    """A current keyframe and T neighbours in the layout of triangulation_scenes (dicts kp, desc, mp, pts, has, node = None, pose) at
    the case's camera.  The neighbours stand max(0.45 * 458.654 / fx, 1.25 baseline) m times (1, 1.5, 1.2, ...) away — beyond the
    baseline test of triangulate_from_neighbors — and the depths are scaled with that step, so the displacement stays under the
    search window."""
    cam, w, h = dict(case["camera"]), float(case["w"]), float(case["h"])
    rng = np.random.default_rng([0xF5CE, seed])
    s = EUROC_FX / cam["fx"]
    step = max(0.45 * s, 1.25 * cam["baseline"])
    zs = step / (0.45 * s)
    n_c = int(corner_share * n_points)
    u = np.concatenate([rng.uniform(max(w - CORNER, 0.0), w, n_c), rng.uniform(0.0, w, n_points - n_c)])
    v = np.concatenate([rng.uniform(max(h - CORNER, 0.0), h, n_c), rng.uniform(0.0, h, n_points - n_c)])
    z = rng.uniform(5.0, 14.0, n_points) * zs
    pose_cur = np.concatenate([_quat([0.1, 1.0, 0.05], 0.0005), [0.0, 0.0, 0.0]])
    X = TS.backproject(pose_cur, np.stack([u, v], 1), z, cam)
    dirs = [np.array([1.0, 0.02, 0.03]), np.array([-1.0, 0.04, 0.08]), np.array([0.9, -0.3, 0.1]), np.array([-0.8, 0.3, -0.1])]
    dist = [1.0, 1.5, 1.2, 1.1]
    pdesc = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    octv = rng.integers(0, 3, n_points)

    def keyframe(pose, sel_all):
        uv, pc = project(cam, pose, X)
        ok = np.ones(n_points, bool) if sel_all else ((pc[:, 2] > 0.5) & (uv[:, 0] > 0) & (uv[:, 0] < w) & (uv[:, 1] > 0) & (uv[:, 1] < h) & (rng.random(n_points) < 0.9))
        sel = np.flatnonzero(ok)
        m, nd = len(sel), n_distractors
        kp = np.zeros(m + nd, KEYPOINT)
        top = lambda a: np.nextafter(np.float32(a), np.float32(0))
        kp["x"] = np.clip(np.concatenate([uv[sel, 0] + rng.normal(0, 0.3, m), rng.uniform(0, w, nd)]), 0.0, top(w)).astype(np.float32)
        kp["y"] = np.clip(np.concatenate([uv[sel, 1] + rng.normal(0, 0.3, m), rng.uniform(0, h, nd)]), 0.0, top(h)).astype(np.float32)
        kp["size"] = 31.0
        kp["octave"] = np.concatenate([octv[sel], rng.integers(0, 3, nd)])
        flips = rng.random((m, 256)) < 0.02
        desc = np.concatenate([np.packbits(np.unpackbits(pdesc[sel], axis=1, bitorder="little") ^ flips.astype(np.uint8), axis=1, bitorder="little"),
                               rng.integers(0, 256, (nd, 32), dtype=np.uint8)])
        has = (rng.random(m + nd) < 0.5).astype(np.uint8)
        pts = np.concatenate([pc[sel] * (1.0 + rng.normal(0, 0.01, m))[:, None], np.stack([np.zeros(nd), np.zeros(nd), rng.uniform(5.0, 14.0, nd) * zs], 1)])
        perm = rng.permutation(m + nd)
        return dict(kp=kp[perm], desc=desc[perm], mp=(rng.random(m + nd) < 0.25).astype(np.uint8), pts=np.ascontiguousarray((pts * has[:, None])[perm]),
                    has=has[perm], node=None, pose=pose)

    cur = keyframe(pose_cur, True)
    nbs = []
    for t in range(T):
        d = dirs[t % 4] / np.linalg.norm(dirs[t % 4])
        q = _quat([0.1, 1.0, 0.05], (-0.03 if t % 2 == 0 else 0.025) * s)
        nbs.append(keyframe(np.concatenate([q, d * step * dist[t % 4]]), False))
    return dict(camera=cam, current=cur, neighbours=nbs)
