"""CPU checks behind tests/test_cameras_gpu.py: the scenes of tests/camera_scenes.py reach the regimes tests/camera_cases.py names
(checked against the oracle alone, with the non-vacuity floors of the table), and the oracle equals a second, independent statement
of each search at every camera — so that what the GPU is compared with is right away from EuRoC too."""
import math
from fractions import Fraction

import numpy as np
import pytest

import camera_cases as CC
import camera_scenes as CS
import tracking_spec as TSPEC
import triangulation_spec as TRI
from test_fuse_search import RADIUS_SCALE, _numpy as fuse_numpy
from test_triangulation_search import _numpy_restatement as tri_numpy

CASES = CC.CASES
IDS = CC.NAMES


def _search(oracle, s, max_dist=50):
    return oracle.search_for_triangulation(oracle.Camera(**s["camera"]), s["kp1"], s["desc1"], s["mp1"], s["stereo1"], s["kp2"], s["desc2"],
                                           s["mp2"], s["pose1_wc"], s["pose2_wc"], max_dist)


# ---- the table ---------------------------------------------------------------------------------------------------------------

def test_table_is_what_it_says(pkg):
    assert CC.BY_NAME["euroc"]["camera"] == pkg.synth.EUROC_CAMERA and (CC.BY_NAME["euroc"]["w"], CC.BY_NAME["euroc"]["h"]) == (752, 480)
    for c in CASES + [CC.REFUSED]:
        assert CS.tri_grid_dims(c["camera"]) == c["grid"], c["name"]
        assert 1 <= c["w"] <= 4095 and 1 <= c["h"] <= 4095
    a, b = CC.BY_NAME["grid63"], CC.BY_NAME["grid64"]
    assert {k for k in a["camera"] if a["camera"][k] != b["camera"][k]} == {"cx", "cy"} and (a["w"], a["h"]) == (b["w"], b["h"])
    k = CC.BY_NAME["kitti"]
    max_d, min_d = CS.disparity_bounds(k["camera"])
    assert max_d > k["w"] and 9.6 < min_d < 9.7 and Fraction(64.0 / k["w"]) != Fraction(64, k["w"])
    t = CC.BY_NAME["tiny"]
    assert t["w"] / 64 == 1.0 and abs(t["h"] / 48 - 4 / 3) < 1e-12
    n = CC.BY_NAME["anisotropic"]
    assert 2 * n["camera"]["cx"] == 256 != n["w"] and n["camera"]["fx"] != n["camera"]["fy"]
    assert CC.BY_NAME["tall"]["h"] == 4095 and CC.REFUSED["camera"]["cx"] * 2 < 1
    # the fuse radius of square512 leaves its lower clamp at 178 m and reaches the upper one at 889 m (EuRoC: 427 m and 2134 m)
    assert RADIUS_SCALE * 900.0 / CC.BY_NAME["square512"]["camera"]["fx"] > 50.0 > RADIUS_SCALE * 2000.0 / CC.EUROC["fx"]


# ---- search_for_triangulation ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_view_scene_reaches_its_regime(oracle, case):
    s = CS.two_view(case)
    m = _search(oracle, s)
    corner = CS.corner_pairs(s, m)
    print("%s: %d pairs, %d of them read the end sentinel" % (case["name"], len(m), len(corner)))
    assert len(m) >= max(50, CC.floor(case["name"], "pairs"))
    if case["name"] in ("grid64", "big"):
        assert len(corner) >= max(20, CC.floor(case["name"], "corner"))
    assert np.all(np.diff(m[:, 0]) > 0) and len(set(m[:, 1].tolist())) == len(m)
    assert not s["mp1"][m[:, 0]].any() and not s["mp2"][m[:, 1]].any()
    # the matches are the scene's true pairs, almost all of them: the search sees the geometry of this camera
    true = {tuple(p) for p in s["gt"].tolist()}
    assert sum(tuple(p) in true for p in m.tolist()) >= 0.95 * len(m)
    assert s["kp1"]["x"].max() < case["w"] and s["kp2"]["y"].max() < case["h"] and s["kp1"]["x"].min() >= 0
    assert s["kp2"]["x"].max() > case["w"] - 8 and s["kp2"]["y"].max() > case["h"] - 8          # the whole image is covered


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_triangulation_search_oracle_equals_numpy_restatement(oracle, case):
    s = CS.two_view(case, seed=5, n_points=350, n_distractors=80)
    got, want = _search(oracle, s), tri_numpy(s)
    assert np.array_equal(got, want) and len(got) > 40


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("two_c", [0.99, 1.0, 32.0, 32.01, 2016.0, 2016.99, 2017.0, 4090.0])
def test_tri_grid_dims_against_the_grid_the_oracle_uses(oracle, axis, two_c):
    """The oracle's grid, measured from outside.  Pure translation along the probed axis and identity rotations: the epipolar line
    of a feature is its own row (column).  Keyframe 2 holds 80 identical features far beyond the image, which fall into the last
    column; feature j of keyframe 1 stands at 32 j + 116, so its window is columns j .. min(j + 7, cols - 1): it finds a partner
    exactly when j <= cols - 1 <= j + 7.  The last feature that matches is number cols - 1 (none where the grid has no column)."""
    want = int(min(np.ceil(np.float32(np.uint32(int(two_c))) / np.float32(32.0)), np.float32(64.0)))
    cam = dict(fx=500.0, fy=500.0, cx=300.0, cy=300.0, baseline=0.1)
    cam["c" + axis] = two_c / 2.0
    assert CS.tri_grid_dims(cam)[0 if axis == "x" else 1] == want
    other = "y" if axis == "x" else "x"
    n1, n2 = 72, 80
    kp1 = np.zeros(n1, CS.KEYPOINT); kp2 = np.zeros(n2, CS.KEYPOINT)
    kp1[axis] = 32.0 * np.arange(n1) + 116.0; kp1[other] = 10.0
    kp2[axis] = 6000.0; kp2[other] = 10.0
    d1 = np.zeros((n1, 32), np.uint8); d2 = np.zeros((n2, 32), np.uint8)
    z1 = np.zeros(n1, np.uint8); z2 = np.zeros(n2, np.uint8)
    t = [0.3, 0.0, 0.0] if axis == "x" else [0.0, 0.3, 0.0]
    m = oracle.search_for_triangulation(oracle.Camera(**cam), kp1, d1, z1, np.ones(n1, np.uint8), kp2, d2, z2, np.array([1.0, 0, 0, 0, 0, 0, 0]),
                                        np.array([1.0, 0, 0, 0] + t), 50)
    assert m[:, 0].tolist() == list(range(max(want - 8, 0), want))


# ---- stereo_match ------------------------------------------------------------------------------------------------------------

def _stereo_numpy(cam, kpL, dL, kpR, dR):
    """stereo.rs:95-156 and :186-216, candidate by candidate in f32 / f64 numpy scalars."""
    max_d, min_d = CS.disparity_bounds(cam)
    nL, nR = len(kpL), len(kpR)
    pop = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1)
    out, pts = [], {}
    for li in range(nL):
        ul, vl = kpL["x"][li], kpL["y"][li]
        min_u = max(np.float32(ul - max_d), np.float32(0))
        lim = np.float32(np.float32(nR) * ul) / np.float32(nL)
        max_u = min(np.float32(ul - min_d), lim)
        ok = (np.abs(vl - kpR["y"]) <= np.float32(2)) & (kpR["x"] >= min_u) & (kpR["x"] <= max_u) & (kpR["x"] < ul)
        best, second, bi = 100, 100, -1
        for ri in np.flatnonzero(ok):
            d = int(pop[dL[li] ^ dR[ri]].sum())
            if d < best:
                second, best, bi = best, d, ri
            elif d < second:
                second = d
        if bi >= 0 and (np.float32(best) < np.float32(0.9) * np.float32(second) or second == 100):
            out.append((li, bi, best))
            disp = float(ul) - float(kpR["x"][bi])
            if abs(disp) >= 0.5:
                z = cam["fx"] * cam["baseline"] / disp
                pts[li] = ((float(ul) - cam["cx"]) * z / cam["fx"], (float(vl) - cam["cy"]) * z / cam["fy"], z)
    return out, pts


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stereo_scene_and_oracle(oracle, case):
    cam = oracle.Camera(**case["camera"])
    f = CS.stereo_features(case, 0, 2100, 2300)
    m, p, h = oracle.stereo_match(cam, *f)
    print("%s: %d stereo matches of %d" % (case["name"], len(m), 2100))
    assert len(m) > 0.2 * 2100 and len(m) >= CC.floor(case["name"], "stereo")
    assert f[0]["y"].max() > case["h"] - 4 and f[2]["y"].max() > case["h"] - 4 and f[2]["x"].min() >= 0.0
    if case["name"] == "tall":
        assert f[0]["y"].max() > 4090.0 and f[0]["y"].max() < 4095.0
    # a second statement on a smaller set
    f = CS.stereo_features(case, 1, 300, 280)
    m, p, h = oracle.stereo_match(cam, *f)
    want, pts = _stereo_numpy(case["camera"], *f)
    assert [(int(a["query_idx"]), int(a["train_idx"]), int(a["distance"])) for a in m] == want and len(want) > 60
    assert np.flatnonzero(h).tolist() == sorted(pts) and all(tuple(p[i]) == pts[i] for i in pts)


# ---- guided_match ------------------------------------------------------------------------------------------------------------

def _guided_numpy(kp, desc, img_w, img_h, q_uv, q_desc, radius, mode):
    """tracking_frame.rs:52-128 and the two search loops, restated with python integers (Rust's saturating float casts; a negative
    i32 cast to usize wraps and clamps to the last cell)."""
    GC, GR = 64, 48
    winv, hinv = GC / img_w, GR / img_h
    sat = lambda v, lo, hi: lo if v != v or v <= lo else (hi if v >= hi else int(v))
    cells = {}
    for i in range(len(kp)):
        cx = min(sat(float(kp["x"][i]) * winv, 0, 2 ** 63), GC - 1); cy = min(sat(float(kp["y"][i]) * hinv, 0, 2 ** 63), GR - 1)
        cells.setdefault((cy, cx), []).append(i)
    pop = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1)
    idx = np.full(len(q_uv), -1, np.int32); dist = np.zeros(len(q_uv), np.uint32)
    i32 = lambda v: sat(v, -2 ** 31, 2 ** 31 - 1)
    for q, (x, y) in enumerate(q_uv):
        mnx, mxx = i32(math.floor((x - radius) * winv)), i32(math.ceil((x + radius) * winv))
        mny, mxy = i32(math.floor((y - radius) * hinv)), i32(math.ceil((y + radius) * hinv))
        x0, y0 = max(mnx, 0), max(mny, 0)
        x1 = GC - 1 if (mxx < 0 or mxx > GC - 1) else mxx
        y1 = GR - 1 if (mxy < 0 or mxy > GR - 1) else mxy
        cand = [i for cy in range(y0, y1 + 1) for cx in range(x0, x1 + 1) for i in cells.get((cy, cx), [])]
        if not cand:
            continue
        d = [int(pop[q_desc[q] ^ desc[i]].sum()) for i in cand]
        k = int(np.argmin(d))                                   # the first of equal minima
        if mode == 0:
            if d[k] < 100:
                idx[q], dist[q] = cand[k], d[k]
        else:
            second = min(d[:k] + d[k + 1:]) if len(d) > 1 else None
            if d[k] > 100 or (second is not None and np.float32(d[k]) > np.float32(0.75) * np.float32(second)):
                continue
            idx[q], dist[q] = cand[k], d[k]
    return idx, dist


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_guided_match_oracle_equals_numpy_restatement(oracle, case, mode):
    kp, desc, uv, qd = CS.guided_features(case, 2, n=400, nq=430)
    w, h = float(case["w"]), float(case["h"])
    i0, d0 = oracle.guided_match(kp, desc, w, h, uv, qd, 15.0, mode)
    i1, d1 = _guided_numpy(kp, desc, w, h, uv, qd, 15.0, mode)
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1)
    assert (i0 >= 0).sum() > 100
    # the scene holds what its text says: keypoints on and beyond the edges, boundary queries
    assert (kp["x"] == np.float32(w)).sum() >= 2 and (kp["y"] == np.float32(h)).sum() >= 2 and (kp["x"] < 0).any() and (kp["x"] > w).any()
    on = lambda a, size, cells: np.isin(np.round(a * cells / size, 9) % 1.0, [0.0]).sum()
    assert on(uv[:, 0] - 15.0, w, 64) >= 4 and on(uv[:, 0] + 15.0, w, 64) >= 4 and on(uv[:, 1] - 15.0, h, 48) >= 4


# ---- track_frames ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tracking_scenes_keep_clear_of_decision_points(oracle, case, mode):
    cfg = TSPEC.default_config(mode, img_w=float(case["w"]), img_h=float(case["h"]))
    frames = CS.track_frames(case)
    cam = case["camera"]
    for f in frames:
        assert TSPEC.margins(cam, cfg, f[4], f[2]) >= 1e-9
        assert len(f[2]) == 150 and len(f[0]) == 400
    off, ms, gs = TSPEC.search_and_gather(oracle, cam, cfg, frames)
    n_corr = np.diff(off)
    print("%s mode %d: correspondences %s" % (case["name"], mode, n_corr.tolist()))
    assert n_corr.min() >= 30
    if case["name"] == "anisotropic":
        for f in frames:                 # points inside the image but outside [0, 2cx): mode 0's bounds reject them, the grid does not
            z, u, v = TSPEC.project(cam, f[4], f[2])
            between = (z > 0) & (u >= 2 * cam["cx"]) & (u < case["w"])
            assert between.sum() >= 10
            below = (z > 0) & (v >= case["h"]) & (v < 2 * cam["cy"])
            assert below.sum() >= 10
        if mode == 1:
            m0 = TSPEC.search_and_gather(oracle, cam, TSPEC.default_config(0, img_w=float(case["w"]), img_h=float(case["h"])), frames)[1]
            for f, a, b in zip(frames, m0, ms):
                z, u, v = TSPEC.project(cam, f[4], f[2])
                between = (z > 0) & (u >= 2 * cam["cx"]) & (u < case["w"])
                assert (a[between] == TSPEC.NONE).all() and (b[between] >= 0).sum() >= 5


# ---- fuse_search -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fuse_search_oracle_equals_numpy_restatement(oracle, pkg, case):
    s = pkg.synth.fuse_scene(3, 400, 3, 500, CS.KEYPOINT, camera=dict(case["camera"]), far_fraction=0.2)
    cam = oracle.Camera(**case["camera"])
    i0, d0 = oracle.fuse_search(cam, s["positions"], s["mp_desc"], s["kf_poses_wc"], s["kf_feat_offset"], s["kps"], s["descs"], RADIUS_SCALE, 50)
    i1, d1 = fuse_numpy(s)
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1)
    assert (i0 >= 0).sum() > 100
    if case["name"] == "square512":
        far = s["positions"][:, 2] > 900.0                                   # the upper clamp: 50 px at every one of these
        assert far.sum() >= 30 and (i0[far] >= 0).sum() >= 20


def test_fuse_edge_points_project_exactly_onto_the_bounds(oracle, pkg):
    """u = 2cx exactly is outside, the f64 below it and 0.0 are inside (search_in_neighbors.rs:291: u < 0 || u >= 2cx), the same for
    v: the oracle finds the feature placed under the inside ones and nothing for the outside ones."""
    for case in CASES:
        s = CS.fuse_scene(pkg, case, 7)
        cam = case["camera"]
        X = s["positions"][s["edge_rows"]]
        for (axis, val), p in zip(s["edge_target"], X):
            f, c = (cam["fx"], cam["cx"]) if axis == 0 else (cam["fy"], cam["cy"])
            assert f * p[axis] / p[2] + c == val
        i0, d0 = oracle.fuse_search(oracle.Camera(**cam), s["positions"], s["mp_desc"], s["kf_poses_wc"], s["kf_feat_offset"], s["kps"], s["descs"],
                                    RADIUS_SCALE, 50)
        got = i0[s["edge_rows"], 0]
        inside = np.array([val < 2 * (cam["cx"], cam["cy"])[axis] for axis, val in s["edge_target"]])
        assert inside.tolist() == [True, False, True] * 2
        assert (got[inside] >= 0).all() and (got[~inside] == -1).all() and (d0[s["edge_rows"], 0][inside] == 0).all(), case["name"]


# ---- triangulate_pairs -------------------------------------------------------------------------------------------------------

_expected = {}


def pair_expected(case, baseline=None):
    key = (case["name"], baseline)
    if key not in _expected:
        s, pairs = CS.pair_case(case)
        cam = dict(s["camera"]) if baseline is None else dict(s["camera"], baseline=baseline)
        _expected[key] = [TRI.triangulate_pair(cam, TRI.default_config(), 0, s["kp1"], s["pts1"], s["has1"], s["pose1_wc"], s["kp2"], s["pts2"], s["has2"],
                                               s["pose2_wc"], int(a), int(b)) for a, b in pairs]
    return _expected[key]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_triangulation_pairs_reach_the_branches(case):
    ev = pair_expected(case)
    st = np.array([e[0] for e in ev]); me = np.array([e[1] for e in ev]); mg = np.array([e[3] for e in ev])
    print("%s: statuses %s, methods %s" % (case["name"], np.bincount(st, minlength=9).tolist(), np.bincount(me, minlength=3).tolist()))
    assert (mg <= 1e-9).sum() <= 0.01 * len(ev)                      # at most 1 % of the pairs sit on a gate
    assert (st == TRI.CREATED).sum() >= 50 and len(set(st.tolist())) >= 3
    if case["name"] == "kitti":
        # the stereo baseline (0.537 m) exceeds the distance between the views: cos(2 atan(b / 2 / z)) falls below the pairs' own
        # parallax cosine, the DLT is refused and the stereo branches run.  With EuRoC's baseline the same pairs take the DLT.
        small = pair_expected(case, baseline=CC.EUROC["baseline"])
        me_small = np.array([e[1] for e in small]); st_small = np.array([e[0] for e in small])
        ran = ~np.isin(st, [TRI.SKIPPED, TRI.DLT_DEGENERATE, TRI.BAD_INDEX])
        assert (ran & (me != TRI.DLT)).sum() >= 20
        moved = ran & (me != TRI.DLT) & (me_small == TRI.DLT) & ~np.isin(st_small, [TRI.SKIPPED, TRI.DLT_DEGENERATE, TRI.BAD_INDEX])
        assert moved.sum() >= 20


@pytest.mark.parametrize("name", ["kitti", "big"])
def test_fused_scenes_create_points_through_every_neighbour(oracle, name):
    case = CC.BY_NAME[name]
    sc = CS.fused_scene(case)
    created, stats, res, ev = TRI.triangulate_from_neighbors(oracle, sc["camera"], TRI.default_config(), 0, sc["current"], sc["neighbours"])
    print("%s: per neighbour %s" % (name, stats.tolist()))
    assert len(sc["neighbours"]) == 3 and stats[:, 0].tolist() == [1, 1, 1]           # none falls to the baseline test
    assert stats[:, 1].min() >= 100 and stats[:, 3].min() >= 20
    assert sum(e[6] <= 1e-9 for e in ev) <= 0.01 * len(ev)
    if name == "big":
        c = sc["current"]
        for t, nb in enumerate(sc["neighbours"]):
            pairs = np.array([(e[1], e[2]) for e in ev if e[0] == t])
            assert len(CS.corner_pairs(dict(kp1=c["kp"], kp2=nb["kp"]), pairs)) >= 20
