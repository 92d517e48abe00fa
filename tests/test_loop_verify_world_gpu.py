"""Loop verification on the GPU where a map merge takes it (loop_verify_kernels.hip against tests/loop_verify_spec.py on the scenes of
tests/loop_verify_world_scenes.py): rotations near pi and every branch of the quaternion conversion, exact data on which every
hypothesis ties, the hypothesis-count and point-count edges of the three kernels, the unrefined exit, points 1e3-1e5 m from the
origin, free scales from 0.05 to 20; the whole call under six cameras with octaves 0-7, in worlds turned and shifted by kilometres,
between maps a half turn and 300 m apart or scaled by 0.8 and 3, with points behind the loop camera and octaves outside 0..31.

Tolerances.  Every integer, list, mask, status and best_hypothesis is exact, as in tests/test_loop_verify_gpu.py, whose helpers do
the comparing: tests/test_loop_verify_world_cpu.py asserts that file's comparison rule for every scene used here.  Scenes of unit
scale near the origin keep that file's figures (1e-9, 1e-8 below 50 inliers; mse 1e-9 relative).  For a scene with an offset or a
scale away from 1 the bound on rotation, translation and scale is max(that figure, 50 x the spread between the specification's SVD
form of Horn's fit and the quaternion-eigenvector form on the same points) and the bound on mse is max(1e-9, 50 x the spread between
the specification's mse and the same sum in np.longdouble), both spreads measured per scene by loop_verify_world_scenes.spread (the
rule of tests/test_global_ba.py).  On the exact sets the mse is rounding alone (1e-31 and below, the specification's own two sums
differ by percents there), so it is bounded absolutely instead: coordinates up to 12 m and a rotation good to a few ulp leave at most
about 20 ulp(12) = 4e-14 m per coordinate, 5e-27 m^2 per point; the bound is 1e-25."""
import numpy as np
import pytest

import loop_verify_spec as S
import loop_verify_world_scenes as W
import pnp_spec
from test_loop_verify_gpu import _bytes, _cfg, _kf, _mse_close, _sim3_close, assert_pair_matches_spec

pytestmark = pytest.mark.gpu
_zero = lambda: dict(angle=0.0, translation=0.0, scale=0.0, mse=0.0)
worst = dict(plain=_zero(), shifted=_zero())           # the largest deviations seen: scenes on the file's figures / on the spread rule
INTS = ("n_matches", "n_pairs", "best_hypothesis", "ransac_inliers", "n_inliers", "refined", "n_verified")


# ---- Sim3 on its own --------------------------------------------------------------------------------------------------
def _solve(gpu_handle, pkg, name, **over):
    p1, p2, _ = W.sim3_set(name)
    sim3, inl, rec = gpu_handle.compute_sim3_ransac_batch([(p1, p2)], pkg.Sim3SolverConfig(**dict(W.SIM3_SETS[name][2], **over)))
    assert np.all(np.isfinite(sim3))
    return sim3[0], inl[0], rec[0]


def _assert_sim3(g, s, where, spreads=None, mse=True):
    g_sim3, g_inl, g_rec = g
    for k in ("status", "best_hypothesis", "ransac_inliers", "n_inliers", "refined"):
        assert int(g_rec[k]) == s[k], (where, k, int(g_rec[k]), s[k])
    assert np.array_equal(g_inl, s["inlier"]), where
    tol, mse_tol = W.tolerances(s["n_inliers"], spreads)
    w = worst["plain" if spreads is None else "shifted"]
    if s["status"] == 0:
        _sim3_close(g_sim3, s["sim3"], s["n_inliers"], where, tol, w)
    else:
        assert g_sim3.tobytes() == S.IDENTITY.tobytes(), where
    if mse:
        _mse_close(float(g_rec["mse"]), s["mse"], where, mse_tol, w)


@pytest.mark.parametrize("name", W.ROTATIONS)
def test_sim3_rotations(gpu_handle, pkg, name):
    """pi, pi - 1e-9, pi - 1e-3 and 2.2 rad about x, y, z, (1, 1, 1) and an oblique axis, and the identity: all four branches of s3_quat
    (the CPU file shows which set takes which).  At pi, w comes back as +0 or -0; either passes `w >= 0` and the angle measure."""
    _assert_sim3(_solve(gpu_handle, pkg, name), W.sim3_spec(name), name)


@pytest.mark.parametrize("name", W.EXACT_SETS)
def test_sim3_exact_data_ties_go_to_hypothesis_zero(gpu_handle, pkg, name):
    """points on the 1/8 grid under an exact rotation and translation, 1024 hypotheses: every one holds all n points, so the tie rule
    decides across every wave of sim3_final_kernel, every 32-chunk of sim3_score_kernel and every 64-block of sim3_hypothesis_kernel"""
    p1, p2, gt = W.sim3_set(name)
    s = W.sim3_spec(name)
    g = _solve(gpu_handle, pkg, name)
    assert int(g[2]["best_hypothesis"]) == 0 and int(g[2]["ransac_inliers"]) == len(p1) and int(g[2]["n_inliers"]) == len(p1) and g[1].all()
    _assert_sim3(g, s, name, mse=False)
    assert 0.0 <= float(g[2]["mse"]) < 1e-25 and s["mse"] < 1e-25, (name, float(g[2]["mse"]), s["mse"])
    truth = np.concatenate([S.quat_from_R(gt["R"]), gt["t"]])
    assert pnp_spec.rotation_angle(g[0][:7], truth) < 1e-13 and np.abs(g[0][4:7] - gt["t"]).max() < 1e-12 and g[0][7] == 1.0, (name, g[0])


def test_sim3_hypothesis_count_edges(gpu_handle, pkg):
    """max_iterations at the edges of the 32-hypothesis chunk, the 64-hypothesis block and the 10-bit key (h = 1023 packs to 0), then
    with the H = 1024 winner b as the last hypothesis (b + 1) and gone (b); b > 64 is asserted by the CPU file"""
    b = W.sim3_spec("h_edges")["best_hypothesis"]
    winners = {}
    for H in W.H_EDGES + (b + 1, b):
        g = _solve(gpu_handle, pkg, "h_edges", max_iterations=H)
        _assert_sim3(g, W.sim3_spec("h_edges", H), "h_edges H=%d" % H)
        winners[H] = int(g[2]["best_hypothesis"])
    assert winners[1024] == b and winners[1023] == b and winners[b + 1] == b and winners[b] != b and winners[b] < b


@pytest.mark.parametrize("name", W.POINT_COUNTS)
def test_sim3_point_count_edges(gpu_handle, pkg, name):
    """3 and 4 points with min_inliers = 3; 255, 256, 257 points around the 256-point tile, 1000 and 2049 (nine tiles)"""
    _assert_sim3(_solve(gpu_handle, pkg, name), W.sim3_spec(name), name)


def test_sim3_batch_of_2049_15_and_2_points_equals_single_calls(gpu_handle, pkg):
    names = ["n2049", "n15", "n2"]
    probs = [W.sim3_set(n)[:2] for n in names]
    sim3, inl, rec = gpu_handle.compute_sim3_ransac_batch(probs)
    for k, n in enumerate(names):
        a, b, c = gpu_handle.compute_sim3_ransac_batch([probs[k]])
        assert a[0].tobytes() == sim3[k].tobytes() and b[0].tobytes() == inl[k].tobytes() and c[0].tobytes() == rec[k].tobytes(), n
        _assert_sim3((sim3[k], inl[k], rec[k]), W.sim3_spec(n), n)
    assert [int(r["status"]) for r in rec] == [0, 0, 1]


@pytest.mark.parametrize("name", W.UNREFINED)
def test_sim3_unrefined_winner(gpu_handle, pkg, name):
    """the refit holds fewer points than the winner: the winner's own model, mask and mse come back, and with a free scale its scale,
    which sim3_final_kernel recovers as a row length of M"""
    s = W.sim3_spec(name)
    g = _solve(gpu_handle, pkg, name)
    assert int(g[2]["refined"]) == 0 and s["refined"] == 0 and np.array_equal(g[1], s["inlier"])
    _assert_sim3(g, s, name, W.sim3_spread(name) if name in W.SPREAD_SETS else None)
    if name in W.SPREAD_SETS:
        assert abs(g[0][7] - 1.0) > 0.05, (name, g[0][7], s["sim3"][7])
    else:
        assert g[0][7] == 1.0


@pytest.mark.parametrize("name", W.OFFSETS + W.SCALES)
def test_sim3_far_from_origin_and_free_scale(gpu_handle, pkg, name):
    """points 1e3, 1e4 and 1e5 m from the origin, where t = c2 - M c1 cancels; free scales 0.05, 0.5 and 20"""
    s = W.sim3_spec(name)
    _assert_sim3(_solve(gpu_handle, pkg, name), s, name, W.sim3_spread(name))
    gt = W.sim3_set(name)[2]
    assert abs(s["sim3"][7] - gt["scale"]) < 0.01 * gt["scale"]


@pytest.mark.parametrize("name", W.RESCALED)
def test_sim3_fixed_scale_on_rescaled_data(gpu_handle, pkg, name):
    """fix_scale on data scaled by 1.02 (a small unrefined model) and by 0.8 (no model): the status and every count are the
    specification's"""
    s = W.sim3_spec(name)
    g = _solve(gpu_handle, pkg, name)
    assert int(g[2]["status"]) == W.SIM3_STATUS.get(name, 0)
    _assert_sim3(g, s, name)


# ---- the whole call ---------------------------------------------------------------------------------------------------
def _camera(pkg, name):
    return pkg.CameraModel(**W.PAIRS[name][0]["camera"])


def _verify(gpu_handle, pkg, name):
    return gpu_handle.verify_loop_candidates(_camera(pkg, name), [W.pair(name)], _cfg(pkg, W.PAIRS[name][1], W.PAIRS[name][2]))[0]


def _assert_pair(r, name):
    s = W.pair_spec(name)
    assert r["status"] == W.PAIRS[name][3], (name, r["status"])
    if name in W.SHIFTED and s["status"] == S.OK:
        tol, mse_tol = W.tolerances(s["n_inliers"], W.pair_spread(name))
        assert_pair_matches_spec(r, s, name, tol, mse_tol, worst["shifted"])
    else:
        assert_pair_matches_spec(r, s, name, worst=worst["plain"])


@pytest.mark.parametrize("name", [n for n in W.PAIRS if n.startswith("cam_")])
def test_pair_under_every_camera(gpu_handle, pkg, name):
    assert int(W.pair(name)[1]["kp"]["octave"].max()) == 7
    _assert_pair(_verify(gpu_handle, pkg, name), name)


def test_world_poses_change_no_integer(gpu_handle, pkg):
    """one scene in eleven turned worlds 1.3 km from the origin and once 22 km from it: each equals the specification, every integer,
    mask and list equals the unturned, unshifted run's, and all of them as one batch equal the single calls byte for byte"""
    base = _verify(gpu_handle, pkg, "world_none")
    _assert_pair(base, "world_none")
    single = {}
    for name in W.WORLD_NAMES:
        r = single[name] = _verify(gpu_handle, pkg, name)
        _assert_pair(r, name)
        assert r["status"] == base["status"] and all(r["stats"][k] == base["stats"][k] for k in INTS), name
        assert r["matches"].tobytes() == base["matches"].tobytes() and np.array_equal(r["feature_matches"], base["feature_matches"]), name
        assert np.array_equal(r["inlier"], base["inlier"]), name
    batch = gpu_handle.verify_loop_candidates(_camera(pkg, "world_none"), [W.pair(n) for n in W.WORLD_NAMES], _cfg(pkg))
    for name, r in zip(W.WORLD_NAMES, batch):
        assert _bytes(r) == _bytes(single[name]), name


@pytest.mark.parametrize("name", [n for n in W.PAIRS if n.startswith("merge_")])
def test_map_merges(gpu_handle, pkg, name):
    """maps 300 m apart and turned by pi - 0.01 (brute-force matcher) and 2.4 rad (FeatureVector matcher); maps scaled by 0.8 and 3 with
    a free scale, through the host form and through resident keyframes; the 0.8 map under a fixed scale: no model"""
    r = _verify(gpu_handle, pkg, name)
    _assert_pair(r, name)
    if W.PAIRS[name][3] == S.OK and W.PAIRS[name][2]:
        scale = 1.0 / W.PAIRS[name][0]["map_scale"]
        assert abs(r["sim3"][7] - scale) < 0.01 * scale, (name, r["sim3"][7])
    cur, loop = _kf(pkg, gpu_handle, W.pair(name)[0]), _kf(pkg, gpu_handle, W.pair(name)[1])
    res = pkg.KeyFrame.verify_loop_candidates(gpu_handle, _camera(pkg, name), [cur], [loop], _cfg(pkg, W.PAIRS[name][1], W.PAIRS[name][2]))
    cur.close(); loop.close()
    assert _bytes(res[0]) == _bytes(r), name


@pytest.mark.parametrize("name", ["behind", "behind_centre"])
def test_points_behind_the_loop_camera_are_not_counted(gpu_handle, pkg, name):
    r = _verify(gpu_handle, pkg, name)
    _assert_pair(r, name)
    assert r["stats"]["n_verified"] == W.pair_spec(name)["n_verified"] < r["stats"]["n_pairs"]


@pytest.mark.parametrize("octave", W.CLAMP_OCTAVES)
def test_octaves_outside_0_31_are_clamped(gpu_handle, pkg, octave):
    """every loop octave at -3 and at 40: the count is the clamped specification's (the CPU file shows that the unclamped count differs)"""
    r = gpu_handle.verify_loop_candidates(_camera(pkg, "cam_euroc"), [W.clamp_pair(octave)], _cfg(pkg))[0]
    s = W.clamp_spec(octave)
    assert_pair_matches_spec(r, s, "octave %d" % octave, worst=worst["plain"])
    assert r["stats"]["n_verified"] == s["n_verified"] != W.pair_spec("cam_euroc")["n_verified"]


def test_zz_report_largest_deviations():
    """not a check of its own: prints the largest deviations the tests above measured (DESIGN.md section 2 quotes them)"""
    for k, w in worst.items():
        print("loop verification, world scenes (%s), largest deviations from the specification: rotation %.3e rad, translation %.3e relative, "
              "scale %.3e relative, mse %.3e relative" % (k, w["angle"], w["translation"], w["scale"], w["mse"]))
