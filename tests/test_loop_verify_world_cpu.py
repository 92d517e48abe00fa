"""CPU checks on the scenes of tests/loop_verify_world_scenes.py, before tests/test_loop_verify_world_gpu.py compares the GPU on them:
every scene meets the comparison rule of tests/test_loop_verify_cpu.py (MIN_MARGIN, MIN_COND, unchanged) and reaches its status;
the scenes reach what they were made for (all four quaternion branches, both unrefined exits, a match behind the loop camera, an
octave clamp that changes the count, a late winner); and the two spreads that set the GPU file's tolerance away from the origin
and from unit scale are measured, with a second formulation of Horn's closed form that is itself checked against ground truth."""
import numpy as np

import loop_verify_spec as S
import loop_verify_world_scenes as W
import pnp_spec
from test_loop_verify_cpu import MIN_COND, MIN_MARGIN


def _comparable(r):
    return r["margin"] > MIN_MARGIN and r["cond"] > MIN_COND


def test_every_world_pair_reaches_its_status_and_may_be_compared():
    for name, (_, _, _, status) in W.PAIRS.items():
        r = W.pair_spec(name)
        assert r["status"] == status, (name, r["status"])
        assert _comparable(r), (name, r["margin"], r["cond"])
        assert r["n_pairs"] >= 150 and len(W.pair(name)[0]["desc"]) == 300, name
    for octave in W.CLAMP_OCTAVES:
        r = W.clamp_spec(octave)
        assert r["status"] == S.OK and _comparable(r), (octave, r["margin"], r["cond"])
    assert "node" in W.pair("merge_2.4")[0] and "node" not in W.pair("merge_pi")[0]


def test_every_world_sim3_set_may_be_compared():
    for name in W.SIM3_SETS:
        r = W.sim3_spec(name)
        assert r["status"] == W.SIM3_STATUS.get(name, 0), (name, r["status"])
        assert _comparable(r), (name, r["margin"], r["cond"])
    for name in W.RESCALED:                                                      # the fixed scale is what these sets are about
        assert W.SIM3_SETS[name][2].get("fix_scale", True)


def test_world_runs_are_the_same_geometry_in_the_specification():
    """what the GPU file asserts of the GPU: a turned and shifted world changes no integer, mask or list"""
    base = W.pair_spec("world_none")
    for name in W.WORLD_NAMES:
        r = W.pair_spec(name)
        assert r["matches"] == base["matches"] and np.array_equal(r["feature_matches"], base["feature_matches"]), name
        assert np.array_equal(r["inlier"], base["inlier"]), name
        for k in ("status", "n_matches", "n_pairs", "best_hypothesis", "ransac_inliers", "n_inliers", "refined", "n_verified"):
            assert r[k] == base[k], (name, k)
    far = np.linalg.norm(W.pair("world_far")[1]["pose_wc"][4:])
    assert far > 2e4 and np.linalg.norm(W.pair(W.WORLD_NAMES[0])[1]["pose_wc"][4:]) > 1e3


def _branch(R):
    """which of quat_from_R's four branches a rotation takes, from its trace and diagonal"""
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return 0
    if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        return 1
    return 2 if R[1, 1] > R[2, 2] else 3


def test_rotation_table_takes_every_quaternion_branch():
    seen = {}
    for name in W.ROTATIONS:
        r = W.sim3_spec(name)
        seen.setdefault(_branch(r["M"]), []).append(name)                       # fix_scale: M is R
        p1, p2, gt = W.sim3_set(name)
        assert np.abs(r["M"] - gt["R"]).max() < 0.02, name
    assert sorted(seen) == [0, 1, 2, 3], seen
    # at pi about a coordinate axis the trace is -1 and the diagonal decides; the oblique and diagonal axes reach the branches too
    assert _branch(W.sim3_spec("rot_x_pi")["M"]) == 1 and _branch(W.sim3_spec("rot_y_pi")["M"]) == 2 and _branch(W.sim3_spec("rot_z_pi")["M"]) == 3
    assert _branch(W.sim3_spec("rot_identity")["M"]) == 0


def test_unrefined_sets_leave_by_the_unrefined_exit():
    fixed = [n for n in W.UNREFINED if W.SIM3_SETS[n][2].get("fix_scale", True)]
    free = [n for n in W.UNREFINED if not W.SIM3_SETS[n][2].get("fix_scale", True)]
    assert len(fixed) >= 2 and len(free) >= 1
    for name in W.UNREFINED:
        r = W.sim3_spec(name)
        assert r["status"] == 0 and r["refined"] == 0, (name, r["status"], r["refined"])
    for name in free:                                                            # the scale of an unrefined free-scale model is its sample's
        p1, p2, _ = W.sim3_set(name)
        idx = pnp_spec.sample(0, W.sim3_spec(name)["best_hypothesis"], len(p1), 3)
        assert W.sim3_spec(name)["sim3"][7] == S.horn(p1[idx], p2[idx], False)[1] and abs(W.sim3_spec(name)["sim3"][7] - 1.4) > 1e-3


def _reprojections(name_or_octave):
    """what the specification's reprojection loop sees: (depth in the loop camera, squared pixel error, loop octave) per gathered match"""
    if isinstance(name_or_octave, str):
        (cur, loop), r, cam = W.pair(name_or_octave), W.pair_spec(name_or_octave), W.PAIRS[name_or_octave][0]["camera"]
    else:
        (cur, loop), r, cam = W.clamp_pair(name_or_octave), W.clamp_spec(name_or_octave), W.PAIRS["cam_euroc"][0]["camera"]
    s = S.sim3_ransac(r["pts_current"], r["pts_loop"])
    inv = pnp_spec.se3_inverse(np.asarray(loop["pose_wc"], np.float64))
    out = []
    for (i, j), x in zip(r["feature_matches"], r["pts_current"]):
        p = S.transform_point(inv, s["M"] @ x + s["t"])
        du = cam["fx"] * p[0] / p[2] + cam["cx"] - float(loop["kp"]["x"][j]); dv = cam["fy"] * p[1] / p[2] + cam["cy"] - float(loop["kp"]["y"][j])
        out.append((p[2], du * du + dv * dv, int(loop["kp"]["octave"][j])))
    return np.array(out), r


def test_behind_scenes_have_matches_behind_the_loop_camera():
    """`behind` mirrors z alone, which also throws the pixel far off; `behind_centre` mirrors the whole point through the camera centre,
    which keeps its pixel: there the depth test alone decides, and leaving it out would change the count"""
    for name, alone in (("behind", 0), ("behind_centre", 1)):
        rows, r = _reprojections(name)
        thr = S.VERIFY_DEFAULTS["chi2"] * (S.VERIFY_DEFAULTS["scale_factor"] ** rows[:, 2]) ** 2
        n_behind, n_alone = int((rows[:, 0] <= 0.0).sum()), int(((rows[:, 0] <= 0.0) & (rows[:, 1] < thr)).sum())
        assert n_behind >= 1 and n_alone >= alone, (name, n_behind, n_alone)
        assert r["n_verified"] == int(((rows[:, 0] > 0.0) & (rows[:, 1] < thr)).sum())
        print("%s: %d of %d gathered matches behind the loop camera, %d of them within the pixel bound" % (name, n_behind, len(rows), n_alone))


def test_octave_clamp_changes_the_count():
    c = S.VERIFY_DEFAULTS
    for octave, clamped in zip(W.CLAMP_OCTAVES, (0, 31)):
        rows, r = _reprojections(octave)
        assert np.all(rows[:, 2] == octave)
        count = lambda o: int(((rows[:, 0] > 0.0) & (rows[:, 1] < c["chi2"] * (c["scale_factor"] ** o) ** 2)).sum())
        assert r["n_verified"] == count(clamped)
        assert count(octave) != count(clamped), octave                           # without the clamp the count differs: the case is not vacuous
        print("octave %d: %d verified with the clamp, %d without" % (octave, count(clamped), count(octave)))


def test_exact_sets_tie_everywhere():
    for name in W.EXACT_SETS:
        p1, p2, gt = W.sim3_set(name)
        r = W.sim3_spec(name)
        assert np.array_equal(p1 * 8, np.round(p1 * 8)) and np.array_equal(p2 * 8, np.round(p2 * 8)), name
        assert r["status"] == 0 and r["best_hypothesis"] == 0 and r["ransac_inliers"] == len(p1) and r["inlier"].all(), name
        assert np.abs(r["M"] - gt["R"]).max() < 1e-13 and np.abs(r["t"] - gt["t"]).max() < 1e-12, name


def test_hypothesis_edges_have_a_late_winner():
    b = W.sim3_spec("h_edges")["best_hypothesis"]
    assert b > 64 and b + 1 < 1024
    for H in W.H_EDGES + (b + 1, b):
        r = W.sim3_spec("h_edges", H)
        assert _comparable(r) or r["best_hypothesis"] < 0, (H, r["margin"], r["cond"])
        assert r["best_hypothesis"] < H
    assert W.sim3_spec("h_edges", b + 1)["best_hypothesis"] == b and W.sim3_spec("h_edges", b)["best_hypothesis"] != b
    assert W.sim3_spec("h_edges", 1023)["best_hypothesis"] == b
    assert len({W.sim3_spec("h_edges", H)["best_hypothesis"] for H in W.H_EDGES}) >= 4       # the edges do not all agree on a winner


def test_second_formulation_recovers_ground_truth():
    rng = np.random.default_rng(1)
    for axis, angle, scale in (((1.0, 0.0, 0.0), np.pi, 1.0), ((0.3, -0.8, 0.52), 2.2, 3.0), ((0.0, 0.0, 1.0), 1e-9, 0.05)):
        R = W._R(W._quat(axis, angle))
        p1 = rng.uniform(-5, 5, (30, 3)); t = rng.uniform(-3, 3, 3)
        q, s, tt = W.horn_quaternion(p1, scale * p1 @ R.T + t, False)
        assert np.abs(pnp_spec.quat_R(q) - R).max() < 1e-14 and abs(s - scale) < 1e-14 * scale and np.abs(tt - t).max() < 1e-13


def test_spreads_are_measured_and_the_plain_scenes_stay_on_the_floor():
    """The two spreads per OK set and pair (printed; DESIGN.md section 2 quotes them).  Near the origin at unit scale 50 x spread lies
    far below the figures of tests/test_loop_verify_gpu.py, which those scenes keep; away from there the GPU file takes the max."""
    rows = [(n, W.sim3_spec(n)["n_inliers"], W.sim3_spread(n)) for n in W.SIM3_SETS if W.sim3_spec(n)["status"] == 0 and n not in W.EXACT_SETS]
    rows += [(n, W.pair_spec(n)["n_inliers"], W.pair_spread(n)) for n in W.PAIRS if W.pair_spec(n)["status"] == S.OK]
    shifted = set(W.SPREAD_SETS) | set(W.SHIFTED)
    for name, n_inl, (model, mse) in rows:
        assert np.isfinite(model) and np.isfinite(mse), name
        if name not in shifted:
            assert 50.0 * model < 1e-9 and 50.0 * mse < 1e-9, (name, model, mse)
    for group, names in (("plain", [r[0] for r in rows if r[0] not in shifted]), ("offset sets", W.OFFSETS), ("scale sets", W.SCALES),
                         ("world pairs", W.WORLD_NAMES), ("merge pairs", [n for n in W.SHIFTED if n.startswith("merge_") and W.pair_spec(n)["status"] == S.OK])):
        sel = [r for r in rows if r[0] in names]
        print("%-12s model spread up to %.2e, mse spread up to %.2e" % (group, max(r[2][0] for r in sel), max(r[2][1] for r in sel)))
    # the bound never falls below the file's figure and follows the spread above it
    assert W.tolerances(100) == (1e-9, 1e-9) and W.tolerances(20) == (1e-8, 1e-9)
    assert W.tolerances(100, (1e-10, 1e-15)) == (5e-9, 1e-9) and W.tolerances(100, (1e-15, 1e-10)) == (1e-9, 5e-9)

