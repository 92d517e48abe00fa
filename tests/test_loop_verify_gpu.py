"""Loop-candidate verification on the GPU (orbx_verify_loop_candidates*, orbx_sim3_ransac_batch*, loop_verify_kernels.hip) against
the numpy restatement of its specification (tests/loop_verify_spec.py): the matcher exactly, distances included; the Sim3 solver
on its own; the whole call with every status; every form against every other byte for byte.

Tolerances.  Every integer, list, mask, status and best_hypothesis is exact: tests/test_loop_verify_cpu.py asserts for every scene
used here that no discrete decision lies within 1e-6 (relative) of its threshold and that no sample's SVD has sigma2 / sigma1 below
1e-5.  The Sim3 is measured as tests/test_pnp_gpu.py measures poses — rotation angle, relative translation, and the scale — to 1e-9
where the final fit has at least 50 inliers and 1e-8 for smaller fits (that file's figures for the same situation); mse to 1e-9
relative."""
import json
import os

import numpy as np
import pytest

import loop_verify_scenes as Z
import loop_verify_spec as S
import pnp_spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_SCENES = [n for n, (_, c, s, _) in Z.PAIRS.items() if not c and not s]      # the scenes that run under the default configuration
worst = dict(angle=0.0, translation=0.0, scale=0.0, mse=0.0)                         # the largest deviations seen (printed at the end)


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.CameraModel(**Z.CAMERA)


def _cfg(pkg, verify=None, sim3=None):
    return pkg.LoopVerifyConfig(**dict(verify or {}, sim3=pkg.Sim3SolverConfig(**(sim3 or {}))))


def _sim3_close(g, s, n_inliers, where, tol=None, worst=worst):
    """tol, worst: for tests/test_loop_verify_world_gpu.py, which states its own bound where a scene lies far from the origin or from
    unit scale and keeps its own record"""
    tol = tol or (1e-9 if n_inliers >= 50 else 1e-8)
    ang = pnp_spec.rotation_angle(g[:7], s[:7])
    dt = np.linalg.norm(g[4:7] - s[4:7]) / max(np.linalg.norm(s[4:7]), 1e-12)
    ds = abs(g[7] - s[7]) / s[7]
    worst.update(angle=max(worst["angle"], ang), translation=max(worst["translation"], dt), scale=max(worst["scale"], ds))
    assert g[0] >= 0.0 and ang < tol and dt < tol and ds < tol, (where, ang, dt, ds)


def _mse_close(g, s, where, tol=1e-9, worst=worst):
    if s == 0.0:
        assert g == 0.0, where
        return
    worst["mse"] = max(worst["mse"], abs(g - s) / s)
    assert abs(g - s) <= tol * s, (where, g, s)


def assert_pair_matches_spec(g, s, where="", tol=None, mse_tol=1e-9, worst=worst):
    assert g["status"] == s["status"], (where, g["status"], s["status"])
    for k in ("n_matches", "n_pairs", "best_hypothesis", "ransac_inliers", "n_inliers", "refined", "n_verified"):
        assert g["stats"][k] == s[k], (where, k, g["stats"][k], s[k])
    m = g["matches"]
    assert [(int(a), int(b), int(c)) for a, b, c in zip(m["query_idx"], m["train_idx"], m["distance"])] == s["matches"], where
    assert np.all(m["img_idx"] == 0) and np.array_equal(m["distance"], np.round(m["distance"]))
    assert np.array_equal(g["feature_matches"], s["feature_matches"]), where
    assert g["pts_current"].tobytes() == s["pts_current"].tobytes() and g["pts_loop"].tobytes() == s["pts_loop"].tobytes(), where
    assert np.array_equal(g["inlier"], s["inlier"]), where
    if s["status"] in (S.OK, S.TOO_FEW_INLIERS, S.TOO_FEW_VERIFIED):
        _sim3_close(g["sim3"], s["sim3"], s["n_inliers"], where, tol, worst)
    else:
        assert g["sim3"].tobytes() == S.IDENTITY.tobytes(), where
    _mse_close(g["stats"]["mse"], s["mse"], where, mse_tol, worst)


def _bytes(r):
    return (r["status"], r["matches"].tobytes(), r["feature_matches"].tobytes(), r["pts_current"].tobytes(), r["pts_loop"].tobytes(),
            r["inlier"].tobytes(), r["sim3"].tobytes(), r["record"].tobytes())


def _matches(r):
    m = r["matches"]
    return [(int(a), int(b), int(c)) for a, b, c in zip(m["query_idx"], m["train_idx"], m["distance"])]


# ---- the matcher ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", Z.MATCH_SHAPES)
def test_matcher_equals_spec(gpu_handle, cam, pkg, shape, ties):
    d1, d2 = Z.descriptor_table(1000 + shape[0] * 7 + shape[1], *shape, ties=ties)
    for ratio, max_dist in ((0.7, 50), (2.0, 256)):
        r = gpu_handle.verify_loop_candidates(cam, [(Z.as_keyframe(d1), Z.as_keyframe(d2))],
                                              _cfg(pkg, dict(Z.MATCH_ONLY, match_ratio=ratio, match_max_dist=max_dist)))[0]
        want = S.match_features(d1, d2, max_dist=max_dist, ratio=ratio)
        assert r["status"] == S.TOO_FEW_PAIRS and _matches(r) == want, (shape, ties, ratio)
        assert [tuple(x) for x in r["feature_matches"]] == [(i, j) for i, j, _ in want]      # every feature has a stereo point here


def test_matcher_2000_by_2000(gpu_handle, cam, pkg):
    d1, d2 = Z.descriptor_table(77, 2000, 2000)
    r = gpu_handle.verify_loop_candidates(cam, [(Z.as_keyframe(d1), Z.as_keyframe(d2))], _cfg(pkg, Z.MATCH_ONLY))[0]
    want = S.match_features(d1, d2)
    assert len(want) > 300 and _matches(r) == want


def test_matcher_decision_table_feature_vector_form(gpu_handle, cam, pkg):
    cases, d1, n1, d2, n2 = Z.decision_table()
    r = gpu_handle.verify_loop_candidates(cam, [(Z.as_keyframe(d1, n1), Z.as_keyframe(d2, n2))], _cfg(pkg, Z.MATCH_ONLY))[0]
    want = S.match_features(d1, d2, n1, n2)
    assert _matches(r) == want
    got = {i for i, _, _ in want}
    for i, (b, s) in enumerate(cases):                      # the rule itself, independent of the spec's loop
        assert (i in got) == (b < 50 and b < 0.7 * (S.U32_MAX if s is None else s)), (b, s)
    assert any(s is None and b == 49 and i in got for i, (b, s) in enumerate(cases))
    assert not any(b == 50 and i in got for i, (b, s) in enumerate(cases))


def test_matcher_boundaries_as_a_brute_force_batch(gpu_handle, cam, pkg):
    cases = [(b, s) for b in range(45, 53) for s in range(b, 81)]
    zero = Z.popcount_rows(0)[None]
    pairs = [(Z.as_keyframe(zero), Z.as_keyframe(np.stack([Z.popcount_rows(s), Z.popcount_rows(b)]) if k % 2 else
                                                 np.stack([Z.popcount_rows(b), Z.popcount_rows(s)]))) for k, (b, s) in enumerate(cases)]
    res = gpu_handle.verify_loop_candidates(cam, pairs, _cfg(pkg, Z.MATCH_ONLY))
    for k, ((b, s), r) in enumerate(zip(cases, res)):
        accept = b < 50 and b < 0.7 * s
        best_j = 0 if b == s else (1 if k % 2 else 0)       # the lowest index keeps a tie
        assert _matches(r) == ([(0, best_j, b)] if accept else []), (b, s, k)
    lone = gpu_handle.verify_loop_candidates(cam, [(Z.as_keyframe(zero), Z.as_keyframe(Z.popcount_rows(b)[None])) for b in (49, 50)],
                                             _cfg(pkg, Z.MATCH_ONLY))
    assert _matches(lone[0]) == [(0, 0, 49)] and _matches(lone[1]) == []


def test_matcher_nodes_absent_or_none(gpu_handle, cam, pkg):
    d1, d2 = Z.descriptor_table(5, 40, 50)
    rng = np.random.default_rng(3)
    n1 = rng.integers(0, 6, 40).astype(np.uint32); n2 = rng.integers(3, 9, 50).astype(np.uint32)       # nodes 0-2 only left, 6-8 only right
    n1[::7] = S.NODE_NONE; n2[::5] = S.NODE_NONE
    cfg = _cfg(pkg, dict(Z.MATCH_ONLY, match_ratio=2.0, match_max_dist=256))
    r = gpu_handle.verify_loop_candidates(cam, [(Z.as_keyframe(d1, n1), Z.as_keyframe(d2, n2))], cfg)[0]
    want = S.match_features(d1, d2, n1, n2, max_dist=256, ratio=2.0)
    assert want and _matches(r) == want and all(n1[i] == n2[j] and n1[i] != S.NODE_NONE for i, j, _ in want)
    none1, none2 = np.full(40, S.NODE_NONE, np.uint32), np.full(50, S.NODE_NONE, np.uint32)
    r = gpu_handle.verify_loop_candidates(cam, [(Z.as_keyframe(d1, none1), Z.as_keyframe(d2, none2))], cfg)[0]
    assert _matches(r) == []


# ---- Sim3 on its own --------------------------------------------------------------------------------------------------
def _assert_sim3(g_sim3, g_inl, g_rec, s, where):
    for k in ("status", "best_hypothesis", "ransac_inliers", "n_inliers", "refined"):
        assert int(g_rec[k]) == s[k], (where, k, int(g_rec[k]), s[k])
    assert np.array_equal(g_inl, s["inlier"]), where
    if s["status"] == 0:
        _sim3_close(g_sim3, s["sim3"], s["n_inliers"], where)
    else:
        assert g_sim3.tobytes() == S.IDENTITY.tobytes(), where
    _mse_close(float(g_rec["mse"]), s["mse"], where)


@pytest.mark.parametrize("name", sorted(Z.SIM3_SETS))
def test_sim3_equals_spec(gpu_handle, pkg, name):
    p1, p2, _ = Z.sim3_set(name)
    sim3, inl, rec = gpu_handle.compute_sim3_ransac_batch([(p1, p2)], pkg.Sim3SolverConfig(**Z.SIM3_SETS[name][1]))
    _assert_sim3(sim3[0], inl[0], rec[0], Z.sim3_spec(name), name)
    assert np.all(np.isfinite(sim3))


def test_sim3_batch_and_device_forms_equal_single_calls(gpu_handle, pkg):
    import torch
    names = [n for n in sorted(Z.SIM3_SETS) if not Z.SIM3_SETS[n][1]]
    probs = [Z.sim3_set(n)[:2] for n in names]
    sim3, inl, rec = gpu_handle.compute_sim3_ransac_batch(probs)
    for k, n in enumerate(names):
        a, b, c = gpu_handle.compute_sim3_ransac_batch([probs[k]])
        assert a[0].tobytes() == sim3[k].tobytes() and b[0].tobytes() == inl[k].tobytes() and c[0].tobytes() == rec[k].tobytes(), n
    off = np.zeros(len(probs) + 1, np.int32); off[1:] = np.cumsum([len(p[0]) for p in probs])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ds, di, dr = gpu_handle.compute_sim3_ransac_batch_device(t(off), t(np.concatenate([p[0] for p in probs])), t(np.concatenate([p[1] for p in probs])),
                                                             max(len(p[0]) for p in probs))
    gpu_handle.synchronize()
    assert ds.cpu().numpy().tobytes() == sim3.tobytes() and di.cpu().numpy().tobytes() == np.concatenate(inl).tobytes()
    assert dr.cpu().numpy().tobytes() == rec.tobytes()


def test_sim3_known_answers_of_the_reference(gpu_handle, pkg):
    """sim3_solver.rs:334-405 through the public call with min_inliers = 3.  The ten points are collinear, so every sample's H and the
    refit's H have rank 1: the rotation about the line is free, and what the reference asserts — scale, translation, transformed
    points — is what is asserted here, with all ten inliers and no NaN.  (No equality with the spec: it is free there too.)"""
    ka = json.load(open(os.path.join(ROOT, "tests", "golden", "loop_verify_known_answers.json")))
    for case in ka["cases"]:
        p1 = np.array([[(i + case["first"]) * k for k in (1.0, 2.0, 3.0)] for i in range(10)])
        p2 = case["scale"] * p1 @ np.array(case["rotation"], np.float64).T + np.array(case["translation"], np.float64)
        sim3, inl, rec = gpu_handle.compute_sim3_ransac_batch([(p1, p2)], pkg.Sim3SolverConfig(min_inliers=3, fix_scale=case["fix_scale"]))
        g = sim3[0]
        assert int(rec[0]["status"]) == 0 and int(rec[0]["n_inliers"]) == 10 and inl[0].all() and np.all(np.isfinite(g)), case["name"]
        assert abs(np.linalg.norm(g[:4]) - 1.0) < 1e-12
        assert abs(g[7] - case["scale"]) < ka["tolerance"] and np.abs(g[4:7] - case["translation"]).max() < ka["tolerance"], (case["name"], g)
        moved = np.array([g[7] * S.quat_rot(g[:4], p) + g[4:7] for p in p1])
        assert np.abs(moved - p2).max() < ka["tolerance"], case["name"]


def test_sim3_degenerate_inputs_give_proper_rotations(gpu_handle, pkg):
    same = np.tile([1.0, 2.0, 3.0], (20, 1))                                # every sample's H is zero
    line = np.outer(np.arange(20.0), [1.0, 0.0, 0.0])
    for p1, p2 in ((same, same + 0.5), (line, line[:, [1, 0, 2]]), (line, line * 0.0)):
        sim3, inl, rec = gpu_handle.compute_sim3_ransac_batch([(p1, p2)], pkg.Sim3SolverConfig(min_inliers=3))
        assert np.all(np.isfinite(sim3)) and abs(np.linalg.norm(sim3[0][:4]) - 1.0) < 1e-12 and sim3[0][0] >= 0.0


def test_sim3_ground_truth(gpu_handle, pkg):
    for name in ("n64_o30", "n300_o60", "coplanar", "reflection", "free_scale"):
        p1, p2, gt = Z.sim3_set(name)
        sim3, inl, rec = gpu_handle.compute_sim3_ransac_batch([(p1, p2)], pkg.Sim3SolverConfig(**Z.SIM3_SETS[name][1]))
        R = pnp_spec.quat_R(sim3[0][:4])
        assert int(rec[0]["status"]) == 0 and abs(np.linalg.det(R) - 1.0) < 1e-12, name
        if name != "reflection":
            assert np.abs(sim3[0][7] * R - gt["scale"] * gt["R"]).max() < 0.02 and np.abs(sim3[0][4:7] - gt["t"]).max() < 0.1, name


# ---- the whole call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(Z.PAIRS))
def test_pair_equals_spec(gpu_handle, cam, pkg, name):
    r = gpu_handle.verify_loop_candidates(cam, [Z.pair(name)], _cfg(pkg, Z.PAIRS[name][1], Z.PAIRS[name][2]))[0]
    assert r["status"] == Z.PAIRS[name][3]
    assert_pair_matches_spec(r, Z.pair_spec(name), name)


def _kf(pkg, h, d):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n = len(d["desc"])
    kp = t(np.ascontiguousarray(d["kp"]).view(np.uint8).reshape(n, 28)) if n else None
    kf = pkg.KeyFrame(h, kp, t(d["desc"]) if n else None, n, t(d["points_cam"]) if n else None, t(d["has_point"]) if n else None, pose_wc=d["pose_wc"])
    if "node" in d:
        kf.set_feature_nodes(d["node"])
    return kf


@pytest.mark.parametrize("B", [1, 7, 16])
def test_batches_equal_single_calls_in_every_form(gpu_handle, cam, pkg, B):
    import torch
    names = [DEFAULT_SCENES[(2 * k) % len(DEFAULT_SCENES)] for k in range(B)]
    single = {n: gpu_handle.verify_loop_candidates(cam, [Z.pair(n)])[0] for n in set(names)}
    for n in set(names):
        assert_pair_matches_spec(single[n], Z.pair_spec(n), n)
    # resident keyframes: brute-force and FeatureVector pairs in one call, keyframes repeated
    kfs = {n: (_kf(pkg, gpu_handle, Z.pair(n)[0]), _kf(pkg, gpu_handle, Z.pair(n)[1])) for n in set(names)}
    res = pkg.KeyFrame.verify_loop_candidates(gpu_handle, cam, [kfs[n][0] for n in names], [kfs[n][1] for n in names])
    assert len({r["status"] for r in res}) >= min(B, 3)
    for n, r in zip(names, res):
        assert _bytes(r) == _bytes(single[n]), n
    for a, b in kfs.values():
        a.close(); b.close()
    # the packed host and device forms, one matcher form per call
    for fv in (False, True):
        sub = [n for n in names if ("node" in Z.pair(n)[0]) == fv]
        if not sub:
            continue
        pairs = [Z.pair(n) for n in sub]
        for n, r in zip(sub, gpu_handle.verify_loop_candidates(cam, pairs)):
            assert _bytes(r) == _bytes(single[n]), n
        a, cn, ln, co, lo, cp, lp = gpu_handle._loop_verify_pack(pairs)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        o = gpu_handle.verify_loop_candidates_device(cam, t(a["cur_desc"]), t(a["cur_pts"]), t(a["cur_has"]), co, cp,
                                                     t(a["loop_kp"].view(np.uint8).reshape(-1, 28)), t(a["loop_desc"]), t(a["loop_pts"]),
                                                     t(a["loop_has"]), lo, lp, cn, ln)
        gpu_handle.synchronize()
        rec = o["results"].cpu().numpy().view(pkg.LOOP_VERIFY_RESULT).reshape(-1)
        dev = gpu_handle._loop_verify_unpack(len(sub), co, o["matches"].cpu().numpy().view(pkg.DMATCH).reshape(-1), o["feature_matches"].cpu().numpy(),
                                             o["pts_current"].cpu().numpy(), o["pts_loop"].cpu().numpy(), o["inlier"].cpu().numpy(),
                                             o["sim3"].cpu().numpy(), rec)
        for n, r in zip(sub, dev):
            assert _bytes(r) == _bytes(single[n]), n


def test_host_mirror_returns_none_where_the_reference_does(gpu_handle, cam, pkg):
    cur, loop = Z.pair("ok_bf")
    cur = dict(cur, map_points=[i if i % 2 else None for i in range(len(cur["desc"]))])
    loop = dict(loop, map_points=list(range(1000, 1000 + len(loop["desc"]))))
    v = pkg.verify_loop_candidate(cur, loop, cam, 7, 3, handle=gpu_handle)
    s = Z.pair_spec("ok_bf")
    assert v is not None and (v.current_kf_id, v.loop_kf_id) == (7, 3) and np.array_equal(v.feature_matches, s["feature_matches"])
    assert v.matched_map_points == [(int(i), 1000 + int(j)) for i, j in s["feature_matches"] if i % 2]
    assert pkg.verify_loop_candidate(*Z.pair("few_verified"), cam, handle=gpu_handle) is None


def test_out_of_range_configurations_are_refused(gpu_handle, cam, pkg):
    p1, p2, _ = Z.sim3_set("n15_o0")
    for bad in (dict(max_iterations=0), dict(max_iterations=1025), dict(inlier_threshold=0.0), dict(min_inliers=2), dict(probability=1.5)):
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.compute_sim3_ransac_batch([(p1, p2)], pkg.Sim3SolverConfig(**bad))
        assert e.value.code == -1, bad
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.verify_loop_candidates(cam, [Z.pair("tiny_fit")], _cfg(pkg, None, bad))
        assert e.value.code == -1, bad
    for bad in (dict(min_matches=-1), dict(match_max_dist=257), dict(match_ratio=0.0), dict(chi2=-1.0), dict(scale_factor=0.0)):
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.verify_loop_candidates(cam, [Z.pair("tiny_fit")], _cfg(pkg, bad))
        assert e.value.code == -1, bad
    sim3, inl, rec = gpu_handle.compute_sim3_ransac_batch([(p1, p2)], pkg.Sim3SolverConfig(max_iterations=1024))
    assert int(rec[0]["status"]) == 0


def test_zz_report_largest_deviations():
    """not a check of its own: prints the largest deviations the tests above measured (DESIGN.md §2 quotes them)"""
    print("loop verification, largest deviations from the specification: rotation %.3e rad, translation %.3e relative, scale %.3e relative, "
          "mse %.3e relative" % (worst["angle"], worst["translation"], worst["scale"], worst["mse"]))
