"""PnP-RANSAC on the GPU (orbx_pnp_ransac*, pnp_kernels.hip) against the numpy restatement of its specification (tests/pnp_spec.py)
and against synthetic ground truth; batch, device and single forms against each other byte for byte; the reference's fallbacks."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pnp_spec as S
from test_pnp_cpu import build_pnp_driver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.CameraModel(**pkg.synth.EUROC_CAMERA)


def assert_matches_spec(g, s, where=""):
    st = g.stats
    for k in ("status", "best_hypothesis", "hypotheses_evaluated", "ransac_inliers", "n_inliers"):
        assert st[k] == s[k], (where, k, st[k], s[k])
    assert np.array_equal(g.inlier_mask, s["inlier_mask"]), where
    # How closely two correct implementations agree on the pose is set by how sharply the cost determines its minimum.  Fewer than
    # three inliers leave the final LM fewer residuals than the pose has parameters: the pose is then the hypothesis LM's last
    # iterate on the sample (4 <= n <= model_points with outliers among the points), an ill-conditioned system on which rounding
    # differs by up to ~1e-8 relative.  A fit to a dozen points has a shallow direction (rotation against translation) along which
    # the cost cannot tell steps of ~1e-9 apart.  From 50 inliers on the stated 1e-9 holds.
    k = s["ransac_inliers"]
    tol_px, tol = (1e-7, 1e-9) if s["status"] != S.OK or k >= 50 else ((1e-6, 1e-8) if k >= 3 else (1e-5, 1e-6))
    e, f = g.reproj_errors, s["reproj_errors"]
    assert np.array_equal(np.isinf(e), np.isinf(f)) and np.array_equal(np.isnan(e), np.isnan(f)), where
    fin = np.isfinite(f)
    assert np.all(np.abs(e[fin] - f[fin]) < tol_px), (where, np.abs(e[fin] - f[fin]).max())
    if s["status"] != S.OK:
        assert g.pose.tobytes() == s["pose"].tobytes(), where
    assert S.rotation_angle(g.pose, s["pose"]) < tol, (where, S.rotation_angle(g.pose, s["pose"]))
    dt = np.linalg.norm(g.pose[4:] - s["pose"][4:]) / max(np.linalg.norm(s["pose"][4:]), 1e-12)
    assert dt < tol, (where, dt)


def _bytes(r):
    return (r.pose.tobytes(), r.inlier_mask.tobytes(), r.reproj_errors.tobytes(), tuple(sorted(r.stats.items())))


@pytest.mark.parametrize("outliers", [0.0, 0.3, 0.6])
@pytest.mark.parametrize("n", [4, 5, 12, 300, 2000, 8192])
def test_parity_with_spec(gpu_handle, cam, pkg, n, outliers):
    for seed in (1, 2):
        s = pkg.synth.pnp_problem(seed * 7919 + n, n, outliers, prior_rot_deg=10.0, prior_trans_m=0.3)
        g = gpu_handle.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], s["prior_wc"])
        want = S.solve(s["camera"], s["points3d"], s["points2d"], s["prior_wc"])
        assert_matches_spec(g, want, (n, outliers, seed))


@pytest.mark.parametrize("outliers", [0.0, 0.3, 0.6])
@pytest.mark.parametrize("n", [100, 400, 1500])
def test_recovers_ground_truth(gpu_handle, cam, pkg, n, outliers):
    cfg = pkg.PnPConfig(max_iterations=1000) if outliers > 0.5 else None     # (as the CPU test: 0.4^5 clean samples)
    for seed in range(3):
        s = pkg.synth.pnp_problem(100 * seed + n, n, outliers, prior_rot_deg=15.0, prior_trans_m=0.5)
        g = gpu_handle.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], s["prior_wc"], cfg)
        assert g.stats["status"] == pkg.PNP_OK
        assert S.rotation_angle(g.pose, s["pose_wc"]) < 1e-3
        assert np.linalg.norm(g.pose[4:] - s["pose_wc"][4:]) < 1e-2
        assert np.array_equal(g.inlier_mask, s["inliers"])


def _mixed_problems(pkg, count=512):
    sizes = [0, 3, 4, 5, 6, 12, 50, 300, 1000, 4000]
    probs = []
    for i in range(count):
        n = sizes[i % len(sizes)] if i % 17 else 200
        of = 1.0 if i % 17 == 0 else (0.0, 0.3, 0.6)[i % 3]          # every 17th: all outliers (NO_MODEL scenes)
        s = pkg.synth.pnp_problem(1000 + i, n, of, prior_rot_deg=10.0, prior_trans_m=0.3)
        probs.append((s["points3d"], s["points2d"], s["prior_wc"]))
    return probs


def test_batch_equals_singles(gpu_handle, cam, pkg):
    probs = _mixed_problems(pkg)
    batch = gpu_handle.solve_pnp_ransac_batch(cam, probs)
    statuses = set()
    for i, (p, b) in enumerate(zip(probs, batch)):
        one = gpu_handle.solve_pnp_ransac_detailed(cam, *p)
        assert _bytes(one) == _bytes(b), i
        statuses.add(b.stats["status"])
    assert statuses == {pkg.PNP_OK, pkg.PNP_NO_MODEL, pkg.PNP_TOO_FEW}


def test_device_form_equals_host_form(gpu_handle, cam, pkg):
    import torch
    probs = _mixed_problems(pkg, 96)
    host = gpu_handle.solve_pnp_ransac_batch(cam, probs)
    n = np.array([len(p[0]) for p in probs])
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    dev = torch.device("cuda", 0)
    max_n = 1000                                                         # the 4000-point problems: OVER_MAX_N
    t = [torch.from_numpy(a).to(dev) for a in (off, np.concatenate([p[0] for p in probs]), np.concatenate([p[1] for p in probs]),
                                               np.stack([p[2] for p in probs]))]
    poses, inl, err, res = gpu_handle.solve_pnp_ransac_batch_device(cam, *t, max_n=max_n)
    torch.cuda.synchronize()
    poses, inl, err = poses.cpu().numpy(), inl.cpu().numpy(), err.cpu().numpy()
    res = res.cpu().numpy().view(pkg.PNP_RESULT).reshape(-1)
    over = 0
    for p, h in enumerate(host):
        sl = slice(off[p], off[p + 1])
        if n[p] > max_n:
            over += 1
            assert res[p]["status"] == pkg.PNP_OVER_MAX_N and poses[p].tobytes() == probs[p][2].tobytes()
            e, m = S.detailed(pkg.synth.EUROC_CAMERA, probs[p][2], probs[p][0], probs[p][1].astype(np.float64), 8.0)
            assert np.array_equal(inl[sl].astype(bool), m) and np.allclose(err[sl], e, rtol=0, atol=1e-7)
            continue
        assert poses[p].tobytes() == h.pose.tobytes(), p
        assert inl[sl].tobytes() == h.inlier_mask.astype(np.uint8).tobytes() and err[sl].tobytes() == h.reproj_errors.tobytes(), p
        assert {k: (float(res[p][k]) if k == "final_rms" else int(res[p][k])) for k in pkg.PNP_RESULT.names} == h.stats, p
    assert over > 0


def test_fallbacks(gpu_handle, cam, pkg):
    # all outliers: no hypothesis passes the walk -> NO_MODEL and the prior's bytes (the reference ignores solvePnPRansac's bool)
    for seed in range(3):
        s = pkg.synth.pnp_problem(seed, 200, 1.0, 5.0, 0.1)
        g = gpu_handle.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], s["prior_wc"])
        assert g.stats["status"] == pkg.PNP_NO_MODEL and g.pose.tobytes() == s["prior_wc"].tobytes()
        assert_matches_spec(g, S.solve(s["camera"], s["points3d"], s["points2d"], s["prior_wc"]))
    # n < 4: TOO_FEW, the prior, and the detailed pass at the prior
    for n in (0, 1, 3):
        s = pkg.synth.pnp_problem(40 + n, n, 0.0, 5.0, 0.1)
        g = gpu_handle.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], s["prior_wc"])
        assert g.stats["status"] == pkg.PNP_TOO_FEW and g.pose.tobytes() == s["prior_wc"].tobytes() and len(g.inlier_mask) == n
        assert_matches_spec(g, S.solve(s["camera"], s["points3d"], s["points2d"], s["prior_wc"]))
    # NaN rows are never inliers; the rest of the problem is still solved
    s = pkg.synth.pnp_problem(77, 400, 0.2, 10.0, 0.3)
    p3, p2 = s["points3d"].copy(), s["points2d"].copy()
    p3[[5, 100]] = np.nan
    p2[[7, 200], 0] = np.nan
    g = gpu_handle.solve_pnp_ransac_detailed(cam, p3, p2, s["prior_wc"])
    assert g.stats["status"] == pkg.PNP_OK
    assert not g.inlier_mask[[5, 7, 100, 200]].any()
    keep = np.ones(400, bool); keep[[5, 7, 100, 200]] = False
    assert np.array_equal(g.inlier_mask[keep], s["inliers"][keep])
    assert S.rotation_angle(g.pose, s["pose_wc"]) < 1e-3 and np.linalg.norm(g.pose[4:] - s["pose_wc"][4:]) < 1e-2


def test_deterministic_and_seeded(gpu_handle, cam, pkg):
    s = pkg.synth.pnp_problem(5, 1500, 0.4, 15.0, 0.5)
    a = gpu_handle.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], s["prior_wc"])
    b = gpu_handle.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], s["prior_wc"])
    assert _bytes(a) == _bytes(b)
    changed = False
    for seed in (1, 2, 3):
        c = gpu_handle.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], s["prior_wc"], pkg.PnPConfig(seed=seed))
        changed |= c.stats["best_hypothesis"] != a.stats["best_hypothesis"]
        assert S.rotation_angle(c.pose, s["pose_wc"]) < 1e-3 and np.linalg.norm(c.pose[4:] - s["pose_wc"][4:]) < 1e-2
        assert np.array_equal(c.inlier_mask, s["inliers"])
        assert_matches_spec(c, S.solve(s["camera"], s["points3d"], s["points2d"], s["prior_wc"], dict(seed=seed)))
    assert changed


def test_module_level_functions(pkg):
    s = pkg.synth.pnp_problem(11, 300, 0.3, 10.0, 0.3)
    camera = pkg.CameraModel(**pkg.synth.EUROC_CAMERA)
    r = pkg.solve_pnp_ransac_detailed(s["points3d"], s["points2d"], camera, s["prior_wc"])
    assert np.array_equal(r.inlier_mask, s["inliers"])
    assert pkg.solve_pnp_ransac(s["points3d"], s["points2d"], camera, s["prior_wc"]).tobytes() == r.pose.tobytes()


def test_cpp_mirror_equals_python(gpu_handle, cam, pkg, tmp_path):
    exe = build_pnp_driver(str(tmp_path))
    for seed, n, of in ((3, 500, 0.3), (4, 2, 0.0), (5, 200, 1.0)):
        s = pkg.synth.pnp_problem(seed, n, of, 10.0, 0.3)
        fin, fout = os.path.join(tmp_path, "in.bin"), os.path.join(tmp_path, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<i", n)); f.write(s["prior_wc"].tobytes())
            f.write(np.ascontiguousarray(s["points3d"]).tobytes()); f.write(np.ascontiguousarray(s["points2d"]).tobytes())
        subprocess.run([exe, fin, fout], check=True, timeout=120)
        out = open(fout, "rb").read()
        g = gpu_handle.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], s["prior_wc"])
        assert out == g.pose.tobytes() + g.inlier_mask.astype(np.uint8).tobytes() + g.reproj_errors.tobytes()
