"""CPU checks of the frame tracker's specification (tests/tracking_spec.py), of the scenes the GPU tests run
(tests/tracking_scenes.py) and of the new ABI (orbx_track_config / orbx_track_result / orbx_track_frames[_device])."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import tracking_scenes as G
import tracking_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = G.CAMERA


@pytest.fixture(scope="module")
def known():
    with open(os.path.join(ROOT, "tests", "golden", "tracking_known_answers.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("mode", [0, 1])
def test_spec_reproduces_hand_written_answers(oracle, known, mode):
    """tests/golden/tracking_known_answers.json: identity pose, fx = fy = 100, principal point (376, 240), five map points and three
    features whose projections, cells and Hamming distances were worked out by hand:
      point 0 (0,0,2)       -> (376, 240); candidates feature 0 (distance 0) and 2 (16): feature 0 in both modes;
      point 1 (1,0,2)       -> (426, 240); one candidate, feature 1 at distance exactly 100: mode 1 accepts (<=), mode 0 does not (<);
      point 2 (0,0,-1)      behind the camera;
      point 3 (10,0,2)      -> (876, 240): outside 2cx = 752 (mode 0 skips it), first cell 73 past the last (mode 1 finds no candidate);
      point 4 (1/32,0,2)    -> (377.5625, 240); features 0 and 2 both at distance 8: mode 0 takes feature 2 (grid row 23 is visited before
                            row 24), mode 1's ratio test (8 > 0.75 * 8) rejects."""
    k = known
    cfg = S.default_config(mode)
    kp = G.keypoints(k["kp_xy"]); desc = np.array(k["desc"], np.uint8); md = np.array(k["mp_desc"], np.uint8)
    z, u, v = S.project(k["camera"], k["pose_wc"], k["positions"])
    assert z.tolist() == k["z"]
    for i, uv in enumerate(k["uv"]):
        if uv is not None:
            assert [u[i], v[i]] == uv
    m = S.search(oracle, k["camera"], cfg, kp, desc, k["positions"], md, k["pose_wc"])
    want = k["mode%d" % mode]
    assert m.tolist() == want["match"] and int((m >= S.NONE).sum()) == k["n_in_front"]
    g = S.gather(kp, k["positions"], m)
    assert g["mp_idx"].tolist() == want["mp_idx"] and g["feat_idx"].tolist() == want["feat_idx"] and g["points2d"].tolist() == want["points2d"]
    assert g["points3d"].tolist() == [k["positions"][i] for i in want["mp_idx"]] and g["points2d"].dtype == np.float32


def test_projection_of_a_general_pose_agrees_with_rotation_matrices():
    rng = np.random.default_rng(3)
    T = G.pose(rng)
    X = rng.uniform(-5.0, 5.0, (50, 3))
    z, u, v = S.project(CAM, T, X)
    w, x, y, zq = T[:4]
    R = np.array([[1 - 2 * (y * y + zq * zq), 2 * (x * y - w * zq), 2 * (x * zq + w * y)], [2 * (x * y + w * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - w * x)],
                  [2 * (x * zq - w * y), 2 * (y * zq + w * x), 1 - 2 * (x * x + y * y)]])
    pc = (X - T[4:]) @ R
    assert np.allclose(z, pc[:, 2], atol=1e-12)
    f = z > 0.1
    assert f.any() and np.allclose(u[f], CAM["fx"] * pc[f, 0] / pc[f, 2] + CAM["cx"], atol=1e-9)
    assert np.allclose(v[f], CAM["fy"] * pc[f, 1] / pc[f, 2] + CAM["cy"], atol=1e-9)


def _match(oracle, f, mode):
    return S.search(oracle, CAM, S.default_config(mode), f[0], f[1], f[2], f[3], f[4])


def test_modes_differ_where_the_reference_does(oracle):
    # bounds test in mode 0 only
    f = G.edge_outside(29)
    m0, m1 = _match(oracle, f, 0), _match(oracle, f, 1)
    assert (m0 == S.NONE).all()
    assert m1.tolist() == [0, 1, 2, -1, 4, 5, -1]      # u = -100 wraps to whole rows; u = 2000 and v = 497 start past the last cell
    # ratio test in mode 1 only
    f = G.edge_ratio(32)
    assert _match(oracle, f, 0).tolist() == [0, 2] and _match(oracle, f, 1).tolist() == [0, -1]
    # `<` against `<=` at TH_HIGH, and no ratio test with one candidate
    f = G.edge_single(31)
    assert _match(oracle, f, 0).tolist() == [0, -1, -1, -1] and _match(oracle, f, 1).tolist() == [0, 1, -1, -1]
    # the tie rule: the first cell wins although it holds the higher feature index
    f = G.edge_ties(30)
    assert _match(oracle, f, 0).tolist() == [1, 3] and _match(oracle, f, 1).tolist() == [-1, 3]


def _finish(cfg, n_feat, match, g, inl, pnp_status=0):
    prior = np.arange(7.0); pnp_pose = np.arange(7.0) + 10.0
    return S.finish(cfg, n_feat, match, g, prior, pnp_pose, inl, pnp_status, int(np.sum(inl))) + (prior, pnp_pose)


def _hand_frame(n_corr, n_feat=12, shared=None):
    """n_corr correspondences: map point i on feature i, or on feature shared[i]"""
    match = np.arange(n_corr, dtype=np.int32)
    for i, f in (shared or {}).items():
        match[i] = f
    kp = G.keypoints(np.stack([np.arange(n_feat) * 10.0, np.arange(n_feat) * 5.0], 1))
    return match, S.gather(kp, np.arange(3.0 * n_corr).reshape(-1, 3), match)


def test_two_inliers_on_one_feature_the_later_one_wins():
    match, g = _hand_frame(6, shared={4: 1})
    rec, pose, matched, prior, pnp_pose = _finish(S.default_config(1), 12, match, g, np.ones(6, bool))
    assert rec == dict(status=S.OK, n_in_front=6, n_correspondences=6, n_inliers=6)
    assert matched.tolist() == [0, 4, 2, 3, -1, 5] + [-1] * 6 and pose.tobytes() == pnp_pose.tobytes()
    # the later one an outlier: the earlier stays
    inl = np.ones(6, bool); inl[4] = False
    assert _finish(S.default_config(1), 12, match, g, inl)[2].tolist() == [0, 1, 2, 3, -1, 5] + [-1] * 6


@pytest.mark.parametrize("mode,n,status", [(1, 3, S.TOO_FEW_CORRESPONDENCES), (1, 4, S.OK), (0, 9, S.TOO_FEW_CORRESPONDENCES), (0, 10, S.OK)])
def test_correspondence_guards(mode, n, status):
    match, g = _hand_frame(n)
    rec, pose, matched, prior, pnp_pose = _finish(S.default_config(mode), 12, match, g, np.ones(n, bool))
    assert rec["status"] == status and rec["n_correspondences"] == n
    if status == S.OK:
        assert pose.tobytes() == pnp_pose.tobytes() and matched[:n].tolist() == list(range(n)) and rec["n_inliers"] == n
    else:
        assert pose.tobytes() == prior.tobytes() and (matched == -1).all() and rec["n_inliers"] == 0


def test_inlier_guard_and_no_model():
    match, g = _hand_frame(12)
    inl = np.zeros(12, bool); inl[:9] = True
    rec, pose, matched, prior, pnp_pose = _finish(S.default_config(0), 12, match, g, inl)
    assert rec["status"] == S.TOO_FEW_INLIERS and rec["n_inliers"] == 9 and pose.tobytes() == prior.tobytes() and matched[:9].tolist() == list(range(9))
    rec, pose, matched, prior, pnp_pose = _finish(S.default_config(1), 12, match, g, inl)          # mode 1 has no inlier guard
    assert rec["status"] == S.OK and pose.tobytes() == pnp_pose.tobytes()
    inl[9] = True
    assert _finish(S.default_config(0), 12, match, g, inl)[0]["status"] == S.OK
    rec, pose, matched, prior, pnp_pose = _finish(S.default_config(1), 12, match, g, inl, pnp_status=S.PNP_NO_MODEL)
    assert rec["status"] == S.NO_MODEL and pose.tobytes() == pnp_pose.tobytes() and matched[:10].tolist() == list(range(10))


@pytest.mark.parametrize("mode", [0, 1])
def test_gpu_scenes_keep_clear_of_every_decision_point(oracle, mode):
    """z, the four cell-range arguments and the mode-0 bounds stay at least 1e-9 away from where a decision flips, so that a
    GPU mismatch is a logic error and not a last-bit one; and the scenes are what their names say."""
    cfg = S.default_config(mode)
    B = G.batches()
    for name, frames in B.items():
        for f in frames:
            assert S.margins(CAM, cfg, f[4], f[2]) >= 1e-9, name
    off = {name: S.search_and_gather(oracle, CAM, cfg, fr) for name, fr in B.items()}
    n_corr = lambda name: np.diff(off[name][0]).tolist()
    assert n_corr("corr_3_4") == [3, 4] and n_corr("corr_9_10") == [9, 10] and n_corr("cand_63_64_65") == [1, 1, 1]
    assert [len(f[0]) for f in B["cand_63_64_65"]] == [63, 64, 65] and [len(f[2]) for f in B["mp_1_4_5"]] == [1, 4, 5]
    assert n_corr("no_features") == [0] and n_corr("middle_without_map_points")[1] == 0 and n_corr("all_behind")[0] == 0
    assert (off["all_behind"][1][0] == S.BEHIND).all() and (off["b2"][1][0] == S.BEHIND).sum() == 7
    assert n_corr("all_outside") == ([0] if mode == 0 else [5])
    g = off["duplicate_inliers"][2][0]
    assert len(set(g["feat_idx"].tolist())) == len(g["feat_idx"]) - 1              # two correspondences share one feature
    assert sorted({len(fr) for fr in B.values()}) == [1, 2, 3]
    for name in ("b1", "b2", "b3"):
        assert min(n_corr(name)) >= 30


def test_new_symbols_and_struct_layouts(pkg, tmp_path):
    """The library exports the tracker's entry points, and orbx_track_config / orbx_track_result are laid out as the ctypes and
    numpy mirrors restate them (40 and 16 bytes)."""
    from orb_slam3_rust_amd.api import _TrackConfig
    L = pkg.load_library()
    for s in ("orbx_default_track_config", "orbx_track_frames", "orbx_track_frames_device"):
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d\\n", '
                   'sizeof(orbx_track_config), offsetof(orbx_track_config, radius), offsetof(orbx_track_config, min_correspondences), '
                   'sizeof(orbx_track_result), offsetof(orbx_track_result, n_inliers), ORBX_TRACK_OK, ORBX_TRACK_NO_MODEL, '
                   'ORBX_TRACK_TOO_FEW_CORRESPONDENCES, ORBX_TRACK_TOO_FEW_INLIERS); return 0; }\n')
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_TrackConfig), _TrackConfig.radius.offset, _TrackConfig.min_correspondences.offset, pkg.TRACK_RESULT.itemsize,
                   pkg.TRACK_RESULT.fields["n_inliers"][1], pkg.TRACK_OK, pkg.TRACK_NO_MODEL, pkg.TRACK_TOO_FEW_CORRESPONDENCES, pkg.TRACK_TOO_FEW_INLIERS]
    assert got[0] == 40 and got[3] == 16
    assert (S.OK, S.NO_MODEL, S.TOO_FEW_CORRESPONDENCES, S.TOO_FEW_INLIERS) == tuple(got[5:])
    for mode, want in ((0, (15.0, 752.0, 480.0, 10, 10)), (1, (15.0, 752.0, 480.0, 4, 0))):
        c = _TrackConfig()
        L.orbx_default_track_config(C.c_int(mode), C.byref(c))
        assert (c.mode, c.radius, c.img_w, c.img_h, c.min_correspondences, c.min_inliers) == (mode,) + want
        d = pkg.TrackConfig.for_mode(mode)
        assert (d.radius, d.img_w, d.img_h, d.min_correspondences, d.min_inliers) == want
        s = S.default_config(mode)
        assert (s["radius"], s["img_w"], s["img_h"], s["min_correspondences"], s["min_inliers"]) == want
