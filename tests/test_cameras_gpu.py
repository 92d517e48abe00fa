"""The matchers and map searches on the GPU at the cameras of tests/camera_cases.py — KITTI-like, short focal length, fx != fy with an
off-centre principal point, a 64 x 64 image, the 63 x 63 and 64 x 64 triangulation grids, 2300 x 2300, 640 x 4095 — against the CPU
oracle and the numpy specifications, by the rules of the files that test the same entry points at EuRoC: matches, indices, distances,
has_point and the f64 points bit-exact; triangulated positions and statuses by tests/test_triangulation_gpu.py's rule (statuses equal
where the spec's margin exceeds 1e-9, positions within 1e-9 relative).  tests/test_cameras_cpu.py checks, without a GPU, that the
scenes reach the regimes the table names and that the oracle equals a second statement at every camera.

The `euroc` rows are the control: the same harness at the camera every other test uses.
"""
import numpy as np
import pytest

import camera_cases as CC
import camera_scenes as CS
import test_tracking_gpu as TG
import test_triangulation_gpu as TRG
import tracking_spec as TSPEC
import triangulation_spec as TRI
from conftest import records_equal
from test_fuse_search import RADIUS_SCALE

pytestmark = pytest.mark.gpu

CASES = CC.CASES
IDS = CC.NAMES
STEREO_SIZES = CS.STEREO_SIZES


@pytest.fixture(scope="module")
def handles(pkg):
    """one handle per camera (stereo_match triangulates with the handle's own camera); no large image workspace: the matchers take keypoints"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = pkg.Handle(pkg.CameraModel(**CC.BY_NAME[name]["camera"]), 1200, device=0, max_w=752, max_h=480, max_batch=1)
        return made[name]
    yield get
    for h in made.values():
        h.close()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kpt(kp):
    import torch
    return torch.from_numpy(np.ascontiguousarray(kp).view(np.float32).reshape(-1, 7).copy()).cuda()


def _same_stereo(a, b):
    (m0, p0, h0), (m1, p1, h1) = a, b
    return records_equal(m0, m1) and np.array_equal(h0, h1) and np.array_equal(p0[h0 == 1], p1[h1 == 1])


# ---- stereo_match ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nL,nR", STEREO_SIZES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stereo_match_parity(handles, oracle, case, nL, nR):
    f = CS.stereo_features(case, nL, nL, nR)
    want = oracle.stereo_match(oracle.Camera(**case["camera"]), *f)
    got = handles(case["name"]).stereo_match(*f)
    assert _same_stereo(want, got)
    if nL >= 1000:
        assert len(want[0]) > 0.2 * min(nL, nR) and len(want[0]) >= CC.floor(case["name"], "stereo") and want[2].sum() > 0.2 * nL


def test_stereo_match_euroc_control(handles, oracle, pkg):
    """the control: this file's handle gives what tests/test_matcher_gpu.py's inputs give there"""
    cam = oracle.Camera(**CC.EUROC)
    for nL, nR, seed in ((2000, 2000, 0), (1200, 1180, 1), (17, 3000, 4)):
        f = pkg.synth.matcher_features(seed, nL, nR, pkg.KEYPOINT)
        assert _same_stereo(oracle.stereo_match(cam, *f), handles("euroc").stereo_match(*f))


@pytest.mark.parametrize("vl", [1000.75, 2047.5, 2048.25, 4090.25])
def test_stereo_vertical_gate_at_high_rows(handles, oracle, pkg, vl):
    """|vl - vr| <= 2 in f32 where an ulp of the row coordinate is 6e-5 (1000) to 4.9e-4 (4090) — 8 to 32 times EuRoC's — and 2048.25 -+ 2
    crosses the binade"""
    case = CC.BY_NAME["tall"]
    f = CS.vertical_edges(vl)
    want = oracle.stereo_match(oracle.Camera(**case["camera"]), *f)
    got = handles("tall").stereo_match(*f)
    assert _same_stereo(want, got)
    assert want[0]["query_idx"].tolist() == [0, 2, 3, 5, 8]            # on the gate and inside it; the float beyond and the rows further out are not


def test_stereo_crowded_rows_at_the_bottom_of_a_tall_image(handles, oracle, pkg):
    case = CC.BY_NAME["tall"]
    f = CS.crowded_tall()
    want = oracle.stereo_match(oracle.Camera(**case["camera"]), *f)
    assert _same_stereo(want, handles("tall").stereo_match(*f)) and len(want[0]) > 50


@pytest.mark.parametrize("name,ul", [("euroc", 600.0), ("kitti", 900.0)])
def test_stereo_horizontal_gate_edges(handles, oracle, pkg, name, ul):
    case = CC.BY_NAME[name]
    cam = oracle.Camera(**case["camera"])
    h = handles(name)
    # nL == nR: lim = ul, max_u = ul - min_disp
    kl, dl, kr, dr, val = CS.horizontal_edges(case, ul, 12, 12, ("min_u", "max_u", "ul"))
    assert val["max_u"] < val["lim"]
    if name == "kitti":
        assert val["min_u"] == 0.0 and kr["x"][0] == 0.0 and kr["x"][1] < 0.0            # ul - max_disp < 0: ur = 0.0 is a candidate
    else:
        assert val["min_u"] > 90.0                                                        # ul > max_disp
    want = oracle.stereo_match(cam, kl, dl, kr, dr)
    assert _same_stereo(want, h.stereo_match(kl, dl, kr, dr))
    assert want[0]["query_idx"].tolist() == [0, 2, 3, 4, 9, 10, 11]                       # on an edge and inside; one float outside is out; ur >= ul is out
    # nR < nL: lim = 0.75 ul < ul - min_disp
    kl, dl, kr, dr, val = CS.horizontal_edges(case, ul, 12, 9, ("lim",))
    assert val["max_u"] == val["lim"] < np.float32(ul) - np.float32(50.0)
    kr["x"][3:] = val["lim"] - np.float32(30.0)
    want = oracle.stereo_match(cam, kl, dl, kr, dr)
    assert _same_stereo(want, h.stereo_match(kl, dl, kr, dr))
    assert want[0]["query_idx"].tolist() == [0, 1, 3, 4, 5, 6, 7, 8]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stereo_disparity_quirk_and_point_formula(handles, oracle, pkg, case):
    """|disparity| < 0.5 keeps the match and gives no point (stereo.rs:205-207) — reachable only where min_disp < 0.5 (square512, tiny);
    a point, where there is one, is fx b / d and (u - cx) z / fx, (v - cy) z / fy of THIS camera, in f64."""
    cam = case["camera"]
    max_d, min_d = (float(x) for x in CS.disparity_bounds(cam))
    ul = 0.75 * case["w"]
    disp = np.array([0.25, 0.49, 0.5, 0.51, 1.0, min_d, 1.5 * min_d + 1.0, 0.5 * min(max_d, ul)])
    n = len(disp)
    kl = np.zeros(n, pkg.KEYPOINT); kr = np.zeros(n, pkg.KEYPOINT)
    kl["x"] = ul; kl["y"] = 3.0 + (case["h"] - 6.0) * np.arange(n) / n
    kr["x"] = (ul - disp).astype(np.float32); kr["y"] = kl["y"]
    d = np.random.default_rng(31).integers(0, 256, (n, 32), dtype=np.uint8)          # one descriptor per pair, some 128 bits from every other
    want = oracle.stereo_match(oracle.Camera(**cam), kl, d, kr, d)
    got = handles(case["name"]).stereo_match(kl, d, kr, d)
    assert _same_stereo(want, got)
    m, pts, has = got
    assert len(m) >= 2 and has.sum() >= 2
    no_point = [int(q) for q in m["query_idx"] if not has[q]]
    assert all(abs(float(kl["x"][q]) - float(kr["x"][q])) < 0.5 for q in no_point)
    if min_d < 0.5:
        assert len(no_point) >= 1
    else:
        assert no_point == []
    for q in np.flatnonzero(has):
        dd = float(kl["x"][q]) - float(kr["x"][q])
        z = cam["fx"] * cam["baseline"] / dd
        assert pts[q].tolist() == [(float(kl["x"][q]) - cam["cx"]) * z / cam["fx"], (float(kl["y"][q]) - cam["cy"]) * z / cam["fy"], z]


def test_stereo_match_three_forms_at_every_camera(pkg, tmp_path):
    """stereo_match_lds_kernel<true> (ORBX_SM_LDS=1), the three-launch form with stereo_match_lds_kernel<false> in the middle (2) and
    stereo_match_kernel (0) give the same bytes at every camera.  Three child processes, one after the other (the switch is read at
    the first stereo-match call); each loops over the cases with one handle per camera, closed before the next."""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import torch
        import orb_slam3_rust_amd as P
        import camera_cases as CC, camera_scenes as CS
        out = {}
        for case in CC.CASES:
            h = P.Handle(P.CameraModel(**case["camera"]), 1200, device=0, max_w=752, max_h=480, max_batch=1)
            sets = [CS.stereo_features(case, nL, nL, nR) for nL, nR in CS.STEREO_SIZES]
            if case["name"] == "tall":
                sets += [CS.crowded_tall(), CS.vertical_edges(4090.25)]
            for i, f in enumerate(sets):
                m, pts, has = h.stereo_match(*f)
                k = "%%s_%%d_" %% (case["name"], i)
                out[k + "m"] = np.frombuffer(m.tobytes(), np.uint8); out[k + "p"] = pts[has == 1]; out[k + "h"] = has
            h.close()
        np.savez(sys.argv[1], **out)
    """ % (root, os.path.join(root, "tests")))
    res = {}
    for mode in ("1", "2", "0"):
        path = str(tmp_path / ("sm%s.npz" % mode))
        subprocess.run([sys.executable, "-c", script, path], check=True, env=dict(os.environ, ORBX_SM_LDS=mode), timeout=600)
        res[mode] = np.load(path)
    assert sorted(res["1"].files) == sorted(res["0"].files) == sorted(res["2"].files) and len(res["1"].files) == 3 * (4 * len(CASES) + 2)
    for k in res["1"].files:
        assert np.array_equal(res["1"][k], res["0"][k]) and np.array_equal(res["1"][k], res["2"][k]), k
    assert all(int(res["1"]["%s_3_h" % c["name"]].sum()) > 400 for c in CASES)


# ---- guided_match ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_guided_match_at_every_image_size(handles, oracle, pkg, case, mode):
    """winv = 64 / img_w, hinv = 48 / img_h; keypoints at x = img_w, y = img_h, beyond and negative (saturating cell casts); queries
    outside the image (the wrap-around quirk) and with x -+ radius, y -+ radius on a cell boundary and one f64 step either side; radius
    15 and 0.  The host form and the device-resident keyframe's."""
    h = handles(case["name"])
    w, hh = float(case["w"]), float(case["h"])
    for radius in (15.0, 0.0):
        kp, desc, uv, qd = CS.guided_features(case, 4, radius=radius)
        i0, d0 = oracle.guided_match(kp, desc, w, hh, uv, qd, radius, mode)
        i1, d1 = h.guided_match(kp, desc, w, hh, uv, qd, radius, mode)
        assert np.array_equal(i0, i1) and np.array_equal(d0, d1), radius
        kf = pkg.KeyFrame(h, _kpt(kp), _t(desc), len(kp))
        try:
            i2, d2 = kf.guided_match(w, hh, uv, qd, radius, mode)
        finally:
            kf.close()
        assert np.array_equal(i0, i2) and np.array_equal(d0, d2), radius
        if radius > 0:
            assert (i0 >= 0).sum() > 300
            assert np.isin(i0, np.arange(8)).sum() >= 1                  # a keypoint on or beyond the edge is somebody's match


def test_guided_match_euroc_control(handles, oracle, pkg):
    kp, d, kq, dq = pkg.synth.matcher_features(200, 2000, 1500, pkg.KEYPOINT)
    rng = np.random.default_rng(0)
    uv = np.stack([kq["x"].astype(np.float64) + rng.uniform(-20, 140, len(kq)), kq["y"].astype(np.float64) + rng.uniform(-3, 3, len(kq))], 1)
    uv[::17] = rng.uniform(-200, 1000, (len(uv[::17]), 2))
    for mode in (0, 1):
        i0, d0 = oracle.guided_match(kp, d, 752.0, 480.0, uv, dq, 15.0, mode)
        i1, d1 = handles("euroc").guided_match(kp, d, 752.0, 480.0, uv, dq, 15.0, mode)
        assert np.array_equal(i0, i1) and np.array_equal(d0, d1) and (i0 >= 0).sum() > 50


# ---- track_frames ------------------------------------------------------------------------------------------------------------

def _run_device(h, pkg, cam, frames, cfg):
    import torch
    o = h.track_frames_device(cam, cfg=cfg, **TG._device_inputs(frames))
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in o.items()}
    r["pnp_results"] = r["pnp_results"].view(pkg.PNP_RESULT).reshape(-1)
    r["results"] = r["results"].view(pkg.TRACK_RESULT).reshape(-1)
    return r


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_track_frames_equals_spec_and_pnp_composition(handles, oracle, pkg, case, mode):
    """tests/test_tracking_gpu.py's comparison — the search, the gather and the records equal tracking_spec; pose, inliers, errors and
    PnP's records equal solve_pnp_ransac_batch_device on the spec's gathered arrays — with the grid from this case's img_w, img_h and the
    bounds from its 2cx, 2cy; the host form gives the device form's bytes."""
    h = handles(case["name"])
    cam_d = case["camera"]
    cam = pkg.CameraModel(**cam_d)
    frames = CS.track_frames(case)
    w, hh = float(case["w"]), float(case["h"])
    cfg = TSPEC.default_config(mode, img_w=w, img_h=hh)
    gcfg = pkg.TrackConfig.for_mode(mode, img_w=w, img_h=hh)
    off, ms, gs = TSPEC.search_and_gather(oracle, cam_d, cfg, frames)
    r = _run_device(h, pkg, cam, frames, gcfg)
    N = int(off[-1])
    assert N >= 90 and r["offsets"].tolist() == off.tolist()
    cat = lambda k: np.concatenate([g[k] for g in gs])
    assert r["mp_idx"][:N].tolist() == cat("mp_idx").tolist() and r["feat_idx"][:N].tolist() == cat("feat_idx").tolist()
    assert r["points3d"][:N].tobytes() == cat("points3d").tobytes() and r["points2d"][:N].tobytes() == cat("points2d").tobytes()
    poses, inl, err, res = TG._pnp_reference(h, cam, off, gs, frames, max(len(f[2]) for f in frames))
    assert r["inlier"][:N].tobytes() == inl.tobytes() and r["err"][:N].tobytes() == err.tobytes()
    assert r["pnp_results"].tobytes() == res.tobytes()
    pres = res.view(pkg.PNP_RESULT).reshape(-1)
    host = h.track_frames(cam, frames, gcfg)
    for b, f in enumerate(frames):
        s = slice(int(off[b]), int(off[b + 1]))
        rec, pose, matched = TSPEC.finish(cfg, len(f[0]), ms[b], gs[b], f[5], poses[b], inl[s], int(pres[b]["status"]), int(pres[b]["n_inliers"]))
        got = r["results"][b]
        assert {k: int(got[k]) for k in pkg.TRACK_RESULT.names} == rec, b
        assert r["poses"][b].tobytes() == pose.tobytes(), b
        assert r["matched"][b, :len(f[0])].tolist() == matched.tolist() and (r["matched"][b, len(f[0]):] == -1).all(), b
        assert TG._frame_bytes_host(pkg, host[b]) == TG._frame_bytes_device(r, b, len(f[0])), (b, "host form")


# ---- search_for_triangulation ------------------------------------------------------------------------------------------------

def _search_args(s):
    return (s["kp1"], s["desc1"], s["mp1"], s["stereo1"], s["kp2"], s["desc2"], s["mp2"], s["pose1_wc"], s["pose2_wc"])


def _oracle_search(oracle, s):
    return oracle.search_for_triangulation(oracle.Camera(**s["camera"]), *_search_args(s), 50)


def _prime(h, oracle, pkg):
    """Leave a stale value where the 64 x 64 grid's end sentinel belongs.  The grid's cell_start occupies the first 4100 ints of the
    handle's matcher workspace and no grid below 64 x 64 writes int 4096.  A EuRoC search of the same size makes the workspace exist
    (it only ever grows); a guided_match of 1500 keypoints then lays its sorted index list over ints 3073 .. 4572, so int 4096 holds
    a keypoint index below 1500 — less than any cell_start of the last grid row of the scenes here, whose keyframe 2 holds over 3000
    features: a search that read it instead of its own sentinel would find grid row 63 empty.  Both calls are valid and checked."""
    s = CS.two_view(CC.BY_NAME["euroc"])
    assert np.array_equal(h.search_for_triangulation(pkg.CameraModel(**s["camera"]), *_search_args(s), 50), _oracle_search(oracle, s))
    kp, desc, uv, qd = CS.guided_features(CC.BY_NAME["euroc"], 4)
    i0, d0 = oracle.guided_match(kp, desc, 752.0, 480.0, uv, qd, 15.0, 1)
    i1, d1 = h.guided_match(kp, desc, 752.0, 480.0, uv, qd, 15.0, 1)
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1) and len(kp) == 1500


def _keyframes(pkg, h, s):
    k1 = pkg.KeyFrame(h, _kpt(s["kp1"]), _t(s["desc1"]), len(s["kp1"]), _t(s["pts1"]), _t(s["has1"]), keyframe_id=1, pose_wc=s["pose1_wc"])
    k2 = pkg.KeyFrame(h, _kpt(s["kp2"]), _t(s["desc2"]), len(s["kp2"]), _t(s["pts2"]), _t(s["has2"]), keyframe_id=2, pose_wc=s["pose2_wc"])
    k1.set_map_points([7 if m else None for m in s["mp1"]]); k2.set_map_points([7 if m else None for m in s["mp2"]])
    return k1, k2


def _all_forms(h, oracle, pkg, s):
    """{form: pairs} of the plain, the device-resident and the keyframe form"""
    cam = pkg.CameraModel(**s["camera"])
    out = {"plain": h.search_for_triangulation(cam, *_search_args(s), 50)}
    pairs, cnt = h.search_for_triangulation_device(cam, _kpt(s["kp1"]), _t(s["desc1"]), _t(s["mp1"]), _t(s["stereo1"]), _kpt(s["kp2"]), _t(s["desc2"]),
                                                   _t(s["mp2"]), s["pose1_wc"], s["pose2_wc"])
    h.synchronize()
    out["device"] = pairs[:int(cnt.item())].cpu().numpy()
    k1, k2 = _keyframes(pkg, h, s)
    try:
        out["keyframe"] = k1.search_for_triangulation(cam, k2, 50)
    finally:
        k1.close(); k2.close()
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_triangulation_search_at_every_camera(handles, oracle, pkg, case):
    """The plain, the device-resident, the keyframe and the FeatureVector form against the oracle, bit-exact.  At the two cameras with
    a 64 x 64 grid the workspace is primed first (see _prime): on a build whose grid kernel does not write cell_start[4096] the pairs
    whose partner lies in grid row 63 are lost."""
    h = handles(case["name"])
    s = CS.two_view(case)
    want = _oracle_search(oracle, s)
    if case["grid"] == (64, 64):
        _prime(h, oracle, pkg)
    for form, got in _all_forms(h, oracle, pkg, s).items():
        missing = len(set(map(tuple, want.tolist())) - set(map(tuple, got.tolist())))
        print("%s %s: %d pairs, oracle %d, %d of the oracle's missing, %d of them corner pairs" % (
            case["name"], form, len(got), len(want), missing, len(CS.corner_pairs(s, want)) - len(CS.corner_pairs(s, got))))
        assert got.dtype == np.int32 and np.array_equal(got, want), form
    assert len(want) >= CC.floor(case["name"], "pairs")
    n = CS.with_nodes(s)
    cam = pkg.CameraModel(**s["camera"])
    a = (n["kp1"], n["desc1"], n["mp1"], n["stereo1"], n["node1"], n["kp2"], n["desc2"], n["mp2"], n["node2"], n["pose1_wc"], n["pose2_wc"], 50)
    wb = oracle.search_for_triangulation_bow(oracle.Camera(**s["camera"]), *a)
    assert np.array_equal(h.search_for_triangulation_bow(cam, *a), wb) and len(wb) >= 50


def test_grid63_against_grid64_isolates_the_end_sentinel(handles, oracle, pkg):
    """Two cameras that differ in the principal point by half a pixel, on ONE primed handle: 63 x 63 cells end at cell_start[3969],
    which every build writes; 64 x 64 cells end at cell_start[4096], past the 1024 x 4 slots of tri_grid_build_body's scan."""
    h = handles("grid64")
    _prime(h, oracle, pkg)
    for name in ("grid63", "grid64", "grid63"):
        s = CS.two_view(CC.BY_NAME[name], seed=8)
        want = _oracle_search(oracle, s)
        got = h.search_for_triangulation(pkg.CameraModel(**s["camera"]), *_search_args(s), 50)
        print("%s: %d pairs, oracle %d" % (name, len(got), len(want)))
        assert np.array_equal(got, want), name
        if name == "grid64":
            assert len(CS.corner_pairs(s, want)) >= 20


def test_triangulation_search_euroc_control(handles, oracle, pkg):
    for seed, n, dup in ((1, 300, 0.0), (3, 2500, 0.6)):
        s = pkg.synth.two_view_features(seed, n, pkg.KEYPOINT, n_distractors=300, dup=dup)
        assert np.array_equal(handles("euroc").search_for_triangulation(pkg.CameraModel(**s["camera"]), *_search_args(s), 50), _oracle_search(oracle, s))


def test_camera_without_grid_cells_is_refused(handles, oracle, pkg):
    """u32(2cx) = 0: no grid column.  Every grid form raises ORBX_ERR_INVALID; the handle goes on working."""
    h = handles("euroc")
    s = CS.two_view(CC.BY_NAME["euroc"], seed=9, n_points=600)
    bad = pkg.CameraModel(**CC.REFUSED["camera"])
    with pytest.raises(pkg.OrbxError) as e:
        h.search_for_triangulation(bad, *_search_args(s), 50)
    assert e.value.code == -1
    with pytest.raises(pkg.OrbxError):
        h.search_for_triangulation_device(bad, _kpt(s["kp1"]), _t(s["desc1"]), _t(s["mp1"]), _t(s["stereo1"]), _kpt(s["kp2"]), _t(s["desc2"]), _t(s["mp2"]),
                                          s["pose1_wc"], s["pose2_wc"])
    h.synchronize()
    k1, k2 = _keyframes(pkg, h, s)
    try:
        with pytest.raises(pkg.OrbxError):
            k1.search_for_triangulation(bad, k2, 50)
        assert np.array_equal(k1.search_for_triangulation(pkg.CameraModel(**s["camera"]), k2, 50), _oracle_search(oracle, s))
    finally:
        k1.close(); k2.close()
    want = _oracle_search(oracle, s)
    assert np.array_equal(h.search_for_triangulation(pkg.CameraModel(**s["camera"]), *_search_args(s), 50), want) and len(want) > 50


# ---- fuse_search -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fuse_search_at_every_camera(handles, oracle, pkg, case):
    """Host, device-resident and keyframe form against the oracle.  Six map points project exactly onto the bounds — u = 0.0, 2cx, the
    f64 below 2cx, the same in v (tests/test_cameras_cpu.py checks the construction): what the oracle says about them decides."""
    h = handles(case["name"])
    s = CS.fuse_scene(pkg, case, 7)
    cam = pkg.CameraModel(**case["camera"])
    a = (s["positions"], s["mp_desc"], s["kf_poses_wc"], s["kf_feat_offset"], s["kps"], s["descs"], RADIUS_SCALE, 50)
    i0, d0 = oracle.fuse_search(oracle.Camera(**case["camera"]), *a)
    i1, d1 = h.fuse_search(cam, *a)
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1)
    idx, dist = h.fuse_search_device(cam, _t(s["positions"]), _t(s["mp_desc"]), s["kf_poses_wc"], _t(s["kf_feat_offset"]), _kpt(s["kps"]), _t(s["descs"]),
                                     RADIUS_SCALE)
    h.synchronize()
    assert np.array_equal(idx.cpu().numpy(), i0) and np.array_equal(dist.cpu().numpy().view(np.uint32), d0)
    off = s["kf_feat_offset"]
    kfs = [pkg.KeyFrame(h, _kpt(s["kps"][off[t]:off[t + 1]]), _t(s["descs"][off[t]:off[t + 1]]), int(off[t + 1] - off[t]), keyframe_id=t,
                        pose_wc=s["kf_poses_wc"][t]) for t in range(len(off) - 1)]
    try:
        i2, d2 = pkg.KeyFrame.fuse_search(h, cam, s["positions"], s["mp_desc"], kfs, RADIUS_SCALE, 50)
    finally:
        for k in kfs:
            k.close()
    assert np.array_equal(i2, i0) and np.array_equal(d2, d0)
    assert (i0 >= 0).sum() > 100
    edge = i0[s["edge_rows"], 0]
    assert (edge >= 0).tolist() == [True, False, True] * 2


# ---- triangulate_pairs, triangulate_from_neighbors -----------------------------------------------------------------------------

_expected = {}


def _pair_expected(case):
    if case["name"] not in _expected:
        s, pairs = CS.pair_case(case)
        _expected[case["name"]] = [TRI.triangulate_pair(s["camera"], TRI.default_config(), 0, s["kp1"], s["pts1"], s["has1"], s["pose1_wc"], s["kp2"],
                                                        s["pts2"], s["has2"], s["pose2_wc"], int(a), int(b)) for a, b in pairs]
    return _expected[case["name"]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_triangulate_pairs_at_every_camera(handles, pkg, case):
    """Back-projection with cx, cy, fx, fy, the stereo-parallax branch cos(2 atan(b / 2 / z)) with this camera's baseline, the
    reprojection checks: host and device form against triangulation_spec by tests/test_triangulation_gpu.py's rule."""
    h = handles(case["name"])
    s, pairs = CS.pair_case(case)
    cam = pkg.CameraModel(**s["camera"])
    expected = _pair_expected(case)
    pts, st = h.triangulate_pairs(cam, s["kp1"], s["pts1"], s["has1"], s["pose1_wc"], s["kp2"], s["pts2"], s["has2"], s["pose2_wc"], pairs)
    TRG._check_against_spec(st, pts, expected, "%s, host form" % case["name"])
    dpts, dst = h.triangulate_pairs_device(cam, _kpt(s["kp1"]), _t(s["pts1"]), _t(s["has1"]), s["pose1_wc"], _kpt(s["kp2"]), _t(s["pts2"]), _t(s["has2"]),
                                           s["pose2_wc"], _t(pairs.reshape(-1, 2)))
    h.synchronize()
    assert np.array_equal(dpts.cpu().numpy(), pts) and np.array_equal(dst.cpu().numpy().view(np.uint16), st)
    if case["name"] == "kitti":
        ran = ~np.isin(st & 0xFF, [TRI.SKIPPED, TRI.DLT_DEGENERATE, TRI.BAD_INDEX])
        assert (ran & ((st >> 8) != TRI.DLT)).sum() >= 20                       # the stereo branches, as the CPU test counts them in the spec


@pytest.mark.parametrize("name", ["kitti", "big"])
def test_triangulate_from_neighbors_three_neighbours(handles, oracle, pkg, name):
    """The fused call with three neighbours: the spec by the existing rule, and byte for byte the per-neighbour sequence
    (KeyFrame.search_for_triangulation + triangulate_pairs).  At `big` (64 x 64 grid) a EuRoC-sized fused call runs first on the same
    handle, so that the call's workspace is not fresh memory."""
    h = handles(name)
    case = CC.BY_NAME[name]
    sc = CS.fused_scene(case)
    cam = pkg.CameraModel(**sc["camera"])
    made = []

    def device(scene):
        ks = [TRG._keyframe(pkg, h, scene["current"], 1)] + [TRG._keyframe(pkg, h, nb, 10 + t) for t, nb in enumerate(scene["neighbours"])]
        made.extend(ks)
        return ks[0], ks[1:]
    try:
        if case["grid"] == (64, 64):
            e = CS.fused_scene(CC.BY_NAME["euroc"])
            ecur, enbs = device(e)
            ewant = TRI.triangulate_from_neighbors(oracle, e["camera"], TRI.default_config(), 0, e["current"], e["neighbours"])
            egot = ecur.triangulate_from_neighbors(pkg.CameraModel(**e["camera"]), enbs)
            assert egot[4].per_neighbour[:, :2].tolist() == ewant[1][:, :2].tolist()
        cur, nbs = device(sc)
        created, stats, res, ev = TRI.triangulate_from_neighbors(oracle, sc["camera"], TRI.default_config(), 0, sc["current"], sc["neighbours"])
        nb, i1, i2, pts, got = cur.triangulate_from_neighbors(cam, nbs)
        print("%s: per neighbour %s, spec %s" % (name, got.per_neighbour.tolist(), stats.tolist()))
        assert got.per_neighbour[:, :2].tolist() == stats[:, :2].tolist()                 # searched, matches_found: the searches are bit-exact
        near = {(e[0], e[1], e[2]) for e in ev if e[6] <= TRG.MARGIN}
        want = {(t, a, b): p for t, a, b, p in created if (t, a, b) not in near}
        have = {(int(t), int(a), int(b)): p for t, a, b, p in zip(nb, i1, i2, pts) if (int(t), int(a), int(b)) not in near}
        assert list(have) == list(want)
        worst = max([float(np.linalg.norm(have[k] - want[k]) / np.linalg.norm(want[k])) for k in want] + [0.0])
        print("%s: %d new points, largest position error %.3e relative" % (name, len(want), worst))
        assert worst <= TRG.POS_TOL and len(want) > 60
        if not near:
            assert got.per_neighbour.tolist() == stats.tolist()
        # the per-neighbour sequence
        c = sc["current"]
        w_nb, w_pairs, w_pts, w_stats = [], [], [], []
        for t, (kf, nbd) in enumerate(zip(nbs, sc["neighbours"])):
            pairs = cur.search_for_triangulation(cam, kf, 50)
            p, st = h.triangulate_pairs(cam, c["kp"], c["pts"], c["has"], c["pose"], nbd["kp"], nbd["pts"], nbd["has"], nbd["pose"], pairs)
            code = st & 0xFF
            ok = code == pkg.TRI_CREATED
            w_nb.append(np.full(ok.sum(), t, np.int32)); w_pairs.append(pairs[ok]); w_pts.append(p[ok])
            w_stats.append([1, len(pairs), int(np.isin(code, [pkg.TRI_SKIPPED, pkg.TRI_DLT_DEGENERATE], invert=True).sum()), int(ok.sum())])
        wp = np.concatenate(w_pairs)
        assert nb.tobytes() == np.concatenate(w_nb).tobytes()
        assert i1.tobytes() == np.ascontiguousarray(wp[:, 0]).tobytes() and i2.tobytes() == np.ascontiguousarray(wp[:, 1]).tobytes()
        assert pts.tobytes() == np.concatenate(w_pts).tobytes() and got.per_neighbour.tolist() == w_stats
    finally:
        for k in made:
            k.close()
