"""The kernels with an ordered append, a block sum, a scan of counts or a counter scan (csrc/block_dev.hpp, and lv_resolve_kernel's
own) at the sizes where such code goes wrong: round boundaries, a second counter that moves apart from the first, a block index
past the thread count, a list carried over a chunk and a neighbour, a scan's second and third round, and the counters of a
counting sort at a thread edge, a wave edge and the end sentinel.  Each case is held to its existing specification with that
module's own tolerances; tests/test_block_primitives_cpu.py checks that the scenes are what they are for."""
import numpy as np
import pytest

import ba_collect_spec as BS
import block_primitive_scenes as B
import loop_verify_spec as LS
import track_reference_spec as RS
import tracking_scenes as G
import tracking_spec as TS
import triangulation_spec as XS
from conftest import assert_ba_close, records_equal
from test_ba_collect_gpu import _BaWorld, _assert_spec
from test_ba_collect_gpu import _collect as ba_collect
from test_loop_verify_gpu import _cfg as loop_cfg
from test_loop_verify_gpu import assert_pair_matches_spec
from test_map_store_gpu import _World, _frame_tensors
from test_map_store_gpu import _np as track_np
from test_track_reference_gpu import _kf_starts
from test_track_reference_gpu import _pnp_reference as ref_pnp_reference
from test_track_reference_gpu import _run_device as ref_run_device
from test_tracking_gpu import _pnp_reference as track_pnp_reference
from test_tracking_gpu import _run_device as track_run_device
from test_triangulation_gpu import MARGIN, POS_TOL
from test_triangulation_gpu import _keyframe as tri_keyframe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.CameraModel(**G.CAMERA)


# ---- track_frames_device, mode 1 (track_gather_kernel) ---------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["track_rounds", "track_many", "track_four_cells", "track_one_cell"])
def test_track_frames_gather_at_round_and_block_boundaries(gpu_handle, pkg, oracle, cam, scene):
    frames = getattr(B, scene)()
    cfg = TS.default_config(1)
    off, ms, gs = TS.search_and_gather(oracle, G.CAMERA, cfg, frames)
    r = track_run_device(gpu_handle, pkg, cam, frames, 1)
    N = int(off[-1])
    assert r["offsets"].tolist() == off.tolist()
    cat = lambda k: np.concatenate([g[k] for g in gs])
    assert r["mp_idx"][:N].tolist() == cat("mp_idx").tolist() and r["feat_idx"][:N].tolist() == cat("feat_idx").tolist()
    assert r["points3d"][:N].tobytes() == cat("points3d").tobytes() and r["points2d"][:N].tobytes() == cat("points2d").tobytes()
    poses, inl, err, res = track_pnp_reference(gpu_handle, cam, off, gs, frames, max(len(f[2]) for f in frames))
    assert r["inlier"][:N].tobytes() == inl.tobytes() and r["err"][:N].tobytes() == err.tobytes() and r["pnp_results"].tobytes() == res.tobytes()
    pres = res.view(pkg.PNP_RESULT).reshape(-1)
    for b, f in enumerate(frames):
        s = slice(int(off[b]), int(off[b + 1]))
        rec, pose, matched = TS.finish(cfg, len(f[0]), ms[b], gs[b], f[5], poses[b], inl[s], int(pres[b]["status"]), int(pres[b]["n_inliers"]))
        assert {k: int(r["results"][b][k]) for k in pkg.TRACK_RESULT.names} == rec, b
        assert r["poses"][b].tobytes() == pose.tobytes() and r["matched"][b, :len(f[0])].tolist() == matched.tolist(), b


# ---- track_reference_device (tref_resolve_kernel, tref_gather_kernel) ------------------------------------------------------
@pytest.mark.parametrize("live", ["edges", "all", "none"])
def test_track_reference_two_counters_at_round_boundaries(gpu_handle, pkg, oracle, cam, live):
    frames = B.reference_rounds(live)
    off, ms, gs = RS.match_and_gather(oracle, frames)
    r = ref_run_device(gpu_handle, pkg, cam, frames)
    N = int(off[-1])
    assert r["offsets"].tolist() == off.tolist()
    for b, k0 in enumerate(_kf_starts(frames)):
        assert int(r["results"][b]["n_matches"]) == len(ms[b]) and int(r["results"][b]["n_correspondences"]) == len(gs[b]["kf_idx"]), b
        assert r["matches"][k0:k0 + len(ms[b])].tobytes() == ms[b].tobytes(), b
    cat = lambda k: np.concatenate([g[k] for g in gs])
    assert r["kf_idx"][:N].tolist() == cat("kf_idx").tolist() and r["feat_idx"][:N].tolist() == cat("feat_idx").tolist()
    assert r["points3d"][:N].tobytes() == cat("points3d").tobytes() and r["points2d"][:N].tobytes() == cat("points2d").tobytes()
    poses, inl, err, res = ref_pnp_reference(gpu_handle, cam, off, gs, frames, max(len(f[2]) for f in frames))
    assert r["inlier"][:N].tobytes() == inl.tobytes() and r["err"][:N].tobytes() == err.tobytes() and r["pnp_results"].tobytes() == res.tobytes()
    pres = res.view(pkg.PNP_RESULT).reshape(-1)
    for b, f in enumerate(frames):
        rec, pose = RS.finish(RS.MIN_CORRESPONDENCES, len(ms[b]), gs[b], f[5], poses[b], int(pres[b]["status"]), int(pres[b]["n_inliers"]))
        assert {k: int(r["results"][b][k]) for k in pkg.TRACK_REF_RESULT.names} == rec and r["poses"][b].tobytes() == pose.tobytes(), b


# ---- verify_loop_candidates, brute-force matcher (lv_resolve_kernel) --------------------------------------------------------
@pytest.mark.parametrize("cfg", ["LOOP_CFG", "LOOP_CFG_SOME"])
@pytest.mark.parametrize("live", ["all", "edges"])
def test_loop_verify_two_counters_at_round_boundaries(gpu_handle, pkg, cam, live, cfg):
    pairs = B.loop_rounds(live)
    c = getattr(B, cfg)
    res = gpu_handle.verify_loop_candidates(cam, pairs, loop_cfg(pkg, c))
    for n, (cur, loop), r in zip(B.SIZES, pairs, res):
        assert_pair_matches_spec(r, LS.verify_pair(G.CAMERA, cur, loop, c), (live, cfg, n))


# ---- triangulate_from_neighbors (tri_compact_kernel) ------------------------------------------------------------------------
def test_triangulate_list_over_two_rounds_and_the_next_neighbour(gpu_handle, pkg, oracle):
    sc = B.tri_scene()
    tcam = pkg.CameraModel(**sc["camera"])
    created, stats, res, ev = B.tri_expected(oracle)
    cur = tri_keyframe(pkg, gpu_handle, sc["current"], 1)
    nbs = [tri_keyframe(pkg, gpu_handle, k, 10 + t) for t, k in enumerate(sc["neighbours"])]
    try:
        nb, i1, i2, pts, got = cur.triangulate_from_neighbors(tcam, nbs)
    finally:
        gpu_handle.synchronize()
        cur.close()
        for k in nbs:
            k.close()
    assert got.per_neighbour[:, :2].tolist() == stats[:, :2].tolist()                     # searched, matches_found: the searches are bit-exact
    near = {(e[0], e[1], e[2]) for e in ev if e[6] <= MARGIN}
    want = {(t, a, b): p for t, a, b, p in created if (t, a, b) not in near}
    have = {(int(t), int(a), int(b)): p for t, a, b, p in zip(nb, i1, i2, pts) if (int(t), int(a), int(b)) not in near}
    assert list(have) == list(want)                                                       # same points, in the reference's creation order
    worst = max([float(np.linalg.norm(have[k] - want[k]) / np.linalg.norm(want[k])) for k in want] + [0.0])
    print("%d new points, %d near a gate, largest position error %.3e relative" % (len(want), len(near), worst))
    assert worst <= POS_TOL
    near_of = np.bincount([k[0] for k in near], minlength=len(nbs))                       # (a near-threshold pair may fall on either side of its gate)
    for t in range(len(nbs)):
        assert np.abs(got.per_neighbour[t, 2:] - stats[t, 2:]).max() <= near_of[t], t
    assert got.num_new_points == len(nb) and abs(got.num_new_points - res["num_new_points"]) <= len(near)
    assert XS.CREATED == 0 and len(want) > B.TRI_CHUNK // 2


# ---- map_track_local_device (cov_seg_kernel: the segments' bases over two and three rounds) ----------------------------------
@pytest.mark.parametrize("n_kfs,n_best,refs", B.COV_SEG_CASES)
def test_local_map_selection_over_more_segments_than_one_round(gpu_handle, pkg, cam, n_kfs, n_best, refs):
    tables, counts, live = B.tiny_world(n_kfs)
    rng = np.random.default_rng(3)
    w = _World(gpu_handle, pkg, rng.uniform(-5.0, 5.0, (B.TINY_CAPACITY, 3)), rng.integers(0, 256, (B.TINY_CAPACITY, 32), dtype=np.uint8), live,
               capacity=B.TINY_CAPACITY)
    try:
        for t, n in zip(tables, counts):
            w.keyframe(t, n=n)
        off, slots, local_kf, _ = B.cov_seg_expected(n_kfs, n_best, refs)
        r = track_np(pkg, gpu_handle.map_track_local_device(cam, w.mp, w.kfs, refs, n_best, cfg=pkg.TrackConfig.for_mode(1), **_frame_tensors([B.tiny_frame()] * len(refs))))
        assert r["list_offsets"].dtype == off.dtype and r["list_offsets"].tobytes() == off.tobytes()
        assert r["list_slot"][:len(slots)].tobytes() == slots.tobytes() and r["local_kf"].dtype == local_kf.dtype and r["local_kf"].tobytes() == local_kf.tobytes()
    finally:
        w.close()


# ---- map_collect_ba_window_device (bac_order_kernel: the observers' starts over two and three rounds) ------------------------
@pytest.mark.parametrize("n_obs,max_cov", B.BA_ORDER_CASES)
def test_ba_window_with_more_observers_than_one_round(gpu_handle, pkg, n_obs, max_cov):
    tables, xy, live = B.ba_order_world(n_obs)
    rng = np.random.default_rng(4)
    pos = rng.uniform(-5.0, 5.0, (B.TINY_CAPACITY, 3))
    w = _BaWorld(gpu_handle, pkg, pos, rng.integers(0, 256, (B.TINY_CAPACITY, 32), dtype=np.uint8), live, capacity=B.TINY_CAPACITY)
    try:
        for t, p in zip(tables, xy):
            w.keyframe(t, p)
        want = BS.collect(tables, xy, live, 0, max_cov)
        K, F = int(want["counts"][0]), int(want["counts"][1])
        assert K + F == n_obs and (max_cov < B.ROUND or K + 1 > B.ROUND)         # the scan's rounds, and local_kf's where max_covisible asks for them
        _assert_spec(ba_collect(gpu_handle, pkg, w.mp, w.kfs, 0, max_cov), want, pos)
    finally:
        w.close()


# ---- ba_solve_visual (ba_prep_scan_kernel, ba_kflist_kernel: 1024 points per round) ------------------------------------------
@pytest.mark.parametrize("M", [63, 64, 65, 1023, 1024, 1025, 2049])
def test_ba_point_counts_around_one_and_two_scan_rounds(gpu_handle, oracle, pkg, M):
    """a wave's edge, the block's edge and the third round of the two scans.  tests/test_ba_gpu.py's bar against the structured oracle; and the bits do not move under a regrouping of the observations that
    keeps every point's own order (tests/test_ba_covis_gpu.py) — which holds only if pt_start and the keyframe lists are right"""
    w = pkg.synth.ba_window(810, 4, M, pkg.BA_OBS)
    assert len(w["points"]) == M and w["obs"]["mp_idx"].max() >= M - 2         # (some points are seen by nobody: counts of zero, at 1025 the last one's)
    cam = pkg.CameraModel(**w["camera"])
    solve = lambda obs: gpu_handle.ba_solve_visual(cam, pkg.LocalBAConfigLM(), w["poses_cw"], w["fixed_cw"], w["points"], obs)
    g = solve(w["obs"])
    keep = dict(g, poses_wc=np.array(g["poses_wc"], copy=True), points=np.array(g["points"], copy=True))
    o = oracle.ba_solve_schur(oracle.Camera(**w["camera"]), oracle.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    assert g["iterations"] == o["iterations"] and abs(g["initial_error"] - o["initial_error"]) < 1e-12 * o["initial_error"]
    assert abs(g["final_error"] - o["final_error"]) < 1e-8 * o["final_error"] and g["final_error"] < 0.6 * g["initial_error"]
    assert_ba_close(g, o, 1e-6)
    label = np.random.default_rng(M).permutation(M)
    by_label = w["obs"][np.argsort(label[w["obs"]["mp_idx"]], kind="stable")]
    assert not np.array_equal(by_label, w["obs"])
    r = solve(by_label)
    assert r["iterations"] == keep["iterations"] and r["final_error"] == keep["final_error"]
    assert np.asarray(r["poses_wc"]).tobytes() == keep["poses_wc"].tobytes() and np.asarray(r["points"]).tobytes() == keep["points"].tobytes()


# ---- the four counting sorts: keypoints in the counters at a thread edge, a wave edge and the end sentinel only, and in one -----
def _same_stereo(a, b):
    (m0, p0, h0), (m1, p1, h1) = a, b
    return records_equal(m0, m1) and np.array_equal(h0, h1) and np.array_equal(p0[h0 == 1], p1[h1 == 1])


@pytest.mark.parametrize("rows", [B.STEREO_ROWS, B.STEREO_ONE], ids=["edges", "one"])
def test_stereo_match_with_the_right_keypoints_in_edge_buckets(gpu_handle, oracle, pkg, rows):
    """the suite's form (conftest: the one-launch stereo_match_lds_kernel<true>, which sorts in LDS)"""
    f = B.stereo_rows(rows)
    assert _same_stereo(oracle.stereo_match(oracle.Camera(**pkg.synth.EUROC_CAMERA), *f), gpu_handle.stereo_match(*f))


def test_stereo_match_three_launch_form_with_the_right_keypoints_in_edge_buckets(oracle, pkg, tmp_path):
    """ORBX_SM_LDS=0: stereo_bucket_kernel / stereo_match_kernel / stereo_compact_kernel.  A child process: the switch is read at the first
    stereo-match call."""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = textwrap.dedent("""
        import sys, numpy as np
        sys.path[:0] = [%r, %r]
        import orb_slam3_rust_amd as P
        import block_primitive_scenes as B
        h = P.Handle(P.CameraModel(**P.synth.EUROC_CAMERA), 1000, device=0, max_w=752, max_h=480, max_batch=1)
        out = {}
        for name, rows in (("edges", B.STEREO_ROWS), ("one", B.STEREO_ONE)):
            m, pts, has = h.stereo_match(*B.stereo_rows(rows))
            out[name + "_m"] = np.frombuffer(m.tobytes(), np.uint8); out[name + "_p"] = pts; out[name + "_h"] = has
        h.close()
        np.savez(sys.argv[1], **out)
    """ % (root, os.path.join(root, "tests")))
    path = str(tmp_path / "sm0.npz")
    subprocess.run([sys.executable, "-c", script, path], check=True, env=dict(os.environ, ORBX_SM_LDS="0"), timeout=300)
    res = np.load(path)
    for name, rows in (("edges", B.STEREO_ROWS), ("one", B.STEREO_ONE)):
        want = oracle.stereo_match(oracle.Camera(**pkg.synth.EUROC_CAMERA), *B.stereo_rows(rows))
        got = (np.frombuffer(res[name + "_m"].tobytes(), pkg.DMATCH), res[name + "_p"], res[name + "_h"])
        assert _same_stereo(want, got), name


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cells", [B.GUIDED_CELLS, B.GUIDED_ONE], ids=["edges", "one"])
def test_guided_match_with_the_keypoints_in_edge_cells(gpu_handle, oracle, cells, mode):
    kp, desc, uv, qd = B.guided_cells(cells)
    i0, d0 = oracle.guided_match(kp, desc, G.W, G.H, uv, qd, 15.0, mode)
    i1, d1 = gpu_handle.guided_match(kp, desc, G.W, G.H, uv, qd, 15.0, mode)
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1)


@pytest.mark.parametrize("cells", [B.TRI_CELLS, B.TRI_ONE], ids=["edges", "one"])
def test_triangulation_search_with_keyframe_2_in_edge_cells_of_a_64_x_64_grid(gpu_handle, oracle, pkg, cells):
    s = B.tri_cells(cells)
    a = (s["kp1"], s["desc1"], s["mp1"], s["stereo1"], s["kp2"], s["desc2"], s["mp2"], s["pose1_wc"], s["pose2_wc"])
    want = oracle.search_for_triangulation(oracle.Camera(**s["camera"]), *a, 50)
    got = gpu_handle.search_for_triangulation(pkg.CameraModel(**s["camera"]), *a, 50)
    assert got.dtype == np.int32 and np.array_equal(got, want)
