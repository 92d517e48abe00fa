"""The kernels with an ordered append or a block sum (csrc/block_dev.hpp, and lv_resolve_kernel's own) at the sizes where such
code goes wrong: round boundaries, a second counter that moves apart from the first, a block index past the thread count, a list
carried over a chunk and a neighbour.  Each case is held to its existing specification with that module's own tolerances;
tests/test_block_primitives_cpu.py checks that the scenes are what they are for."""
import numpy as np
import pytest

import block_primitive_scenes as B
import loop_verify_spec as LS
import track_reference_spec as RS
import tracking_scenes as G
import tracking_spec as TS
import triangulation_spec as XS
from test_loop_verify_gpu import _cfg as loop_cfg
from test_loop_verify_gpu import assert_pair_matches_spec
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
@pytest.mark.parametrize("scene", ["track_rounds", "track_many"])
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
