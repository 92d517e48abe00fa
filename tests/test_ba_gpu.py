"""GPU parity of visual local BA (solve_visual_ba, local_ba_lm.rs:912-1098) through the C ABI.
f64 throughout; tolerance: optimised poses and points within 1e-6 relative (BASELINE north_star) of
the oracle's literal dense-LM formulation, per-iteration bookkeeping identical."""
import numpy as np
import pytest

from conftest import assert_ba_close, pose_errors, point_errors

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-6   # north_star: per keyframe — rotation angle of the difference (rad) and |dt|/|t|; per point |dX|/|X|


def _rel(a, b):
    """poses [K,7] -> max(rotation angle, relative translation error) over the keyframes; points [M,3] -> max relative error"""
    a = np.asarray(a); b = np.asarray(b)
    if a.shape[-1] == 7:
        return max(pose_errors(a, b))
    return point_errors(a, b)


def _solve_both(gpu_handle, oracle, pkg, w, dense=True, **kw):
    cam = pkg.CameraModel(**w["camera"]); ocam = oracle.Camera(**w["camera"])
    g = gpu_handle.ba_solve_visual(cam, pkg.LocalBAConfigLM(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"], **kw)
    solve = oracle.ba_solve_dense if dense else oracle.ba_solve_schur
    o = solve(ocam, oracle.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    return g, o


@pytest.mark.parametrize("seed,K,M,extra", [(1, 5, 120, 0), (2, 8, 300, 2), (3, 3, 40, 0), (4, 12, 200, 1)])
def test_ba_matches_dense_reference_formulation(gpu_handle, oracle, pkg, seed, K, M, extra):
    w = pkg.synth.ba_window(seed, K, M, pkg.BA_OBS, n_fixed_extra=extra)
    g, o = _solve_both(gpu_handle, oracle, pkg, w, dense=True)
    assert g["iterations"] == o["iterations"]
    assert abs(g["initial_error"] - o["initial_error"]) < 1e-12 * o["initial_error"]
    assert abs(g["final_error"] - o["final_error"]) < 1e-8 * o["final_error"]
    assert _rel(g["poses_wc"], o["poses_wc"]) < POSE_TOL
    assert _rel(g["points"], o["points"]) < POSE_TOL
    assert g["final_error"] < 0.6 * g["initial_error"]


def test_ba_config3_size_vs_structured_oracle(gpu_handle, oracle, pkg):
    """BASELINE configs[2]: 20 keyframes / 2000 points (dense formulation does not fit -> Schur oracle)"""
    w = pkg.synth.ba_window(42, 20, 2000, pkg.BA_OBS)
    g, o = _solve_both(gpu_handle, oracle, pkg, w, dense=False)
    assert g["iterations"] == o["iterations"] == 10
    assert abs(g["final_error"] - o["final_error"]) < 1e-8 * o["final_error"]
    assert _rel(g["poses_wc"], o["poses_wc"]) < POSE_TOL
    assert _rel(g["points"], o["points"]) < POSE_TOL
    # run-to-run determinism (fixed-order reductions)
    g2, _ = _solve_both(gpu_handle, oracle, pkg, w, dense=False)
    assert np.array_equal(g["poses_wc"], g2["poses_wc"]) and np.array_equal(g["points"], g2["points"])


def test_ba_large_window_gmem_cholesky(gpu_handle, oracle, pkg):
    """K=30 -> n=174: reduced system no longer fits LDS, global-memory Cholesky path"""
    w = pkg.synth.ba_window(7, 31, 600, pkg.BA_OBS)
    g, o = _solve_both(gpu_handle, oracle, pkg, w, dense=False)
    assert g["iterations"] == o["iterations"]
    assert _rel(g["poses_wc"], o["poses_wc"]) < POSE_TOL and _rel(g["points"], o["points"]) < POSE_TOL


def test_ba_one_launch_global_cholesky_and_its_boundary(gpu_handle, oracle, pkg):
    """Reduced systems beyond the LDS tiles: up to 320 unknowns one workgroup factors them in one launch (ba_big_factor_kernel, left-looking
    with a panel of look-ahead), beyond that one launch per panel.  n = 192 (full panels only), 318 (the largest one-launch size: a short
    last panel and two rows per thread below the first panels) and 324 (the first multi-launch size) against the structured oracle."""
    for seed, K, M in ((31, 33, 500), (32, 54, 700), (33, 55, 700)):
        w = pkg.synth.ba_window(seed, K, M, pkg.BA_OBS)
        g, o = _solve_both(gpu_handle, oracle, pkg, w, dense=False)
        assert g["iterations"] == o["iterations"], (K, M)
        assert _rel(g["poses_wc"], o["poses_wc"]) < POSE_TOL and _rel(g["points"], o["points"]) < POSE_TOL, (K, M)


def test_ba_multi_block_schur_last_column_block_widths(gpu_handle, oracle, pkg):
    """The Schur product of a window with more than 128 reduced unknowns multiplies only the 16-column tiles that exist in its last
    128-column block, with the tile count as a compile-time bound of 2, 4, 6 or 8: 14 tiles (8 + 6: n = 210), 15 (8 + 7: n = 234, the
    8-variant on a partial block) and 17 (8 + 8 + 1: n = 258, three column blocks, the 2-variant) against the structured oracle (9 to 11
    tiles — the 2- and 4-variants with two blocks — are test_ba_mid_window_tiled_lds_cholesky's sizes, 19 and 20 configs[4]'s and n = 318)."""
    for seed, K, M in ((34, 36, 500), (35, 40, 500), (36, 44, 550)):
        w = pkg.synth.ba_window(seed, K, M, pkg.BA_OBS)
        g, o = _solve_both(gpu_handle, oracle, pkg, w, dense=False)
        assert g["iterations"] == o["iterations"], (K, M)
        assert _rel(g["poses_wc"], o["poses_wc"]) < POSE_TOL and _rel(g["points"], o["points"]) < POSE_TOL, (K, M)


def test_ba_batch_with_global_cholesky_windows_equals_single(gpu_handle, pkg):
    """A batch that mixes every reduced-system path — LDS square (n = 114), LDS tiles (n = 150), one-launch global (n = 186, 300) and
    multi-launch global (n = 330) — returns each window's single-window result bit for bit."""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA)
    cfg = pkg.LocalBAConfigLM()
    wins = [pkg.synth.ba_window(40 + i, K, M, pkg.BA_OBS) for i, (K, M) in enumerate(((20, 300), (32, 400), (56, 600), (26, 350), (51, 500)))]
    batch = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    for w, b in zip(wins, batch):
        s = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        assert b["iterations"] == s["iterations"]
        assert np.array_equal(np.asarray(b["poses_wc"]), np.asarray(s["poses_wc"])) and np.array_equal(b["points"], s["points"])


def test_ba_reduced_system_sizes_around_panel_boundaries(gpu_handle, oracle, pkg):
    """The LDS solve walks 16-column panels, the rows below a panel following the factorisation through flags in LDS: reduced systems of
    exactly 3 and 6 panels (no short last panel: n = 48, 96), of one short panel only (n = 12), and of full panels plus a 2- and a
    14-column one (n = 18, 114, 126) against the structured oracle."""
    # (a two-keyframe window needs a few hundred points to be well conditioned: at 60 the oracle's own dense and Schur forms differ by 2.5e-6)
    for seed, K, M in ((21, 9, 200), (22, 17, 320), (27, 3, 200), (24, 4, 80), (25, 20, 400), (26, 22, 420)):
        w = pkg.synth.ba_window(seed, K, M, pkg.BA_OBS)
        g, o = _solve_both(gpu_handle, oracle, pkg, w, dense=False)
        assert g["iterations"] == o["iterations"], (K, M)
        assert _rel(g["poses_wc"], o["poses_wc"]) < POSE_TOL and _rel(g["points"], o["points"]) < POSE_TOL, (K, M)


def test_ba_mid_window_tiled_lds_cholesky(gpu_handle, oracle, pkg):
    """22..29 optimised keyframes (n = 132..174): the reduced system does not fit LDS as a square but does as lower 16 x 16 tiles — one
    launch (ba_solve_tiled_kernel) instead of the multi-launch path; against the structured oracle at both ends and at an odd tile count."""
    for seed, K, M in ((8, 23, 500), (9, 26, 450), (10, 30, 400)):
        w = pkg.synth.ba_window(seed, K, M, pkg.BA_OBS)
        g, o = _solve_both(gpu_handle, oracle, pkg, w, dense=False)
        assert g["iterations"] == o["iterations"], (K, M)
        assert _rel(g["poses_wc"], o["poses_wc"]) < POSE_TOL and _rel(g["points"], o["points"]) < POSE_TOL, (K, M)


def test_ba_noise_free_and_golden(gpu_handle, oracle, pkg, golden):
    w = pkg.synth.ba_window(1, 5, 60, pkg.BA_OBS, noise_px=0.0, perturb=False)
    g, o = _solve_both(gpu_handle, oracle, pkg, w)
    assert g["iterations"] == 1 and g["final_error"] < 1e-9
    assert np.allclose(g["points"], w["points"], atol=1e-12)
    # one observation at the reference test's inputs (local_ba_lm.rs:1166-1185): initial error = |r|/sqrt(2)
    gj = golden["ba_jacobian_identity"]
    obs = np.array([(-1, 0, 0, 0, gj["observed"][0], gj["observed"][1])], pkg.BA_OBS)
    cam = pkg.CameraModel(**gj["camera"])
    cfg = pkg.LocalBAConfigLM(max_iterations=0)
    r = gpu_handle.ba_solve_visual(cam, cfg, np.zeros((0, 7)), [gj["pose_cw"]], [gj["point"]], obs)
    want = np.linalg.norm(gj["huber_default"]["residual"]) / np.sqrt(2.0)
    assert abs(r["initial_error"] - want) < 1e-12 * want and r["iterations"] == 0


def test_ba_failed_factorisation_ends_the_solve_on_every_reduced_system_path(gpu_handle, pkg):
    """local_ba_lm.rs:1036-1039: when the reduced system cannot be factored the loop ends and the parameters stay as they are.  One
    observation with a NaN pixel makes every pivot fail; each path of the reduced solve — LDS square (n = 114), LDS tiles (n = 150), the
    one-launch global factorisation with its folded backward substitution (n = 192, 294) and the multi-launch one (n = 330) — must stop
    after that iteration and hand back exactly what a zero-iteration call returns, alone and inside a batch."""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA)
    wins = []
    for seed, K, M in ((61, 20, 300), (62, 26, 350), (63, 33, 400), (64, 50, 600), (65, 56, 600)):
        w = pkg.synth.ba_window(seed, K, M, pkg.BA_OBS)
        w["obs"] = w["obs"].copy(); w["obs"]["u"][7] = np.nan
        wins.append(w)
    cfg, cfg0 = pkg.LocalBAConfigLM(), pkg.LocalBAConfigLM(max_iterations=0)
    batch = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    for w, b in zip(wins, batch):
        r = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        z = gpu_handle.ba_solve_visual(cam, cfg0, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        for got in (r, b):
            assert got["iterations"] == 1, len(w["poses_cw"])
            assert np.array_equal(np.asarray(got["poses_wc"]), np.asarray(z["poses_wc"])) and np.array_equal(got["points"], z["points"])


def test_ba_abort_and_none(gpu_handle, oracle, pkg):
    w = pkg.synth.ba_window(3, 4, 40, pkg.BA_OBS)
    cam = pkg.CameraModel(**w["camera"])
    cfg = pkg.LocalBAConfigLM()
    calls = []
    r = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"],
                                   should_stop=lambda: (calls.append(1) or len(calls) > 2))
    assert r["iterations"] == 2 and len(calls) == 3                 # polled once per iteration (:1013)
    o = oracle.ba_solve_schur(oracle.Camera(**w["camera"]), oracle.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"], stop_after=2)
    assert _rel(r["poses_wc"], o["poses_wc"]) < POSE_TOL
    assert gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"][:0]) is None
    bad = w["obs"].copy(); bad["mp_idx"][0] = 10 ** 6
    with pytest.raises(pkg.OrbxError):
        gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], bad)


def test_solve_visual_ba_mirror(gpu_handle, oracle, pkg):
    """the reference-shaped entry point: VisualBAProblemData keyed by ids -> VisualBAResultData"""
    w = pkg.synth.ba_window(5, 6, 100, pkg.BA_OBS)
    K = len(w["poses_cw"])
    kf_ids = [100 + 7 * i for i in range(K)]; anchor = 3; mp_ids = [5000 + 3 * j for j in range(len(w["points"]))]
    obs = [pkg.VisualObservation(kf_ids[o["kf_idx"]] if o["kf_idx"] >= 0 else anchor, mp_ids[o["mp_idx"]],
                                 (float(o["u"]), float(o["v"])), bool(o["kf_idx"] >= 0)) for o in w["obs"]]
    prob = pkg.VisualBAProblemData({k: w["poses_cw"][i] for i, k in enumerate(kf_ids)},
                                   {m: w["points"][j] for j, m in enumerate(mp_ids)},
                                   {anchor: w["fixed_cw"][0]}, anchor, obs, kf_ids, mp_ids)
    res = pkg.solve_visual_ba(prob, pkg.CameraModel(**w["camera"]), pkg.LocalBAConfigLM(), lambda: False, handle=gpu_handle)
    o = oracle.ba_solve_dense(oracle.Camera(**w["camera"]), oracle.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    assert res.iterations == o["iterations"] and set(res.optimized_poses) == set(kf_ids)
    got = np.array([res.optimized_poses[k] for k in kf_ids])
    assert _rel(got, o["poses_wc"]) < POSE_TOL


def _solve_partitioned_on_one_gpu(pkg, w, world):
    """`world` ranks = `world` handles driven by `world` host threads of this process on ONE GPU; the all-reduce hook sums their device
    buffers in place (every rank adds the slots in rank order, so all ranks hold the same bits).  Returns (per-rank results, handles)."""
    import threading
    import torch
    cam = pkg.CameraModel(**w["camera"]); cfg = pkg.LocalBAConfigLM()
    dev = torch.device("cuda", 0)
    hs = [pkg.Handle(cam, 100, device=0) for _ in range(world)]
    bar = threading.Barrier(world)
    slots = [None] * world
    out = [None] * world
    errs = []

    def hook_for(rank):
        def hook(ptr, n, stream):
            torch.cuda.synchronize()
            slots[rank] = pkg.dist.device_tensor(ptr, n, dev)
            bar.wait()
            total = slots[0].clone()
            for r in range(1, world):
                total += slots[r]
            torch.cuda.synchronize()
            bar.wait()
            slots[rank].copy_(total)
            torch.cuda.synchronize()
            bar.wait()
        return hook

    def run(rank):
        try:
            out[rank] = pkg.dist.ba_solve_partitioned(hs[rank], cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"],
                                                      w["obs"], rank, world, hook_for(rank))
        except Exception as e:  # pragma: no cover
            errs.append(e); bar.abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts: t.start()
    for t in ts: t.join(300)
    assert not errs, errs
    return out, hs


@pytest.mark.parametrize("world,seed,K,M,extra", [(2, 21, 10, 400, 1),                       # a small window with a second fixed observer
                                                  (2, 42, 20, 2000, 0), (4, 42, 20, 2000, 0), (8, 42, 20, 2000, 0),   # configs[2] / configs[3]: synth_ba(42, 20, 2000)
                                                  (8, 43, 50, 8000, 0)])                     # configs[4]: synth_ba(43, 50, 8000) over 8 ranks
def test_ba_point_partition_ranks_on_one_gpu(oracle, pkg, world, seed, K, M, extra):
    """Point-partitioned BA on the real kernels at the sizes and rank counts configs[3] / configs[4] name: the map points dealt
    round-robin to `world` ranks, each rank building complete V_j / W_j for its points and partial U, g_p, S_red, b_red, chi2; one all-reduce of
    (6K)^2 + 48K + 2 doubles before the solve and one of 4 after the back-substitution, per iteration.  Against the ORACLE's structured
    solve of the whole problem (iteration counts, errors, poses and points within the 1e-6 bar of every other BA test), against the
    library's own single-handle solve (rounding only: the summation order differs), and identical bits on every rank."""
    w = pkg.synth.ba_window(seed, K, M, pkg.BA_OBS, n_fixed_extra=extra)
    out, hs = _solve_partitioned_on_one_gpu(pkg, w, world)
    cam = pkg.CameraModel(**w["camera"]); cfg = pkg.LocalBAConfigLM()
    single = hs[0].ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    o = oracle.ba_solve_schur(oracle.Camera(**w["camera"]), oracle.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    sizes = [len(pkg.dist.partition_observations(w["obs"], r, world)) for r in range(world)]
    assert sum(sizes) == len(w["obs"]) and min(sizes) > 0
    for r in range(world):
        assert out[r]["iterations"] == single["iterations"] == o["iterations"]
        assert _rel(out[r]["poses_wc"], single["poses_wc"]) < 1e-9
        assert _rel(out[r]["points"], single["points"]) < 1e-9
        assert abs(out[r]["final_error"] - single["final_error"]) < 1e-10 * single["final_error"]
        ang, dt = pose_errors(out[r]["poses_wc"], o["poses_wc"])
        assert ang < POSE_TOL and dt < POSE_TOL, (r, ang, dt)
        assert _rel(out[r]["points"], o["points"]) < POSE_TOL
        assert abs(out[r]["initial_error"] - o["initial_error"]) < 1e-8 * o["initial_error"]
        assert abs(out[r]["final_error"] - o["final_error"]) < 1e-8 * o["final_error"]
        assert np.array_equal(out[r]["poses_wc"], out[0]["poses_wc"]) and np.array_equal(out[r]["points"], out[0]["points"])
    for h in hs: h.close()


def test_ba_allreduce_hook_rccl_world1(gpu_handle, pkg):
    """The torch.distributed hook itself (backend nccl = RCCL), world_size 1 on this one GPU: the
    collective runs on the library's stream through torch.cuda.ExternalStream and must leave the
    single-rank result unchanged bit for bit."""
    import os, socket
    import torch
    import torch.distributed as dist
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        w = pkg.synth.ba_window(9, 7, 250, pkg.BA_OBS)
        cam = pkg.CameraModel(**w["camera"]); cfg = pkg.LocalBAConfigLM()
        ref = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        got = pkg.dist.ba_solve_partitioned(gpu_handle, cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"],
                                            0, 1, pkg.dist.make_allreduce_hook(dev))
        assert got["iterations"] == ref["iterations"]
        # poses are bit-identical; points go through the cross-rank merge init + sum(delta), which rounds once more
        assert np.array_equal(got["poses_wc"], ref["poses_wc"])
        assert _rel(got["points"], ref["points"]) < 1e-14
        assert got["final_error"] == ref["final_error"]
    finally:
        dist.destroy_process_group()


def test_ba_config5_size(gpu_handle, oracle, pkg):
    """BASELINE configs[4]: 50 keyframes / 8000 points (n = 294: one-launch global-memory factorisation, multi-block Schur product on
    19 x 19 MFMA tiles) over the metric's own loop — LocalBAConfigLM::default(), 10 LM iterations (local_ba_lm.rs:1012-1056): iteration
    count, the accept / reject outcome of every iteration (through the error trace's end points), final error and every pose / point
    against the structured oracle (about 0.12 s of CPU per oracle iteration)."""
    w = pkg.synth.ba_window(43, 50, 8000, pkg.BA_OBS)
    cam = pkg.CameraModel(**w["camera"]); ocam = oracle.Camera(**w["camera"])
    cfg = pkg.LocalBAConfigLM(); ocfg = oracle.ba_config()
    assert cfg.max_iterations == ocfg.max_iterations == 10
    g = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    o = oracle.ba_solve_schur(ocam, ocfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    assert g["iterations"] == o["iterations"] == 10 and len(w["obs"]) > 150000
    assert abs(g["initial_error"] - o["initial_error"]) < 1e-12 * o["initial_error"]
    assert abs(g["final_error"] - o["final_error"]) < 1e-8 * o["final_error"]
    assert _rel(g["poses_wc"], o["poses_wc"]) < POSE_TOL and _rel(g["points"], o["points"]) < POSE_TOL
    # every prefix of the loop too: the state after 3 and after 7 iterations (an accept / reject decision that differed at iteration
    # i would leave a different lambda, hence different poses, in every later prefix)
    for it in (3, 7):
        cfg_i = pkg.LocalBAConfigLM(max_iterations=it); ocfg_i = oracle.ba_config(); ocfg_i.max_iterations = it
        gi = gpu_handle.ba_solve_visual(cam, cfg_i, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        oi = oracle.ba_solve_schur(ocam, ocfg_i, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        assert gi["iterations"] == oi["iterations"] == it
        assert abs(gi["final_error"] - oi["final_error"]) < 1e-8 * oi["final_error"], it
        assert _rel(gi["poses_wc"], oi["poses_wc"]) < POSE_TOL and _rel(gi["points"], oi["points"]) < POSE_TOL, it


def test_ba_batch_equals_single_bit_for_bit(gpu_handle, pkg):
    """orbx_ba_solve_visual_batch: every window of a batch — different sizes, the LDS and the global-memory factorisation
    mixed, one window the reference answers None for — equals orbx_ba_solve_visual on that window bit for bit."""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    wins = [pkg.synth.ba_window(100 + i, K, M, pkg.BA_OBS, n_fixed_extra=x) for i, (K, M, x) in
            enumerate([(6, 150, 0), (20, 2000, 0), (4, 60, 1), (31, 500, 0), (9, 333, 2), (20, 1200, 0), (3, 40, 0)])]
    empty = dict(wins[2]); empty["obs"] = wins[2]["obs"][:0]
    wins.insert(3, empty)
    single = [gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"]) for w in wins]
    batch = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    assert len(batch) == len(wins) and batch[3] is None and single[3] is None
    for i, (s, b) in enumerate(zip(single, batch)):
        if s is None:
            continue
        assert b["iterations"] == s["iterations"], i
        assert b["initial_error"] == s["initial_error"] and b["final_error"] == s["final_error"], i
        assert np.array_equal(b["poses_wc"], s["poses_wc"]) and np.array_equal(b["points"], s["points"]), i
    # the same batch again, shuffled: results do not depend on what else is in the batch or where
    order = [5, 0, 7, 2, 1, 6, 4]
    again = gpu_handle.ba_solve_visual_batch(cam, cfg, [wins[i] for i in order])
    for k, i in enumerate(order):
        assert np.array_equal(again[k]["poses_wc"], single[i]["poses_wc"]) and np.array_equal(again[k]["points"], single[i]["points"])


def test_ba_batch_lane_groups_do_not_enter_the_sums(gpu_handle, pkg):
    """A batch of 8 or more windows runs the per-point kernels with 16 lanes per point, one window with 32 (ba_kernels.hip group_sum):
    points seen by 1..16, 17..32, 33..48 and more than 48 keyframes must come out bit for bit as in the single-window solve."""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    shapes = [(40, 300), (70, 200), (50, 400), (12, 500), (24, 350), (33, 260), (18, 640), (66, 120), (5, 80)]
    wins = [pkg.synth.ba_window(900 + i, K, M, pkg.BA_OBS) for i, (K, M) in enumerate(shapes)]
    counts = np.concatenate([np.bincount(w["obs"]["mp_idx"], minlength=len(w["points"])) for w in wins])
    assert (counts <= 16).any() and ((counts > 16) & (counts <= 32)).any() and ((counts > 32) & (counts <= 48)).any() and (counts > 48).any()
    batch = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    for i, w in enumerate(wins):
        s = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        assert batch[i]["iterations"] == s["iterations"], i
        assert batch[i]["initial_error"] == s["initial_error"] and batch[i]["final_error"] == s["final_error"], i
        assert np.array_equal(batch[i]["poses_wc"], s["poses_wc"]) and np.array_equal(batch[i]["points"], s["points"]), i


def test_ba_batch_32_windows_config3(gpu_handle, oracle, pkg):
    """32 windows of BASELINE configs[2] size in one call (the bench's batched leg): all converge like the single solve,
    window 0 against the Schur oracle."""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    wins = [pkg.synth.ba_window(300 + i, 20, 2000, pkg.BA_OBS) for i in range(32)]
    res = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    assert all(r["iterations"] == 10 and r["final_error"] < 0.6 * r["initial_error"] for r in res)
    o = oracle.ba_solve_schur(oracle.Camera(**pkg.synth.EUROC_CAMERA), oracle.ba_config(), wins[0]["poses_cw"], wins[0]["fixed_cw"],
                              wins[0]["points"], wins[0]["obs"])
    assert_ba_close(res[0], o, POSE_TOL)
    one = gpu_handle.ba_solve_visual(cam, cfg, wins[31]["poses_cw"], wins[31]["fixed_cw"], wins[31]["points"], wins[31]["obs"])
    assert np.array_equal(one["poses_wc"], res[31]["poses_wc"]) and np.array_equal(one["points"], res[31]["points"])


def test_ba_batch_two_streams_path(gpu_handle, pkg):
    """16 or more windows without a callback run as two halves on two streams inside the call (orbx.h): windows of mixed sizes
    across both halves, a window the reference answers None for in the second half, equality with the single-window solves, and an
    observation index out of range in the second half failing the whole call with its window named."""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    shapes = [(5, 90, 0), (12, 400, 1), (20, 900, 0), (3, 40, 0), (8, 250, 2), (25, 600, 0)]
    wins = [pkg.synth.ba_window(700 + i, *shapes[i % len(shapes)][:2], pkg.BA_OBS, n_fixed_extra=shapes[i % len(shapes)][2]) for i in range(18)]
    empty = dict(wins[13]); empty["obs"] = wins[13]["obs"][:0]
    wins[13] = empty
    batch = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    assert batch[13] is None
    for i in (0, 4, 8, 9, 12, 17):
        w = wins[i]
        s = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        assert batch[i]["iterations"] == s["iterations"] and np.array_equal(batch[i]["poses_wc"], s["poses_wc"]) and \
            np.array_equal(batch[i]["points"], s["points"]), i
    bad = [dict(w) for w in wins]
    o = bad[15]["obs"].copy(); o["mp_idx"][7] = len(bad[15]["points"]) + 3
    bad[15]["obs"] = o
    with pytest.raises(pkg.OrbxError) as e:
        gpu_handle.ba_solve_visual_batch(cam, cfg, bad)
    assert "out of range" in str(e.value) and "numbered from 9" in str(e.value)
    # and the handle still works afterwards
    again = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    assert np.array_equal(again[17]["poses_wc"], batch[17]["poses_wc"])


def test_ba_batch_half_refused_while_planning_leaves_nothing_behind(gpu_handle, pkg):
    """16 tiny windows run as two halves.  Window 2, in the first half, hands in 129 optimised keyframes: that half is refused by the size
    check, before any GPU work and before the point at which it would open the upload gate for the second half — the call must come back
    (the second half never waits for a gate nobody opens) with ORBX_ERR_INVALID and the library's text.  What a half is told about the
    batch (thread cap, peer windows, gate) is an argument of that one call: the same batch without the oversized window then solves on the
    same handle, and its window 15 equals its own single-window solve bit for bit."""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    wins = [pkg.synth.ba_window(3100 + i, 3, 40, pkg.BA_OBS) for i in range(16)]
    bad = list(wins)
    bad[2] = dict(wins[2], poses_cw=np.repeat(wins[2]["poses_cw"][:1], 129, axis=0))
    with pytest.raises(pkg.OrbxError) as e:
        gpu_handle.ba_solve_visual_batch(cam, cfg, bad)
    assert e.value.code == -1 and "window 2: at most 128 optimised keyframes per window" in str(e.value)      # ORBX_ERR_INVALID
    batch = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    w = wins[15]
    s = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    assert batch[15]["iterations"] == s["iterations"] and batch[15]["initial_error"] == s["initial_error"] and batch[15]["final_error"] == s["final_error"]
    assert np.array_equal(batch[15]["poses_wc"], s["poses_wc"]) and np.array_equal(batch[15]["points"], s["points"])


def test_ba_observations_from_pinned_memory_equal_staged(gpu_handle, pkg):
    """The observation CSR is built on the device from the observations as handed over (ba_prep_*_kernel).  Windows whose `obs` arrays are
    consecutive slices of one page-locked buffer are read by the copy engine where they lie, one copy per half (Handle.pack_ba_windows);
    pageable arrays go through the handle's pinned staging blob.  Both, and the single-window entry point (one pinned, one pageable), give
    the same bits — 18 windows (two streams), mixed sizes, a window the reference answers None for, points seen twice by one keyframe."""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    shapes = [(20, 1200), (6, 150), (12, 400), (3, 40), (25, 600), (9, 333)]
    wins = [pkg.synth.ba_window(2100 + i, *shapes[i % len(shapes)], pkg.BA_OBS, n_fixed_extra=i % 3) for i in range(18)]
    dup = wins[4]["obs"][:50].copy(); dup["u"] += 0.25                      # 50 (point, keyframe) pairs observed twice
    wins[4] = dict(wins[4]); wins[4]["obs"] = np.concatenate([wins[4]["obs"], dup])
    empty = dict(wins[11]); empty["obs"] = wins[11]["obs"][:0]
    wins[11] = empty
    packed = pkg.Handle.pack_ba_windows(wins)
    full = [p for p in packed if len(p["obs"])]                            # (the address of an empty slice says nothing)
    assert all(p["obs"].ctypes.data + p["obs"].nbytes == q["obs"].ctypes.data for p, q in zip(full[:-1], full[1:]))
    a = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    b = gpu_handle.ba_solve_visual_batch(cam, cfg, packed)
    assert a[11] is None and b[11] is None
    for i, (x, y) in enumerate(zip(a, b)):
        if x is None:
            continue
        assert x["iterations"] == y["iterations"] and x["final_error"] == y["final_error"], i
        assert np.array_equal(x["poses_wc"], y["poses_wc"]) and np.array_equal(x["points"], y["points"]), i
    for i in (0, 4, 17):
        for w in (wins[i], packed[i]):
            s = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
            assert np.array_equal(s["poses_wc"], a[i]["poses_wc"]) and np.array_equal(s["points"], a[i]["points"]), i
    # the prepared form (api.BaBatch: the windows kept in the ABI's layout) gives the same bits, call after call
    prepared = gpu_handle.prepare_ba_batch(wins)
    for _ in range(2):
        c = prepared.solve(cam, cfg)
        assert c[11] is None
        for i, (x, y) in enumerate(zip(a, c)):
            if x is not None:
                assert x["iterations"] == y["iterations"] and np.array_equal(x["poses_wc"], y["poses_wc"]) and np.array_equal(x["points"], y["points"]), i
    # the 16-byte wire format (orbx_ba_obs32: f32 coordinates, widened on the device) on windows whose coordinates are f32, as the reference's:
    # the same bits as the 32-byte form of the same windows; coordinates that are not f32 are refused by the mirror
    w32 = [pkg.synth.keypoint_precision(w) for w in wins]
    ref32 = gpu_handle.ba_solve_visual_batch(cam, cfg, w32)
    got32 = gpu_handle.prepare_ba_batch(w32, obs32=True).solve(cam, cfg)
    for i, (x, y) in enumerate(zip(ref32, got32)):
        if x is None:
            assert y is None
            continue
        assert x["iterations"] == y["iterations"] and x["initial_error"] == y["initial_error"] and x["final_error"] == y["final_error"], i
        assert np.array_equal(x["poses_wc"], y["poses_wc"]) and np.array_equal(x["points"], y["points"]), i
    with pytest.raises(ValueError):
        gpu_handle.prepare_ba_batch(wins, obs32=True)
    # ... and through the single-window entry points (orbx_ba_solve_visual_obs32 / orbx_ba_solve_global_obs32, round 5): pageable and pinned
    p32 = pkg.Handle.pack_ba_windows(w32, obs32=True)
    assert p32[0]["obs"].dtype == pkg.BA_OBS32 and p32[0]["obs"].itemsize == 16
    for i in (0, 4, 17):
        for o in (pkg.ba_obs_to_obs32(w32[i]["obs"], len(w32[i]["fixed_cw"])), p32[i]["obs"]):
            s = gpu_handle.ba_solve_visual(cam, cfg, w32[i]["poses_cw"], w32[i]["fixed_cw"], w32[i]["points"], o)
            assert s["iterations"] == ref32[i]["iterations"] and s["initial_error"] == ref32[i]["initial_error"] and s["final_error"] == ref32[i]["final_error"], i
            assert np.array_equal(s["poses_wc"], ref32[i]["poses_wc"]) and np.array_equal(s["points"], ref32[i]["points"]), i
    gw = pkg.synth.keypoint_precision(pkg.synth.ba_window(2177, 7, 300, pkg.BA_OBS))        # global BA: one fixed keyframe, kf_idx -1 - 0
    g64 = gpu_handle.ba_solve_global(cam, cfg, gw["poses_cw"], gw["fixed_cw"][0], gw["points"], gw["obs"])
    g32 = gpu_handle.ba_solve_global(cam, cfg, gw["poses_cw"], gw["fixed_cw"][0], gw["points"], pkg.ba_obs_to_obs32(gw["obs"], 1))
    assert g64["iterations"] == g32["iterations"] and np.array_equal(g64["poses_wc"], g32["poses_wc"]) and np.array_equal(g64["points"], g32["points"])
    with pytest.raises(ValueError):
        pkg.Handle.pack_ba_windows(wins, obs32=True)
    # an index out of range inside pinned memory is found by the device-side check and named
    o = packed[15]["obs"]; keep = int(o["mp_idx"][7]); o["mp_idx"][7] = len(packed[15]["points"]) + 3
    with pytest.raises(pkg.OrbxError) as e:
        gpu_handle.ba_solve_visual_batch(cam, cfg, packed)
    assert "out of range" in str(e.value) and "observation 7" in str(e.value)
    o["mp_idx"][7] = keep
    again = gpu_handle.ba_solve_visual_batch(cam, cfg, packed)
    assert np.array_equal(again[17]["points"], a[17]["points"])


def test_ba_batch_through_the_c_abi_from_a_compiled_caller(gpu_handle, pkg, tmp_path):
    """tests/cpp/ba_batch_driver.cpp: orbx_ba_solve_visual_batch called from C++ with no Python in the process — observations in one
    orbx_host_alloc buffer, and again in pageable memory — returns what the Python mirror returns, bit for bit (20 windows: two streams)."""
    import json, os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "orb-slam3-rust_amd")
    exe = str(tmp_path / "ba_batch_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "ba_batch_driver.cpp"),
                    "-o", exe, "-L", libdir, "-lorbx_hip", "-Wl,-rpath," + libdir], check=True)
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    shapes = [(20, 900), (7, 200), (14, 500), (4, 60)]
    wins = [pkg.synth.ba_window(2300 + i, *shapes[i % 4], pkg.BA_OBS, n_fixed_extra=i % 2) for i in range(20)]
    want = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    pkg.synth.write_ba_batch_file(str(tmp_path / "batch.bin"), wins, pkg.BA_OBS)
    wins = [pkg.synth.keypoint_precision(w) for w in wins]                    # f32 pixel coordinates, as the reference's: the 16-byte wire format applies
    want = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    pkg.synth.write_ba_batch_file(str(tmp_path / "batch.bin"), wins, pkg.BA_OBS)
    for mode in ("pinned", "pageable", "pinned32"):
        r = subprocess.run([exe, str(tmp_path / "batch.bin"), str(tmp_path / "out.bin"), "2", mode], check=True, capture_output=True, text=True)
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["windows"] == 20 and line["reps"] == 2 and len(line["ms_per_call"]) == 2
        got = pkg.synth.read_ba_batch_results(str(tmp_path / "out.bin"), wins)
        for i, (g, w_) in enumerate(zip(got, want)):
            assert g["status"] == 0 and g["iterations"] == w_["iterations"], (mode, i)
            assert g["initial_error"] == w_["initial_error"] and g["final_error"] == w_["final_error"], (mode, i)
            assert np.array_equal(g["poses_wc"], w_["poses_wc"]) and np.array_equal(g["points"], w_["points"]), (mode, i)


def test_ba_fused_step_equals_the_two_kernels_bit_for_bit(pkg, tmp_path):
    """Calls of up to seven windows run the back-substitution and the next iteration's build pass as ONE launch (ba_step_kernel: two sets of
    build results, the rejected step's point matrices beside them); ORBX_BA_FUSED=0 keeps the two kernels.  Same arithmetic, same order:
    the results of the two forms must be the same bits — windows of every reduced-system path, a call of three windows, one of nine
    (which keeps the two kernels either way), and a window with a poor start whose first steps are rejected (the lambda * 10 branch).  Two child processes: the switch is
    read once per process."""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r)
        import orb_slam3_rust_amd as P
        cam = P.CameraModel(**P.synth.EUROC_CAMERA); cfg = P.LocalBAConfigLM()
        h = P.Handle(cam, 100)
        out = {}
        shapes = [(71, 5, 80), (72, 20, 600), (73, 26, 350), (74, 33, 400), (75, 56, 500)]
        wins = [P.synth.ba_window(s, K, M, P.BA_OBS) for s, K, M in shapes]
        bad = P.synth.ba_window(76, 12, 300, P.BA_OBS)
        bad["points"] = bad["points"] + 0.6 * np.random.default_rng(5).standard_normal(bad["points"].shape)     # far off: rejected steps
        wins.append(bad)
        for i, w in enumerate(wins):
            r = h.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
            out["p%%d" %% i] = np.asarray(r["poses_wc"]); out["x%%d" %% i] = np.asarray(r["points"])
            out["e%%d" %% i] = np.array([r["iterations"], r["initial_error"], r["final_error"]])
        for i, r in enumerate(h.ba_solve_visual_batch(cam, cfg, wins[:3])):
            out["bp%%d" %% i] = np.asarray(r["poses_wc"]); out["bx%%d" %% i] = np.asarray(r["points"])
        for i, r in enumerate(h.ba_solve_visual_batch(cam, cfg, wins + wins[:3])):      # nine windows: 16 lanes per point
            out["cp%%d" %% i] = np.asarray(r["poses_wc"]); out["cx%%d" %% i] = np.asarray(r["points"])
        np.savez(sys.argv[1], **out)
    """ % root)
    res = {}
    for mode in ("1", "0"):
        path = str(tmp_path / ("fused%s.npz" % mode))
        env = dict(os.environ, ORBX_BA_FUSED=mode)
        subprocess.run([sys.executable, "-c", script, path], check=True, env=env, timeout=300)
        res[mode] = np.load(path)
    assert sorted(res["1"].files) == sorted(res["0"].files) and len(res["1"].files) == 42
    for k in res["1"].files:
        assert np.array_equal(res["1"][k], res["0"][k]), k
    assert res["1"]["e5"][0] >= 2                                             # (the poor start did iterate)


def test_ba_large_batch_share_sums_mixed_sizes(gpu_handle, pkg):
    """A batch large enough that every Schur workgroup owns one share of its window's k-splits and writes the share's sum instead of
    the partials (BaWin::part_sums; 32 windows x 8 shares = one workgroup per CU): windows of very different sizes in one call — 1 to 63
    k-splits, so shares of 0, 1 and several k-splits, a window of a single keyframe, one the reference answers None for — each equal to
    its single-window solve bit for bit; then the same windows with one 30-keyframe window added, which sends the whole batch through the
    general Schur body (no share sums): the same results again."""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    shapes = [(20, 2000), (3, 40), (8, 100), (21, 900), (2, 30), (12, 260), (20, 1500), (5, 64), (16, 333), (10, 7 * 32 + 1)]
    wins = [pkg.synth.ba_window(1500 + i, *shapes[i % len(shapes)], pkg.BA_OBS) for i in range(34)]
    empty = dict(wins[9]); empty["obs"] = wins[9]["obs"][:0]
    wins[20] = empty
    batch = gpu_handle.ba_solve_visual_batch(cam, cfg, wins, should_stop=lambda: False)     # (a callback also keeps the call on one stream)
    assert batch[20] is None
    check = (0, 1, 3, 4, 7, 9, 13, 19, 26, 33)
    single = {i: gpu_handle.ba_solve_visual(cam, cfg, wins[i]["poses_cw"], wins[i]["fixed_cw"], wins[i]["points"], wins[i]["obs"]) for i in check}
    for i in check:
        assert batch[i]["iterations"] == single[i]["iterations"], i
        assert np.array_equal(batch[i]["poses_wc"], single[i]["poses_wc"]) and np.array_equal(batch[i]["points"], single[i]["points"]), i
    big = pkg.synth.ba_window(1600, 30, 400, pkg.BA_OBS)
    again = gpu_handle.ba_solve_visual_batch(cam, cfg, wins + [big], should_stop=lambda: False)
    for i in check:
        assert np.array_equal(again[i]["poses_wc"], single[i]["poses_wc"]) and np.array_equal(again[i]["points"], single[i]["points"]), i
    sb = gpu_handle.ba_solve_visual(cam, cfg, big["poses_cw"], big["fixed_cw"], big["points"], big["obs"])
    assert np.array_equal(again[-1]["poses_wc"], sb["poses_wc"]) and np.array_equal(again[-1]["points"], sb["points"])


def test_ba_two_handles_two_host_threads(gpu_handle, pkg):
    """Two handles driven by two host threads at once (each a batch of 16 windows: its own stream, workspaces, persistent
    preprocessing workers and internal two-stream split), three rounds: every window equals the result of the same batch solved alone."""
    import threading
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    shapes = [(20, 700), (9, 300), (14, 520), (6, 150)]
    batches = [[pkg.synth.ba_window(1200 + 40 * b + i, *shapes[(i + b) % 4], pkg.BA_OBS) for i in range(16)] for b in range(2)]
    want = [gpu_handle.ba_solve_visual_batch(cam, cfg, ws) for ws in batches]
    handles = [pkg.Handle(cam, 100) for _ in range(2)]
    try:
        for _ in range(3):
            got = [None, None]; err = []

            def run(k):
                try:
                    got[k] = handles[k].ba_solve_visual_batch(cam, cfg, batches[k])
                except Exception as e:       # noqa: BLE001 - reported below
                    err.append(e)
            th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
            [t.start() for t in th]; [t.join() for t in th]
            assert not err, err
            for k in range(2):
                for a, b in zip(got[k], want[k]):
                    assert a["iterations"] == b["iterations"] and np.array_equal(a["poses_wc"], b["poses_wc"]) and np.array_equal(a["points"], b["points"])
    finally:
        for h in handles:
            h.close()


def test_ba_batch_abort(gpu_handle, pkg):
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    wins = [pkg.synth.ba_window(400 + i, 5, 80, pkg.BA_OBS) for i in range(3)]
    calls = []
    res = gpu_handle.ba_solve_visual_batch(cam, cfg, wins, should_stop=lambda: (calls.append(1) or len(calls) > 1))
    assert [r["iterations"] for r in res] == [1, 1, 1] and len(calls) == 2      # polled once per iteration for the batch


def test_ba_abort_while_draining(gpu_handle, pkg):
    """a stop requested after every iteration has been enqueued (the polls at enqueue time are over within the
    first milliseconds) must still end the solve at an iteration boundary.  Tolerances 0 keep the LM loop running for all
    100 iterations (16 ms of GPU work); should_stop turns true on its 150th call — 100 polls at enqueue time, the rest while
    the iterations drain."""
    w = pkg.synth.ba_window(42, 20, 2000, pkg.BA_OBS)
    cam = pkg.CameraModel(**w["camera"])
    cfg = pkg.LocalBAConfigLM(max_iterations=100, param_tolerance=0.0, gradient_tolerance=0.0)
    full = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    assert full["iterations"] == 100
    calls = []
    r = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"],
                                   should_stop=lambda: (calls.append(1) or len(calls) >= 150))
    assert len(calls) == 150 and 1 <= r["iterations"] < 100, (len(calls), r["iterations"])


def test_ba_blocks_known_answers_on_gpu(gpu_handle, pkg, golden):
    """The reference's Jacobian / residual known answer (test_jacobian_pose_numerical, local_ba_lm.rs:1163-1243: identity
    pose, X = (0.5, 0.3, 3), fx = fy = 400, observed (320, 240)) evaluated by the solver's own device functions
    (orbx_debug_ba_blocks), for the pose held fixed and for the pose as an optimised keyframe, with both Huber thresholds."""
    gj = golden["ba_jacobian_identity"]
    cam = pkg.CameraModel(**gj["camera"])
    Jp = np.array(gj["J_pose"]); Jx = np.array(gj["J_point"])
    for name, th in (("huber_default", None), ("huber_test", 2.5)):
        cfg = pkg.LocalBAConfigLM() if th is None else pkg.LocalBAConfigLM(huber_threshold=th)
        sw = gj[name]["sqrt_w"]
        for optimised in (True, False):
            obs = np.array([(0 if optimised else -1, -1 if optimised else 0, 0, 0, gj["observed"][0], gj["observed"][1])], pkg.BA_OBS)
            poses = [gj["pose_cw"]] if optimised else np.zeros((0, 7))
            fixed = np.zeros((0, 7)) if optimised else [gj["pose_cw"]]
            r, A, B = gpu_handle.debug_ba_blocks(cam, cfg, poses, fixed, [gj["point"]], obs)
            assert np.allclose(r[0], gj[name]["residual"], rtol=1e-14, atol=0)
            assert np.allclose(A[0], Jp * sw, rtol=1e-13, atol=1e-13)
            assert np.allclose(B[0], Jx * sw, rtol=1e-13, atol=1e-13)
    # against central differences of the residual on a real window (what the reference's own test does, :1186-1243)
    w = pkg.synth.ba_window(77, 4, 60, pkg.BA_OBS, noise_px=0.5, perturb=False)
    cam = pkg.CameraModel(**w["camera"]); cfg = pkg.LocalBAConfigLM()
    r0, A, B = gpu_handle.debug_ba_blocks(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    eps = 1e-6
    for c in range(3):
        pp = w["points"].copy(); pp[:, c] += eps
        pm = w["points"].copy(); pm[:, c] -= eps
        rp, _, _ = gpu_handle.debug_ba_blocks(cam, cfg, w["poses_cw"], w["fixed_cw"], pp, w["obs"])
        rm, _, _ = gpu_handle.debug_ba_blocks(cam, cfg, w["poses_cw"], w["fixed_cw"], pm, w["obs"])
        num = (rp - rm) / (2 * eps)
        inl = np.linalg.norm(r0, axis=1) < 0.9 * cfg.huber_threshold      # the analytic blocks hold sqrt(w) fixed (:632-636)
        assert inl.sum() > 20 and np.allclose(num[inl], B[inl, :, c], rtol=1e-5, atol=1e-5)


def test_ba_native_rccl_world1(gpu_handle, pkg):
    """The library's own collective: orbx_rccl_unique_id + orbx_ba_init_rccl (ncclCommInitRank) and ncclAllReduce(ncclDouble,
    ncclSum) issued by the library on its stream — no torch.distributed, no Python in the loop.  World size 1 on this one
    GPU: the partitioned code path (two collectives per iteration, stop votes, point merge) must leave the single-rank result
    unchanged: poses bit for bit."""
    w = pkg.synth.ba_window(9, 7, 250, pkg.BA_OBS)
    cam = pkg.CameraModel(**w["camera"]); cfg = pkg.LocalBAConfigLM()
    ref = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    h = pkg.Handle(cam, 100, device=0)
    try:
        uid = h.rccl_unique_id()
        assert len(uid) == 128
        h.init_rccl(uid, 0, 1)
        assert h.rccl_world() == (1, 0)                              # ncclCommCount / ncclCommUserRank of the communicator the library made
        got = pkg.dist.ba_solve_partitioned(h, cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"], 0, 1)
        assert got["iterations"] == ref["iterations"] and got["final_error"] == ref["final_error"]
        assert np.array_equal(got["poses_wc"], ref["poses_wc"])
        assert _rel(got["points"], ref["points"]) < 1e-14          # the cross-rank point merge rounds once more
        # stop vote through the collective: the third poll asks -> 2 iterations, as the unpartitioned solve
        calls = []
        r = pkg.dist.ba_solve_partitioned(h, cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"], 0, 1,
                                          should_stop=lambda: (calls.append(1) or len(calls) > 2))
        r0 = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"], should_stop=(lambda c=[]: (c.append(1) or len(c) > 2)))
        assert r["iterations"] == r0["iterations"] == 2 and np.array_equal(r["poses_wc"], r0["poses_wc"])
        # a bad index on "some rank" fails the call on every rank, after the collective that carries the flag
        bad = w["obs"].copy(); bad["mp_idx"][0] = 10 ** 6
        with pytest.raises(pkg.OrbxError):
            h.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], bad)
        # windows in a batch never use the communicator
        b = h.ba_solve_visual_batch(cam, cfg, [w])[0]
        assert np.array_equal(b["poses_wc"], ref["poses_wc"]) and np.array_equal(b["points"], ref["points"])
    finally:
        h.close()


def test_ba_partition_stop_requested_by_one_rank(pkg):
    """in the partitioned solve every rank must issue the same sequence of collectives.  Two ranks (two handles,
    two threads, the hook sums their buffers); ONLY rank 1's should_stop ever answers yes (on its third poll).  Both ranks must
    stop before the same iteration with identical results — and not hang."""
    import threading
    import torch
    w = pkg.synth.ba_window(23, 8, 300, pkg.BA_OBS)
    cam = pkg.CameraModel(**w["camera"]); cfg = pkg.LocalBAConfigLM()
    dev = torch.device("cuda", 0)
    hs = [pkg.Handle(cam, 100, device=0) for _ in range(2)]
    bar = threading.Barrier(2, timeout=60)
    slots = [None, None]; out = [None, None]; errs = []; polls = [[], []]

    def hook_for(rank):
        def hook(ptr, n, stream):
            torch.cuda.synchronize()
            slots[rank] = pkg.dist.device_tensor(ptr, n, dev)
            bar.wait()
            total = slots[0] + slots[1]
            torch.cuda.synchronize()
            bar.wait()
            slots[rank].copy_(total)
            torch.cuda.synchronize()
            bar.wait()
        return hook

    def run(rank):
        try:
            stop = (lambda: (polls[1].append(1) or len(polls[1]) > 2)) if rank == 1 else (lambda: (polls[0].append(1) and False))
            out[rank] = pkg.dist.ba_solve_partitioned(hs[rank], cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"], rank, 2,
                                                      hook_for(rank), should_stop=stop)
        except Exception as e:  # pragma: no cover
            errs.append(e); bar.abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ts: t.start()
    for t in ts: t.join(120)
    assert not errs and not any(t.is_alive() for t in ts), errs
    assert out[0]["iterations"] == out[1]["iterations"] == 2
    assert np.array_equal(out[0]["poses_wc"], out[1]["poses_wc"]) and np.array_equal(out[0]["points"], out[1]["points"])
    assert len(polls[0]) == cfg.max_iterations           # rank 0 kept polling (and enqueueing) once per iteration
    for h in hs: h.close()


def test_ba_point_seen_twice_by_one_keyframe(gpu_handle, oracle, pkg):
    """Two features of one keyframe carrying the same map point (the reference's maps allow it): both rows enter J^T J, so
    W_jk is the SUM of the two W blocks.  The dense W operand of round 1 let the second overwrite the first; the tile slot
    of the Schur kernel now sums the chain.  Against the oracle's literal dense formulation."""
    w = pkg.synth.ba_window(61, 7, 120, pkg.BA_OBS, n_fixed_extra=1)     # two fixed keyframes: no free scale gauge for rounding to drift along
    rng = np.random.default_rng(61)
    opt = np.nonzero(w["obs"]["kf_idx"] >= 0)[0]
    dup = w["obs"][rng.choice(opt, 40, replace=False)].copy()
    dup["u"] += rng.normal(0, 0.7, len(dup)); dup["v"] += rng.normal(0, 0.7, len(dup))
    obs = np.concatenate([w["obs"], dup, dup[:5]])               # some pairs three times
    cam = pkg.CameraModel(**w["camera"]); ocam = oracle.Camera(**w["camera"])
    g = gpu_handle.ba_solve_visual(cam, pkg.LocalBAConfigLM(), w["poses_cw"], w["fixed_cw"], w["points"], obs)
    o = oracle.ba_solve_dense(ocam, oracle.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], obs)
    assert g["iterations"] == o["iterations"] and abs(g["final_error"] - o["final_error"]) < 1e-8 * o["final_error"]
    assert_ba_close(g, o, POSE_TOL)


@pytest.mark.gpu
def test_ba_batch_of_one_empty_window(gpu_handle, pkg):
    """A batch holding exactly one window the reference answers None for (local_ba_lm.rs:923-925): the call returns ORBX_OK with
    ORBX_ERR_EMPTY in the window's status — [None] — as include/orbx.h says, not an error for the whole call; the
    single-window entry point keeps returning ORBX_ERR_EMPTY (None) for the same window."""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    w = pkg.synth.ba_window(5, 4, 60, pkg.BA_OBS)
    empty = dict(w); empty["obs"] = w["obs"][:0]
    assert gpu_handle.ba_solve_visual_batch(cam, cfg, [empty]) == [None]
    assert gpu_handle.ba_solve_visual_batch(cam, cfg, [empty, empty]) == [None, None]
    assert gpu_handle.ba_solve_visual(cam, cfg, empty["poses_cw"], empty["fixed_cw"], empty["points"], empty["obs"]) is None
    one = gpu_handle.ba_solve_visual_batch(cam, cfg, [w])
    s = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    assert np.array_equal(one[0]["poses_wc"], s["poses_wc"]) and np.array_equal(one[0]["points"], s["points"])


@pytest.mark.gpu
def test_ba_partitioned_without_transport_refuses(gpu_handle, pkg):
    """dist.ba_solve_partitioned(world > 1, hook=None) on a handle without an RCCL communicator must raise instead of letting every
    rank solve its own partition as if it were the whole problem; orbx_ba_has_collective reports what is installed."""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    w = pkg.synth.ba_window(5, 4, 60, pkg.BA_OBS)
    assert gpu_handle.has_collective() == 0
    with pytest.raises(RuntimeError, match="no RCCL communicator"):
        pkg.dist.ba_solve_partitioned(gpu_handle, cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"], 0, 2)
    gpu_handle.set_allreduce(lambda ptr, n, stream: None)
    assert gpu_handle.has_collective() == 2
    gpu_handle.set_allreduce(None)
    assert gpu_handle.has_collective() == 0
    # world == 1 needs no transport
    r = pkg.dist.ba_solve_partitioned(gpu_handle, cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"], 0, 1)
    assert r["iterations"] > 0
