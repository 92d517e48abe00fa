"""GPU tests of the whole-map global BA (orbx_ba_solve_global_map[_obs32[_device]], csrc/global_ba_kernels.hip) on the maps of
tests/global_map_edge_cases.py: keyframe lists of 575 to 649 observations, keyframes with no, one and two observations, observations by
the identity pose in both wire formats, (keyframe, point) pairs observed two and three times, a reduced system with a far corner, the
three input orders, runs that the gradient and the parameter rule end, and a stop requested while the enqueued iterations drain.
tests/test_global_map_edges_cpu.py proves on the reference alone that every case pins its answer, so the tolerances are the project's
own, unchanged (tests/test_global_map_gpu.py): iterations equal, initial_error 1e-12, final_error 1e-8, poses and points 1e-6 and
tests/test_global_ba.py's TOL.  The one new figure is for the map that starts converged, whose errors of 1e-13 px have no meaningful
relative error: both errors below 1e-9 px, poses and points within 1e-9 of the input (four orders above the reference's own 1.2e-13,
three below a millipixel).

Measured on an MI355X (largest over the cases; the bound beside it):
- parity with the reference (dense 3 iterations, edges 6, loop 10; iteration counts equal everywhere): initial_error <= 1.4e-15 (1e-12),
  final_error <= 4.6e-11 (1e-8), poses <= 1.3e-10 and points <= 3.9e-11 (1e-6); the points behind the cameras and the unobserved points
  the same bits as the input, every other observed point moved; the three empty keyframes of edges 8.4e-18 from their input poses
  (1e-12), every other keyframe moved; a second run the same bits.
- the window solver (ba_solve_global) takes all three maps, none refused: the same iteration counts, 1.7e-13 (dense), 2.6e-10 (edges)
  and 3.5e-12 (loop) from the whole-map path (1e-6), and itself within final_error 1.4e-10, poses 3.7e-10, points 2.8e-10 of the
  reference.
- edges at keypoint precision: final_error 6.7e-11, poses 3.4e-10, points 5.2e-10; the 16-byte form from the host and from device memory
  the same bits as the 32-byte form, its identity rows kf_idx -2 and its anchor rows -1; without the identity rows another answer.
  edges_plain: poses 2.8e-10, points 5.6e-10 from the reference, and 4.7e-10 from the local solver's F = 2 form with the identity as a
  second fixed keyframe.  kf_idx -1 with fixed_idx 1 (32-byte form) and kf_idx -3 (16-byte form): refused naming the observation, the
  output arrays as they were; kf_idx -5 with fixed_idx -9: the identity row's bits.
- the three input orders of edges: within final_error 2.2e-10, poses 4.5e-10, points 5.0e-10 of the reference on the same order; across
  orders 8.4e-12; a second run of the reversed array the same bits.
- stop rules: converged 1 / 1 iterations, errors 1.4e-13 px (1e-9), poses 1.8e-16 and points 0 from the input, no entry further than
  3.6e-15 (1e-9); gtol_stop and ptol_stop 4 / 4, natural_stop 5 / 5: initial_error 2.1e-15, final_error <= 1.1e-13, poses <= 3.0e-13,
  points <= 4.6e-14.  Every stop, by either rule, gives the bits of the call limited to one iteration fewer (errors, poses, points).
- a stop requested while the 10 enqueued iterations of k129 drain: should_stop was called 11 times and the call reported r = 1; the
  reference stopped after 1 iteration agrees to the bit in poses and points and to 1.6e-16 in both errors (k129's first step is a
  rejected one; twice the same r).  global_k20 next on
  the same handle: the bits of a fresh handle.
The slowest test is the drain test, 0.45 s (it makes a second handle); every other takes 0.01 to 0.06 s once the session's handle exists.
"""
import numpy as np
import pytest

import covis_windows as W
import global_map_cases as G
import global_map_edge_cases as E
from test_global_map_gpu import PATTERN, POSE_TOL, _assert_parity, _gpu, _old_path_still_refuses_and_small_solve_succeeds, _raw, _same_bits

pytestmark = pytest.mark.gpu

EMPTY = [0, 17, 39]                                       # the keyframes of edges without an observation


def _solve(h, pkg, name, order="shuffled", **override):
    return _gpu(h, pkg, E.case(name, order), **E.config(name, **override))


def _window_solver(h, pkg, name):
    w = E.case(name)
    return h.ba_solve_global(pkg.CameraModel(**w["camera"]), pkg.GlobalBAConfig(**E.config(name)), w["poses_cw"], w["fixed_cw"][0], w["points"], w["obs"])


def _agree(a, b, tag, tol=POSE_TOL):
    d = max(W.rel(a["poses_wc"], b["poses_wc"]), W.rel(a["points"], b["points"]))
    print("%s: iterations %d / %d, poses and points %.2e" % (tag, a["iterations"], b["iterations"], d))
    assert a["iterations"] == b["iterations"] and d < tol, (tag, d)


def _assert_untouched(g, w, name):
    assert np.array_equal(g["points"][w["behind"]], w["points"][w["behind"]])                 # no Jacobian rows: no step
    assert np.array_equal(g["points"][w["unobserved"]], w["points"][w["unobserved"]])         # V = 0, g = 0: no step
    moved = np.setdiff1d(np.unique(w["obs"]["mp_idx"]), w["behind"])
    assert np.abs(g["points"][moved] - w["points"][moved]).max() > 1e-4
    if name == "edges":                                   # an empty keyframe's step is exactly zero; params -> pose rounds
        d = W.rel(np.asarray(g["poses_wc"])[EMPTY], E.poses_wc(w["poses_cw"][EMPTY]))
        print("edges: empty keyframes against their input poses %.2e" % d)
        assert d < 1e-12
        others = np.setdiff1d(np.arange(len(w["poses_cw"])), EMPTY)
        assert min(max(W.pose_errors(np.asarray(g["poses_wc"])[k:k + 1], E.poses_wc(w["poses_cw"][k:k + 1]))) for k in others) > 1e-5


# ---- 1. parity per case, 2. the window solver as a second implementation --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense", "edges", "loop"])
def test_edge_case_parity(gpu_handle, oracle, pkg, name):
    w = E.case(name)
    g = _solve(gpu_handle, pkg, name)
    _assert_parity(g, E.oracle_answer(oracle, name), "%s (limit %d)" % (name, E.config(name)["max_iterations"]))
    _assert_untouched(g, w, name)
    assert _same_bits(_solve(gpu_handle, pkg, name), g)


@pytest.mark.parametrize("name", ["dense", "edges", "loop"])
def test_window_solver_agrees(gpu_handle, oracle, pkg, name):
    """ba_solve_global (ba_kernels.hip: other lists, other Schur product, other factorisation) takes every one of these maps"""
    assert len(E.case(name)["poses_cw"]) <= 128
    g = _solve(gpu_handle, pkg, name)
    old = _window_solver(gpu_handle, pkg, name)
    _agree(g, old, "%s: whole-map path against the window solver" % name)
    _assert_parity(old, E.oracle_answer(oracle, name), "%s, window solver" % name)


# ---- 3. the wire formats on edges -----------------------------------------------------------------------------------------------------------
def test_edges_wire_formats_and_the_identity_pose(gpu_handle, oracle, pkg):
    import torch
    w = pkg.synth.keypoint_precision(E.case("edges"))
    cfg_kw = E.config("edges")
    cam, cfg = pkg.CameraModel(**w["camera"]), pkg.GlobalBAConfig(**cfg_kw)
    ref = _gpu(gpu_handle, pkg, w, **cfg_kw)
    ocfg = oracle.BaConfig(cfg_kw["max_iterations"], cfg_kw["param_tolerance"], cfg_kw["gradient_tolerance"], E.HUBER, 0)
    _assert_parity(ref, oracle.global_ba_solve_schur(oracle.Camera(**w["camera"]), ocfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"]), "edges at keypoint precision")
    ident = E.is_identity(w["obs"]); anchor = (w["obs"]["kf_idx"] < 0) & ~ident
    o32 = pkg.ba_obs_to_obs32(w["obs"], 1)
    assert o32 is not None and o32.dtype == pkg.BA_OBS32 and len(o32) == len(w["obs"])
    assert ident.sum() == 30 and np.all(o32["kf_idx"][ident] == -2) and anchor.sum() > 0 and np.all(o32["kf_idx"][anchor] == -1)
    assert np.array_equal(o32["kf_idx"][~ident & ~anchor], w["obs"]["kf_idx"][~ident & ~anchor])
    assert _same_bits(gpu_handle.ba_solve_global_map_obs32(cam, cfg, w["poses_cw"], w["fixed_cw"][0], w["points"], o32), ref)
    dev = torch.from_numpy(np.ascontiguousarray(o32).view(np.uint8).copy()).cuda()
    assert _same_bits(gpu_handle.ba_solve_global_map_obs32_device(cam, cfg, w["poses_cw"], w["fixed_cw"][0], w["points"], dev, len(o32)), ref)
    # without the identity rows the answer is another one
    w3 = dict(w); w3["obs"] = w["obs"][~ident]
    assert W.rel(_gpu(gpu_handle, pkg, w3, **cfg_kw)["points"], ref["points"]) > 1e-6


def test_identity_rows_are_observations_by_the_identity_pose(gpu_handle, oracle, pkg):
    """the identity is a pose, not a slot: the same rows as observations of a second fixed keyframe that IS the identity, through the
    local window solver's F = 2 form (edges_plain: no point behind a camera, where the local and the global solver differ)"""
    w = E.case("edges_plain"); c = E.config("edges_plain")
    g = _solve(gpu_handle, pkg, "edges_plain")
    _assert_parity(g, E.oracle_answer(oracle, "edges_plain"), "edges_plain")
    w2 = E.identity_as_second_fixed(w)
    assert len(w2["fixed_cw"]) == 2 and (w2["obs"]["fixed_idx"] == 1).sum() == 30
    v = gpu_handle.ba_solve_visual(pkg.CameraModel(**w["camera"]), pkg.LocalBAConfigLM(**c), w2["poses_cw"], w2["fixed_cw"], w2["points"], w2["obs"])
    _agree(g, v, "identity rows against a second fixed keyframe at the identity (local solver, F = 2)")


def test_edges_index_rules_of_both_wire_formats(gpu_handle, pkg):
    w = pkg.synth.keypoint_precision(E.case("edges"))
    obs = np.ascontiguousarray(w["obs"], pkg.BA_OBS)
    o32 = pkg.ba_obs_to_obs32(obs, 1)
    rows = np.flatnonzero(E.is_identity(obs))
    i = int(rows[7])
    # 32-byte form: a fixed observer other than the anchor
    bad = obs.copy(); bad["kf_idx"][i] = -1; bad["fixed_idx"][i] = 1
    rc, msg, out, pts, it, e0, e1 = _raw(gpu_handle, pkg, "orbx_ba_solve_global_map", w, w["poses_cw"], w["points"], bad)
    assert rc == -1 and "observation %d" % i in msg and "out of range" in msg, msg
    assert np.all(out == PATTERN) and np.array_equal(pts, w["points"]) and it == 0
    # 16-byte form: below the identity pose's -2
    bad32 = o32.copy(); bad32["kf_idx"][i] = -3
    rc, msg, out, pts, it, e0, e1 = _raw(gpu_handle, pkg, "orbx_ba_solve_global_map_obs32", w, w["poses_cw"], w["points"], bad32)
    assert rc == -1 and "observation %d" % i in msg and "out of range" in msg, msg
    assert np.all(out == PATTERN) and np.array_equal(pts, w["points"]) and it == 0
    _old_path_still_refuses_and_small_solve_succeeds(gpu_handle, pkg)
    # 32-byte form: any two negative indices name the identity pose
    ref = _gpu(gpu_handle, pkg, w)                        # (_raw solves with the default configuration)
    other = obs.copy(); other["kf_idx"][rows] = -5; other["fixed_idx"][rows] = -9
    rc, msg, out, pts, it, e0, e1 = _raw(gpu_handle, pkg, "orbx_ba_solve_global_map", w, w["poses_cw"], w["points"], other)
    assert rc == 0, msg
    assert it == ref["iterations"] > 0 and e0 == ref["initial_error"] and e1 == ref["final_error"]
    assert out.tobytes() == np.ascontiguousarray(ref["poses_wc"]).tobytes() and pts.tobytes() == ref["points"].tobytes()


# ---- 4. input order ---------------------------------------------------------------------------------------------------------------------
def test_edges_every_input_order(gpu_handle, oracle, pkg):
    got = {}
    for order in E.EDGE_ORDERS:
        got[order] = _solve(gpu_handle, pkg, "edges", order)
        _assert_parity(got[order], E.oracle_answer(oracle, "edges", order), "edges, %s" % order)
        _assert_untouched(got[order], E.case("edges", order), "edges")
    for order in E.EDGE_ORDERS[1:]:
        _agree(got[order], got["shuffled"], "edges: %s against shuffled" % order)
    assert _same_bits(_solve(gpu_handle, pkg, "edges", "reversed"), got["reversed"])


# ---- 5. the stop rules ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.STOP))
def test_stop_rules(gpu_handle, oracle, pkg, name):
    rule, j = E.STOP[name]
    w = E.case(name)
    o = E.oracle_answer(oracle, name)
    g = _solve(gpu_handle, pkg, name)
    assert o["iterations"] == j
    if name == "converged":
        dp, dx = W.rel(g["poses_wc"], E.poses_wc(w["poses_cw"])), W.rel(g["points"], w["points"])
        da = max(np.abs(np.asarray(g["poses_wc"]) - E.poses_wc(w["poses_cw"])).max(), np.abs(g["points"] - w["points"]).max())
        print("converged: iterations %d / %d, errors %.2e and %.2e px (reference %.2e), poses %.2e, points %.2e, largest entry %.2e from the input" % (
            g["iterations"], o["iterations"], g["initial_error"], g["final_error"], o["initial_error"], dp, dx, da))
        assert g["iterations"] == 1                                                        # a gradient stop counts its iteration
        assert 0 <= g["initial_error"] < 1e-9 and 0 <= g["final_error"] < 1e-9
        assert dp < 1e-9 and dx < 1e-9 and da < 1e-9
    else:
        _assert_parity(g, o, "%s (%s rule, iteration %d)" % (name, rule, j))
    # the stop fires before any step of iteration j is applied: the result of j - 1 iterations, counted as j
    z = _solve(gpu_handle, pkg, name, max_iterations=j - 1)
    assert z["iterations"] == j - 1
    if j == 1:
        assert np.array_equal(z["points"], w["points"])
    else:
        assert np.abs(z["points"] - w["points"]).max() > 1e-4
    same = (g["initial_error"] == z["initial_error"], g["final_error"] == z["final_error"], np.asarray(g["poses_wc"]).tobytes() == np.asarray(z["poses_wc"]).tobytes(),
            g["points"].tobytes() == z["points"].tobytes())
    print("%s: against %d iterations: initial_error, final_error, poses, points the same bits: %s (final_error %.17g / %.17g)" % (name, j - 1, same, g["final_error"], z["final_error"]))
    assert all(same)


# ---- 6. a stop requested while the enqueued iterations drain --------------------------------------------------------------------------------
def test_stop_while_draining_and_the_flag_does_not_leak(gpu_handle, oracle, pkg):
    from test_global_ba import TOL, _rel
    w = G.case("k129")
    assert G.oracle_answer(oracle, "k129")["iterations"] == 10
    calls = []
    r = gpu_handle.ba_solve_global_map(pkg.CameraModel(**w["camera"]), pkg.GlobalBAConfig(), w["poses_cw"], w["fixed_cw"][0], w["points"], w["obs"],
                                       should_stop=lambda: (calls.append(1) or len(calls) > 10))
    n = r["iterations"]
    print("stop while draining: %d calls of should_stop, r = %d iterations" % (len(calls), n))
    assert len(calls) >= 10 and 1 <= n <= 10              # all 10 iterations were enqueued: the request reached the device through the flag, or too late
    o = G.oracle_answer(oracle, "k129") if n == 10 else \
        oracle.global_ba_solve_schur(oracle.Camera(**w["camera"]), G.L._gcfg(oracle), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"], stop_after=n)
    assert o["iterations"] == n
    dp, dx = _rel(r["poses_wc"], o["poses_wc"]), _rel(r["points"], o["points"])
    e0, e1 = abs(r["initial_error"] - o["initial_error"]) / o["initial_error"], abs(r["final_error"] - o["final_error"]) / o["final_error"]
    print("stop while draining: against the reference stopped after %d: poses %.2e, points %.2e, initial_error %.2e, final_error %.2e" % (n, dp, dx, e0, e1))
    assert dp < TOL and dx < TOL
    assert e0 < 1e-12 and e1 < 1e-8
    # the flag is the handle's: the next call must not see it
    small = W.covis_window(**W.GLOBAL_CASES["global_k20"])
    after = _gpu(gpu_handle, pkg, small)
    fresh = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), 600, device=0, max_w=752, max_h=480, max_batch=1)
    try:
        want = _gpu(fresh, pkg, small)
    finally:
        fresh.close()
    assert want["iterations"] == 10 and want["final_error"] < want["initial_error"]
    assert _same_bits(after, want)
