"""orbx_ba_solve_inertial on IMU edge graphs other than an ascending chain (tests/inertial_edge_windows.py): edges listed newer -> older,
in both orientations and unsorted, a keyframe without an IMU edge, no edge at all, a second band of edges with another dt, an edge listed
twice, a keyframe without a visual observation — on the tiled LDS assembly (K = 5, 11), the one-launch global one (K = 13) and the
per-panel one (K = 22), against the CPU oracle with the tolerances of tests/test_inertial_ba.py:

- iterations equal; initial_error within 1e-10 relative; final_error within 1e-7 relative;
- poses_wc, velocities, biases and points within 1e-6 (that file's _rel: largest absolute difference over max(1, largest entry)).

Every scene is chosen by seed so that the oracle's LM decisions are 1e-7 (relative) from a tie, the rule of tests/test_orientation_gpu.py.
tests/test_inertial_edges_cpu.py shows that the oracle is invariant under the relabelling (to ~1e-11) and that an edge applied the wrong
way round or with the wrong dt moves its answer by 1e3 .. 1e6 times the tolerance here.  Every comparison prints its largest errors before
it asserts.  A self edge (ki == kj) is rejected on the host."""
import numpy as np
import pytest

import orb_slam3_rust_amd as P
import inertial_edge_windows as W

pytestmark = pytest.mark.gpu
TOL = 1e-6


def _gpu(h, w, **kw):
    return h.ba_solve_inertial(P.CameraModel(**w["camera"]), P.LocalInertialBAConfig(), w["poses_wc"], w["velocities"], w["biases"],
                               w["fixed_cw"], w["points"], w["obs"], w["edge_kf"], w["preint"], **kw)


def compare(label, g, o, rows=slice(None)):
    """g: the device's result, o: the oracle's (per-keyframe outputs cut to `rows`).  Prints the largest error of each kind, then asserts."""
    e0 = abs(g["initial_error"] - o["initial_error"]) / o["initial_error"]
    e1 = abs(g["final_error"] - o["final_error"]) / o["final_error"]
    d = {k: W.rel(g[k] if k == "points" else g[k][rows], o[k] if k == "points" else o[k][rows]) for k in W.OUTPUTS}
    print("%s: iterations %d / %d, initial_error %.3e rel, final_error %.3e rel, %s" % (label, g["iterations"], o["iterations"], e0, e1,
                                                                                        ", ".join("%s %.3e" % kv for kv in d.items())))
    assert g["iterations"] == o["iterations"]
    assert e0 < 1e-10 and e1 < 1e-7
    for k, v in d.items():
        assert v < TOL, k
    return d


def _bytes(r):
    return tuple(r[k].tobytes() for k in W.OUTPUTS)


@pytest.mark.parametrize("name,K", W.CASES)
def test_parity_with_the_oracle(gpu_handle, name, K):
    seed, w, o = W.case(name, K)
    compare("%s K=%d seed %d E=%d" % (name, K, seed, len(w["edge_kf"])), _gpu(gpu_handle, w), o)


@pytest.mark.parametrize("K", [11, 13])
def test_relabelling_the_keyframes_relabels_the_result(gpu_handle, K):
    """The descending window's result, mapped back, against the ascending window of the same seed, device against device (K = 11: the
    tiled assembly, K = 13: the global one).  Each is within 1e-6 of its own oracle and the two oracles within `spread` of each other
    (tests/test_inertial_edges_cpu.py), so the bound is 2e-6 + spread: nothing new is measured, the oracle drops out."""
    seed, spread = W.relabel_spread("descending", K)
    _, w, _ = W.case("descending", K)
    wc, _ = W.solved("chain", seed, K, W.POINTS[K])
    g, gc = W.map_back(_gpu(gpu_handle, w), W.permutation("descending", K)), _gpu(gpu_handle, wc)
    d = {k: W.rel(g[k], gc[k]) for k in W.OUTPUTS}
    print("descending against chain, K=%d seed %d: %s (oracle spread %.3e)" % (K, seed, ", ".join("%s %.3e" % kv for kv in d.items()), spread))
    assert g["iterations"] == gc["iterations"]
    assert all(v < 2 * TOL + spread for v in d.values()), d


def test_tiled_and_global_assembly_agree_off_the_chain(gpu_handle):
    """One edge graph (mixed orientations, unsorted) through both assemblies: the shuffled window at K = 11 (tiled, in LDS) and the same
    window with a twelfth keyframe that has no edge and no observation (global; its 15 rows carry only the damping and give a zero step).
    The first 11 keyframes and all points of each against its own oracle; then the two device results against each other within
    2e-6 + the spread of the two oracles."""
    seed, (w11, o11), (w12, o12) = W.padded_pair()
    g11 = _gpu(gpu_handle, w11)
    g12 = _gpu(gpu_handle, w12)
    compare("shuffled K=11 (tiled) seed %d" % seed, g11, o11)
    compare("shuffled K=11 padded to 12 (global) seed %d" % seed, g12, o12, slice(0, 11))
    spread = max(W.rel(o12[k] if k == "points" else o12[k][:11], o11[k]) for k in W.OUTPUTS)
    d = {k: W.rel(g12[k] if k == "points" else g12[k][:11], g11[k]) for k in W.OUTPUTS}
    print("global against tiled: %s (oracle spread %.3e)" % (", ".join("%s %.3e" % kv for kv in d.items()), spread))
    assert all(v < 2 * TOL + spread for v in d.values()), d
    # the padding keyframe: no term touches it
    assert W.rel(g12["poses_wc"][11], w12["poses_wc"][11]) < 1e-12 and np.array_equal(g12["velocities"][11], w12["velocities"][11])
    assert np.array_equal(g12["biases"][11], w12["biases"][11])


@pytest.mark.parametrize("K", [11, 13])
def test_an_unsorted_edge_list_solves_to_the_same_bytes_twice(gpu_handle, K):
    """fixed-order reductions, where the order of the edge list is not the order of the keyframes"""
    _, w, _ = W.case("shuffled", K)
    a = _gpu(gpu_handle, w); b = _gpu(gpu_handle, w)
    assert (a["iterations"], a["initial_error"], a["final_error"]) == (b["iterations"], b["initial_error"], b["final_error"])
    assert _bytes(a) == _bytes(b)


def _keyed_problem(w, kf_ids):
    """the InertialBAProblemData of window `w` whose keyframe i has the id kf_ids[i]"""
    mp_ids = [9000 + 2 * j for j in range(len(w["points"]))]
    obs = [P.InertialVisualObs(kf_ids[o["kf_idx"]] if o["kf_idx"] >= 0 else 7, mp_ids[o["mp_idx"]], (o["u"], o["v"]), bool(o["_pad"] & 1),
                               o["kf_idx"] >= 0) for o in w["obs"]]
    edges = [P.ImuEdgeData(kf_ids[i], kf_ids[j], w["preint"][e]) for e, (i, j) in enumerate(w["edge_kf"])]
    return P.InertialBAProblemData({k: w["poses_wc"][i] for i, k in enumerate(kf_ids)}, {k: w["velocities"][i] for i, k in enumerate(kf_ids)},
                                   {k: w["biases"][i] for i, k in enumerate(kf_ids)}, {m: w["points"][j] for j, m in enumerate(mp_ids)},
                                   {7: w["fixed_cw"][0]}, obs, edges, list(kf_ids), mp_ids), mp_ids


def test_keyed_entry_with_the_window_listed_newest_first(gpu_handle):
    """solve_inertial_ba with opt_kf_ids newest-first and every ImuEdgeData (older id, newer id): the edges map to (k + 1, k), the
    results come back under the right ids, and the keyframe not reported is opt_kf_ids[0] — here the newest."""
    K = 5
    seed, w, o = W.case("descending", K)
    perm = W.permutation("descending", K)
    kf_ids = [500 + 11 * int(k) for k in perm]                                   # a later keyframe has the larger id; keyframe i of `w` is the generator's perm[i]
    assert kf_ids == sorted(kf_ids, reverse=True)
    prob, mp_ids = _keyed_problem(w, kf_ids)
    assert all(e.kf_i_id < e.kf_j_id for e in prob.imu_edges) and len(prob.imu_edges) == K - 1
    r = P.solve_inertial_ba(prob, P.CameraModel(**w["camera"]), P.LocalInertialBAConfig(), lambda: False, handle=gpu_handle)
    assert set(r.optimized_poses) == set(r.optimized_velocities) == set(r.optimized_biases) == set(kf_ids[1:])
    assert max(kf_ids) not in r.optimized_poses and set(r.optimized_points) == set(mp_ids)
    g = dict(poses_wc=np.array([r.optimized_poses[k] for k in kf_ids[1:]]), velocities=np.array([r.optimized_velocities[k] for k in kf_ids[1:]]),
             biases=np.array([r.optimized_biases[k] for k in kf_ids[1:]]), points=np.array([r.optimized_points[m] for m in mp_ids]),
             iterations=r.iterations, initial_error=r.initial_error, final_error=r.final_error)
    o1 = dict(o); o1.update({k: o[k][1:] for k in ("poses_wc", "velocities", "biases")})
    compare("keyed, newest first, K=%d seed %d" % (K, seed), g, o1)


def test_a_self_edge_is_rejected_on_the_host(gpu_handle):
    """An IMU edge with ki == kj: several entries of its 18 x 18 record would fall on one entry of the system, so the flat call
    and the keyed call refuse it, naming the edge and the keyframe, before anything is enqueued — and the next valid solve on the handle
    gives the bytes of the solve before (the pattern of test_gpu_inertial_ba_failed_call_leaves_no_copy_of_caller_memory_in_flight: the
    page-locked observations are scribbled over the moment the failed call is back).  The debug residual entry assembles nothing and
    keeps taking such an edge."""
    w = P.Handle.pack_ba_windows([W.case("shuffled", 5)[1]])[0]
    ref = _gpu(gpu_handle, w)
    keep = w["obs"].copy()
    bad = dict(w); bad["edge_kf"] = w["edge_kf"].copy(); bad["edge_kf"][2] = (3, 3)
    with pytest.raises(P.OrbxError) as e:
        _gpu(gpu_handle, bad)
    assert "IMU edge 2: both ends are keyframe 3" in str(e.value)
    w["obs"]["u"][:] = -1.0e9; w["obs"]["mp_idx"][:] = 0                       # reuse at once
    w["obs"][:] = keep
    kf_ids = [40 + 3 * k for k in range(5)]
    prob, _ = _keyed_problem(w, kf_ids)
    prob.imu_edges.insert(1, P.ImuEdgeData(kf_ids[4], kf_ids[4], w["preint"][0]))
    with pytest.raises(P.OrbxError) as e:
        P.solve_inertial_ba(prob, P.CameraModel(**w["camera"]), P.LocalInertialBAConfig(), lambda: False, handle=gpu_handle)
    assert "IMU edge 1: both ends are keyframe 4" in str(e.value)
    again = _gpu(gpu_handle, w)
    assert again["iterations"] == ref["iterations"] and _bytes(again) == _bytes(ref)
    r = gpu_handle.debug_imu_residual(w["poses_wc"], w["velocities"], [[3, 3]], w["preint"][:1])
    assert r.shape == (1, 9) and np.all(np.isfinite(r))
