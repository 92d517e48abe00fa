"""The inertial-BA windows of tests/inertial_edge_windows.py on the CPU oracle: a seed with decision margins exists for every (case, K)
that tests/test_inertial_edges_gpu.py solves; every case has the structure its name promises; relabelling the keyframes is a symmetry of
the oracle (so the GPU comparison of a relabelled window measures the kernels, not the oracle); applying an edge the wrong way round or
with the wrong dt moves the oracle's answer by far more than the GPU tolerance (so that comparison can see such a bug); and the
preintegration skip_edge builds is consistent with the ground truth.  No GPU."""
import numpy as np
import pytest

from oracle import oracle as O
import orientation_cases as C
import inertial_edge_windows as W

GPU_TOL = 1e-6                      # tests/test_inertial_ba.py's TOL


def _degree(w):
    return np.bincount(w["edge_kf"].reshape(-1), minlength=len(w["poses_wc"]))


@pytest.mark.parametrize("name,K", W.CASES)
def test_every_case_has_a_seed_with_margins_and_the_structure_of_its_name(name, K):
    seed, w, o = W.case(name, K)
    print("%s K=%d: seed %d, lm margin %.3e, %d iterations, |r|^2 %.4f -> %.4f, %d edges, %d observations"
          % (name, K, seed, C.lm_margin(o["trace"]), o["iterations"], o["initial_error"], o["final_error"], len(w["edge_kf"]), len(w["obs"])))
    ek = w["edge_kf"]
    assert ek.dtype == np.int32 and ek.shape == (len(w["preint"]), 2) and w["preint"].shape[1:] == (11,)
    assert len(ek) == 0 or (ek.min() >= 0 and ek.max() < K and np.all(ek[:, 0] != ek[:, 1]))
    assert 1 <= o["iterations"] <= 10 and o["final_error"] < o["initial_error"]
    if name.startswith("descending"):
        assert np.all(ek[:, 0] > ek[:, 1])
    if name == "descending":
        assert np.array_equal(ek, np.array([(k + 1, k) for k in range(K - 1)])[::-1])
    if name == "shuffled":
        assert np.any(ek[:, 0] > ek[:, 1]) and np.any(ek[:, 0] < ek[:, 1])
        assert not np.array_equal(ek, ek[np.lexsort((ek[:, 1], ek[:, 0]))]) and len(ek) == K - 1 and np.all(_degree(w)[_degree(w) != 2] == 1)
    if name == "gap":
        assert _degree(w)[0] == 0 and len(ek) == K - 3
    if name == "no_edges":
        assert len(ek) == 0 and w["preint"].shape == (0, 11)
    if name in ("skip", "descending_skip_gap"):
        assert sorted(np.unique(w["preint"][:, 10]).tolist()) == [0.25, 0.5]
    if name == "skip":
        assert _degree(w).max() >= 4 and len(ek) == (K - 1) + (K - 1) // 2
    if name == "descending_skip_gap":
        assert len(ek) == (K - 1) + (K - 1) // 2 - 1
    if name == "duplicate":
        assert len(ek) == K and np.array_equal(ek[-1], ek[1]) and np.array_equal(w["preint"][-1], w["preint"][1])
    if name == "blind":
        assert np.count_nonzero(w["obs"]["kf_idx"] == 2) == 0 and all(np.count_nonzero(w["obs"]["kf_idx"] == k) > 0 for k in range(K) if k != 2)
    else:
        assert all(np.count_nonzero(w["obs"]["kf_idx"] == k) > 0 for k in range(K))


@pytest.mark.parametrize("name,K", [("descending", 5), ("shuffled", 5), ("descending", 11), ("shuffled", 11), ("descending", 13)])
def test_relabelling_is_a_symmetry_of_the_oracle(name, K):
    """The relabelled window's result, mapped back, is the chain's: the spread between the two oracle runs (dense LU of the same system
    with its rows and columns permuted, the observations summed in the same order) is rounding."""
    seed, spread = W.relabel_spread(name, K)
    _, oc = W.solved("chain", seed, K, W.POINTS[K])
    print("%s K=%d seed %d: oracle relabel spread %.3e, chain margin %.3e" % (name, K, seed, spread, C.lm_margin(oc["trace"])))
    assert spread < 1e-9
    assert C.lm_margin(oc["trace"]) >= 0.99 * W.MARGIN          # the chain of the seed is as far from a tie as its relabelling


def test_relabel_moves_labels_only():
    w = W.build("chain", 31, 5, 60)
    perm = np.array([3, 0, 4, 1, 2])
    r = W.relabel(w, perm)
    assert np.array_equal(r["poses_wc"], w["poses_wc"][perm]) and np.array_equal(r["gt_velocities"], w["gt_velocities"][perm])
    assert np.array_equal(perm[r["edge_kf"]], w["edge_kf"]) and np.array_equal(r["preint"], w["preint"])
    opt = w["obs"]["kf_idx"] >= 0
    assert np.array_equal(perm[r["obs"]["kf_idx"][opt]], w["obs"]["kf_idx"][opt]) and np.array_equal(r["obs"]["kf_idx"][~opt], w["obs"]["kf_idx"][~opt])
    for f in ("fixed_idx", "mp_idx", "u", "v", "_pad"):
        assert np.array_equal(r["obs"][f], w["obs"][f])
    back = W.relabel(r, np.argsort(perm))
    assert all(np.array_equal(back[k], w[k]) for k in ("poses_wc", "velocities", "biases", "edge_kf")) and back["obs"].tobytes() == w["obs"].tobytes()
    assert np.array_equal(w["edge_kf"], [(k, k + 1) for k in range(4)])        # the input is not written to


def _moved(label, o_wrong, o_right):
    d = {k: W.rel(o_wrong[k], o_right[k]) for k in W.OUTPUTS}
    print("%s: the oracle's answer moves by %s (x tolerance: %s)" % (label, ", ".join("%s %.3e" % kv for kv in d.items()),
                                                                    ", ".join("%.1e" % (v / GPU_TOL) for v in d.values())))
    return d


def test_a_reversed_edge_and_a_wrong_dt_move_the_answer_far_beyond_the_gpu_tolerance():
    """What a kernel that applied an edge the wrong way round would compute: the descending window with the two columns of edge_kf swapped
    and nothing relabelled.  And what one that took one dt for every edge would: a skip edge's dt of 0.5 replaced by 0.25.  The GPU
    comparison asserts poses_wc and velocities each within 1e-6 (rel): it sees the bug if EITHER moves, and the assertion here is that the
    larger of the two moves by more than 1000 x that tolerance.  Measured (rel; every figure is printed):
      reversed edges:  velocities 1.557 (1.6e6 x), poses_wc 9.77e-4 (977 x; 3.6e-3 as relative translation per pose), points 1.09e-3,
                       biases 0 (the random walk is symmetric in its two ends and the IMU rows have no bias column);
      dt 0.5 -> 0.25:  velocities 1.593, poses_wc 1.92e-2, points 2.16e-2.
    Reversing every edge leaves the cost of the visual terms almost where it was (final |r|^2 21.00727 against 21.00725): it is the
    velocities, which only the IMU rows hold, that it moves by more than their own size."""
    _, w, o = W.case("descending", 5)
    bad = dict(w); bad["edge_kf"] = w["edge_kf"][:, ::-1].copy()
    d = _moved("descending K=5, every edge reversed", W.oracle(bad), o)
    assert max(d["poses_wc"], d["velocities"]) > 1000 * GPU_TOL
    _, w, o = W.case("skip", 5)
    e = int(np.flatnonzero(w["preint"][:, 10] == 0.5)[0])
    bad = dict(w); bad["preint"] = w["preint"].copy(); bad["preint"][e, 10] = 0.25
    d = _moved("skip K=5, dt of edge %d taken as 0.25" % e, W.oracle(bad), o)
    assert min(d["poses_wc"], d["velocities"]) > 1000 * GPU_TOL


def test_skip_edge_is_consistent_with_the_ground_truth():
    """at the ground-truth states and without noise the velocity and position blocks of the residual of a skip edge vanish (the closed form of
    tests/test_inertial_ba.py); the rotation block too"""
    w = W.build("chain", 31, 6, 30)
    for i, j in ((0, 2), (1, 4), (0, 5)):
        s = W.skip_edge(w, i, j)
        assert np.array_equal(s["edge_kf"][-1], (i, j)) and s["preint"][-1, 10] == (j - i) * 0.25 and len(s["edge_kf"]) == len(w["edge_kf"]) + 1
        st = [np.concatenate([O.se3_to_params(w["gt_poses_wc"][k]), w["gt_velocities"][k]]) for k in (i, j)]
        r = O.inertial_imu_residual(st[0], st[1], s["preint"][-1])
        assert np.abs(r[3:]).max() < 1e-12 and np.abs(r[:3]).max() < 1e-12, (i, j, r)
        n = W.skip_edge(w, i, j, np.random.default_rng(1))
        rn = O.inertial_imu_residual(st[0], st[1], n["preint"][-1])
        assert 1e-5 < np.abs(rn).max() < 3e-2                     # noise of the generator's magnitudes


def test_the_padded_pair_shares_its_edge_graph():
    seed, (w11, o11), (w12, o12) = W.padded_pair()
    print("padded pair: seed %d, margins %.3e (K=11) %.3e (K=12)" % (seed, C.lm_margin(o11["trace"]), C.lm_margin(o12["trace"])))
    assert np.array_equal(w12["edge_kf"], w11["edge_kf"]) and w12["obs"].tobytes() == w11["obs"].tobytes() and len(w12["poses_wc"]) == 12
    assert 11 not in w12["edge_kf"] and 11 not in w12["obs"]["kf_idx"]
    # the padding keyframe does not move, and the others end where they end without it (to the oracle's rounding: print it)
    # (its pose goes through the scaled axis and back: rounding of a unit quaternion and a ~1 m translation)
    assert np.abs(o12["poses_wc"][11] - w12["poses_wc"][11]).max() < 1e-12 and np.array_equal(o12["velocities"][11], w12["velocities"][11])
    d = max(W.rel(o12[k][:11], o11[k]) for k in ("poses_wc", "velocities", "biases"))
    print("padded pair: oracle K=12 vs K=11 on the shared keyframes %.3e" % d)
    assert o12["iterations"] == o11["iterations"] and d < 1e-9
