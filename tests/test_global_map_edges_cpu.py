"""The maps of tests/global_map_edge_cases.py on the CPU: conditions on the REFERENCE alone (the oracle's global_ba_solve_schur), checked
without the code under test.  They are what lets tests/test_global_map_edges_gpu.py demand equal iteration counts at the project's
tolerances, unchanged: each map has the structure it exists for, every accept / reject decision of the reference up to the case's
iteration limit is at least 1e-3 (relative) from a tie and the limit is the largest such one, and every stop is pinned with a factor of
2: with the tolerance halved the reference stops in the same iteration for the same reason, with it doubled not before.

Measured (N observations, lists = observations per optimised keyframe, decisions A = accepted, r = rejected, g / p = ended by the
gradient / parameter rule, margin = smallest |trial - current| / current over the decisions, next = the margin of the decision one past
the limit, spread = the reference against itself with the observation array reversed or regrouped by keyframe, poses and points):

case          K   n    M     N     lists      limit  decisions   margin   next     spread
dense         12  72   1200  7989  575..649   3      AAA         3.5e-03  1.6e-05  1.4e-13
edges         40  240  1500  5456  0..174     6      AAAAAA      1.9e-03  1.8e-04  5.1e-10   (the same row for each of the three input orders)
edges_plain   40  240  1500  5456  0..174     6      AAAAAA      6.0e-03  7.5e-04  9.0e-10
loop          40  240  820   1484  18..61     10     AArrrAAArA  9.1e-02  -        1.0e-11
converged     20  120  600   696   23..44     10     g           -        -        0         |g| 4.8e-09, error 1.2e-13 px
gtol_stop     12  72   1200  8535  617..692   10     AAAg        6.0e-01  -        9.6e-14   |g| 6.7e+02 < 2.3e+03; 7.9e+03 the iteration before
ptol_stop     12  72   1200  8535  617..692   10     AAAp        6.0e-01  -        9.6e-14   |delta| 5.0e-03; 6.4e-02 the iteration before
natural_stop  12  72   1200  8535  617..692   10     AAAAp       1.1e-02  -        4.0e-13   |delta| 6.4e-05; 5.0e-03 the iteration before

dense: the list lengths take 10 different values modulo 64 (9 to 63) and 9 to 11 chunks of 64.  edges: keyframes 0, 17 and 39 empty,
keyframe 5 one observation and keyframe 6 two, 60 duplicated pairs of which 8 are triples, 30 identity observations, 416 unobserved
points, 12 points behind their cameras (52 observations at depths of -11.0 to -7.7 m).  loop: the 16 blocks (36..39) x (0..3) are
coupled, 517 of the 780 pairs are not.  The identity rows rewritten as observations of a second fixed keyframe at the identity: the
same bits from the reference's global and local forms.  An oracle solve takes 0.02 to 0.1 s.

What did not serve: global_k20 for the stop rules (see global_map_edge_cases.STOP: the reference's own answer moves by 3e-6 to 3e-5 with
the input order once it converges), and the banded generator's seed 1 for loop (4e-7 after 10 iterations; seed 2 gives 1e-11).
"""
import numpy as np
import pytest

import covis_windows as W
import global_map_edge_cases as E
from large_ba_windows import kf_obs
from orientation_cases import lm_margin

MARGIN = 1e-3                                             # tests/test_global_map_cpu.py
POSE_TOL = 1e-6                                           # tests/test_global_map_gpu.py


def _decisions(o, rule=None):
    return "".join(("A" if t[3] < t[0] else "r") if t[3] > 0 else (rule or "?")[0] for t in o["trace"])


def _row(name, tag, w, o, extra=""):
    d = kf_obs(w)
    K = len(w["poses_cw"])
    m = lm_margin(o["trace"])
    print("%-13s K %d  n %d  M %d  N %d  lists %d..%d  limit %d  decisions %s  margin %s  %s" % (
        tag, K, 6 * K, len(w["points"]), len(w["obs"]), d.min(), d.max(), E.config(name)["max_iterations"], _decisions(o, E.STOP.get(name, ("?",))[0]),
        "%.1e" % m if np.isfinite(m) else "-", extra))


# ---- the structure each case exists for -----------------------------------------------------------------------------------------------------
def test_dense_lists():
    w = E.case("dense")
    d = kf_obs(w)
    print("dense: lists %s, modulo 64 %s" % (sorted(d), sorted(d % 64)))
    assert len(w["poses_cw"]) == 12 and len(w["fixed_cw"]) == 1
    assert d.min() > 512                                  # the 256-stride loop of gba_kforder_kernel: three trips in every keyframe
    assert len(set(d % 64)) >= 6 and 0 not in set(d % 64)  # the last 64-entry chunk of gba_kf_schur_kernel is short, differently per keyframe
    assert len(set(-(-d // 64))) >= 2                     # and the number of chunks differs


def test_edges_structure():
    seen = {}
    for order in E.EDGE_ORDERS:
        w = E.case("edges", order)
        o = w["obs"]; s = W.stats(w); d = s["kf_obs"]
        assert len(w["poses_cw"]) == 40 and len(w["fixed_cw"]) == 1 and len(w["points"]) == 1500
        assert list(np.flatnonzero(d == 0)) == [0, 17, 39] and d[5] == 1 and d[6] == 2
        opt = o[o["kf_idx"] >= 0]
        n_per_pair = np.unique(opt["mp_idx"].astype(np.int64) * 40 + opt["kf_idx"], return_counts=True)[1]
        assert (n_per_pair >= 2).sum() >= 60 and (n_per_pair == 3).sum() >= 4 and n_per_pair.max() == 3
        assert E.is_identity(o).sum() == 30 == s["identity_obs"]
        assert np.all(o["fixed_idx"][(o["kf_idx"] < 0) & ~E.is_identity(o)] == 0)
        assert len(w["unobserved"]) >= 100
        depth = E.behind_depths(w)
        assert len(w["behind"]) == 12 and len(depth) >= 12 and depth.max() < -1.0
        seen[order] = (len(o), (n_per_pair >= 2).sum(), (n_per_pair == 3).sum(), len(w["unobserved"]), len(depth), depth.min(), depth.max())
    print("edges: N %d, duplicated pairs %d of which triples %d, unobserved points %d, observations of points behind %d at depths %.1f to %.1f m" % seen["shuffled"])
    assert len(set(seen.values())) == 1                   # the orders hold the same observations ...
    a, b, c = (E.case("edges", order)["obs"] for order in E.EDGE_ORDERS)
    assert a.tobytes() != b.tobytes() and a.tobytes() != c.tobytes() and np.array_equal(np.sort(a, order=list(a.dtype.names)), np.sort(b, order=list(b.dtype.names)))
    assert np.array_equal(a[::-1], c)                     # ... and "reversed" is the shuffled array back to front
    # some duplicates of one pair are far apart in the shuffled array, and the identity rows are scattered through it
    assert np.ptp(np.flatnonzero(E.is_identity(a))) > len(a) // 2
    p = E.case("edges_plain")
    assert len(p["behind"]) == 0 and p["obs"].tobytes() == a.tobytes()


def test_loop_blocks():
    w = E.case("loop")
    pairs = E.shared_point_pairs(w)
    K = len(w["poses_cw"])
    assert K == 40 and len(w["loop_points"]) == E.LOOP_POINTS
    near, far = E.LOOP_KEYFRAMES[:4], E.LOOP_KEYFRAMES[4:]
    assert pairs[np.ix_(far, near)].all()                 # the far corner of the reduced system
    zero = ~pairs[np.tril_indices(K, -1)]
    print("loop: %d of the %d keyframe pairs share no point" % (zero.sum(), len(zero)))
    assert not pairs[20, 0] and not pairs[35, 4] and not pairs[36, 4] and zero.sum() > len(zero) // 2      # neither all pairs ...
    band = max(abs(i - j) for i in range(K) for j in range(K) if pairs[i, j] and not (min(i, j) in near and max(i, j) in far))
    assert band < 20                                      # ... nor a band: without the loop points no pair is further apart than this
    # only the loop keyframes observe the loop points
    o = w["obs"][np.isin(w["obs"]["mp_idx"], w["loop_points"])]
    assert set(o["kf_idx"]) == set(E.LOOP_KEYFRAMES) and len(o) == 8 * E.LOOP_POINTS
    d = E.behind_depths(w)
    assert len(w["behind"]) == 6 and len(d) >= 6 and d.max() < -1.0


# ---- the LM decisions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", [(n, "shuffled") for n in E.CASES] + [("edges", o) for o in E.EDGE_ORDERS[1:]])
def test_reference_decisions_are_far_from_a_tie(oracle, name, order):
    w = E.case(name, order)
    limit = E.config(name)["max_iterations"]
    o = E.oracle_answer(oracle, name, order)
    margin = lm_margin(o["trace"])
    nxt = ""
    assert 3 <= limit <= 10
    if name in E.STOP:
        assert o["iterations"] == E.STOP[name][1] <= limit
    else:
        assert o["iterations"] == limit and np.all(o["trace"][:, 3] > 0)         # `limit` decisions, none skipped by a stop rule
        assert "A" in _decisions(o) and o["final_error"] < o["initial_error"]
    if limit < 10:                                        # the largest limit: the next decision is nearer a tie than MARGIN
        more = E.oracle_answer(oracle, name, order, max_iterations=limit + 1)
        assert more["iterations"] == limit + 1 and np.array_equal(more["trace"][:limit], o["trace"])
        t = more["trace"][limit]
        assert t[3] > 0 and abs(t[3] - t[0]) / t[0] < MARGIN
        nxt = "next %.1e" % (abs(t[3] - t[0]) / t[0])
    _row(name, name if order == "shuffled" else name + "/" + order, w, o, nxt)
    assert margin >= MARGIN
    # what must come back as it went in does so in the reference
    assert np.array_equal(o["points"][w["behind"]], w["points"][w["behind"]]) and np.array_equal(o["points"][w["unobserved"]], w["points"][w["unobserved"]])
    if name == "edges":
        assert W.rel(o["poses_wc"][[0, 17, 39]], E.poses_wc(w["poses_cw"][[0, 17, 39]])) < 1e-12
        moved = np.setdiff1d(np.arange(40), [0, 17, 39])
        assert min(max(W.pose_errors(o["poses_wc"][k:k + 1], E.poses_wc(w["poses_cw"][k:k + 1]))) for k in moved) > 1e-5


@pytest.mark.parametrize("name", list(E.CASES))
def test_reference_pins_the_answer_whatever_the_input_order(oracle, name):
    """the reference against itself on the array reversed and regrouped by keyframe: 50 times its own spread stays below the 1e-6 that
    the GPU tests hold the kernels to (tests/test_ba_covis_cpu.py's rule), at equal iteration counts"""
    a = E.oracle_answer(oracle, name)
    worst = 0.0
    for order in E.EDGE_ORDERS[1:]:
        b = E.oracle_answer(oracle, name, order)
        assert a["iterations"] == b["iterations"]
        worst = max(worst, W.rel(a["poses_wc"], b["poses_wc"]), W.rel(a["points"], b["points"]))
    print("%s: the reference against itself across input orders: %.2e" % (name, worst))
    assert 50.0 * worst <= POSE_TOL


def test_identity_observer_is_the_identity_pose(oracle):
    """on the reference: the identity rows as observations of a second fixed keyframe that is the identity pose give the same answer,
    through the global form and (no point is behind a camera in edges_plain) through the local one; without them the answer is another"""
    w = E.case("edges_plain"); c = E.config("edges_plain")
    a = E.oracle_answer(oracle, "edges_plain")
    w2 = E.identity_as_second_fixed(w)
    assert len(w2["fixed_cw"]) == 2 and (w2["obs"]["fixed_idx"] == 1).sum() == 30 and not E.is_identity(w2["obs"]).any()
    cfg = oracle.BaConfig(c["max_iterations"], c["param_tolerance"], c["gradient_tolerance"], E.HUBER, 0)
    cam = oracle.Camera(**w["camera"])
    g2 = oracle.global_ba_solve_schur(cam, cfg, w2["poses_cw"], w2["fixed_cw"], w2["points"], w2["obs"])
    l2 = oracle.ba_solve_schur(cam, cfg, w2["poses_cw"], w2["fixed_cw"], w2["points"], w2["obs"])
    for tag, b in (("global form, F = 2", g2), ("local form, F = 2", l2)):
        d = max(W.rel(a["poses_wc"], b["poses_wc"]), W.rel(a["points"], b["points"]))
        print("identity observer: %s against the identity rows: %.2e, margin %.1e" % (tag, d, lm_margin(b["trace"])))
        assert a["iterations"] == b["iterations"] == c["max_iterations"] and d < 1e-9 and lm_margin(b["trace"]) >= MARGIN
    w3 = dict(w); w3["obs"] = w["obs"][~E.is_identity(w["obs"])]
    b = oracle.global_ba_solve_schur(cam, cfg, w3["poses_cw"], w3["fixed_cw"], w3["points"], w3["obs"])
    assert W.rel(a["points"], b["points"]) > 1e-6


# ---- the stop rules -----------------------------------------------------------------------------------------------------------------------
def _stopped(o, rule, tol):
    """the last trace row is a stop by `rule`: no trial; a gradient stop has |g| below the tolerance and no step, a parameter stop a step"""
    t = o["trace"][-1]
    if rule == "gradient":
        return t[3] == 0 and t[2] == 0 and t[1] < tol
    return t[3] == 0 and t[2] > 0


@pytest.mark.parametrize("name", list(E.STOP))
def test_stop_is_pinned_with_a_factor_of_two(oracle, name):
    rule, j = E.STOP[name]
    c = E.config(name)
    field = "gradient_tolerance" if rule == "gradient" else "param_tolerance"
    tol = c[field]
    o = E.oracle_answer(oracle, name)
    half = E.oracle_answer(oracle, name, **{field: tol / 2})
    twice = E.oracle_answer(oracle, name, **{field: 2 * tol})
    t = o["trace"][-1]
    print("%s: %s rule in iteration %d at tolerance %.1e: |g| %.2e, |delta| %.2e; the iteration before |g| %.2e, |delta| %.2e; error %.3e -> %.3e px" % (
        name, rule, o["iterations"], tol, t[1], t[2], o["trace"][-2][1] if j > 1 else np.nan, o["trace"][-2][2] if j > 1 else np.nan, o["initial_error"], o["final_error"]))
    assert o["iterations"] == j and _stopped(o, rule, tol) and np.all(o["trace"][:-1, 3] > 0)
    assert half["iterations"] == j and _stopped(half, rule, tol / 2) and np.all(half["trace"][:-1, 3] > 0)
    assert twice["iterations"] >= j and np.all(twice["trace"][:j - 1, 3] > 0)                  # no stop before iteration j
    assert j < c["max_iterations"]                                                             # a stop rule, not the limit, ends the run
    if name == "converged":
        assert t[1] < 1e-2 * tol and o["initial_error"] < 1e-12 and o["final_error"] == o["initial_error"]


def test_each_rule_stops_in_mid_course_and_one_at_once():
    assert any(r == "gradient" and j > 1 for r, j in E.STOP.values()) and any(r == "param" and j > 1 for r, j in E.STOP.values())
    assert any(j == 1 for r, j in E.STOP.values())
    assert all(1 <= j <= 9 for r, j in E.STOP.values())
