"""The specification of triangulate_from_neighbors' pair loop (tests/triangulation_spec.py, reference
src/local_mapping/triangulation.rs:117-294, :715-850) and the scenes the GPU tests run it on (tests/triangulation_scenes.py):
known answers, branch coverage, the share of near-threshold pairs, and the invariants of the neighbour loop.  No GPU."""
import json
import os

import numpy as np
import pytest

import triangulation_scenes as G
import triangulation_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def known():
    with open(os.path.join(ROOT, "tests", "golden", "triangulation_known_answers.json")) as f:
        return json.load(f)


def test_reference_dlt_known_answer(known):
    """test_triangulate_dlt (triangulation.rs:870-891): identity pose, second pose 1 m along x, point (0, 0, 5)."""
    k = known["dlt_known_answer"]
    p = S.triangulate_dlt(np.array(k["xn1"]), np.array(k["xn2"]), np.array(k["pose1_wc"], np.float64), np.array(k["pose2_wc"], np.float64))
    assert p is not None and np.abs(p - np.array(k["point"])).max() < 1e-12
    # the same from a projection, as the reference's test builds it
    X = np.array([0.0, 0.0, 5.0])
    xn = []
    for pose in (k["pose1_wc"], k["pose2_wc"]):
        pc = S.transform_point(S.pose_inverse(pose), X)
        xn.append(np.array([pc[0] / pc[2], pc[1] / pc[2], 1.0]))
    assert np.abs(S.triangulate_dlt(xn[0], xn[1], np.array(k["pose1_wc"], np.float64), np.array(k["pose2_wc"], np.float64)) - X).max() < 1e-12


def test_golden_pairs(known):
    """One recorded pair per status and per method: the spec reproduces its recorded answers."""
    seen_s, seen_m = set(), set()
    for g in known["pairs"]:
        kp = []
        for k in ("kp1", "kp2"):
            a = np.zeros(1, G.KEYPOINT); a["x"] = g[k][0]; a["y"] = g[k][1]; a["octave"] = g[k][2]
            assert float(a["x"][0]) == g[k][0] and float(a["y"][0]) == g[k][1]          # recorded coordinates are f32 values
            kp.append(a)
        st, me, p, _ = S.triangulate_pair(g["camera"], S.default_config(), g["is_inertial"], kp[0], np.array([g["pts1"]]), [g["has1"]], g["pose1_wc"],
                                          kp[1], np.array([g["pts2"]]), [g["has2"]], g["pose2_wc"], 0, 0)
        assert (st, me) == (g["status"], g["method"])
        want = np.array(g["point"])
        assert np.linalg.norm(p - want) <= 1e-12 * max(np.linalg.norm(want), 1.0)
        seen_s.add(st)
        if st == S.CREATED:
            seen_m.add(me)
    assert seen_s == set(range(8)) and seen_m == {0, 1, 2}


def test_bad_index_and_defaults():
    sc = G.pair_scene()
    c, nb = sc["current"], sc["neighbours"][0]
    a = (sc["camera"], S.default_config(), 0, c["kp"], c["pts"], c["has"], c["pose"], nb["kp"], nb["pts"], nb["has"], nb["pose"])
    assert S.triangulate_pair(*a, len(c["kp"]), 0)[0] == S.BAD_INDEX and S.triangulate_pair(*a, 0, -1)[0] == S.BAD_INDEX
    cfg = S.default_config()                                                              # triangulation.rs:39-52
    assert (cfg["num_neighbors"], cfg["max_descriptor_dist"], cfg["max_reproj_error_mono"], cfg["max_reproj_error_stereo"], cfg["scale_ratio_factor"]) == \
        (10, 50, 5.991, 7.8, 1.5)
    assert S.min_parallax_cos(cfg, True) == np.cos(np.arccos(0.9996)) and S.min_parallax_cos(cfg, False) == np.cos(np.arccos(0.9998))


def _all_evaluations(oracle):
    """name -> [(status, method, margin)] for every scene the GPU tests use."""
    out = {}
    for name in G.FUSED_CASES:
        for inertial in (0, 1):
            out[(name, inertial)] = [(e[3], e[4], e[6]) for e in G.fused_expected(oracle, name, inertial)[3]]
    for n in G.PAIR_COUNTS:
        out[("pairs", n)] = [(e[0], e[1], e[3]) for e in G.pair_expected(n)]
    return out


def test_branch_coverage(oracle):
    """Every status 0-7 and every method occurs on the scenes of the GPU tests — in their union, and in the largest fused scene alone."""
    ev = _all_evaluations(oracle)
    cover = lambda rows: ({r[0] for r in rows}, {r[1] for r in rows if r[0] not in (S.SKIPPED, S.BAD_INDEX)})
    s_all, m_all = cover([r for rows in ev.values() for r in rows])
    assert s_all == set(range(8)) and m_all == {0, 1, 2}
    s_one, m_one = cover(ev[("t10_nodes", 0)])
    assert s_one == set(range(8)) and m_one == {0, 1, 2}
    # methods among the CREATED points too, in the fused scenes taken together
    created = {r[1] for k, rows in ev.items() if k[0] != "pairs" for r in rows if r[0] == S.CREATED}
    assert created == {0, 1, 2}


def test_near_threshold_share(oracle):
    """Pairs with margin <= 1e-9 are excluded from the GPU tests' status comparison; they are at most 1 % of each scene's pairs."""
    for key, rows in _all_evaluations(oracle).items():
        near = sum(1 for r in rows if r[2] <= 1e-9)
        print(key, "pairs %d, near-threshold %d" % (len(rows), near))
        assert near <= 0.01 * len(rows), (key, near, len(rows))


@pytest.mark.parametrize("name", list(G.FUSED_CASES))
def test_neighbour_loop_invariants(oracle, name):
    sc = G.fused_scene(name)
    created, stats, res, ev = G.fused_expected(oracle, name, 0)
    T = len(sc["neighbours"])
    assert res["num_pairs_checked"] == T and res["num_new_points"] == len(created) == res["num_validated"] > 20
    keys = [(t, i1) for t, i1, _, _ in created]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)                          # neighbour, then ascending idx1
    for t in range(T):
        if t % 4 == 1:                                                                   # the 0.05 m neighbours: below the stereo baseline
            assert stats[t].tolist() == [0, 0, 0, 0]
        assert stats[t, 1] >= stats[t, 2] >= stats[t, 3]
    empty, full = G.FUSED_CASES[name].get("empty"), G.FUSED_CASES[name].get("full_mp")
    if empty is not None:
        assert stats[empty].tolist() == [0, 0, 0, 0]
    if full is not None:
        assert stats[full].tolist() == [1, 0, 0, 0]
    assert stats[:, 1].sum() == res["num_matches_found"] == len(ev) and stats[:, 3].sum() == len(created)
    # is_inertial only lowers the parallax a pair without stereo depth needs: it can only turn DLT pairs into SKIPPED ones
    ev1 = G.fused_expected(oracle, name, 1)[3]
    assert [(e[0], e[1], e[2]) for e in ev1] == [(e[0], e[1], e[2]) for e in ev]
    changed = 0
    for a, b in zip(ev, ev1):
        if (a[3], a[4]) != (b[3], b[4]):
            changed += 1
            assert b[3] == S.SKIPPED and a[4] == S.DLT and a[3] != S.SKIPPED
            c, nb = sc["current"], sc["neighbours"][a[0]]
            assert not c["has"][a[1]] and not nb["has"][a[2]]
    assert changed > 0


def test_abi_lists_the_new_entry_points(pkg):
    for name in ("orbx_default_triangulation_config", "orbx_triangulate_pairs", "orbx_triangulate_pairs_device", "orbx_keyframe_set_feature_nodes",
                 "orbx_keyframe_triangulate_from_neighbors"):
        assert name in pkg.ABI_SYMBOLS
    import ctypes as C
    from orb_slam3_rust_amd.api import _TriangulationConfig
    c = _TriangulationConfig()
    pkg.load_library().orbx_default_triangulation_config(C.byref(c))
    d = pkg.TriangulationConfig()
    for f, _ in _TriangulationConfig._fields_:
        assert getattr(c, f) == getattr(d, f) == S.default_config()[f], f
