"""CPU checks around loop-candidate verification: the specification's matcher (tests/loop_verify_spec.py) against an independent
dense-table statement, its sampler, the conditions under which a scene may be compared discretely with the GPU (every scene the GPU
tests run must meet them), and the new ABI's layout, defaults and symbols."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import loop_verify_scenes as Z
import loop_verify_spec as S
import pnp_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_MARGIN, MIN_COND = 1e-6, 1e-5         # the rule for scenes compared discretely


def dense_matches(d1, d2, max_dist=50, ratio=0.7):
    """The brute-force matcher as order statistics of a uint16 distance table: best = the row minimum at its first index, second =
    the smallest value of the row with that one entry taken out (a repeated minimum is therefore the second)."""
    n1, n2 = len(d1), len(d2)
    if n1 == 0 or n2 == 0:
        return []
    table = np.unpackbits(d1[:, None, :] ^ d2[None, :, :], axis=2).sum(2).astype(np.uint16)
    out = []
    for i in range(n1):
        row = table[i]
        j = int(np.argmin(row))
        rest = np.delete(row, j)
        second = float(rest.min()) if len(rest) else float(S.U32_MAX)
        if row[j] < max_dist and float(row[j]) < ratio * second:
            out.append((i, j, int(row[j])))
    return out


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", [(0, 9), (9, 0), (1, 1), (1, 2), (15, 17), (17, 16), (257, 65), (300, 2)])
def test_spec_matcher_equals_dense_table(shape, ties):
    d1, d2 = Z.descriptor_table(1000 + shape[0] * 7 + shape[1], *shape, ties=ties)
    # a ratio of 2 lets tie rows through the ratio test as well, so that their best index and distance are compared
    for ratio, max_dist in ((0.7, 50), (2.0, 257)):
        assert S.match_features(d1, d2, max_dist=max_dist, ratio=ratio) == dense_matches(d1, d2, max_dist, ratio)


def test_spec_matcher_hand_written_ties():
    z = Z.popcount_rows
    d1 = np.stack([z(0)])
    # (loop rows' distances to the zero row) -> the match, or None
    table = [([10, 10], None),              # a repeated best is the second: 10 < 0.7 * 10 fails
             ([10, 15], (0, 0, 10)),    # 10 < 10.5
             ([15, 10], (0, 1, 10)),
             ([10, 14], None),              # 10 < 9.8 fails
             ([20, 10, 10], None),
             ([10, 20, 10], None),
             ([12, 30, 12, 5], (0, 3, 5)),  # 5 < 8.4
             ([49], (0, 0, 49)),            # a lone candidate: second stays u32::MAX
             ([50], None),                  # best < 50 is strict
             ([30, 40, 30], None)]
    for dists, want in table:
        got = S.match_features(d1, np.stack([z(k) for k in dists]))
        assert got == ([want] if want else []), (dists, got)


def test_spec_matcher_feature_vector_form():
    cases, d1, n1, d2, n2 = Z.decision_table()
    got = {i: (j, d) for i, j, d in S.match_features(d1, d2, n1, n2)}
    for i, (b, s) in enumerate(cases):
        want = b < 50 and float(b) < 0.7 * float(S.U32_MAX if s is None else s)
        assert (i in got) == want, (b, s)
        if want:
            assert got[i][1] == b and n2[got[i][0]] == i
    # a node the other keyframe lacks, and features in no list, have no match; the walk is per node in ascending index
    d = np.stack([Z.popcount_rows(0), Z.popcount_rows(3), Z.popcount_rows(3)])
    assert S.match_features(d[:1], d, np.array([7], np.uint32), np.array([7, 8, 8], np.uint32)) == [(0, 0, 0)]
    assert S.match_features(d[:1], d, np.array([9], np.uint32), np.array([7, 8, 8], np.uint32)) == []
    assert S.match_features(d[:1], d, np.array([S.NODE_NONE], np.uint32), np.array([S.NODE_NONE] * 3, np.uint32)) == []
    assert S.match_features(d[:1], d[1:], np.array([8], np.uint32), np.array([8, 8], np.uint32)) == []          # 3, 3: a tie


def _splitmix(x):
    m = (1 << 64) - 1
    z = x & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


@pytest.mark.parametrize("n", [3, 4, 15, 600])
def test_sampler_first_three_indices(n):
    for seed in (0, 12345):
        for h in (0, 1, 299):
            want = []
            for a in range(64):
                i = ((_splitmix(seed + 0x9E3779B97F4A7C15 * (h * 64 + a + 1)) >> 32) * n) >> 32
                if i not in want:
                    want.append(i)
                if len(want) == 3:
                    break
            assert pnp_spec.sample(seed, h, n, 3) == (want if len(want) == 3 else None)


def test_every_pair_scene_reaches_its_status_and_may_be_compared():
    seen = set()
    for name, (_, _, _, status) in Z.PAIRS.items():
        r = Z.pair_spec(name)
        assert r["status"] == status, name
        assert r["margin"] > MIN_MARGIN and r["cond"] > MIN_COND, (name, r["margin"], r["cond"])
        seen.add(status)
    assert seen == set(range(7))
    assert any("node" in Z.pair(n)[0] for n in Z.PAIRS) and any("node" not in Z.pair(n)[0] for n in Z.PAIRS)


def test_every_sim3_set_may_be_compared():
    for name in Z.SIM3_SETS:
        r = Z.sim3_spec(name)
        assert r["margin"] > MIN_MARGIN and r["cond"] > MIN_COND, (name, r["margin"], r["cond"])
    assert Z.sim3_spec("n2")["status"] == 1 and Z.sim3_spec("n14")["status"] == 1 and Z.sim3_spec("all_outliers")["status"] == 1
    assert Z.sim3_spec("n15_o0")["status"] == 0 and Z.sim3_spec("n300_o60")["status"] == 0


def test_reflection_set_is_one_and_spec_recovers_ground_truth():
    p1, p2, gt = Z.sim3_set("reflection")
    a, b = p1 - p1.mean(0), p2 - p2.mean(0)
    U, _, Vt = np.linalg.svd(a.T @ b)
    assert np.linalg.det(Vt.T @ U.T) < 0                    # the unrestricted orthogonal fit is a reflection
    r = Z.sim3_spec("reflection")
    assert r["status"] == 0 and abs(np.linalg.det(r["M"]) - 1.0) < 1e-12
    for name in ("n64_o30", "n300_o60", "coplanar", "free_scale"):
        p1, p2, gt = Z.sim3_set(name)
        r = Z.sim3_spec(name)
        assert r["status"] == 0 and np.abs(r["M"] - gt["scale"] * gt["R"]).max() < 0.02 and np.abs(r["t"] - gt["t"]).max() < 0.1, name


def test_known_answers_in_the_spec():
    ka = json.load(open(os.path.join(ROOT, "tests", "golden", "loop_verify_known_answers.json")))
    for case in ka["cases"]:
        p1 = np.array([[(i + case["first"]) * k for k in (1.0, 2.0, 3.0)] for i in range(10)])
        p2 = case["scale"] * p1 @ np.array(case["rotation"], np.float64).T + np.array(case["translation"], np.float64)
        R, scale, M, t, _ = S.horn(p1, p2, case["fix_scale"])
        assert abs(scale - case["scale"]) < ka["tolerance"] and np.abs(t - case["translation"]).max() < ka["tolerance"], case["name"]
        assert np.abs(p1 @ M.T + t - p2).max() < ka["tolerance"], case["name"]


# ---- the ABI ----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["orbx_default_sim3_config", "orbx_default_loop_verify_config", "orbx_sim3_ransac_batch", "orbx_sim3_ransac_batch_device",
               "orbx_verify_loop_candidates", "orbx_verify_loop_candidates_device", "orbx_keyframe_verify_loop_candidates"]


def test_new_symbols_are_exported_and_listed(pkg):
    L = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS, s


def test_struct_layouts_match_header(pkg, tmp_path):
    from orb_slam3_rust_amd.api import _LoopVerifyConfig, _Sim3Config
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(orbx_sim3_config), offsetof(orbx_sim3_config, seed), sizeof(orbx_loop_verify_config), '
                   'offsetof(orbx_loop_verify_config, match_ratio), offsetof(orbx_loop_verify_config, sim3), sizeof(orbx_sim3_result), '
                   'sizeof(orbx_loop_verify_result), offsetof(orbx_loop_verify_result, mse)); return 0; }\n')
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_Sim3Config), _Sim3Config.seed.offset, C.sizeof(_LoopVerifyConfig), _LoopVerifyConfig.match_ratio.offset,
                   _LoopVerifyConfig.sim3.offset, pkg.SIM3_RESULT.itemsize, pkg.LOOP_VERIFY_RESULT.itemsize, pkg.LOOP_VERIFY_RESULT.fields["mse"][1]]
    assert pkg.SIM3_RESULT.itemsize == 32 and pkg.LOOP_VERIFY_RESULT.itemsize == 40


def test_defaults_mirror_reference(pkg):
    from orb_slam3_rust_amd.api import _LoopVerifyConfig, _Sim3Config
    L = pkg.load_library()
    s = _Sim3Config(); L.orbx_default_sim3_config(C.byref(s))
    assert (s.max_iterations, s.inlier_threshold, s.min_inliers, s.fix_scale, s.probability, s.seed) == (300, 0.075, 15, 1, 0.99, 0)   # sim3_solver.rs:26-36
    d = pkg.Sim3SolverConfig()
    assert (d.max_iterations, d.inlier_threshold, d.min_inliers, d.fix_scale, d.probability, d.seed) == (300, 0.075, 15, True, 0.99, 0)
    c = _LoopVerifyConfig(); L.orbx_default_loop_verify_config(C.byref(c))
    assert (c.min_stereo_points, c.min_matches, c.min_pairs, c.min_inliers, c.min_verified, c.match_max_dist, c.match_ratio, c.chi2,
            c.scale_factor) == (20, 15, 15, 15, 50, 50, 0.7, 5.991, 1.2)                                                               # corrector.rs
    assert (c.sim3.max_iterations, c.sim3.fix_scale) == (300, 1)
    p = pkg.LoopVerifyConfig()._c()
    assert bytes(p) == bytes(c)
    assert {k: v for k, v in S.VERIFY_DEFAULTS.items()} == {k: getattr(pkg.LoopVerifyConfig(), k) for k in S.VERIFY_DEFAULTS}
    assert {k: v for k, v in S.SIM3_DEFAULTS.items()} == {k: getattr(d, k) for k in S.SIM3_DEFAULTS}


def test_null_handle_is_invalid(pkg):
    L = pkg.load_library()
    assert L.orbx_sim3_ransac_batch(None, None, 0, None, None, None, None, None, None) == -1
    assert L.orbx_sim3_ransac_batch_device(None, None, 0, 0, None, None, None, None, None, None) == -1
    assert L.orbx_verify_loop_candidates(*([None] * 3), 0, *([None] * 20)) == -1
    assert L.orbx_verify_loop_candidates_device(*([None] * 3), 0, *([None] * 20)) == -1
    assert L.orbx_keyframe_verify_loop_candidates(*([None] * 3), 0, *([None] * 9)) == -1
    L.orbx_default_sim3_config(None); L.orbx_default_loop_verify_config(None)          # tolerated


def test_loop_verify_driver_compiles_and_links(pkg, tmp_path):
    from test_loop_verify_cpp import _build
    pkg.load_library()
    assert os.path.exists(_build(str(tmp_path)))
