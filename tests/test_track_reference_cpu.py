"""CPU checks of tracking against the reference keyframe: the specification's matcher (tests/track_reference_spec.py) against an
independent dense-table statement, the scenes the GPU tests run (tests/track_reference_scenes.py), the new ABI
(orbx_track_ref_result, orbx_track_reference[_device], orbx_keyframe_track_reference) and the C++ mirror's driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import track_reference_scenes as R
import track_reference_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam3-rust_amd")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
SYMBOLS = ("orbx_track_reference", "orbx_track_reference_device", "orbx_keyframe_track_reference")


def build_driver(tmp):
    exe = os.path.join(tmp, "track_reference_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "track_reference_driver.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lorbx_hip", "-L", ROCM_LIB, "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ROCM_LIB], check=True)
    return exe


def _same(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("nq,nt", [(1, 1), (15, 17), (64, 300), (257, 65), (300, 2), (2, 300), (0, 9), (9, 0)])
def test_spec_matcher_equals_dense_table_on_random_rows(oracle, nq, nt):
    rng = np.random.default_rng(100 + nq + 7 * nt)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8); t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    assert _same(S.match(oracle, q, t), S.dense_match(q, t))


def test_spec_matcher_equals_dense_table_on_ties(oracle):
    """rows drawn from a few base rows: groups of equal distances in both directions; and all rows equal: the one pair (0, 0)"""
    for seed, nb, nq, nt in ((1, 8, 500, 700), (2, 3, 70, 90), (3, 2, 5, 300)):
        rng = np.random.default_rng(seed)
        base = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
        q = base[rng.integers(0, nb, nq)]; t = base[rng.integers(0, nb, nt)]
        m = S.dense_match(q, t)
        assert _same(S.match(oracle, q, t), m) and 1 <= len(m) <= nb
    s = R.identical(79)
    m = S.match(oracle, s[2], s[1])
    assert _same(m, S.dense_match(s[2], s[1])) and [(int(a), int(b), float(d)) for a, b, _, d in m.tolist()] == [(0, 0, 0.0)]


def test_hand_written_tie_table(oracle):
    """rows as sets of set bits, q = [{0}, {}, {1}, {}], t = [{0,1,2}, {3}, {}, {0,1}]; distance = size of the symmetric difference:
                 t0 t1 t2 t3
         q0       2  2  1  1     q0 -> t2 (the first of its two 1s)
         q1       3  1  0  2     q1 -> t2
         q2       2  2  1  1     q2 -> t2
         q3       3  1  0  2     q3 -> t2
       t0 -> q0 (first of q0, q2), t1 -> q1 (first of q1, q3), t2 -> q1 (first of q1, q3), t3 -> q0 (first of q0, q2).
    The only mutual pair is (q1, t2).  A matcher that let the last index win a tie would also report (q2, t3) or (q0, t3) on the
    rows' side, or (q3, t2) instead of (q1, t2) on the columns' side."""
    def row(bits):
        b = np.zeros(256, np.uint8); b[list(bits)] = 1
        return np.packbits(b)
    q = np.stack([row([0]), row([]), row([1]), row([])]); t = np.stack([row([0, 1, 2]), row([3]), row([]), row([0, 1])])
    assert S.distance_table(q, t).tolist() == [[2, 2, 1, 1], [3, 1, 0, 2], [2, 2, 1, 1], [3, 1, 0, 2]]
    for m in (S.dense_match(q, t), S.match(oracle, q, t)):
        assert m.tolist() == [(1, 2, 0, 0.0)]


def test_gather_and_finish_rules():
    kp = R.G.keypoints(np.stack([np.arange(6) * 10.0, np.arange(6) * 5.0 + 1.0], 1))
    m = np.zeros(5, S.DMATCH)
    m["query_idx"] = [0, 2, 3, 5, 6]; m["train_idx"] = [4, 1, 0, 5, 2]
    pos = np.arange(21.0).reshape(7, 3)
    valid = np.array([1, 1, 0, 1, 1, 2, 1], np.uint8)              # row 2 has no map point; any nonzero byte counts
    g = S.gather(kp, pos, valid, m)
    assert g["kf_idx"].tolist() == [0, 3, 5, 6] and g["feat_idx"].tolist() == [4, 0, 5, 2]
    assert g["points3d"].tolist() == pos[[0, 3, 5, 6]].tolist() and g["points2d"].dtype == np.float32
    assert g["points2d"].tolist() == [[40.0, 21.0], [0.0, 1.0], [50.0, 26.0], [20.0, 11.0]]
    prior = np.arange(7.0); pnp_pose = prior + 10.0
    rec, pose = S.finish(4, 5, g, prior, pnp_pose, 0, 3)
    assert rec == dict(status=S.OK, n_matches=5, n_correspondences=4, n_inliers=3) and pose.tobytes() == pnp_pose.tobytes()
    rec, pose = S.finish(5, 5, g, prior, pnp_pose, 0, 3)              # one short of the guard: the prior, no inliers reported
    assert rec == dict(status=S.TOO_FEW_CORRESPONDENCES, n_matches=5, n_correspondences=4, n_inliers=0) and pose.tobytes() == prior.tobytes()
    rec, pose = S.finish(4, 5, g, prior, prior, S.PNP_NO_MODEL, 0)    # PnP hands the prior back itself
    assert rec["status"] == S.NO_MODEL and pose.tobytes() == prior.tobytes()
    rec, _ = S.finish(4, 5, g, prior, pnp_pose, 0, 0)                 # no inlier guard on this path
    assert rec["status"] == S.OK


def test_scenes_are_what_their_names_say(oracle):
    B = R.batches()
    shapes = {name: [(len(f[2]), len(f[0])) for f in fr] for name, fr in B.items()}
    assert shapes["small"] == [(1, 1), (15, 17), (16, 256)] and shapes["thin"] == [(300, 2), (2, 300)]
    assert shapes["tile_edges"] == [(R.TILE - 1, 70), (R.TILE, 70), (R.TILE + 1, 70)]
    assert [s[0] for s in shapes["block_edges_keyframe"]] == [255, 256, 257] and [s[1] for s in shapes["block_edges_frame"]] == [255, 257]
    assert shapes["empty_sides"][:2] == [(0, 40), (40, 0)] and shapes["realistic"] == [(2000, 2000)] and shapes["ties"] == [(500, 700)]
    for fr in B.values():
        for kp, desc, kd, pos, valid, prior in fr:
            assert len(kp) == len(desc) and len(kd) == len(pos) == len(valid) and valid.dtype == np.uint8 and prior.shape == (7,)
    res = {name: S.match_and_gather(oracle, fr) for name, fr in B.items()}
    n_corr = lambda name: np.diff(res[name][0]).tolist()
    n_match = lambda name: [len(m) for m in res[name][1]]
    assert n_corr("corr_3_4") == [3, 4] and n_match("corr_3_4") == [3, 4]
    assert n_corr("empty_sides")[:2] == [0, 0] and n_match("empty_sides")[:2] == [0, 0] and n_corr("empty_sides")[2] >= 10
    assert n_match("identical") == [1] and n_corr("identical") == [1]
    assert n_corr("valid_all_zero") == [0] and n_match("valid_all_zero")[0] >= 20
    assert 1 <= n_match("ties")[0] <= 8
    assert 900 <= n_corr("realistic")[0] <= 1100 and n_match("realistic")[0] > n_corr("realistic")[0]      # 1200 map-point rows, a fifth of them holes
    a, b, c = B["b3_shared_keyframe"]
    assert a[2] is c[2] and a[3] is c[3] and a[4] is c[4] and len({len(f[0]) for f in (a, b, c)}) == 3
    assert min(n_corr("b3_shared_keyframe")) >= 30 and min(n_corr("no_model_next_to_good")) >= 15
    for name in ("small", "tile_edges", "block_edges_keyframe", "block_edges_frame", "realistic", "b3_shared_keyframe"):
        for m, g in zip(res[name][1], res[name][2]):                  # matches without a map point exist: the two compactions differ
            assert len(g["kf_idx"]) <= len(m)
    assert any(len(g["kf_idx"]) < len(m) for name in res for m, g in zip(res[name][1], res[name][2]))


def test_new_symbols_and_struct_layout(pkg, tmp_path):
    """The library exports the entry points, and orbx_track_ref_result is laid out as the numpy mirror restates it (16 bytes)."""
    L = pkg.load_library()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d\\n", '
                   'sizeof(orbx_track_ref_result), offsetof(orbx_track_ref_result, status), offsetof(orbx_track_ref_result, n_matches), '
                   'offsetof(orbx_track_ref_result, n_correspondences), offsetof(orbx_track_ref_result, n_inliers), ORBX_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = pkg.TRACK_REF_RESULT
    assert got == [T.itemsize] + [T.fields[k][1] for k in ("status", "n_matches", "n_correspondences", "n_inliers")] + [pkg.api.ABI_VERSION]
    assert T.itemsize == 16 and T.names == ("status", "n_matches", "n_correspondences", "n_inliers") and got[-1] == 2
    assert (S.OK, S.NO_MODEL, S.TOO_FEW_CORRESPONDENCES, S.TOO_FEW_INLIERS) == (pkg.TRACK_OK, pkg.TRACK_NO_MODEL, pkg.TRACK_TOO_FEW_CORRESPONDENCES,
                                                                                 pkg.TRACK_TOO_FEW_INLIERS)
    assert S.DMATCH == pkg.DMATCH


def test_min_correspondences_below_four_is_refused_without_a_device(pkg):
    """The guard sits in front of everything that needs a GPU: the module-level function refuses 3 with ORBX_ERR_INVALID where
    making its handle would fail with ORBX_ERR_NO_DEVICE, and the C entry points return ORBX_ERR_INVALID without a handle."""
    s = R.ref_frame(62, 15, 17)
    with pytest.raises(pkg.OrbxError) as e:
        pkg.track_with_reference_kf(s[0], s[1], s[2], s[3], s[4], pkg.CameraModel(**R.CAMERA), s[5], min_correspondences=3)
    assert e.value.code == -1 and "min_correspondences" in str(e.value)
    L = pkg.load_library()
    for name in SYMBOLS:
        fn = getattr(L, name)
        n_args = {"orbx_track_reference": 24, "orbx_track_reference_device": 27, "orbx_keyframe_track_reference": 27}[name]
        args = [None, None, None, C.c_int(3), C.c_int(1)] + [None] * (n_args - 5)
        for k in ((9, 10) if name != "orbx_track_reference" else ()):
            args[k] = C.c_int(1)
        assert fn(*args) == -1


def test_track_reference_driver_compiles_and_links(pkg, tmp_path):
    pkg.load_library()
    assert os.path.exists(build_driver(str(tmp_path)))
