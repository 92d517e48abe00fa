"""CPU checks behind the map-point refresh (orbx_refresh_map_points): the specification (tests/map_point_refresh_spec.py) against the
hand-derived answers, the new ABI, the two snapshot helpers in Python against include/orbx_map.hpp compiled with g++, and — on the
specification alone — the two conditions the GPU tests' tolerances and permutation test rest on."""
import os
import struct
import subprocess

import numpy as np
import pytest

import map_point_refresh_scenes as G
import map_point_refresh_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spec_reproduces_the_hand_derived_answers():
    cases = G.golden_cases()
    assert {c["name"] for c in cases} >= {"reference_hamming_vectors_b_chosen", "all_descriptors_equal", "two_way_tie_earlier_wins", "single_observer_along_z",
                                          "opposite_observers_normal_kept", "observer_at_the_point_skipped", "no_observers"}
    a, b, c = (np.array(k["descriptors"][0], np.uint8) for k in cases[0]["keyframes"])
    assert (S.hamming(a, b), S.hamming(a, c), S.hamming(b, c)) == (8, 12, 4)
    sc, want = G.golden_scene(cases)
    r = S.refresh(sc)
    for p, w in enumerate(want):
        rec = r["records"][p]
        assert (rec["chosen"], rec["best_max_dist"], rec["n_desc"], rec["n_observers"]) == (w["chosen"], w["best_max_dist"], w["n_desc"], w["n_observers"]), w["name"]
        assert np.array_equal(r["mp_desc"][p], w["descriptor"]) and np.array_equal(r["normals"][p], w["normal"]), w["name"]
        assert r["min_distance"][p] == w["min_distance"] and r["max_distance"][p] == w["max_distance"], w["name"]
    s = 1.2 ** 7
    single = want[[w["name"] for w in want].index("single_observer_along_z")]
    assert (single["min_distance"], single["max_distance"]) == (2 / s, 2 * s)
    none = want[[w["name"] for w in want].index("no_observers")]
    assert none["min_distance"] == float("inf") and none["max_distance"] == 0.0


def test_new_symbols_and_record_layout(pkg, tmp_path):
    """The library exports the three entry points and orbx_mp_refresh_record is laid out as the numpy mirror restates it (16 bytes)."""
    L = pkg.load_library()
    for s in ("orbx_refresh_map_points", "orbx_refresh_map_points_device", "orbx_keyframe_refresh_map_points"):
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS
    assert L.orbx_abi_version() == 2
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d\\n", '
                   'sizeof(orbx_mp_refresh_record), offsetof(orbx_mp_refresh_record, chosen), offsetof(orbx_mp_refresh_record, best_max_dist), '
                   'offsetof(orbx_mp_refresh_record, n_desc), offsetof(orbx_mp_refresh_record, n_observers), ORBX_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    R = pkg.MP_REFRESH_RECORD
    assert got == [R.itemsize] + [R.fields[k][1] for k in ("chosen", "best_max_dist", "n_desc", "n_observers")] + [pkg.api.ABI_VERSION]
    assert got[0] == 16 and R == S.RECORD


def _affected_reference(arrays, cur, neighbours):
    """search_in_neighbors.rs:93-102, :116-120, :141-143 over the arrays, written independently of api.MapSnapshot."""
    ids = list(arrays["kf_ids"])
    if cur not in ids:
        return []
    out = []
    for kid in [cur] + list(neighbours):
        if kid in ids:
            k = ids.index(kid)
            for m in arrays["feat_mp_id"][arrays["kf_feat_start"][k]:arrays["kf_feat_start"][k + 1]]:
                if m >= 0 and int(m) not in out:
                    out.append(int(m))
    return out


@pytest.mark.parametrize("sanitize", [False, True])
def test_snapshot_helpers_python_equals_cpp(pkg, tmp_path, sanitize):
    """search_in_neighbors_affected and collect_map_point_refresh: api.MapSnapshot against include/orbx_map.hpp compiled as a
    stand-alone host program (once more with -fsanitize=address,undefined)."""
    arrays, cur, neighbours, _ = G.neighbourhood()
    snap = pkg.MapSnapshot(**arrays)
    affected = snap.search_in_neighbors_affected(cur, neighbours)
    assert affected == _affected_reference(arrays, cur, neighbours) and len(set(affected)) == len(affected) > 500
    assert any(m >= 999000 for m in affected)                                      # dangling ids are affected too (:98) ...
    d = snap.collect_map_point_refresh(affected + [31337])
    held = set(arrays["mp_ids"])
    assert d.mp_ids == [m for m in affected if m in held] and len(d.mp_ids) < len(affected)          # ... and left out here
    assert snap.search_in_neighbors_affected(424242, neighbours) == []
    # the lists as they stand in the snapshot, keyframes in first-seen order
    j = list(arrays["mp_ids"]).index(d.mp_ids[0])
    s, e = arrays["mp_obs_start"][j], arrays["mp_obs_start"][j + 1]
    assert [d.kf_ids[k] for k in d.obs_kf[:e - s]] == list(arrays["mp_obs_kf_id"][s:e]) and list(d.obs_feat[:e - s]) == list(arrays["mp_obs_feat_idx"][s:e])
    seen = [d.kf_ids[k] for k in d.obs_kf if k >= 0]
    assert d.kf_ids == list(dict.fromkeys(seen)) and set(d.kf_ids) <= set(arrays["kf_ids"])
    if arrays["mp_ids"][3] in d.mp_ids:
        assert (d.obs_kf == -1).sum() == 1
    exe = str(tmp_path / "driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "map_point_refresh_driver.cpp"),
                    "-o", exe] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []), check=True)
    open(tmp_path / "snap.bin", "wb").write(snap.to_bytes())
    subprocess.run([exe, str(tmp_path / "snap.bin"), str(cur), str(tmp_path / "out.bin")] + [str(n) for n in neighbours], check=True)
    b = open(tmp_path / "out.bin", "rb").read()
    na, = struct.unpack_from("<Q", b, 0); off = 8
    assert list(np.frombuffer(b, np.uint64, na, off)) == affected; off += 8 * na
    nm, no, nk = struct.unpack_from("<3Q", b, off); off += 24
    assert list(np.frombuffer(b, np.uint64, nm, off)) == d.mp_ids; off += 8 * nm
    assert list(np.frombuffer(b, np.uint64, nk, off)) == d.kf_ids; off += 8 * nk
    assert np.frombuffer(b, np.float64, 3 * nm, off).tobytes() == d.positions.tobytes(); off += 24 * nm
    assert np.array_equal(np.frombuffer(b, np.int32, nm + 1, off), d.obs_start); off += 4 * (nm + 1)
    assert np.array_equal(np.frombuffer(b, np.int32, no, off), d.obs_kf); off += 4 * no
    assert np.array_equal(np.frombuffer(b, np.int32, no, off), d.obs_feat) and off + 4 * no == len(b)


def _cone(aux):
    """smallest cosine between two viewing directions of a point, and |sum| / n"""
    u = np.array(aux["dirs"])
    return float((u @ u.T).min()), aux["sum_norm"] / len(u)


@pytest.mark.parametrize("name", list(G.RANDOM_SCENES) + ["neighbourhood", "golden"])
def test_cone_condition_of_every_gpu_scene(pkg, name):
    """Every point's observers lie inside a 60 degree cone, so |sum| >= n / 2: what the normal tolerance of the GPU tests rests on.
    The exact-construction golden cases G.CONE_EXEMPT lists are exempt (their normals are compared exactly)."""
    exempt = []
    if name == "golden":
        sc, want = G.golden_scene(G.golden_cases())
        exempt = [i for i, w in enumerate(want) if w["name"] in G.CONE_EXEMPT["golden"]]
        assert len(exempt) == len(G.CONE_EXEMPT["golden"])
    elif name == "neighbourhood":
        arrays, cur, neighbours, descs = G.neighbourhood()
        snap = pkg.MapSnapshot(**arrays)
        d = snap.collect_map_point_refresh(snap.search_in_neighbors_affected(cur, neighbours))
        M, T = len(d.mp_ids), len(d.kf_ids)
        sc = dict(positions=d.positions, obs_start=d.obs_start, obs_kf=d.obs_kf, obs_feat=d.obs_feat,
                  kf_poses_wc=np.array([arrays["kf_pose_wc"][arrays["kf_ids"].index(k)] for k in d.kf_ids]), kf_feat_offset=np.arange(T + 1) * 400,
                  descs=np.zeros((400 * T, 32), np.uint8), scale_range=G.SCALE_RANGE, mp_desc=np.zeros((M, 32), np.uint8), normals=np.zeros((M, 3)))
    else:
        sc = G.RANDOM_SCENES[name]()
    r = S.refresh(sc)
    checked = 0
    for p, aux in enumerate(r["aux"]):
        if p in exempt or aux["n_dirs"] == 0:
            continue
        cos, ratio = _cone(aux)
        assert cos >= 0.5 and ratio >= 0.5 and not aux["normal_kept"], (name, p, cos, ratio)
        checked += 1
    assert checked >= (5 if name == "golden" else 4)


def test_unique_minimum_condition_of_the_permutation_scene():
    """In the permutation scene every point's smallest maximum is reached by one row only, so the chosen descriptor cannot depend on
    the order of the list; the other scenes do hold ties (the tie rule is theirs to test)."""
    r = S.refresh(G.permutation())
    assert all(a["unique_min"] for a in r["aux"]) and (r["records"]["n_desc"] >= 3).all()
    assert not any(a["unique_min"] for a in S.refresh(G.ties())["aux"])
