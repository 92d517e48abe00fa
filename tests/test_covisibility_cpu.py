"""CPU checks of covisibility on the resident map: the specification (tests/covisibility_spec.py) against hand-written answers and
against a literal replay of the reference's incremental update, the scenes the GPU tests run (tests/covisibility_scenes.py), the new
ABI and the C++ driver."""
import json
import os
import subprocess

import numpy as np
import pytest

import covisibility_scenes as V
import covisibility_spec as S
import map_store_scenes as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam3-rust_amd")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")


def build_driver(tmp):
    exe = os.path.join(tmp, "covisibility_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "covisibility_driver.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lorbx_hip", "-L", ROCM_LIB, "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ROCM_LIB], check=True)
    return exe


def _tables(k):
    return [None if t is None else np.array(t, np.int32) for t in k["tables"]]


def test_spec_reproduces_hand_written_answers():
    """tests/golden/covisibility_known_answers.json: seven keyframes over a store of 12 slots — a slot twice in one keyframe, a dead
    slot shared by two, a keyframe without a table, one with zero features, a three-way tie, fewer positive weights than n_best."""
    with open(os.path.join(ROOT, "tests", "golden", "covisibility_known_answers.json")) as f:
        k = json.load(f)
    tables, live = _tables(k), np.array(k["live"], np.uint8)
    assert [sorted(S.observed(t, live)) for t in tables] == k["observed"]
    w = S.weights(tables, live, range(len(tables)))
    assert w.dtype == np.int32 and w.tolist() == k["weights"] and (w == w.T).all()
    b, n = S.best_rows(w, 3)
    assert b.dtype == np.int32 and b.tolist() == k["best_3"] and n.tolist() == k["n_best_3"]
    b0, n0 = S.best(w[0], 10)
    assert b0.tolist() == k["best_10_row_0"] and n0 == k["n_best_10_row_0"]
    assert S.best(w[0], 0)[0].tolist() == [] and S.best(w[0], 0)[1] == 0
    for c in k["local_keyframes"]:
        lst, row = S.local_keyframes(tables, live, c["ref"], c["n_best"])
        assert lst == c["list"] and row.tolist() == c["row"], c


@pytest.mark.parametrize("seed,n_kfs", [(1, 3), (2, 11), (3, 64)])
def test_spec_equals_the_replayed_incremental_update(seed, n_kfs):
    """Where every point is associated once per keyframe (the repeats inside a table removed), the derived weight is what
    Map::associate's incremental update (map.rs:361-383) leaves."""
    tables, _, live = V.world(seed, n_kfs)
    once = []
    for t in tables:
        if t is None:
            once.append(None)
            continue
        _, first = np.unique(t, return_index=True)
        once.append(t[np.sort(first)])
    w = S.weights(once, live, range(n_kfs))
    assert w.tolist() == S.associate_replay(once, live).tolist() and (n_kfs < 11 or w.max() > 3)
    assert w.tolist() == S.weights(tables, live, range(n_kfs)).tolist()         # and the repeats do not change the derived weight


@pytest.mark.parametrize("n_kfs", V.N_KFS)
def test_worlds_are_what_they_claim(n_kfs):
    tables, counts, live = V.world(20 + n_kfs, n_kfs)
    assert len(tables) == n_kfs and [0 if t is None else len(t) for t in tables if t is not None] == [c for c, t in zip(counts, tables) if t is not None]
    if n_kfs >= 11:
        assert set(counts) == set(V.SIZES) and any(t is None for t in tables)
        cat = np.concatenate([t for t in tables if t is not None])
        assert (cat == -1).any() and (live[cat[cat >= 0]] == 0).any()                          # -1 entries and slots that are not live
        assert any(len(np.unique(t[t >= 0])) < (t >= 0).sum() for t in tables if t is not None)     # repeats inside a table
        w = S.weights(tables, live, range(n_kfs))
        assert (w > 0).sum() > n_kfs and any(len(set(r[r > 0].tolist())) < (r > 0).sum() for r in w)   # ties inside a row


@pytest.mark.parametrize("n_kfs", [3, 65, 257])
def test_row_worlds_are_what_they_claim(n_kfs):
    rows = {kind: S.weights(*V.row_world(kind, n_kfs)[::2], [0])[0] for kind in ("equal", "zero", "rising")}
    assert rows["equal"][0] == 0 and (rows["equal"][1:] == 3).all()                          # an (n_kfs - 1)-way tie
    assert not rows["zero"].any()
    assert rows["rising"].tolist() == list(range(n_kfs))
    assert S.best(rows["rising"], n_kfs + 3)[0][:n_kfs - 1].tolist() == list(range(n_kfs - 1, 0, -1))
    assert S.best(rows["equal"], 10)[1] == min(10, n_kfs - 1) and S.best(rows["zero"], 10)[1] == 0     # n_positive < n_best at n_kfs = 3


def test_tracking_world_has_the_references_it_claims():
    store, scs, tables, first = V.tracking_world()
    w = S.weights(tables, store.live, range(len(tables)))
    a0, c0 = first[0], first[2]
    assert (w[a0] > 0).sum() > 2 and not w[c0].any() and len(tables) == 9                      # more covisibles than n_best = 2; none at all
    lst, row = S.local_keyframes(tables, store.live, a0, 2)
    assert len(lst) == 3 and lst[0] == a0 and row.tolist() == lst                              # the query is listed first, once
    assert S.local_keyframes(tables, store.live, c0, 2)[1].tolist() == [c0, -1, -1]
    assert S.local_keyframes(tables, store.live, -1, 2)[0] == list(range(9))                   # no reference: the query is not listed apart


def test_new_symbols(pkg):
    L = pkg.load_library()
    for s in ("orbx_map_covisibility_device", "orbx_map_covisibility", "orbx_map_track_local_device", "orbx_map_track_local"):
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS, s
    for m in ("map_covisibility_device", "map_covisibility", "map_track_local_device", "map_track_local"):
        assert hasattr(pkg.Handle, m), m
    # best rows into MapSnapshot's covisibility lists
    start, ids = pkg.covisibility_lists([10, 20, 30], [[2, 1, -1], [-1, -1, -1], [0, -1, -1]], [2, 0, 1])
    assert start.dtype == np.int32 and ids.dtype == np.uint64 and start.tolist() == [0, 2, 2, 3] and ids.tolist() == [30, 20, 10]


def test_covisibility_driver_compiles_and_links(pkg, tmp_path):
    pkg.load_library()
    assert os.path.exists(build_driver(str(tmp_path)))
