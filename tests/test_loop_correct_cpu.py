"""CPU checks of the loop correction on the resident map: the specification (tests/loop_correct_spec.py) against hand-made answers,
one per rule; its FIFO walk against the distance form; against a sequential replay of the reference on worlds where no slot is in
two pairs; the new ABI as the library exports it and as the Python wrappers name it."""
import os

import numpy as np
import pytest

import loop_correct_scenes as Z
import loop_correct_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("orbx_default_loop_correct_config", "orbx_map_loop_max_keyframes", "orbx_map_correct_loop_device", "orbx_map_correct_loop", "orbx_map_close_loop")


def _run(sc, **kw):
    a = dict(min_weight=sc["min_weight"], max_depth=sc["max_depth"]); a.update(kw)
    return S.correct_loop(sc["tables"], sc["live"], sc["positions"], sc["poses"], sc["parent"], sc["cur"], sc["loop"], sc["sim3"], sc["matches"], **a)


def _t(*rows):
    return [None if r is None else np.array(r, np.int32) for r in rows]


# ---- reach -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(Z.REACH))
def test_reach_scenes_give_the_sets_written_beside_them(name):
    sc = Z.REACH[name]()
    r = _run(sc)
    assert np.flatnonzero(r["affected"]).tolist() == Z.REACH_WANT[name] and r["counts"][0] == len(Z.REACH_WANT[name])
    d = S.affected_by_distance(sc["tables"], sc["live"], sc["parent"], sc["cur"], sc["min_weight"], sc["max_depth"])
    assert d.tobytes() == r["affected"].tobytes()


@pytest.mark.parametrize("N", Z.RANDOM_N[:2])
def test_fifo_walk_equals_distances_on_random_graphs(N):
    sc = Z.random_graph(N)
    for depth in (0, 1, 2, 5, 100):
        a = S.affected(sc["tables"], sc["live"], sc["parent"], sc["cur"], sc["min_weight"], depth)
        assert a.tobytes() == S.affected_by_distance(sc["tables"], sc["live"], sc["parent"], sc["cur"], sc["min_weight"], depth).tobytes()
        assert a[sc["cur"]] == 1
    assert 1 < a.sum()


def test_a_dead_shared_point_is_no_weight():
    live = np.ones(8, np.uint8); live[2] = 0
    t = _t([0, 1, 2], [0, 1, 2])
    assert S.affected(t, live, [-1, -1], 0, 3, 100).tolist() == [1, 0] and S.affected(t, live, [-1, -1], 0, 2, 100).tolist() == [1, 1]


# ---- points and the correction -------------------------------------------------------------------------------------------------

def test_points_are_listed_once_in_walking_order_and_only_they_move():
    sc = Z.points()
    r = _run(sc)
    assert r["affected"].tolist() == [1, 1, 0, 0]
    assert r["list_slot"].tolist() == [0, 1, 2, 4, 3]          # keyframe 0: its shares, the repeated slot (once); keyframe 1: the slot keyframes 2 and 3 also see
    moved = np.any(r["positions"] != sc["positions"], axis=1)
    assert np.flatnonzero(moved).tolist() == [0, 1, 2, 3, 4]
    assert Z.no_points() and _run(Z.no_points())["counts"].tolist() == [2, 0, 0, 0]


def test_correction_is_the_inverse_transform():
    """a quarter turn about z, scale 2, t = (1, 0, 0): p' = R^T (p - t) / 2"""
    s = np.sqrt(0.5)
    sim3 = [s, 0, 0, s, 1.0, 0.0, 0.0, 2.0]
    assert np.allclose(S.correct_points(sim3, [[1.0, 2.0, 3.0]]), [[1.0, 0.0, 1.5]], atol=1e-15)
    pose = S.correct_pose(sim3, [1, 0, 0, 0, 1.0, 2.0, 3.0])
    assert np.allclose(pose, [s, 0, 0, -s, 1.0, 0.0, 1.5], atol=1e-15)
    # forward then back: sim3 (s R p + t) undone
    rng = np.random.default_rng(3)
    for name, sm in Z.SIM3S.items():
        p = rng.uniform(-10, 10, (5, 3))
        q = np.asarray(sm[:4], np.float64)
        fwd = sm[7] * (p @ S._rot(q).T) + np.asarray(sm[4:7])
        assert np.all(np.abs(S.correct_points(sm, fwd) - p) <= 10 * S.tolerance(sm, fwd)[:, None]), name
    # the product is not renormalised and keeps the sign it falls on
    assert S.correct_pose([-1, 0, 0, 0, 0, 0, 0, 1], [0.5, 0.5, 0.5, 0.5, 0, 0, 0])[:4].tolist() == [-0.5, -0.5, -0.5, -0.5]


# ---- pairs and fuse ------------------------------------------------------------------------------------------------------------

def test_pairs_need_two_live_different_points():
    live = np.ones(8, np.uint8); live[5] = 0
    t = _t([1, 2, 5, -1], [1, 3, 4, 9])
    pr = S.pairs(t, live, 0, 1, [(0, 0), (1, 1), (2, 2), (3, 1), (1, 3), (7, 0), (0, -1)])
    assert pr.tolist() == [[-1, -1], [2, 3], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]


def test_keeper_rules():
    live = np.ones(8, np.uint8)
    # a tie: the current keyframe's point keeps
    new, g, k = S.fuse(_t([1], [2]), live, np.array([[1, 2]], np.int32))
    assert (g.tolist(), k.tolist(), [t.tolist() for t in new]) == ([2], [1], [[1], [1]])
    # more observers keep, whichever side
    new, g, k = S.fuse(_t([1], [2], [2]), live, np.array([[1, 2]], np.int32))
    assert (g.tolist(), k.tolist(), [t.tolist() for t in new]) == ([1], [2], [[2], [2], [2]])
    # a class of three through a shared member; a tie inside it goes to the first in a0 b0 a1 b1
    new, g, k = S.fuse(_t([1, 2], [2, 3]), live, np.array([[1, 2], [2, 3]], np.int32))
    assert (g.tolist(), k.tolist(), [t.tolist() for t in new]) == ([1, 3], [2, 2], [[2, 2], [2, 2]])
    new, g, k = S.fuse(_t([1, 4], [2, 3]), live, np.array([[1, 2], [4, 2]], np.int32))
    assert (g.tolist(), k.tolist()) == ([2, 4], [1, 1])
    # a goner at two features of one keyframe is replaced at both; a keyframe no pair names is rewritten too
    new, g, k = S.fuse(_t([1], [2], [2, 7, 2], [1, 1]), live, np.array([[1, 2]], np.int32))
    assert (g.tolist(), k.tolist(), [t.tolist() for t in new]) == ([2], [1], [[1], [1], [1, 7, 1], [1, 1]])
    assert S.uniq(new[2]).tolist() == [1, 7, -1]


def test_fuse_scene_shows_every_rule():
    sc = Z.fuse_scene()
    r = _run(sc)
    assert r["affected"].tolist() == [1, 1, 1, 0] and r["counts"].tolist() == [3, 26, 7, 6]
    assert (r["pairs"][:, 0] >= 0).tolist() == [False, False, True, True, True, True, True, True, True, False]
    pr = r["pairs"]
    assert pr[2].tolist() == pr[3].tolist() and pr[4][1] == pr[5][0]                       # the duplicate; the class of three's shared member
    to = dict(zip(r["goner"].tolist(), r["keeper"].tolist()))
    assert to[pr[2][1]] == pr[2][0] and to[pr[6][1]] == pr[6][0]                             # ties keep the current keyframe's point
    assert to[pr[4][0]] == to[pr[4][1]] == pr[5][1]                                          # c keeps a and b
    assert to[pr[7][0]] == pr[7][1] and to[pr[8][1]] == pr[8][0]
    assert (sc["tables"][2] == pr[7][0]).sum() == 2 and (r["tables"][2] == pr[7][1]).sum() == 3   # two features re-pointed beside the keeper's own
    assert (r["tables"][3] == pr[8][0]).sum() == 2 and r["affected"][3] == 0                 # outside A, and it named the keeper already
    assert not np.isin(np.concatenate(r["tables"]), r["goner"]).any()
    assert _run(Z.no_pairs())["counts"].tolist() == [2, 3, 0, 0]


@pytest.mark.parametrize("seed", range(6))
def test_spec_equals_the_reference_replayed_where_no_slot_is_in_two_pairs(seed):
    sc = Z.agree_world(seed)
    r = _run(sc)
    flat = r["pairs"][r["pairs"] >= 0]
    assert len(flat) == len(set(flat.tolist())) == 16 and r["counts"][3] == 8
    tabs, live, pos, poses = S.replay_reference(sc["tables"], sc["live"], sc["positions"], sc["poses"], sc["parent"], sc["cur"], sc["loop"], sc["sim3"], sc["matches"],
                                                sc["min_weight"], sc["max_depth"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(tabs, r["tables"]))
    assert live.tobytes() == r["live_after"].tobytes() and pos.tobytes() == r["positions"].tobytes() and poses.tobytes() == r["poses_wc"].tobytes()
    keeps_loop = sum(int(k) in set(r["pairs"][:, 1].tolist()) for k in r["keeper"])
    assert 0 < keeps_loop < 8                                                                # both directions occur in every world


# ---- the ABI -------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_wrapped(pkg):
    import ctypes as C
    L = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS, s
    for m in ("map_correct_loop_device", "map_correct_loop", "map_close_loop"):
        assert callable(getattr(pkg.Handle, m))
    from orb_slam3_rust_amd.api import _LoopCorrectConfig
    c = _LoopCorrectConfig()
    L.orbx_default_loop_correct_config(C.byref(c))
    d = pkg.LoopCorrectConfig()
    assert (c.min_covisibility_weight, c.max_propagation_depth) == (d.min_covisibility_weight, d.max_propagation_depth) == (15, 100)      # corrector.rs:97-104
    assert L.orbx_map_loop_max_keyframes() == 4096
    # refusals that need no device: a null handle
    assert L.orbx_map_correct_loop(None, None, None, 0, None, None, 0, 0, None, 0, None, 0, None, None, None, None, None, None) == pkg.api.ORBX_ERR_INVALID
