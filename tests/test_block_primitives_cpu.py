"""The scenes of tests/block_primitive_scenes.py are what tests/test_block_primitives_gpu.py needs them to be, checked on the
specifications alone: flagged entries on both sides of every round boundary, counters that differ, a pair list longer than one
chunk, and the tracking scenes clear of every decision point."""
import numpy as np
import pytest

import block_primitive_scenes as B
import loop_verify_spec as LS
import track_reference_spec as RS
import tracking_scenes as G
import tracking_spec as TS


def test_tracking_scenes_flag_some_points_and_keep_clear_of_decision_points(oracle):
    cfg = TS.default_config(1)
    rounds, many = B.track_rounds(), B.track_many()
    assert [len(f[2]) for f in rounds] == [0, 255, 256, 257, 513] and len(many) == B.ROUND + 1
    for f in rounds + many:
        assert TS.margins(G.CAMERA, cfg, f[4], f[2]) >= 1e-9
    off, ms, _ = TS.search_and_gather(oracle, G.CAMERA, cfg, rounds)
    for m in ms[1:]:
        flag = m >= 0
        assert 0 < flag.sum() < len(flag)                                     # some points match, some do not
        for e in range(B.ROUND, len(m), B.ROUND):                              # both kinds on either side of every round boundary
            assert 0 < flag[e - 8:e].sum() < 8 or 0 < flag[e:e + 8].sum() < 8 or flag[e - 1] != flag[e], e
    assert np.diff(off).tolist()[0] == 0
    off, ms, _ = TS.search_and_gather(oracle, G.CAMERA, cfg, many)
    n = np.diff(off)
    assert n.min() >= 4 and n.max() <= 8 and off[B.ROUND] != off[B.ROUND + 1]      # every frame reaches PnP; the last block has an offsets[B] of its own


def test_reference_scenes_flag_the_round_edges(oracle):
    for live, want in (("edges", [0, 1, 2, 4]), ("all", None), ("none", [0, 0, 0, 0])):
        frames = B.reference_rounds(live)
        assert [len(f[2]) for f in frames] == list(B.SIZES)
        off, ms, gs = RS.match_and_gather(oracle, frames)
        n_corr = np.diff(off).tolist()
        for f, m, g in zip(frames, ms, gs):
            assert len(m) > 0.9 * len(f[2])                                   # nearly every row is a mutual match
            if live == "edges":                                               # every live row is matched: the second counter moves where the first does
                assert g["kf_idx"].tolist() == B.round_edges(len(f[2]))
        assert n_corr == (want if want is not None else [len(m) for m in ms])


@pytest.mark.parametrize("live", ["all", "edges"])
def test_loop_scenes_match_nearly_every_feature_or_some(live):
    for (cur, loop), n in zip(B.loop_rounds(live), B.SIZES):
        assert len(cur["desc"]) == n
        for cfg, lo, hi in ((B.LOOP_CFG, 0.9 * n, n + 1), (B.LOOP_CFG_SOME, 0, n)):
            s = LS.verify_pair(G.CAMERA, cur, loop, cfg)
            assert s["status"] == LS.TOO_FEW_PAIRS and lo < s["n_matches"] < hi
            matched = [i for i, _, _ in s["matches"]]
            if live == "all":
                assert s["n_pairs"] == s["n_matches"]
            else:
                assert s["feature_matches"][:, 0].tolist() == [i for i in B.round_edges(n) if i in matched]


def test_triangulation_scene_exceeds_one_chunk(oracle):
    created, stats, res, ev = B.tri_expected(oracle)
    assert len(B.tri_scene()["neighbours"]) == 3
    assert stats[0, 1] > B.TRI_CHUNK                                           # neighbour 0's search leaves more than one round of pairs
    made = [st == 0 for t, _, _, st, _, _, _ in ev if t == 0]
    assert any(made[:B.TRI_CHUNK]) and any(made[B.TRI_CHUNK:]) and not all(made)   # created pairs in both rounds
    assert stats[1].tolist() == [0, 0, 0, 0] and stats[2, 3] > 0               # neighbour 2's points continue neighbour 0's list
    assert 0 < stats[0, 3] < stats[0, 2] < stats[0, 1]                         # the two counters differ
