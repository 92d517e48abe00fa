"""The scenes of tests/block_primitive_scenes.py are what tests/test_block_primitives_gpu.py needs them to be, checked on the
specifications alone: flagged entries on both sides of every round boundary, counters that differ, a pair list longer than one
chunk, the tracking scenes clear of every decision point; for the scans, segment and observer counts at a wave's edge, the block's
edge and in a second and third round, and keypoints in nothing but the edge counters of each counting sort, with matches in each."""
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


# ---- the scan of counts over rounds ----------------------------------------------------------------------------------------------
def test_cov_seg_cases_take_a_second_and_a_third_round():
    """per frame the segments S = n_kfs (ref -1) or 1 + n_best: 63 .. 65, 255 .. 513, with candidates on both sides of every round boundary,
    keyframes without a table and without features among them, and slots seen for the first time behind the first round"""
    import covisibility_spec as CV
    import map_store_spec as MS
    seen = set()
    for n_kfs, n_best, refs in B.COV_SEG_CASES:
        tables, counts, live = B.tiny_world(n_kfs)
        assert len(tables) == n_kfs and max(counts) == 3 and min(counts) == 0 and any(t is None for t in tables)
        off, slots, local_kf, keys = B.cov_seg_expected(n_kfs, n_best, refs)
        assert local_kf.shape == (len(refs), 1 + n_best)
        for b, r in enumerate(refs):
            S = n_kfs if r < 0 else 1 + n_best
            seen.add(S)
            n = [counts[k] for k in keys[b]]
            if r < 0:
                assert (local_kf[b] == -1).all() and len(keys[b]) == S
                for e in range(B.ROUND, S, B.ROUND):
                    assert max(n[e - 4:e]) > 0 and max(n[e:e + 4]) > 0, (n_kfs, e)
                first = {}
                for j, k in enumerate(keys[b]):
                    for s in MS.select_keyframes([tables[k]], live).tolist():
                        first.setdefault(s, j)
                if S > B.ROUND:
                    assert max(first.values()) >= B.ROUND                       # a slot whose first sighting lies in the second round
            elif r == 0 and n_best in (2, B.ROUND - 1, B.ROUND):
                assert len(keys[b]) == S and n[-1] > 0                         # the best list is full: real segments up to the last
            elif r == 0:
                assert (n_best < B.ROUND or B.ROUND + 1 < len(keys[b])) and 1 < len(keys[b]) < S and (local_kf[b, len(keys[b]):] == -1).all()      # ... here it ends in padding
            else:
                assert len(keys[b]) == 1                                       # a reference nobody shares a point with
        assert off[-1] == len(slots) and (np.diff(off) > 0).sum() >= len(refs) - 1
    assert seen >= {63, 64, 65, 255, 256, 257, 513, 301}                         # a wave's edge, the block's edge, three rounds, padding behind the second


def test_ba_order_cases_have_the_observer_counts_they_are_for():
    import ba_collect_spec as BS
    for n_obs, max_cov in B.BA_ORDER_CASES:
        tables, xy, live = B.ba_order_world(n_obs)
        s = BS.collect(tables, xy, live, 0, max_cov)
        K, F, M, N = (int(x) for x in s["counts"])
        assert K + F == n_obs and K == min(max_cov, n_obs - 1) and N > n_obs and M >= 3
        assert len(tables) > n_obs and any(t is None for t in tables)          # keyframes that observe nothing stand among the observers
    assert [n for n, _ in B.BA_ORDER_CASES][:2] == [B.ROUND, B.ROUND + 1] and B.BA_ORDER_CASES[2][0] > 2 * B.ROUND and B.BA_ORDER_CASES[2][1] >= B.ROUND


# ---- the counter scan of the counting sorts --------------------------------------------------------------------------------------
def test_stereo_scenes_fill_only_the_edge_buckets_and_match_in_each(oracle, pkg):
    cam = oracle.Camera(**pkg.synth.EUROC_CAMERA)
    for rows in (B.STEREO_ROWS, B.STEREO_ONE):
        kpL, dL, kpR, dR = B.stereo_rows(rows)
        bucket = B.row_bucket(kpR["y"])
        assert sorted(set(bucket.tolist())) == sorted(rows)
        m, _, has = oracle.stereo_match(cam, kpL, dL, kpR, dR)
        assert sorted(set(bucket[m["train_idx"]].tolist())) == sorted(rows) and len(m) > 0.8 * len(kpL) and has.sum() > 0.8 * len(kpL)
    assert B.STEREO_ROWS == (0, 255, 256, 4095) and (B.stereo_rows(B.STEREO_ROWS)[2]["y"] >= 4096).sum() > 5


def test_guided_and_track_scenes_fill_only_the_edge_cells_and_match_in_each(oracle):
    cfg = TS.default_config(1)
    for cells, frames in ((B.GUIDED_CELLS, B.track_four_cells()), (B.GUIDED_ONE, B.track_one_cell())):
        kp, desc, uv, qd = B.guided_cells(cells)
        cell = B.guided_cell_of(kp)
        assert sorted(set(cell.tolist())) == sorted(cells)
        for mode in (0, 1):
            idx, _ = oracle.guided_match(kp, desc, G.W, G.H, uv, qd, 15.0, mode)
            assert sorted(set(cell[idx[idx >= 0]].tolist())) == sorted(cells) and (idx >= 0).sum() > 0.8 * len(uv)
        f = frames[0]
        assert sorted(set(B.guided_cell_of(f[0]).tolist())) == sorted(cells) and TS.margins(G.CAMERA, cfg, f[4], f[2]) >= 1e-9
        off, ms, gs = TS.search_and_gather(oracle, G.CAMERA, cfg, frames)
        assert off[1] > 0.8 * len(f[2]) and sorted(set(B.guided_cell_of(f[0])[gs[0]["feat_idx"]].tolist())) == sorted(cells)
    assert B.GUIDED_CELLS == (0, 191, 192, 3071)


def test_triangulation_scenes_fill_only_the_edge_cells_of_a_64_x_64_grid_and_pair_in_each(oracle):
    import camera_scenes as CS
    for cells in (B.TRI_CELLS, B.TRI_ONE):
        s = B.tri_cells(cells)
        assert CS.tri_grid_dims(s["camera"]) == (64, 64)
        cell = B.tri_cell_of(s["kp2"])
        assert sorted(set(cell.tolist())) == sorted(cells)
        pairs = oracle.search_for_triangulation(oracle.Camera(**s["camera"]), s["kp1"], s["desc1"], s["mp1"], s["stereo1"], s["kp2"], s["desc2"], s["mp2"],
                                                s["pose1_wc"], s["pose2_wc"], 50)
        assert sorted(set(cell[pairs[:, 1]].tolist())) == sorted(cells) and len(pairs) >= 10 * len(cells)
    assert B.TRI_CELLS == (0, 255, 256, 4095)
