"""CPU checks of the resident map-point store: the specification (tests/map_store_spec.py) against hand-written answers, the
scenes the GPU tests run (tests/map_store_scenes.py) and the new ABI."""
import json
import os

import numpy as np
import pytest

import map_store_scenes as M
import map_store_spec as S
import tracking_scenes as G
import tracking_spec as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def known():
    with open(os.path.join(ROOT, "tests", "golden", "map_store_known_answers.json")) as f:
        return json.load(f)


def test_spec_reproduces_hand_written_answers(known):
    """tests/golden/map_store_known_answers.json: keyframes of 5 / 0 / 4 features over a store of 12 slots.  Slot 7 is in keyframes 0
    and 2 (kept where keyframe 0 shows it), slot 3 twice in keyframe 0 (kept once), slot 9 is not live, one feature has no point."""
    k = known
    live = np.array(k["live"], np.uint8)
    assert S.select_keyframes([np.array(t, np.int32) for t in k["tables"]], live).tolist() == k["select_keyframes"]
    assert S.select_slots(k["src"], live).tolist() == k["select_slots"]             # repeats kept, -1 and the dead slot dropped
    pos, valid = S.reference_rows(k["reference_table"], live, k["positions"])
    assert valid.tolist() == k["reference_valid"] and pos.tolist() == k["reference_positions"]
    assert S.matched_slot(k["matched"], k["select_keyframes"]).tolist() == k["matched_slot"]
    assert S.select_keyframes([None, np.array(k["tables"][2], np.int32)], live).tolist() == [5, 7, 2, 11]     # a keyframe without a table


@pytest.mark.parametrize("n_kf", [1, 3, 11])
def test_scenes_cover_their_frames_and_keep_the_margins(n_kf):
    """a scene's list is a permutation of its frame's map points (nothing dead, nothing twice), and since the positions are
    tracking_scenes' own, the decision margins of that module hold on the gathered rows"""
    sc = M.scene(40 + n_kf, 120, 200, n_kf)
    st = sc["store"]
    lst = S.select_keyframes(sc["tables"], st.live)
    assert sorted(lst.tolist()) == sorted(sc["slots"].tolist()) and len(sc["tables"]) == n_kf
    assert not st.live[sc["dead"]].any() and any((t == -1).any() for t in sc["tables"])
    cand = np.concatenate(sc["tables"])
    assert len(cand) > len(lst) and np.isin(sc["dead"], cand).any()
    pos, desc = S.gathered(lst, st.positions, st.desc)
    f = sc["track_frame"]
    order = {int(s): i for i, s in enumerate(sc["slots"])}
    assert pos.tobytes() == f[2][[order[int(s)] for s in lst]].tobytes()
    for mode in (0, 1):
        assert T.margins(G.CAMERA, T.default_config(mode), f[4], pos) >= 1e-9


@pytest.mark.parametrize("total", [0, 1, 2, 63, M.CHUNK - 1, M.CHUNK, M.CHUNK + 1, 2 * M.CHUNK + 1])
def test_tables_with_total_are_what_they_say(total):
    tables, live = M.tables_with_total(7 + total, total)
    c = np.concatenate(tables)
    assert len(c) == total and len(tables) == 3
    lst = S.select_keyframes(tables, live)
    assert len(set(lst.tolist())) == len(lst) and all(live[s] for s in lst)
    if total >= 3:
        assert c[0] == c[-2] and lst[0] == c[0] and lst[-1] == c[-1] and (c[:-1] != c[-1]).all()      # first seen first / as the very last candidate


def test_new_symbols(pkg):
    L = pkg.load_library()
    for s in ("orbx_map_points_create", "orbx_map_points_set", "orbx_map_points_set_device", "orbx_map_points_erase", "orbx_map_points_download",
              "orbx_keyframe_set_map_point_slots", "orbx_map_select_points_device", "orbx_map_track_frames_device", "orbx_map_track_frames",
              "orbx_map_track_reference_device"):
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS
    assert (pkg.MAP_SOURCE_KEYFRAMES, pkg.MAP_SOURCE_SLOTS) == (0, 1) and hasattr(pkg, "MapPointStore")
