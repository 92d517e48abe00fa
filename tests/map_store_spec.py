"""Specification of the resident map-point store's selections (include/orbx.h, "resident map points"), in numpy.

select_keyframes   tracker.rs:826-867: the distinct live slots of a frame's keyframes in first-seen order ([spec]: the reference
                   collects into a HashSet, whose order is unspecified)
select_slots       tracker.rs:1093-1102: the live entries of a slot array in order, repeats kept
reference_rows     tracker.rs:1024-1036: per keyframe feature, valid and the position
The tracking that follows a selection is tests/tracking_spec.py's, on the gathered rows: the new calls add no arithmetic.
"""
import numpy as np


def select_keyframes(slot_tables, live):
    """slot_tables: the frame's keyframes in order, each an int array [n_k] (-1 = None) or None (no table) -> int32 list"""
    seen, out = set(), []
    for t in slot_tables:
        for s in ([] if t is None else np.asarray(t).tolist()):
            if s >= 0 and live[s] and s not in seen:
                seen.add(s); out.append(s)
    return np.array(out, np.int32)


def select_slots(src, live):
    return np.array([s for s in np.asarray(src).tolist() if s >= 0 and live[s]], np.int32)


def reference_rows(slot_table, live, positions):
    """(positions [n,3] f64, valid [n] u8) of one keyframe: None as a table = every feature -1"""
    t = np.asarray(slot_table, np.int64).reshape(-1)
    live = np.asarray(live); positions = np.asarray(positions, np.float64)
    ok = (t >= 0) & (live[np.maximum(t, 0)] != 0)
    pos = np.zeros((len(t), 3))
    pos[ok] = positions[t[ok]]
    return pos, ok.astype(np.uint8)


def gathered(list_slot, positions, desc):
    i = np.asarray(list_slot, np.int64)
    return np.ascontiguousarray(np.asarray(positions, np.float64)[i]), np.ascontiguousarray(np.asarray(desc, np.uint8)[i])


def matched_slot(matched, list_slot):
    m = np.asarray(matched, np.int64)
    ls = np.concatenate([np.asarray(list_slot, np.int32), np.array([-1], np.int32)])
    return np.where(m >= 0, ls[np.where(m >= 0, m, len(ls) - 1)], -1).astype(np.int32)
