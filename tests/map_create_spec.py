"""Specification of point creation and removal on the resident map (include/orbx.h, "create and cull map points on the resident
map"), in numpy; the searches and the pair loop are tests/triangulation_spec.py's, fed the derived flags.

flags             flag(k, i): the table of keyframe k names a live point at feature i (None as a table: every flag 0)
create_points     both phases: lists, counts, stats and the tables afterwards          (local_mapper.rs:232-268, triangulation.rs:71-308)
create_replay     the reference's sequential loop on dict-based tables, literally: create_map_point + associate per point
remove_points     remove_map_point_full for a list                                     (map.rs:609-631)
remove_replay     the same through mp.observations on dict-based tables
cull_points       the candidates with fewer than min_observations observers, removed   (local_mapper.rs:421-469)
A table is an int32 array [n] or None; tables[0] is the current keyframe's, tables[1 + t] neighbour t's.
"""
import numpy as np

import map_observations_spec as OBS
import triangulation_spec as TS

STEREO, NEIGHBOURS = 1, 2


def flags(table, live, n):
    live = np.asarray(live)
    if table is None:
        return np.zeros(n, np.uint8)
    t = np.asarray(table).reshape(-1)
    ok = (t >= 0) & (t < len(live))
    out = np.zeros(n, np.uint8)
    out[ok] = live[t[ok]] != 0
    return out


def _with_tables(tables, counts):
    """a keyframe without a table is given one, every entry -1, when the call is accepted"""
    return [np.full(n, -1, np.int32) if t is None else np.array(t, np.int32, copy=True) for t, n in zip(tables, counts)]


def create_points(oracle, cam, cfg, is_inertial, current, neighbours, tables, live, free_slots, phases=STEREO | NEIGHBOURS):
    """-> dict(counts [4], new_slot, new_neighbour, new_idx1, new_idx2 int32 [created], new_points [created,3], new_desc [created,32],
    stats [T,4], tables (afterwards, [1 + T]), evaluated (the pair loop's records), created_pairs [(t, idx1, idx2, p)] of ALL validated pairs)"""
    free_slots = np.asarray(free_slots, np.int32).reshape(-1)
    T, n1, nf = len(neighbours), len(current["kp"]), len(free_slots)
    out = _with_tables(tables, [n1] + [len(nb["kp"]) for nb in neighbours])
    fl = [flags(t, live, len(o)) for t, o in zip(tables, out)]
    rows = []                                                              # (slot, neighbour, idx1, idx2, point, descriptor row)
    S = 0
    given = fl[0].copy()
    if phases & STEREO:
        for i in range(n1):
            if current["has"][i] and not fl[0][i]:
                r = S
                S += 1
                if r < nf:
                    p = TS.transform_point(current["pose"], current["pts"][i])
                    rows.append((int(free_slots[r]), -1, i, -1, p, current["desc"][i]))
                    out[0][i] = free_slots[r]; given[i] = 1
    Sp = min(S, nf)
    stats = np.zeros((T, 4), np.int32)
    created, evaluated = [], []
    if phases & NEIGHBOURS:
        cur = dict(current, mp=given)
        nbs = [dict(nb, mp=fl[1 + t]) for t, nb in enumerate(neighbours)]
        created, stats, _, evaluated = TS.triangulate_from_neighbors(oracle, cam, cfg, is_inertial, cur, nbs)
    N = len(created)
    for e, (t, i1, i2, p) in enumerate(created):
        if Sp + e >= nf:
            break
        slot = int(free_slots[Sp + e])
        rows.append((slot, t, i1, i2, np.asarray(p, np.float64), current["desc"][i1]))
        out[1 + t][i2] = slot
        out[0][i1] = slot                                                  # in order: the last created pair of a feature stays (:289)
    n_created = min(S + N, nf)
    assert len(rows) == n_created
    col = lambda j, dt: np.array([r[j] for r in rows], dt).reshape(-1)
    return dict(counts=np.array([S, N, n_created, S + N - n_created], np.int32), new_slot=col(0, np.int32), new_neighbour=col(1, np.int32),
                new_idx1=col(2, np.int32), new_idx2=col(3, np.int32), new_points=np.array([r[4] for r in rows], np.float64).reshape(-1, 3),
                new_desc=np.array([r[5] for r in rows], np.uint8).reshape(-1, 32), stats=np.asarray(stats, np.int32), tables=out,
                evaluated=evaluated, created_pairs=created)


def live_after(live, spec):
    out = np.array(live, np.uint8, copy=True)
    out[spec["new_slot"]] = 1
    return out


def create_replay(current, neighbours, tables, live, free_slots, created_pairs, phases=STEREO | NEIGHBOURS):
    """local_mapper.rs:232-268 + triangulation.rs:94-107, :286-290 on a host map: kf_points[k] = {feature: map point} (a dead or
    out-of-range entry is no point: the reference's lookup fails), map points named by their slots.  created_pairs: the validated
    pairs the searches gave, in creation order.  -> kf_points afterwards"""
    live = np.asarray(live)
    kf_points = [{} if t is None else {i: int(s) for i, s in enumerate(np.asarray(t).tolist()) if 0 <= s < len(live) and live[s]} for t in tables]
    free = list(np.asarray(free_slots).tolist())
    if phases & STEREO:
        for i in range(len(current["kp"])):                                # :240-266
            if not current["has"][i] or i in kf_points[0]:
                continue
            if not free:
                continue                                                   # no slot left: the point is dropped
            kf_points[0][i] = free.pop(0)                                  # create_map_point + associate
    if phases & NEIGHBOURS:
        for t, i1, i2, _ in created_pairs:                                 # :286-290 (the flags were cloned before the loop: no re-check)
            if not free:
                break
            mp = free.pop(0)
            kf_points[0][i1] = mp                                          # associate(current, idx1): overwrites
            kf_points[1 + t][i2] = mp
    return kf_points


def tables_as_points(tables, live):
    """what a reader sees of tables: {feature: live slot} per keyframe"""
    live = np.asarray(live)
    return [{} if t is None else {i: int(s) for i, s in enumerate(np.asarray(t).tolist()) if 0 <= s < len(live) and live[s]} for t in tables]


def remove_points(tables, live, slots):
    """-> (tables afterwards (None stays None), live afterwards, n_cleared)"""
    gone = set(int(s) for s in np.asarray(slots).reshape(-1).tolist())
    out, n = [], 0
    for t in tables:
        if t is None:
            out.append(None)
            continue
        a = np.array(t, np.int32, copy=True)
        hit = np.isin(a, list(gone)) if gone else np.zeros(len(a), bool)
        n += int(hit.sum())
        a[hit] = -1
        out.append(a)
    lv = np.array(live, np.uint8, copy=True)
    if gone:
        lv[list(gone)] = 0
    return out, lv, n


def remove_replay(kf_points, slots):
    """map.rs:609-631 on {feature: map point} tables: for every observation of the point, kf.map_point_ids[feat] = None; then the
    point goes.  The reference's observations hold one feature per keyframe; a table that names a point twice is purged wholly here
    as in the specification (a stale entry would name the slot's next owner)."""
    gone = set(int(s) for s in slots)
    return [{i: s for i, s in kp.items() if s not in gone} for kp in kf_points]


def cull_points(tables, live, cand, min_observations):
    """-> (culled int32, tables afterwards, live afterwards, n_cleared)"""
    n = OBS.n_observers(tables, live)
    culled = np.array([s for s in np.asarray(cand).reshape(-1).tolist() if n[s] < min_observations], np.int32)
    t, lv, c = remove_points(tables, live, culled)
    return culled, t, lv, c
