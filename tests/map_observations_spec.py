"""Specification of the observation calls on the resident map (include/orbx.h, "observations from the resident map"), in numpy.

observed_at       obs(k) with the observing feature: {slot: the first feature of the keyframe that names it}, live slots only
observations      per asked slot the pairs (k, feat) by ascending k, as CSR arrays        (map_point.rs:140-156: mp.observations)
n_observers       |observations(s)| for every slot of the store
refresh           tests/map_point_refresh_spec.py on the derived lists and the store's rows   (search_in_neighbors.rs:139-150)
redundancy        total / redundant / cull of candidate keyframes                             (local_mapper.rs:487-583)
cull_keyframes_replay  the reference's loop on a dict-of-sets map, literally: what `redundancy` must reproduce
"""
import numpy as np

import map_point_refresh_spec as R


def observed_at(table, live):
    out = {}
    if table is None:
        return out
    live = np.asarray(live)
    for i, s in enumerate(np.asarray(table).reshape(-1).tolist()):
        if 0 <= s < len(live) and live[s] and s not in out:
            out[s] = i
    return out


def observations(tables, live, slots):
    """-> (obs_start int32 [M+1], obs_kf int32 [N], obs_feat int32 [N])"""
    at = [observed_at(t, live) for t in tables]
    start, kf, feat = [0], [], []
    for s in np.asarray(slots).reshape(-1).tolist():
        for k in range(len(tables)):
            if s in at[k]:
                kf.append(k); feat.append(at[k][s])
        start.append(len(kf))
    return np.array(start, np.int32), np.array(kf, np.int32), np.array(feat, np.int32)


def n_observers(tables, live):
    """-> int32 [capacity]"""
    n = np.zeros(len(live), np.int32)
    for t in tables:
        for s in observed_at(t, live):
            n[s] += 1
    return n


def refresh(tables, live, slots, positions, desc, kf_poses_wc, kf_descs, scale_range, normals):
    """positions [capacity,3] / desc [capacity,32]: the store's rows; kf_descs: per keyframe its descriptors [n,32]; normals [M,3]:
    the points' normals before the call.  -> (map_point_refresh_spec.refresh's dict for the M points, the scene it was given: the
    arguments of the existing refresh calls)"""
    slots = np.asarray(slots, np.int32).reshape(-1)
    start, kf, feat = observations(tables, live, slots)
    off = np.zeros(len(tables) + 1, np.int32); off[1:] = np.cumsum([len(d) for d in kf_descs])
    sc = dict(positions=np.ascontiguousarray(np.asarray(positions)[slots]), obs_start=start, obs_kf=kf, obs_feat=feat,
              kf_poses_wc=np.asarray(kf_poses_wc, np.float64).reshape(-1, 7), kf_feat_offset=off,
              descs=np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in kf_descs] + [np.zeros((0, 32), np.uint8)]), scale_range=scale_range,
              mp_desc=np.ascontiguousarray(np.asarray(desc)[slots]), normals=np.asarray(normals, np.float64).reshape(-1, 3))
    return R.refresh(sc), sc


def redundancy(tables, live, cand, min_observations, threshold):
    """-> (total int32 [n_cand], redundant int32 [n_cand], cull u8 [n_cand])"""
    live = np.asarray(live)
    n = n_observers(tables, live)
    total, red, cull = [], [], []
    for c in np.asarray(cand).reshape(-1).tolist():
        t = r = 0
        for s in ([] if tables[c] is None else np.asarray(tables[c]).reshape(-1).tolist()):
            if 0 <= s < len(live) and live[s]:
                t += 1
                r += int(n[s]) - 1 >= min_observations
        total.append(t); red.append(r)
        cull.append(1 if t > 0 and float(r) / float(t) > threshold else 0)          # Python floats are f64: one IEEE division
    return np.array(total, np.int32), np.array(red, np.int32), np.array(cull, np.uint8)


def cull_keyframes_replay(kf_points, mp_observers, candidates, min_observations, threshold):
    """local_mapper.rs:536-570 on a host map: kf_points {kf: [map point id or None per feature]} (map_point_ids), mp_observers
    {map point id: set of keyframes} (mp.observations' keys; a point that is not in it is gone).  Decisions are collected first and
    nothing is removed in between (to_cull, :571-583).  -> {kf: (total, redundant, cull)}"""
    out = {}
    for kf in candidates:
        total = redundant = 0
        for mp in kf_points[kf]:                                            # :539-547
            if mp is None or mp not in mp_observers:
                continue
            total += 1
            others = sum(1 for o in mp_observers[mp] if o != kf)            # :549-555
            if others >= min_observations:
                redundant += 1
        out[kf] = (total, redundant, total > 0 and float(redundant) / float(total) > threshold)      # :561-565, strict
    return out
