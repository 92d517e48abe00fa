"""The specification of orbx_refresh_map_points (include/orbx.h) as plain Python / numpy in f64 — test infrastructure only.

Restates, for a batch of map points, Map::compute_distinctive_descriptors (src/atlas/map/map.rs:880-944) and
Map::update_map_point_normal_and_depth (map.rs:716-742) with MapPoint::update_normal_and_depth (src/atlas/map/map_point.rs:173-203)
of the reference.  The reference iterates HashMaps at both places; the stated order is the order of the point's observation list as
the caller hands it over (the convention of include/orbx_map.hpp).  scale_range = scale_factor.powi(num_levels - 1) is computed by the
caller.  Every float expression is one IEEE operation at a time, in the order written here (Python floats are f64, math.sqrt is
correctly rounded).

A scene is a dict: positions [M,3], obs_start [M+1], obs_kf [N], obs_feat [N], kf_poses_wc [T,7] (camera centre = columns 4..6),
kf_feat_offset [T+1], descs [F,32] u8, scale_range, mp_desc [M,32] u8, normals [M,3] (the points' values before the call)."""
import math

import numpy as np

RECORD = np.dtype([("chosen", "<i4"), ("best_max_dist", "<u4"), ("n_desc", "<u4"), ("n_observers", "<u4")])
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint32)


def hamming(a, b):
    """descriptor_distance (tracking/frame.rs): bits that differ between two 32-byte rows."""
    return int(_POP[np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))].sum())


def distinctive_descriptor(rows):
    """map.rs:916-936 over the collected rows [c,32], c >= 2 -> (index among the collected, best_max_dist, maxima [c])."""
    rows = np.asarray(rows, np.uint8)
    d = _POP[rows[:, None, :] ^ rows[None, :, :]].sum(-1)           # d[i,i] = 0 and max_dist starts at 0: the row maximum is max over j != i
    maxima = d.max(1)
    best_idx, best = 0, 0xFFFFFFFF
    for i, m in enumerate(maxima):                                   # strict <: the earliest of equal maxima (:932)
        if int(m) < best:
            best, best_idx = int(m), i
    return best_idx, best, maxima


def refresh_point(position, obs, kf_centres, kf_descs, scale_range, desc_in, normal_in):
    """One map point.  obs: [(kf, feat)] in list order; kf_centres [T,3]; kf_descs: list of T arrays [n_t,32].
    Returns (desc [32], normal (3), min_distance, max_distance, record tuple, aux dict)."""
    T = len(kf_centres)
    # ---- descriptor (map.rs:880-944)
    rows, at = [], []
    for k, (kf, feat) in enumerate(obs):
        if 0 <= kf < T and 0 <= feat < len(kf_descs[kf]):            # keyframes.get(kf) is Some, descriptors.row(feat) is Ok
            rows.append(kf_descs[kf][feat]); at.append(k)
    unique_min = True
    if len(rows) == 0:
        desc, chosen, best = np.array(desc_in, np.uint8), -1, 0
    elif len(rows) == 1:
        desc, chosen, best = np.array(rows[0], np.uint8), at[0], 0
    else:
        i, best, maxima = distinctive_descriptor(rows)
        desc, chosen = np.array(rows[i], np.uint8), at[i]
        unique_min = int((maxima == best).sum()) == 1
    # ---- normal and depth (map_point.rs:179-202)
    sx = sy = sz = 0.0
    min_dist, max_dist = math.inf, 0.0
    n_observers, dirs = 0, []
    px, py, pz = (float(v) for v in position)
    for kf, _ in obs:
        if not 0 <= kf < T:
            continue
        n_observers += 1
        cx, cy, cz = (float(v) for v in kf_centres[kf])
        dx, dy, dz = px - cx, py - cy, pz - cz
        dist = math.sqrt((dx * dx + dy * dy) + dz * dz)
        if dist > 1e-10:
            ux, uy, uz = dx / dist, dy / dist, dz / dist
            sx += ux; sy += uy; sz += uz
            min_dist = min(min_dist, dist)
            max_dist = max(max_dist, dist)
            dirs.append((ux, uy, uz))
    norm = math.sqrt((sx * sx + sy * sy) + sz * sz)
    kept = not norm > 1e-10
    normal = tuple(float(v) for v in normal_in) if kept else (sx / norm, sy / norm, sz / norm)
    aux = dict(unique_min=unique_min, sum_norm=norm, n_dirs=len(dirs), dirs=dirs, normal_kept=kept)
    return desc, normal, min_dist / scale_range, max_dist * scale_range, (chosen, best, len(rows), n_observers), aux


def refresh(scene):
    """Every point of a scene -> dict(mp_desc, normals, min_distance, max_distance, records, aux [M])."""
    M = len(scene["positions"])
    off = np.asarray(scene["kf_feat_offset"], np.int64)
    descs = np.asarray(scene["descs"], np.uint8).reshape(-1, 32)
    kf_descs = [descs[off[t]:off[t + 1]] for t in range(len(off) - 1)]
    centres = np.asarray(scene["kf_poses_wc"], np.float64).reshape(-1, 7)[:, 4:7]
    out = dict(mp_desc=np.zeros((M, 32), np.uint8), normals=np.zeros((M, 3)), min_distance=np.zeros(M), max_distance=np.zeros(M),
               records=np.zeros(M, RECORD), aux=[])
    for p in range(M):
        s, e = int(scene["obs_start"][p]), int(scene["obs_start"][p + 1])
        obs = [(int(scene["obs_kf"][o]), int(scene["obs_feat"][o])) for o in range(s, e)]
        d, n, mn, mx, rec, aux = refresh_point(scene["positions"][p], obs, centres, kf_descs, float(scene["scale_range"]), scene["mp_desc"][p],
                                               scene["normals"][p])
        out["mp_desc"][p] = d; out["normals"][p] = n; out["min_distance"][p] = mn; out["max_distance"][p] = mx
        out["records"][p] = rec
        out["aux"].append(aux)
    return out
