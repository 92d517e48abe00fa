"""Specification of the loop correction on the resident map (include/orbx.h, "loop correction on the resident map"), in numpy f64.

affected          A: the keyframes within max_depth arcs of cur, written as the reference's FIFO walk        (corrector.rs:433-465)
affected_by_distance  the same set as a distance computation: the two forms check each other
affected_points   the distinct live slots of A's tables, keyframes ascending, features in index order          (:467-480)
sim3_inverse      C = sim3^-1 as (q_c, t_c, s_c)                                                                (sim3.rs:144-154)
correct_points / correct_pose   s_c (R_c p) + t_c; (q_c * q, s_c (R_c t) + t_c)                                (:493-515)
pairs             the matches as slot pairs, -1 where a match is no pair                                        (loop_closer.rs:168-173)
fuse              classes, keepers, goners and the rewritten tables                                             (:572-619, order-free)
correct_loop      all of it: what orbx_map_correct_loop_device computes
replay_reference  apply_correction + fuse_map_points restated sequentially, with observation counts that change as it goes
"""
from collections import deque

import numpy as np

import covisibility_spec as CS
import map_observations_spec as OS


def affected(tables, live, parent, cur, min_weight, max_depth):
    """-> uint8 [K].  The reference's walk: a queue of (keyframe, depth), visited on push, skipped past max_depth on pop."""
    K = len(tables)
    w = CS.weights(tables, live, range(K))
    out = np.zeros(K, np.uint8)
    visited = {cur}
    queue = deque([(cur, 0)])
    while queue:
        k, depth = queue.popleft()
        if depth > max_depth:
            continue
        out[k] = 1
        for c in range(K):                                   # spanning-tree children
            if parent[c] == k and c not in visited:
                visited.add(c); queue.append((c, depth + 1))
        for j in range(K):                                   # strong covisibility
            if j != k and w[k, j] >= min_weight and j not in visited:
                visited.add(j); queue.append((j, depth + 1))
    return out


def affected_by_distance(tables, live, parent, cur, min_weight, max_depth):
    """-> uint8 [K]: arc distance from cur <= max_depth, by relaxation to the fixed point"""
    K = len(tables)
    w = CS.weights(tables, live, range(K))
    arc = (w >= min_weight) & ~np.eye(K, dtype=bool)
    for c in range(K):
        if parent[c] >= 0:
            arc[parent[c], c] = True
    INF = 1 << 30
    d = np.full(K, INF, np.int64); d[cur] = 0
    for _ in range(K):
        nd = d.copy()
        for k in range(K):
            if d[k] < INF:
                nd[arc[k]] = np.minimum(nd[arc[k]], d[k] + 1)
        if np.array_equal(nd, d):
            break
        d = nd
    return (d <= max_depth).astype(np.uint8)


def affected_points(tables, live, aff):
    """-> int32 [P]"""
    seen, out = set(), []
    for k, t in enumerate(tables):
        if not aff[k] or t is None:
            continue
        for s in np.asarray(t).reshape(-1).tolist():
            if 0 <= s < len(live) and live[s] and s not in seen:
                seen.add(s); out.append(s)
    return np.array(out, np.int32)


def _rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def sim3_inverse(sim3):
    """(qw,qx,qy,qz, tx,ty,tz, s) -> (q_c [4], t_c [3], s_c)"""
    s = np.asarray(sim3, np.float64)
    qc = s[:4] * np.array([1.0, -1.0, -1.0, -1.0])
    sc = 1.0 / s[7]
    return qc, -(_rot(qc) @ s[4:7]) * sc, sc


def correct_points(sim3, p):
    qc, tc, sc = sim3_inverse(sim3)
    return sc * (np.asarray(p, np.float64).reshape(-1, 3) @ _rot(qc).T) + tc


def correct_pose(sim3, pose):
    qc, tc, sc = sim3_inverse(sim3)
    pose = np.asarray(pose, np.float64)
    return np.concatenate([_qmul(qc, pose[:4]), sc * (_rot(qc) @ pose[4:]) + tc])


def tolerance(sim3, p):
    """per point (or translation) the bound of the module's docstring in tests/test_loop_correct_gpu.py: 1e-13 (s_c |p| + |t_c|)"""
    qc, tc, sc = sim3_inverse(sim3)
    return 1e-13 * (sc * np.linalg.norm(np.asarray(p, np.float64).reshape(-1, 3), axis=1) + np.linalg.norm(tc))


def pairs(tables, live, cur, loop, matches):
    """-> int32 [n][2]: (a, b), or (-1, -1) where the match is no pair"""
    out = np.full((len(matches), 2), -1, np.int32)
    ok = lambda s: 0 <= s < len(live) and live[s]
    for m, (fc, fl) in enumerate(np.asarray(matches).reshape(-1, 2).tolist()):
        tc, tl = tables[cur], tables[loop]
        a = int(tc[fc]) if tc is not None and 0 <= fc < len(tc) else -1
        b = int(tl[fl]) if tl is not None and 0 <= fl < len(tl) else -1
        if ok(a) and ok(b) and a != b:
            out[m] = (a, b)
    return out


def fuse(tables, live, pr):
    """pr: pairs()' output -> (new tables, goner int32 [G], keeper int32 [G]) by ascending goner slot"""
    nobs = OS.n_observers(tables, live)
    flat = [int(s) for s in pr.reshape(-1).tolist() if s >= 0]
    first = {}
    for i, s in enumerate(flat):
        first.setdefault(s, i)
    root = {s: s for s in first}

    def find(s):
        while root[s] != s:
            root[s] = root[root[s]]; s = root[s]
        return s
    for a, b in pr.tolist():
        if a >= 0:
            root[find(a)] = find(b)
    classes = {}
    for s in first:
        classes.setdefault(find(s), []).append(s)
    to = {}
    for members in classes.values():
        keeper = min(members, key=lambda s: (-int(nobs[s]), first[s]))
        for s in members:
            if s != keeper:
                to[s] = keeper
    new = [None if t is None else np.array([to.get(int(s), int(s)) for s in np.asarray(t).tolist()], np.int32).reshape(-1) for t in tables]
    goner = np.array(sorted(to), np.int32)
    return new, goner, np.array([to[int(g)] for g in goner], np.int32)


def uniq(table):
    """d_mp_uniq: the table with every repeat of a slot set to -1"""
    seen, out = set(), []
    for s in np.asarray(table).tolist():
        out.append(s if s >= 0 and s not in seen else -1)
        seen.add(s)
    return np.array(out, np.int32)


def correct_loop(tables, live, positions, poses, parent, cur, loop, sim3, matches, min_weight=15, max_depth=100):
    """-> dict: counts [4], affected [K], poses_wc [K][7], list_slot [P], goner, keeper, tables (after), positions (after; goners keep
    their rows: only the live byte goes, in the host form), live_after"""
    live = np.asarray(live, np.uint8)
    aff = affected(tables, live, parent, cur, min_weight, max_depth)
    lst = affected_points(tables, live, aff)
    pos = np.array(positions, np.float64, copy=True)
    if len(lst):
        pos[lst] = correct_points(sim3, pos[lst])
    pw = np.array([correct_pose(sim3, p) if a else np.asarray(p, np.float64) for p, a in zip(poses, aff)]).reshape(-1, 7)
    pr = pairs(tables, live, cur, loop, matches) if len(matches) else np.zeros((0, 2), np.int32)
    new, goner, keeper = fuse(tables, live, pr)
    la = live.copy(); la[goner] = 0
    counts = np.array([int(aff.sum()), len(lst), int((pr[:, 0] >= 0).sum()), len(goner)], np.int32)
    return dict(counts=counts, affected=aff, poses_wc=pw, list_slot=lst, goner=goner, keeper=keeper, tables=new, positions=pos, live_after=la, pairs=pr)


def replay_reference(tables, live, positions, poses, parent, cur, loop, sim3, matches, min_weight=15, max_depth=100):
    """apply_correction (:520-555) and fuse_map_points (:572-619) as the reference runs them: the corrected poses and points written,
    then the pairs one after another — skip a == b, observation counts read NOW (mp.observations: one feature per keyframe, the first
    that names the point), the current keyframe's point kept on ties, the goner's observers re-pointed at the recorded feature if it
    still names the goner, the observation added to the keeper (the last add wins the keyframe's feature), the goner removed.
    Meaningful where every point is associated once per keyframe.  -> (tables, live_after, positions, poses_wc)"""
    live = np.asarray(live, np.uint8).copy()
    aff = affected(tables, live, parent, cur, min_weight, max_depth)
    pos = np.array(positions, np.float64, copy=True)
    for s in affected_points(tables, live, aff).tolist():
        pos[s] = correct_points(sim3, pos[s])[0]
    pw = np.array([correct_pose(sim3, p) if a else np.asarray(p, np.float64) for p, a in zip(poses, aff)]).reshape(-1, 7)
    tabs = [None if t is None else np.array(t, np.int32, copy=True) for t in tables]
    obs = {}                                                  # slot -> {keyframe: feature}
    for k, t in enumerate(tabs):
        for s, f in OS.observed_at(t, live).items():
            obs.setdefault(s, {})[k] = f
    for a, b in pairs(tables, live, cur, loop, matches).tolist() if len(matches) else []:
        if a < 0 or a == b or not live[a] or not live[b]:
            continue
        keep, gone = (a, b) if len(obs.get(a, {})) >= len(obs.get(b, {})) else (b, a)
        for k, f in list(obs.get(gone, {}).items()):
            if tabs[k][f] == gone:
                tabs[k][f] = keep
            obs.setdefault(keep, {})[k] = f
        obs.pop(gone, None)
        live[gone] = 0
        for t in tabs:                                       # remove_map_point: whatever still names it
            if t is not None:
                t[t == gone] = -1
    return tabs, live, pos, pw
