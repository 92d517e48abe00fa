"""Specification of covisibility on the resident map (include/orbx.h, "covisibility from the resident map"), in numpy.

observed          obs(k): the distinct live slots of a keyframe's slot table (None as a table: nothing)
weights           weight[q][k] = |obs(query[q]) & obs(k)|, 0 for k == query[q]            (map.rs:361-383, keyframe.rs:270-273)
best              weight > 0, weight descending then index ascending, at most n, -1 padded (keyframe.rs:313-345, map.rs:476-489)
local_keyframes   [r] ++ best(r, n_best), or every keyframe for r == -1                    (tracker.rs:826-843)
associate_replay  the reference's incremental update, literally: the case the derived definition must reproduce
"""
import numpy as np


def observed(table, live):
    if table is None:
        return set()
    live = np.asarray(live)
    return {int(s) for s in np.asarray(table).reshape(-1).tolist() if 0 <= s < len(live) and live[s]}


def weights(tables, live, queries):
    """-> int32 [len(queries), len(tables)]"""
    obs = [observed(t, live) for t in tables]
    w = np.zeros((len(queries), len(tables)), np.int32)
    for i, q in enumerate(queries):
        for k in range(len(tables)):
            if k != q:
                w[i, k] = len(obs[q] & obs[k])
    return w


def best(row, n):
    """one weight row -> (int32 [n] indices, -1 padded; how many are not padding)"""
    row = np.asarray(row)
    order = sorted((k for k in range(len(row)) if row[k] > 0), key=lambda k: (-int(row[k]), k))[:max(n, 0)]
    out = np.full(max(n, 0), -1, np.int32)
    out[:len(order)] = order
    return out, len(order)


def best_rows(w, n):
    """weights [Q, K] -> (best int32 [Q, n], n_best int32 [Q])"""
    rows = [best(r, n) for r in w]
    return (np.stack([r[0] for r in rows]) if rows else np.zeros((0, max(n, 0)), np.int32)), np.array([r[1] for r in rows], np.int32)


def local_keyframes(tables, live, ref, n_best):
    """-> (the frame's keyframe indices in order, the local_kf row int32 [1 + n_best] the call reports)"""
    if ref < 0:
        return list(range(len(tables))), np.full(1 + n_best, -1, np.int32)
    b, n = best(weights(tables, live, [ref])[0], n_best)
    return [int(ref)] + b[:n].tolist(), np.concatenate([[ref], b]).astype(np.int32)


def associate_replay(tables, live):
    """Map::associate (map.rs:339-386) replayed: the keyframes are inserted in order and every feature that carries a live point is
    associated once, in feature order; each association adds 1 to the weight between the new observer and every earlier observer of
    the point (:361-383), both ways.  Meaningful where every point is associated once per keyframe (no repeats inside a table).
    -> int32 [K, K] (symmetric, zero diagonal)"""
    K = len(tables)
    w = np.zeros((K, K), np.int32)
    observers = {}
    live = np.asarray(live)
    for k, t in enumerate(tables):
        for s in ([] if t is None else np.asarray(t).reshape(-1).tolist()):
            if s < 0 or not live[s]:
                continue
            for o in observers.setdefault(s, []):
                if o != k:
                    w[k, o] += 1; w[o, k] += 1
            observers[s].append(k)
    return w
