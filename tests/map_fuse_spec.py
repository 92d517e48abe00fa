"""Specification of fuse and merge on the resident map (include/orbx.h, "fuse and merge on the resident map"), in numpy / plain
Python, taking the search as a function.

fuse              one pass fuse(src, tgt): L, the skipped pairs, the matches, classes by union-find, keepers, the rewritten tables
search_in_neighbors   pass A = fuse([cur], nb), pass B = fuse(nb, [cur]) on A's tables, the goners erased, the affected list
reference_replay  fuse_points_into_keyframes (search_in_neighbors.rs:254-387) and Map::merge_map_points (map.rs:770-868), literally
                  and sequentially over tables, in L order and target order: what `fuse` equals under the four agreement conditions

search(positions [P,3], desc [P,32], tgt) -> int32 [P, len(tgt)]: the feature orbx_keyframe_fuse_search returns for every point
against every keyframe tgt[t], or -1, with no pair skipped.  The tests pass the oracle's fuse_search.
"""
import numpy as np

import map_observations_spec as OSP
import map_store_spec as MSP


def _live(live, s):
    return 0 <= s < len(live) and bool(live[s])


def fuse(tables, live, positions, desc, src, tgt, search):
    """tables: per keyframe an int array or None; live [capacity]; positions / desc: the store's rows; src / tgt: positions in tables.
    -> dict(counts int32 [4], list_slot int32 [P], match int32 [P, n_tgt], goner / keeper int32 [goners], tables (the new ones: a
    target's None becomes an array, every other None stays), skipped (pairs skipped as observed), stats)"""
    live = np.asarray(live)
    src, tgt = [int(i) for i in src], [int(i) for i in tgt]
    T = len(tgt)
    tabs = [None if t is None else np.array(t, np.int32).reshape(-1) for t in tables]
    L = MSP.select_keyframes([tabs[i] for i in src], live)
    P = len(L)
    obs = [OSP.observed_at(t, live) for t in tabs]
    nobs = OSP.n_observers(tabs, live)
    match = np.full((P, T), -1, np.int32)
    skipped = 0
    if P and T:
        raw = np.asarray(search(np.ascontiguousarray(np.asarray(positions)[L]), np.ascontiguousarray(np.asarray(desc)[L]), tgt), np.int32).reshape(P, T)
        for j in range(P):
            for t in range(T):
                if int(L[j]) in obs[tgt[t]]:
                    skipped += 1                                             # :272
                else:
                    match[j, t] = raw[j, t]
    # classes: union-find over slots
    parent = {}

    def find(s):
        parent.setdefault(s, s)
        while parent[s] != s:
            parent[s] = parent[parent[s]]
            s = parent[s]
        return s

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    claims = {}                                                              # (t, f) -> the claimants, as positions in L
    for j in range(P):
        find(int(L[j]))
        for t in range(T):
            f = int(match[j, t])
            if f < 0:
                continue
            tab = tabs[tgt[t]]
            e = -1 if tab is None else int(tab[f])
            if _live(live, e):
                union(int(L[j]), e)
            else:
                claims.setdefault((t, f), []).append(j)
    for js in claims.values():
        for j in js[1:]:
            union(int(L[js[0]]), int(L[j]))
    members = {}
    for s in list(parent):
        members.setdefault(find(s), []).append(s)
    claimed = {find(int(L[js[0]])) for js in claims.values()}
    place = {int(s): j for j, s in enumerate(L)}
    keeper_of, goners = {}, []
    for r, ms in members.items():
        if len(ms) < 2 and r not in claimed:
            continue
        k = max(ms, key=lambda s: (int(nobs[s]), 1, -place[s]) if s in place else (int(nobs[s]), 0, -s))
        keeper_of[r] = k
        goners += [(s, k) for s in ms if s != k]
    goners.sort()
    # tables
    out = [None if t is None else t.copy() for t in tabs]
    for t in tgt:
        if out[t] is None:
            out[t] = np.full(len_of(tables, t), -1, np.int32)
    added = 0
    names_and_claims = 0
    for k in range(len(tabs)):
        if out[k] is None:
            continue
        old = out[k].copy()
        G = {}
        for i, e in enumerate(old.tolist()):
            if _live(live, e) and e in parent and find(e) in keeper_of:
                G.setdefault(find(e), []).append(i)
        named, claiming = set(G), set()
        for (t, f), js in claims.items():
            if tgt[t] == k:
                r = find(int(L[js[0]]))
                G.setdefault(r, []).append(f)
                claiming.add(r)
        names_and_claims += 1 if named & claiming else 0                  # keyframes where a class both names and claims
        for r, feats in G.items():
            feats = sorted(set(feats))
            kp = keeper_of[r]
            if any(old[i] == kp for i in feats):
                for i in feats:
                    if old[i] != kp:
                        out[k][i] = -1
            else:
                out[k][feats[0]] = kp
                for i in feats[1:]:
                    out[k][i] = -1
        added += sum(1 for o, n in zip(old.tolist(), out[k].tolist()) if n != o and n >= 0 and not _live(live, o))
    counts = np.array([P, int((match >= 0).sum()), added, len(goners)], np.int32)
    stats = dict(members=members, keeper_of=keeper_of, claims=claims, place=place, nobs=nobs, names_and_claims=names_and_claims)
    return dict(counts=counts, list_slot=np.asarray(L, np.int32), match=match, goner=np.array([g for g, _ in goners], np.int32),
                keeper=np.array([k for _, k in goners], np.int32), tables=out, skipped=skipped, stats=stats)


def len_of(tables, k):
    """features of a keyframe without a table: the scenes keep them in tables.counts where they have one"""
    n = getattr(tables, "counts", None)
    if n is None:
        raise ValueError("a target without a table needs tables.counts")
    return int(n[k])


class Tables(list):
    """a list of tables that also knows every keyframe's feature count (a keyframe without a table has one too)"""

    def __init__(self, tables, counts):
        super().__init__(tables)
        self.counts = [int(c) for c in counts]


def search_in_neighbors(tables, live, positions, desc, cur, nb, search):
    """-> dict(a, b: the two passes' `fuse` results, live: the live bytes after the erase, tables: the final tables, affected int32 [M])"""
    nb = [int(i) for i in nb]
    a = fuse(tables, live, positions, desc, [cur], nb, search)
    ta = Tables(a["tables"], tables.counts)
    b = fuse(ta, live, positions, desc, nb, [cur], search)
    after = np.array(live, np.uint8, copy=True)
    after[a["goner"]] = 0; after[b["goner"]] = 0
    final = Tables(b["tables"], tables.counts)
    affected = MSP.select_keyframes([final[i] for i in [cur] + nb], after)
    return dict(a=a, b=b, live=after, tables=final, affected=np.asarray(affected, np.int32))


def reference_replay(tables, live, positions, desc, src, tgt, search):
    """The reference's loop over a host map made from the tables: kf.map_point_ids = the table (a slot that is not live: None),
    mp.observations = {keyframe: feature} filled in feature order (add_observation: the last one wins).  The goner's observations
    are walked by ascending keyframe.  -> (tables after the walk, goners in the order they were removed, num_fused, num_obs_added)"""
    live = np.asarray(live)
    src, tgt = [int(i) for i in src], [int(i) for i in tgt]
    kf_mp = [[] if t is None else [int(e) if _live(live, int(e)) else None for e in np.asarray(t).tolist()] for t in tables]
    for t in tgt:
        if tables[t] is None:
            kf_mp[t] = [None] * len_of(tables, t)
    observations = {int(s): {} for s in np.flatnonzero(live)}
    for k, ids in enumerate(kf_mp):
        for i, m in enumerate(ids):
            if m is not None:
                observations[m][k] = i
    L = MSP.select_keyframes([tables[i] for i in src], live)
    raw = np.asarray(search(np.ascontiguousarray(np.asarray(positions)[L]), np.ascontiguousarray(np.asarray(desc)[L]), tgt), np.int32).reshape(len(L), len(tgt))
    removed, num_fused, num_obs_added = [], 0, 0

    def merge(keeper, goner):                                                # map.rs:770-868
        if keeper == goner or goner not in observations or keeper not in observations:
            return False
        for kf, feat in sorted(observations[goner].items()):
            if kf in observations[keeper]:
                kf_mp[kf][feat] = None                                       # erase_map_point
            else:
                kf_mp[kf][feat] = keeper
                observations[keeper][kf] = feat
        del observations[goner]
        removed.append(goner)
        return True

    for j, mp in enumerate(int(s) for s in L):                               # :254
        if mp not in observations:
            continue                                                         # :256-263: the point is gone
        observers = set(observations[mp])                                    # :260: taken once per point
        for t, kf in enumerate(tgt):                                         # :270
            if kf in observers:
                continue
            f = int(raw[j, t])
            if f < 0:
                continue
            existing = kf_mp[kf][f]                                          # :347-349
            if existing is not None and existing != mp:
                a = len(observations.get(mp, ()))
                b = len(observations.get(existing, ()))
                keeper, goner = (mp, existing) if a >= b else (existing, mp)     # :365-369
                if merge(keeper, goner):
                    num_fused += 1
            elif existing is None:
                if mp in observations:                                       # Map::associate: false where the point is gone
                    observations[mp][kf] = f
                    kf_mp[kf][f] = mp
                num_obs_added += 1
    out = [None if (tables[k] is None and k not in tgt) else np.array([-1 if m is None else m for m in ids], np.int32) for k, ids in enumerate(kf_mp)]
    return out, removed, num_fused, num_obs_added
