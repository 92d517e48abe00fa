"""Seeded worlds for fuse and merge on the resident map, on tests/map_store_scenes.py's stores: keyframes with poses, keypoints and
descriptors; landmarks that really project into them; descriptors a few bits from their features.

A landmark has a position and a 256-bit descriptor, and one to three slots in the store (duplicates: what the pass merges), each
with the landmark's position and its descriptor a few bits off.  A keyframe that sees a landmark has a feature at its projection
whose descriptor is a few bits off too and whose table entry is one of the slots, -1 or a slot that is not live.  Random
descriptors are about 128 bits apart, landmark rows 16 at most: a point matches features of its own landmark only, far from the
threshold, and every feature lies within a pixel of its projection where the search radius is 10: no decision is near its edge.

world(seed)        keyframe 0 is the current one; 1, 2, 3 regular targets; 4, 5 observers that are not targets; 6 a keyframe of 2100
                   features (FUSE_CHUNK is 2048); 7 a keyframe without a table; 8 an empty one.  TGT = [1, 2, 3, 6, 7, 8].
agree_world(seed)  a world that meets the four conditions under which the pass equals the sequential reference
"""
import numpy as np

import ba_collect_scenes as B
import map_fuse_spec as S
import tracking_scenes as G

CAPACITY = 1024
CAMERA = G.CAMERA
RADIUS_SCALE = 3.0 * (1.2 * (1.2 * 1.2) * ((1.2 * 1.2) * (1.2 * 1.2)))      # radius_factor * 1.2.powi(7) (search_in_neighbors.rs:303)
SCALE_RANGE = 1.2 ** 7
CUR, TGT, ALL_NB = 0, [1, 2, 3, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7, 8]


def _flip(rng, d, k):
    out = d.copy()
    for b in rng.permutation(256)[:k]:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


class _Builder:
    def __init__(self, seed, n_kf, capacity):
        self.rng = np.random.default_rng(seed)
        self.capacity = capacity
        self.free = list(self.rng.permutation(capacity))
        self.positions = np.zeros((capacity, 3)); self.desc = np.zeros((capacity, 32), np.uint8); self.live = np.zeros(capacity, np.uint8)
        self.feats = [[] for _ in range(n_kf)]                               # per keyframe (xyz, desc, entry)
        self.poses = np.zeros((n_kf, 7)); self.poses[:, 0] = 1.0
        for k in range(n_kf):
            a = self.rng.uniform(-0.02, 0.02)
            self.poses[k, :4] = [np.cos(a / 2), 0.0, np.sin(a / 2), 0.0]
            self.poses[k, 4:] = self.rng.uniform(-0.3, 0.3, 3)

    def landmark(self):
        rng = self.rng
        return np.array([rng.uniform(-1.8, 1.8), rng.uniform(-1.0, 1.0), rng.uniform(5.0, 9.0)]), rng.integers(0, 256, 32, dtype=np.uint8)

    def slot(self, lm, live=True):
        s = int(self.free.pop())
        self.positions[s] = lm[0] + self.rng.uniform(-1e-3, 1e-3, 3)
        self.desc[s] = _flip(self.rng, lm[1], int(self.rng.integers(1, 6)))
        self.live[s] = 1 if live else 0
        return s

    def see(self, k, lm, entry, desc=None):
        """keyframe k gets a feature at the landmark's projection; desc: the feature's descriptor, exactly"""
        d = _flip(self.rng, lm[1], int(self.rng.integers(0, 6))) if desc is None else desc.copy()
        self.feats[k].append((lm[0], d, int(entry), True))

    def clutter(self, k, n, entries):
        for i in range(n):
            lm = self.landmark()
            self.feats[k].append((lm[0], lm[1], int(entries[i]) if i < len(entries) else -1, False))

    def finish(self, no_table=(), counts=None):
        rng = self.rng
        tables, xys, descs = [], [], []
        for k, fs in enumerate(self.feats):
            order = rng.permutation(len(fs))
            fs = [fs[i] for i in order]
            if len(fs) > 2048:                                              # a landmark's features past the search's first chunk of 2048
                fs.sort(key=lambda f: f[3] and f[2] == -1)
            if fs:
                uv, _ = B._project(self.poses[k], np.stack([f[0] for f in fs]), CAMERA)
                uv = uv + rng.uniform(-0.4, 0.4, uv.shape)
            else:
                uv = np.zeros((0, 2))
            xys.append(uv.astype(np.float32)); descs.append(np.stack([f[1] for f in fs]) if fs else np.zeros((0, 32), np.uint8))
            tables.append(None if k in no_table else np.array([f[2] for f in fs], np.int32))
        return dict(tables=S.Tables(tables, [len(x) for x in xys]), xy=xys, descs=descs, poses=self.poses, positions=self.positions, desc=self.desc,
                    live=self.live, capacity=self.capacity)


def keypoints(xy, dtype):
    kp = np.zeros(len(xy), dtype)
    kp["x"] = xy[:, 0]; kp["y"] = xy[:, 1]; kp["size"] = 31.0; kp["angle"] = -1.0
    return kp


def world(seed, capacity=CAPACITY):
    """-> dict(tables (map_fuse_spec.Tables), xy / descs per keyframe, poses [9,7], positions / desc / live: the store's host image)"""
    b = _Builder(seed, 9, capacity)
    rng = b.rng
    reg = [1, 2, 3, 6]
    pick = lambda pool, n: [int(x) for x in rng.permutation(pool)[:n]]
    for _ in range(70):                                                      # associations, and pairs skipped as observed
        lm = b.landmark(); s = b.slot(lm)
        b.see(0, lm, s)
        for k in pick([1, 2, 3, 6, 7], int(rng.integers(1, 4))):
            b.see(k, lm, -1)
        for k in pick([1, 2, 3, 4, 5], int(rng.integers(0, 3))):
            if not any(f[0] is lm[0] for f in b.feats[k]):
                b.see(k, lm, s)
    for _ in range(45):                                                      # observed by several targets already
        lm = b.landmark(); s = b.slot(lm)
        b.see(0, lm, s)
        for k in pick(reg, int(rng.integers(2, 4))):
            b.see(k, lm, s)
    for _ in range(30):                                                      # a duplicate with fewer observers: the projected point keeps
        lm = b.landmark(); s, s2 = b.slot(lm), b.slot(lm)
        x, y = pick([1, 2, 3], 2)
        b.see(0, lm, s); b.see(5, lm, s); b.see(x, lm, s); b.see(6, lm, s)
        b.see(y, lm, s2); b.see(4, lm, s2)                                   # (keyframe 4 is no target and observes the goner)
    for _ in range(25):                                                      # a duplicate with more observers: the existing point keeps
        lm = b.landmark(); s, s2 = b.slot(lm), b.slot(lm)
        b.see(0, lm, s)
        for k in (1, 2, 4):
            b.see(k, lm, s2)
        b.see(3, lm, -1)
    for _ in range(10):                                                      # three slots of one landmark
        lm = b.landmark(); s, s2, s3 = b.slot(lm), b.slot(lm), b.slot(lm)
        b.see(0, lm, s); b.see(5, lm, s); b.see(1, lm, s2); b.see(2, lm, s3); b.see(4, lm, s3)
    for _ in range(10):                                                      # two points of the current keyframe claim one feature
        lm = b.landmark(); s, s2 = b.slot(lm), b.slot(lm)
        b.see(0, lm, s); b.see(0, lm, s2)
        for k in pick([1, 2, 3, 7], 2):
            b.see(k, lm, -1)
    for i in range(12):                                                      # a class that a keyframe both names and is claimed by
        lm = b.landmark(); s, s2 = b.slot(lm), b.slot(lm)
        b.see(0, lm, s); b.see(1, lm, s2)
        if i % 2:
            b.see(4, lm, s); b.see(5, lm, s)                                 # the projected point keeps; else the existing one
        for k in ((2,) if i % 2 else (2, 3, 6)):
            b.see(k, lm, s2, desc=b.desc[s2]); b.see(k, lm, -1, desc=b.desc[s])
    for _ in range(6):                                                       # an entry that names a slot that is not live
        lm = b.landmark(); s = b.slot(lm); dead = b.slot(lm, live=False)
        b.see(0, lm, s); b.see(1, lm, dead); b.see(6, lm, dead)
    for _ in range(6):                                                       # equal counts: the projected point keeps
        lm = b.landmark(); s, s2 = b.slot(lm), b.slot(lm)
        b.see(0, lm, s); b.see(4, lm, s); b.see(1, lm, s2); b.see(5, lm, s2)
    for i in range(20):                                                      # points of the neighbours that the current keyframe sees unassociated:
        lm = b.landmark(); s = b.slot(lm)                                    # the pass back, fuse(neighbours, [current]); every fourth as two slots
        s2 = b.slot(lm) if i % 4 == 0 else s
        b.see(0, lm, -1); b.see(1, lm, s); b.see(2, lm, s2)
    others = [b.slot(b.landmark()) for _ in range(60)]                       # points only the other keyframes see
    b.clutter(0, 299 - len(b.feats[0]), [-1] * 20 + others[:10])
    for k in (1, 2, 3, 4, 5):
        b.clutter(k, 300 + k - len(b.feats[k]), pick(others, 40) + [-1] * 30 + pick(others, 3))
    b.clutter(6, 2100 - len(b.feats[6]), pick(others, 50))
    b.clutter(7, 301 - len(b.feats[7]), [])
    sc = b.finish(no_table=(7,))
    assert [len(x) for x in sc["xy"]] == [299, 301, 302, 303, 304, 305, 2100, 301, 0]
    return sc


def agree_world(seed, capacity=CAPACITY):
    """Classes of at most two members, no feature matched twice, every merge kept by the projected point, counts of a merged pair
    more than n_tgt = 3 apart; no repeats and no dead entries.  Keyframe 0 is the current one, 1..3 the targets, 4..9 observers."""
    b = _Builder(seed + 500, 10, capacity)
    rng = b.rng
    pick = lambda pool, n: [int(x) for x in rng.permutation(pool)[:n]]
    for _ in range(60):
        lm = b.landmark(); s = b.slot(lm)
        b.see(0, lm, s)
        ks = pick([1, 2, 3], int(rng.integers(1, 4)))
        for i, k in enumerate(ks):
            b.see(k, lm, s if i == 2 else -1)
    for _ in range(40):
        lm = b.landmark(); s, s2 = b.slot(lm), b.slot(lm)
        b.see(0, lm, s)
        for k in (4, 5, 6, 7, 8):
            b.see(k, lm, s)
        x, y = pick([1, 2, 3], 2)
        b.see(x, lm, s2); b.see(9, lm, s2)
        if rng.uniform() < 0.5:
            b.see(y, lm, -1)
    others = [b.slot(b.landmark()) for _ in range(40)]
    for k in range(10):
        b.clutter(k, 20, pick(others, 10))
    return b.finish()


def oracle_search(oracle, sc):
    """the search map_fuse_spec takes: the oracle's fuse_search against the scene's keyframes"""
    kps = [keypoints(xy, oracle.KEYPOINT) for xy in sc["xy"]]

    def search(positions, desc, tgt):
        off = np.zeros(len(tgt) + 1, np.int32); off[1:] = np.cumsum([len(kps[t]) for t in tgt])
        idx, _ = oracle.fuse_search(oracle.Camera(**CAMERA), positions, desc, sc["poses"][list(tgt)], off,
                                    np.concatenate([kps[t] for t in tgt] + [np.zeros(0, oracle.KEYPOINT)]),
                                    np.concatenate([sc["descs"][t] for t in tgt] + [np.zeros((0, 32), np.uint8)]), RADIUS_SCALE, 50)
        return idx
    return search


def scene_counts(sc, r, tgt):
    """what a scene is required to show, counted from a `fuse` result by the specification alone"""
    st, live = r["stats"], sc["live"]
    L = set(int(s) for s in r["list_slot"])
    kept_proj = sum(1 for g, k in zip(r["goner"], r["keeper"]) if int(k) in L and int(g) not in L)
    kept_exist = sum(1 for g, k in zip(r["goner"], r["keeper"]) if int(k) not in L and int(g) in L)
    big = sum(1 for ms in st["members"].values() if len(ms) >= 3)
    twice = sum(1 for js in st["claims"].values() if len(js) >= 2)
    goners = set(int(g) for g in r["goner"])
    outside = set()
    for k, t in enumerate(sc["tables"]):
        if k not in tgt and t is not None:
            outside |= goners & set(int(e) for e in np.asarray(t).tolist())
    dead = 0
    for j in range(len(r["list_slot"])):
        for t, k in enumerate(tgt):
            f = int(r["match"][j, t])
            if f >= 0 and sc["tables"][k] is not None:
                e = int(sc["tables"][k][f])
                dead += e >= 0 and not live[e]
    return dict(added=int(r["counts"][2]), kept_proj=kept_proj, kept_exist=kept_exist, big=big, twice=twice, names_and_claims=st["names_and_claims"],
                outside=len(outside), skipped=r["skipped"], dead=dead)


REQUIRED = dict(added=20, kept_proj=10, kept_exist=10, big=3, twice=3, names_and_claims=3, outside=3, skipped=20, dead=1)
