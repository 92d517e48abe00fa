"""Scenes of the loop correction on the resident map (tests/loop_correct_spec.py; include/orbx.h, "loop correction on the resident
map"): small stores and slot tables built by hand, each for one rule of the definition, and random graphs that cross the wave and
block edges of the kernels.  A scene is a dict: capacity, live [capacity] u8, positions [capacity][3], desc [capacity][32], tables
(int32 arrays, None = no table), n [K] (the keyframes' feature counts), poses [K][7], parent [K], cur, loop, matches [n][2], min_weight, max_depth, sim3 [8].

Weights are made by sharing fresh slots: share(k, j, w) gives keyframes k and j w points nobody else sees.  MIN is 3, so that a
scene needs a handful of features; the kernels compare against whatever the configuration says.
"""
import functools

import numpy as np

import orientation_cases as OC
from pnp_spec import quat_mul

MIN = 3
SIM3 = np.array([np.cos(0.2), 0.0, np.sin(0.2), 0.0, 0.3, -0.1, 0.25, 1.0])      # a modest drift: 0.4 rad about y, 0.4 m


def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


class _Builder:
    def __init__(self, K, capacity=256, seed=0):
        self.rng = np.random.default_rng(seed)
        self.K, self.capacity, self.next = K, capacity, 0
        self.rows = [[] for _ in range(K)]
        self.dead = set()
        self.parent = [-1] * K

    def slot(self, live=True):
        s = self.next
        self.next += 1
        if not live:
            self.dead.add(s)
        return s

    def see(self, k, s):
        self.rows[k].append(s)
        return len(self.rows[k]) - 1                         # the feature

    def share(self, k, j, w):
        for _ in range(w):
            s = self.slot()
            self.see(k, s); self.see(j, s)

    def own(self, k, n):
        return [self.see(k, self.slot()) for _ in range(n)]

    def finish(self, cur, loop=-1, matches=(), no_table=(), min_weight=MIN, max_depth=100, sim3=SIM3, poses=None):
        assert self.next <= self.capacity
        live = np.ones(self.capacity, np.uint8)
        live[self.next:] = 0
        live[list(self.dead)] = 0
        rng = self.rng
        if poses is None:
            poses = np.concatenate([np.array([_unit(rng.normal(size=4)) for _ in range(self.K)]), rng.uniform(-5, 5, (self.K, 3))], 1)
        return dict(n=[len(r) for r in self.rows], capacity=self.capacity, live=live, positions=rng.uniform(-20, 20, (self.capacity, 3)), desc=rng.integers(0, 256, (self.capacity, 32), dtype=np.uint8),
                    tables=[None if k in no_table else np.array(r, np.int32) for k, r in enumerate(self.rows)], poses=np.asarray(poses, np.float64),
                    parent=np.array(self.parent, np.int32), cur=cur, loop=loop, matches=np.array(matches, np.int32).reshape(-1, 2), min_weight=min_weight,
                    max_depth=max_depth, sim3=np.asarray(sim3, np.float64))


# ---- reach -------------------------------------------------------------------------------------------------------------------

def chain(depth):
    """five keyframes in a covisibility chain 0 - 1 - 2 - 3 - 4, cur = 0: A is the first depth + 1 of them"""
    b = _Builder(5)
    for k in range(4):
        b.share(k, k + 1, MIN)
    return b.finish(0, max_depth=depth)


def parent_arc(cur):
    """0 is the parent of 1 and shares nothing with it: from 0 the child is reached, from 1 the parent stays out"""
    b = _Builder(2)
    b.own(0, 4); b.own(1, 4)
    b.parent[1] = 0
    return b.finish(cur)


def weight_edge():
    """weight exactly MIN reaches 1, MIN - 1 leaves 2 out"""
    b = _Builder(3)
    b.share(0, 1, MIN); b.share(0, 2, MIN - 1)
    return b.finish(0)


def cycle():
    """0 - 1 - 2 - 3 - 0 by covisibility and a spanning tree 0 -> 1 -> 2 -> 3 on top; 4 hangs off nothing"""
    b = _Builder(5)
    for k in range(4):
        b.share(k, (k + 1) % 4, MIN)
    b.parent[1:4] = [0, 1, 2]
    b.own(4, 3)
    return b.finish(2)


def two_components():
    b = _Builder(5)
    b.share(0, 1, MIN); b.share(2, 3, MIN + 2); b.share(3, 4, MIN)
    b.parent[3] = 2
    return b.finish(0)


def through_child():
    """cur 0 -> child 1 (no covisibility between them); 1 - 2 by covisibility: 2 is reached only through the child, at depth 2; 3, the
    parent of 2, stays out"""
    b = _Builder(4)
    b.own(0, 3)
    b.share(1, 2, MIN)
    b.own(3, 3)
    b.parent[1] = 0; b.parent[2] = 3
    return b.finish(0)


def cur_without_table():
    """cur has no table (it observes nothing): its child is still reached, and the list holds the child's points"""
    b = _Builder(3)
    b.own(0, 5); b.own(1, 4); b.share(1, 2, MIN)
    b.parent[1] = 0
    return b.finish(0, no_table=(0,))


def single():
    b = _Builder(1)
    b.own(0, 6)
    return b.finish(0)


@functools.lru_cache(maxsize=None)
def random_graph(N, seed=None):
    """N keyframes of 8 to 40 features walking along a band of slots, so that neighbours share a random number of points; a random
    spanning forest; dead slots, -1 and out-of-range entries, repeats; a few matches between cur and a loop keyframe that shares none
    of cur's points.  N = 65, 130, 1100 cross the wave (64), the feature-chunk and the 1024-thread edges of the single-workgroup kernels."""
    rng = np.random.default_rng(N if seed is None else seed)
    capacity = 6 * N + 64
    live = (rng.random(capacity) > 0.05).astype(np.uint8)
    tables, parent = [], []
    for k in range(N):
        n = int(rng.integers(8, 41))
        lo = 6 * k if rng.random() > 0.1 else int(rng.integers(0, 6 * N))          # most follow the band, some jump: components and shortcuts
        t = rng.integers(lo, min(lo + 48, capacity), n).astype(np.int32)
        t[rng.random(n) < 0.1] = -1
        if n > 10:
            t[3] = capacity + 7; t[5] = t[4]                                        # out of range; a repeat inside the keyframe
        tables.append(t)
        parent.append(int(rng.integers(0, k)) if k and rng.random() > 0.2 else -1)
    cur, loop = N // 2, 0
    live[tables[cur][(tables[cur] >= 0) & (tables[cur] < capacity)][:4]] = 1
    live[tables[loop][(tables[loop] >= 0) & (tables[loop] < capacity)][:4]] = 1
    matches = [(int(rng.integers(0, len(tables[cur]))), int(rng.integers(0, len(tables[loop])))) for _ in range(12)]
    poses = np.concatenate([np.array([_unit(rng.normal(size=4)) for _ in range(N)]), rng.uniform(-50, 50, (N, 3))], 1)
    return dict(n=[len(t) for t in tables], capacity=capacity, live=live, positions=rng.uniform(-50, 50, (capacity, 3)), desc=rng.integers(0, 256, (capacity, 32), dtype=np.uint8), tables=tables,
                poses=poses, parent=np.array(parent, np.int32), cur=cur, loop=loop, matches=np.array(matches, np.int32), min_weight=MIN, max_depth=100 if N > 1000 else 2 if N < 100 else 4,
                sim3=SIM3)


REACH = dict(chain0=lambda: chain(0), chain1=lambda: chain(1), chain2=lambda: chain(2), chain100=lambda: chain(100), parent_from_parent=lambda: parent_arc(0),
             parent_from_child=lambda: parent_arc(1), weight_edge=weight_edge, cycle=cycle, two_components=two_components, through_child=through_child,
             cur_without_table=cur_without_table, single=single)
REACH_WANT = dict(chain0=[0], chain1=[0, 1], chain2=[0, 1, 2], chain100=[0, 1, 2, 3, 4], parent_from_parent=[0, 1], parent_from_child=[1], weight_edge=[0, 1],
                  cycle=[0, 1, 2, 3], two_components=[0, 1], through_child=[0, 1, 2], cur_without_table=[0, 1, 2], single=[0])
RANDOM_N = (65, 130, 1100)


# ---- points and Sim3 ---------------------------------------------------------------------------------------------------------

def points(sim3=SIM3, poses=None):
    """0 - 1 affected, 2 and 3 outside.  A slot seen from inside and outside A (it is corrected, once); a slot repeated inside keyframe
    0; dead, -1 and out-of-range entries; a slot only 2 and 3 see (untouched)."""
    b = _Builder(4, capacity=64)
    b.share(0, 1, MIN)
    inout = b.slot(); b.see(1, inout); b.see(2, inout); b.see(3, inout)
    rep = b.slot(); b.see(0, rep); b.see(0, rep); b.see(1, rep)
    dead = b.slot(live=False); b.see(0, dead); b.see(2, dead)
    b.see(0, -1); b.see(1, 64 + 5); b.see(0, 63)             # (63: in range, never set: not live)
    b.share(2, 3, 2)
    return b.finish(0, sim3=sim3, poses=poses)


def no_points():
    """A = {0, 1}: one without a table, the other naming only dead and empty entries: a list of 0 points, two poses corrected"""
    b = _Builder(3, capacity=32)
    d = b.slot(live=False)
    b.see(0, 1); b.see(1, d); b.see(1, -1); b.own(2, 3)
    b.parent[1] = 0
    return b.finish(0, no_table=(0,))


def _axis_angle(axis, angle):
    a = _unit(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])


SIM3S = dict(identity=[1, 0, 0, 0, 0, 0, 0, 1], half=np.concatenate([_axis_angle([1, 2, 3], 0.7), [0.5, 1.0, -2.0, 0.5]]),
             double=np.concatenate([_axis_angle([-1, 0.2, 0.4], 2.9), [-3.0, 0.1, 7.0, 2.0]]), pi=np.concatenate([_axis_angle(OC.AXIS, np.pi) * [0, 1, 1, 1], [0.2, 0.3, 0.4, 1.0]]),
             negative_w=np.concatenate([-_axis_angle([0.5, 0.5, -1], 1.1), [1.0, 2.0, 3.0, 1.0]]), far=np.concatenate([_axis_angle([0, 0, 1], 0.3), [4.0e6, -2.5e6, 1.0e5, 1.0]]))
SIM3S.update({"world_" + n: np.concatenate([_unit(q), [0.4, -0.6, 0.2, 1.0]]) for n, q in OC.PLAIN})


def orientation_poses():
    """four keyframe poses from the pose list that covers real-world orientations (tests/orientation_cases.py: PLAIN), cycled per scene"""
    qs = [np.asarray(q, np.float64) for _, q in OC.PLAIN]
    return [np.array([np.concatenate([qs[(i + k) % len(qs)], [1.5 * k - 2.0, 0.3 * i, 4.0 - k]]) for k in range(4)]) for i in range(len(qs))]


# ---- fuse --------------------------------------------------------------------------------------------------------------------

def fuse_scene():
    """cur = 0, loop = 1; 2 is affected with them, 3 is outside A (min_weight 6 here: 3 shares at most 4 points with anyone).  The
    matches, in order:
      m0  a == b (the shared point itself): no pair          m1  a dead loop side: no pair          m2, m3  one pair listed twice (a tie of
      one observer each: the current keyframe's point keeps)
      m4, m5  a class of three, a - b and b - c: c has the most observers and keeps both
      m6  a tie of two observers each: the current keyframe's point keeps
      m7  the loop point has more observers: it keeps; the goner sits at two features of keyframe 2, which already names the keeper
      m8  the current point keeps; the goner is named by keyframe 3, outside A, which already names the keeper
      m9  a -1 entry on the current side: no pair"""
    W = 6
    b = _Builder(4, capacity=128)
    b.share(0, 1, W); b.share(0, 2, W)
    m = []
    same = b.slot(); m.append((b.see(0, same), b.see(1, same)))
    dead = b.slot(live=False); m.append((b.own(0, 1)[0], b.see(1, dead)))
    f0, f1 = b.own(0, 1)[0], b.own(1, 1)[0]; m += [(f0, f1), (f0, f1)]
    a, bb, c = b.slot(), b.slot(), b.slot()
    m.append((b.see(0, a), b.see(1, bb)))
    m.append((b.see(0, bb), b.see(1, c)))
    b.see(2, c); b.see(3, c)
    x, y = b.slot(), b.slot()
    m.append((b.see(0, x), b.see(1, y)))
    b.see(2, x); b.see(3, y)
    lone, big = b.slot(), b.slot()
    m.append((b.see(0, lone), b.see(1, big)))
    b.see(2, lone); b.see(2, big); b.see(2, lone); b.see(3, big)
    g, kp = b.slot(), b.slot()
    m.append((b.see(0, kp), b.see(1, g)))
    b.see(2, kp); b.see(3, g); b.see(3, kp)
    m.append((b.see(0, -1), b.own(1, 1)[0]))
    b.own(3, 2)
    return b.finish(0, 1, m, min_weight=W)


def no_pairs():
    """matches, none of them a pair (a == b, dead, empty): counts[2] = 0, no goner, no table changes"""
    b = _Builder(2, capacity=32)
    b.share(0, 1, MIN)
    d = b.slot(live=False)
    return b.finish(0, 1, [(0, 0), (1, 1), (b.see(0, d), 2), (b.see(0, -1), b.see(1, -1))])


def agree_world(seed):
    """twelve keyframes of 30 features, every point associated once per keyframe, no slot in two pairs: the scenes on which the
    definition must equal the reference replayed in list order"""
    rng = np.random.default_rng(seed)
    K, n = 12, 30
    b = _Builder(K, capacity=1024, seed=seed)
    for k in range(K - 1):
        b.share(k, k + 1, int(rng.integers(1, 6)))
    for k in range(K):
        b.own(k, n - len(b.rows[k]))
        if k:
            b.parent[k] = k - 1
    cur, loop = K - 1, 0
    # extra observers, so that counts differ: some points of cur / loop are also seen by a third keyframe that has room
    m = []
    fcs = rng.permutation(n)[:8]; fls = rng.permutation(n)[:8]
    for fc, fl in zip(fcs.tolist(), fls.tolist()):
        m.append((fc, fl))
        for k in rng.permutation(np.arange(1, K - 1))[:int(rng.integers(0, 4))].tolist():
            s = b.rows[cur][fc] if rng.random() < 0.5 else b.rows[loop][fl]
            if s not in b.rows[k]:
                b.see(k, s)
    return b.finish(cur, loop, m, max_depth=int(rng.integers(1, 5)))


# ---- one session ---------------------------------------------------------------------------------------------------------------

CAMERA = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, baseline=0.11007)
KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def _R(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def session(seed=7):
    """Twelve keyframes of 200 features on a circle of radius 6 that look at 700 landmarks around its centre, with a drift that grows
    along the trajectory: keyframe k believes the pose D_k T_k, D_k a rotation of 0.004 k rad about y and a shift of 0.01 k m, and
    the points it created lie at D_k X.  Keyframes 0 to 10 see the landmarks [50 k, 50 k + 200); keyframe 11 comes back to where
    keyframe 0 stood: it sees 60 of keyframe 10's points and the landmarks 0 to 139 again, as 140 NEW map points of its own — the
    duplicates the loop closer fuses.  Features carry their true projection (0.3 px noise), their stereo point and the landmark's
    descriptor with a few bits flipped.  kfs[] is in ascending id, parent[k] = k - 1, cur = 11, loop = 0."""
    rng = np.random.default_rng(seed)
    K, n, L = 12, 200, 700
    X = rng.normal(size=(L, 3)); X = 2.0 * X / np.linalg.norm(X, axis=1, keepdims=True) * rng.random((L, 1)) ** (1 / 3)
    base = rng.integers(0, 256, (L, 32), dtype=np.uint8)
    ang = np.concatenate([np.arange(11) * (2 * np.pi / 12), [0.03]])
    kfs, tables = [], []
    capacity = 1024
    positions = np.zeros((capacity, 3)); desc = np.zeros((capacity, 32), np.uint8); live = np.zeros(capacity, np.uint8)

    def drift(k):
        q = np.array([np.cos(0.002 * k), 0.0, np.sin(0.002 * k), 0.0])
        return q, 0.01 * k * np.array([1.0, 0.0, 0.5])
    for j in range(L):
        q, t = drift(min(j // 50, 10))
        positions[j] = _R(q) @ X[j] + t; desc[j] = base[j]; live[j] = 1
    for k in range(K):
        c = 6.0 * np.array([np.sin(ang[k]), 0.0, -np.cos(ang[k])])                  # the camera centre; it looks at the origin
        q_true = np.array([np.cos(-ang[k] / 2), 0.0, np.sin(-ang[k] / 2), 0.0])      # z axis towards the origin
        Rt = _R(q_true)
        lm = np.arange(50 * k, 50 * k + n) if k < 11 else np.concatenate([np.arange(640, 700), np.arange(0, 140)])
        slots = lm.copy()
        if k == 11:
            slots[60:] = 700 + np.arange(140)
            q, t = drift(11)
            positions[700:840] = X[:140] @ _R(q).T + t; desc[700:840] = base[:140]; live[700:840] = 1
        Xc = (X[lm] - c) @ Rt
        assert Xc[:, 2].min() > 2.0
        uv = np.stack([CAMERA["fx"] * Xc[:, 0] / Xc[:, 2] + CAMERA["cx"], CAMERA["fy"] * Xc[:, 1] / Xc[:, 2] + CAMERA["cy"]], 1) + rng.normal(0, 0.3, (n, 2))
        kp = np.zeros(n, KEYPOINT)
        kp["x"], kp["y"], kp["octave"] = uv[:, 0], uv[:, 1], rng.integers(0, 4, n)
        d = base[lm].copy()
        for r in range(n):
            for bit in rng.choice(256, int(rng.integers(0, 9)), replace=False):
                d[r, bit >> 3] ^= np.uint8(1 << (bit & 7))
        qd, td = drift(k)
        pose = np.concatenate([quat_mul(qd, q_true), _R(qd) @ c + td])
        perm = rng.permutation(n)
        kfs.append(dict(kp=kp[perm], desc=d[perm], points_cam=(Xc + rng.normal(0, 0.01, Xc.shape))[perm], has_point=np.ones(n, np.uint8), pose_wc=pose))
        tables.append(slots[perm].astype(np.int32))
    return dict(capacity=capacity, live=live, positions=positions, desc=desc, tables=tables, kfs=kfs, poses=np.array([k["pose_wc"] for k in kfs]),
                parent=np.arange(-1, K - 1, dtype=np.int32), cur=11, loop=0)
