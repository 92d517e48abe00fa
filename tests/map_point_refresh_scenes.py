"""Deterministic scenes for the map-point refresh (orbx_refresh_map_points): the inputs of tests/test_map_point_refresh_gpu.py, and of
the CPU checks of the two conditions its tolerances rest on (tests/test_map_point_refresh_cpu.py).

Geometry of every random scene: camera centres inside a ball of radius 0.5 about the origin, map points at x, y in [-2, 2] and
z in [4, 10].  Two viewing directions of one point are then at most 2 asin(0.5 / 4) < 15 degrees apart: inside a 60 degree cone.
Scene layout: tests/map_point_refresh_spec.py."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE_RANGE = 1.2 ** 7           # the reference's default pyramid: scale_factor 1.2, 8 levels
SHORT_MAX = 64                   # mp_refresh_kernel's longest point; longer ones go to mp_refresh_long_kernel
WINDOW = 256                     # observations per workgroup window of mp_refresh_kernel


def _keyframes(rng, T, n_feat):
    """T keyframes of n_feat features each (n_feat an int or one count per keyframe): poses [T,7], offsets [T+1], descs [F,32]."""
    counts = [n_feat] * T if np.isscalar(n_feat) else list(n_feat)
    q = rng.normal(0, 1, (T, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    c = rng.normal(0, 1, (T, 3)); c *= (0.5 * rng.uniform(0.2, 1.0, (T, 1))) / np.linalg.norm(c, axis=1, keepdims=True)
    off = np.zeros(T + 1, np.int32); off[1:] = np.cumsum(counts)
    return np.concatenate([q, c], 1), off, rng.integers(0, 256, (int(off[-1]), 32), dtype=np.uint8)


def _points(rng, M):
    return np.stack([rng.uniform(-2, 2, M), rng.uniform(-2, 2, M), rng.uniform(4, 10, M)], 1)


def _scene(rng, lengths, T, n_feat):
    """Points of the given track lengths; every observation a random (keyframe, feature) of a keyframe that has features."""
    poses, off, descs = _keyframes(rng, T, n_feat)
    M = len(lengths)
    start = np.zeros(M + 1, np.int32); start[1:] = np.cumsum(lengths)
    N = int(start[-1])
    counts = np.diff(off)
    kf = rng.choice(np.flatnonzero(counts > 0), N).astype(np.int32)
    feat = (rng.random(N) * counts[kf]).astype(np.int32)
    nrm = rng.normal(0, 1, (M, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return dict(positions=_points(rng, M), obs_start=start, obs_kf=kf, obs_feat=feat, kf_poses_wc=poses, kf_feat_offset=off, descs=descs,
                scale_range=SCALE_RANGE, mp_desc=rng.integers(0, 256, (M, 32), dtype=np.uint8), normals=nrm)


BOUNDARY_LENGTHS = [0, 1, 2, 3, 63, 64, 65, 66, 130, 255, 256, 257, 300]


def boundaries():
    """One point of every track length at which the code takes another path: none, one, two rows; the last short and the first long
    point; one tile of the long kernel less one, exactly, plus one; more than a tile."""
    return _scene(np.random.default_rng(101), BOUNDARY_LENGTHS, T=5, n_feat=300)


def _fill_to(rng, lengths, target):
    """Appends random lengths 0..12 until the running sum is exactly `target`."""
    total = int(sum(lengths))
    assert total <= target
    while total < target:
        n = int(min(rng.integers(0, 13), target - total))
        lengths.append(n); total += n


def straddle(variant):
    """M = 700 points of 0..12 observations, about 4000 observations (16 windows), with points of 64 observations that start at the
    last observation of a window and reach 63 rows into the next (starts 255 and 511: variant "a"), or at a window's first observation
    (start 256, and 511 again: variant "b") — a point of 64 observations that starts at 255 covers observation 256, so the three starts
    cannot be in one list.  Long points (65 and 200 observations) are interleaved."""
    rng = np.random.default_rng({"a": 202, "b": 203}[variant])
    lengths = []
    _fill_to(rng, lengths, 120); lengths.append(65)                       # a long point inside window 0
    _fill_to(rng, lengths, 255 if variant == "a" else 256); lengths.append(64)
    _fill_to(rng, lengths, 511); lengths.append(64)
    _fill_to(rng, lengths, 900); lengths.append(200)                      # a long point across a window boundary (900..1100)
    while len(lengths) < 700:
        lengths.append(int(rng.integers(0, 13)))
    s = _scene(rng, lengths, T=5, n_feat=300)
    starts = {int(s["obs_start"][p]) for p in range(700) if lengths[p] == 64}
    assert starts == ({255, 511} if variant == "a" else {256, 511}) and 3500 < int(s["obs_start"][-1]) < 4800
    return s


def skips():
    """Observations the reference skips: obs_kf = -1 and = T (keyframes.get -> None), obs_feat = -1 and = n_features (row() -> Err), a
    keyframe with 0 features, and points all of whose rows are invalid while their observers exist — in both kernels' ranges."""
    rng = np.random.default_rng(303)
    T = 5
    lengths = [6, 5, 4, 3, 1, 8, 100, 70] + [int(rng.integers(1, 13)) for _ in range(40)]
    s = _scene(rng, lengths, T, n_feat=[300, 300, 0, 300, 300])          # keyframe 2 has no features
    st, kf, feat = s["obs_start"], s["obs_kf"], s["obs_feat"]
    nf = np.diff(s["kf_feat_offset"])
    kf[st[0]] = -1; kf[st[0] + 1] = T; feat[st[0] + 2] = -1; feat[st[0] + 3] = nf[kf[st[0] + 3]]        # point 0: two rows left
    kf[st[1]:st[2]] = 2; feat[st[1]:st[2]] = 0                             # point 1: observers exist, the keyframe has no rows
    feat[st[2]:st[3]] = -1                                                 # point 2: observers exist, every feature index invalid
    kf[st[3]:st[4]] = [-1, T, -7]                                          # point 3: no observer at all
    feat[st[4]] = nf[kf[st[4]]]                                            # point 4: its only row is out of range
    kf[st[5]] = 2; feat[st[5]] = 0; kf[st[5] + 1] = 2; feat[st[5] + 1] = 5                             # point 5: the first two rows skipped
    feat[st[6]:st[7]] = -1                                                 # point 6 (long): every feature index invalid
    kf[st[7]:st[8]:3] = T; feat[st[7] + 1:st[8]:3] = -1                    # point 7 (long): a third without keyframe, a third without row
    for p in range(8, len(lengths)):                                       # the rest: a random tenth of either kind
        for o in range(st[p], st[p + 1]):
            r = rng.random()
            if r < 0.1:
                kf[o] = rng.choice([-1, T, 2])
            elif r < 0.2:
                feat[o] = rng.choice([-1, int(nf[kf[o]])])
    return s


def ties():
    """Equal maxima by construction, in both kernels' ranges.  Rows z, x, y, w over disjoint bit blocks A, B (4 bits each) and C (8 bits):
    x = A, y = B, w = none, z = A + B + C, so xy 8, xw 4, yw 4, zx 12, zy 12, zw 16 and the maxima are z 16, x 12, y 12, w 16: x and y tie
    and the earlier one is chosen with best_max_dist 12.  All rows are XORed with one random mask, which keeps every distance.
    Points: (z,x,y,w), (w,y,x,z), (z,w,y,x) with n = 4, and the three patterns repeated 25 times (n = 100); equal rows are 0 apart."""
    rng = np.random.default_rng(404)
    x = np.zeros(32, np.uint8); y = np.zeros(32, np.uint8); z = np.zeros(32, np.uint8); w = np.zeros(32, np.uint8)
    x[3] = 0x0F; y[17] = 0xF0; z[3] = 0x0F; z[17] = 0xF0; z[30] = 0xFF
    mask = rng.integers(0, 256, 32, dtype=np.uint8)
    proto = {k: v ^ mask for k, v in dict(x=x, y=y, z=z, w=w).items()}
    patterns = ["zxyw", "wyxz", "zwyx"]
    lists = patterns + [p * 25 for p in patterns]
    T = 4
    poses, _, _ = _keyframes(rng, T, 1)
    rows, start, okf, ofeat = [[] for _ in range(T)], [0], [], []
    for lst in lists:
        for k, ch in enumerate(lst):
            t = (k * 7 + len(lst)) % T
            okf.append(t); ofeat.append(len(rows[t])); rows[t].append(proto[ch])
        start.append(len(okf))
    off = np.zeros(T + 1, np.int32); off[1:] = np.cumsum([len(r) for r in rows])
    M = len(lists)
    nrm = np.tile([0.0, 0.0, 1.0], (M, 1))
    return dict(positions=_points(rng, M), obs_start=np.array(start, np.int32), obs_kf=np.array(okf, np.int32), obs_feat=np.array(ofeat, np.int32),
                kf_poses_wc=poses, kf_feat_offset=off, descs=np.concatenate([np.array(r, np.uint8).reshape(-1, 32) for r in rows]),
                scale_range=SCALE_RANGE, mp_desc=np.zeros((M, 32), np.uint8), normals=nrm)


def permutation():
    """Every observation has a feature row of its own, and every point's smallest maximum is reached by one row only (rows of a point
    are drawn again until it is; tests/test_map_point_refresh_cpu.py asserts it on the result): the chosen descriptor then does not
    depend on the order of the list.  150 points of 3..40 observations (two rows always tie) and two long ones (70, 130)."""
    import map_point_refresh_spec as S
    rng = np.random.default_rng(505)
    lengths = [int(rng.integers(3, 41)) for _ in range(150)] + [70, 130]
    N = sum(lengths)
    T = 6
    n_feat = -(-N // T) + 8
    s = _scene(rng, lengths, T, n_feat)
    slot = rng.permutation(T * n_feat)[:N]                                # a row of its own for every observation
    s["obs_kf"] = (slot // n_feat).astype(np.int32); s["obs_feat"] = (slot % n_feat).astype(np.int32)
    for p, n in enumerate(lengths):
        rows = s["kf_feat_offset"][s["obs_kf"][s["obs_start"][p]:s["obs_start"][p + 1]]] + s["obs_feat"][s["obs_start"][p]:s["obs_start"][p + 1]]
        proto = rng.integers(0, 256, 32, dtype=np.uint8)
        while True:                                                        # observations of one point: the prototype with 0..60 bits flipped
            for r in rows:
                bits = np.zeros(256, np.uint8); bits[rng.permutation(256)[:int(rng.integers(0, 61))]] = 1
                s["descs"][r] = proto ^ np.packbits(bits)
            maxima = S.distinctive_descriptor(s["descs"][rows])[2]
            if int((maxima == maxima.min()).sum()) == 1:
                break
    return s


def shuffled(scene, seed):
    """The scene with every point's observation list shuffled -> (scene, perm) with new list[k] = old list[perm[k]] (perm holds
    positions inside the point's list, concatenated)."""
    rng = np.random.default_rng(seed)
    s = dict(scene)
    st = scene["obs_start"]
    order, perm = [], []
    for p in range(len(st) - 1):
        q = rng.permutation(int(st[p + 1] - st[p]))
        perm.extend(q.tolist()); order.extend((int(st[p]) + q).tolist())
    order = np.array(order, np.int64)
    s["obs_kf"] = scene["obs_kf"][order]; s["obs_feat"] = scene["obs_feat"][order]
    return s, np.array(perm, np.int64)


# ---- the hand-derived answers (tests/golden/map_point_refresh_known_answers.json) ----------------------------------------------------
def golden_cases():
    with open(os.path.join(ROOT, "tests", "golden", "map_point_refresh_known_answers.json")) as f:
        return json.load(f)["cases"]


def _f(v):
    return float(v)                                                        # "inf" is a string in the file


def golden_scene(cases):
    """All cases as one scene (every case brings its own keyframes) -> (scene, expected list)."""
    pos, start, okf, ofeat, poses, off, descs, mpd, nrm, want = [], [0], [], [], [], [0], [], [], [], []
    for c in cases:
        t0 = len(poses)
        for k in c["keyframes"]:
            poses.append([1.0, 0.0, 0.0, 0.0] + [float(v) for v in k["centre"]])
            descs.extend(k["descriptors"]); off.append(len(descs))
        for kf, feat in c["observations"]:
            okf.append(kf + t0 if 0 <= kf < len(c["keyframes"]) else -1); ofeat.append(feat)
        start.append(len(okf))
        pos.append(c["position"]); mpd.append(c["descriptor_in"]); nrm.append(c["normal_in"])
        e = c["expect"]
        want.append(dict(name=c["name"], descriptor=np.array(e["descriptor"], np.uint8), chosen=e["chosen"], best_max_dist=e["best_max_dist"],
                         n_desc=e["n_desc"], n_observers=e["n_observers"], normal=np.array(e["normal"], np.float64),
                         min_distance=_f(e["min_distance"]), max_distance=_f(e["max_distance"])))
    scale = {float(c["scale_range"]) for c in cases}
    assert len(scale) == 1
    return dict(positions=np.array(pos, np.float64), obs_start=np.array(start, np.int32), obs_kf=np.array(okf, np.int32),
                obs_feat=np.array(ofeat, np.int32), kf_poses_wc=np.array(poses, np.float64).reshape(-1, 7), kf_feat_offset=np.array(off, np.int32),
                descs=np.array(descs, np.uint8).reshape(-1, 32), scale_range=scale.pop(), mp_desc=np.array(mpd, np.uint8),
                normals=np.array(nrm, np.float64)), want


# the golden cases whose geometry is exact by construction and outside the cone condition on purpose
CONE_EXEMPT = {"golden": ["opposite_observers_normal_kept", "observer_at_the_point_skipped", "no_observers"]}


# ---- search_in_neighbors: a map as MapSnapshot arrays ------------------------------------------------------------------------------------
def neighbourhood(seed=606, n_neighbours=6, n_other=2, n_feat=400, n_mp=900):
    """A current keyframe, its neighbours and two more keyframes that observe some of the same map points, 400 features each, as the
    arrays of api.MapSnapshot (observer lists in keyframe-then-feature order, the stated order).  Irregularities: features without a
    map point, features whose map point is gone (dangling id), a map point nobody in the neighbourhood sees, an observer id that is
    not in the map, an observation whose feature index is out of range.
    Returns (MapSnapshot kwargs, current id, neighbour ids, per keyframe descriptors [n_kf][n_feat,32])."""
    rng = np.random.default_rng(seed)
    n_kf = 1 + n_neighbours + n_other
    kf_ids = [100 + 7 * i for i in range(n_kf)]
    poses, _, descs = _keyframes(rng, n_kf, n_feat)
    mp_ids = [5000 + 3 * j for j in range(n_mp)]
    feat_mp = np.full((n_kf, n_feat), -1, np.int64)
    for i in range(n_kf):
        seen = rng.permutation(n_mp)[:int(0.6 * n_feat)]                   # a map point at most once per keyframe
        at = rng.permutation(n_feat)[:len(seen)]
        feat_mp[i, at] = np.array(mp_ids)[seen]
        feat_mp[i, rng.permutation(np.flatnonzero(feat_mp[i] < 0))[:5]] = 999000 + i      # dangling ids
    obs = {m: [] for m in mp_ids}
    for i in range(n_kf):
        for f in range(n_feat):
            if feat_mp[i, f] in obs:
                obs[int(feat_mp[i, f])].append((kf_ids[i], f))
    obs[mp_ids[3]].insert(1, (777777, 0))                                  # an observer that is not in the map any more
    if obs[mp_ids[4]]:
        obs[mp_ids[4]][0] = (obs[mp_ids[4]][0][0], n_feat)                 # a feature index past the keyframe's rows
    start = [0]; okf = []; ofeat = []
    for m in mp_ids:
        okf.extend(k for k, _ in obs[m]); ofeat.extend(f for _, f in obs[m]); start.append(len(okf))
    arrays = dict(kf_ids=kf_ids, kf_bad=np.zeros(n_kf, np.uint8), kf_pose_wc=poses, kf_n_keypoints=[n_feat] * n_kf,
                  kf_feat_start=np.arange(n_kf + 1) * n_feat, feat_mp_id=feat_mp.reshape(-1), feat_uv=np.zeros((n_kf * n_feat, 2), np.float32),
                  cov_start=np.zeros(n_kf + 1, np.int32), cov_kf_id=np.zeros(0, np.uint64), mp_ids=mp_ids, mp_bad=np.zeros(n_mp, np.uint8),
                  mp_pos=_points(rng, n_mp), mp_obs_start=start, mp_obs_kf_id=okf, mp_obs_feat_idx=ofeat)
    return arrays, kf_ids[0], kf_ids[1:1 + n_neighbours] + [424242], descs.reshape(n_kf, n_feat, 32)


RANDOM_SCENES = {"boundaries": boundaries, "straddle_a": lambda: straddle("a"), "straddle_b": lambda: straddle("b"), "skips": skips,
                 "ties": ties, "permutation": permutation}
