"""Specification of the whole map's global-BA problem collected from the resident map (include/orbx.h, "global BA from the resident
map"; collect_global_ba_data, global_ba.rs:100-181), in numpy.

collect   kfs[0] is the anchor, kfs[1..] the K = n_kfs - 1 optimised keyframes in list order                   (:116-124)
          P = the distinct live slots of all tables in first-seen order: keyframes in list order, features in index order
          one BA_OBS32 per feature whose table entry is a live slot, keyframes in list order, features in index order:
          kf_idx = i - 1 (-1: the anchor), mp_idx = the position in P, u, v = the keypoint's f32                 (:133-175)
"""
import numpy as np

BA_OBS32 = np.dtype([("kf_idx", "<i4"), ("mp_idx", "<i4"), ("u", "<f4"), ("v", "<f4")])


def collect(tables, keypoints_xy, live):
    """tables [n_kfs]: int32 arrays or None; keypoints_xy [n_kfs]: f32 [n_k, 2]; live u8 [capacity].
    -> dict(counts int32 [4] = (K, 1, M, N), list_slot int32 [M], obs32 BA_OBS32 [N], empty: M == 0)"""
    live = np.asarray(live)
    index, P, rows = {}, [], []
    for i, t in enumerate(tables):
        if t is None:
            continue
        xy = np.asarray(keypoints_xy[i], np.float32).reshape(-1, 2)
        for f, s in enumerate(np.asarray(t).tolist()):
            if not (0 <= s < len(live) and live[s]):
                continue
            if s not in index:
                index[s] = len(P); P.append(s)
            rows.append((i - 1, index[s], xy[f, 0], xy[f, 1]))
    obs = np.array(rows, BA_OBS32) if rows else np.zeros(0, BA_OBS32)
    return dict(counts=np.array([len(tables) - 1, 1, len(P), len(obs)], np.int32), list_slot=np.array(P, np.int32), obs32=obs, empty=len(P) == 0)
