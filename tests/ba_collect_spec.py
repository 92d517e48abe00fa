"""Specification of the local-BA window collected from the resident map (include/orbx.h, "local BA from the resident map"), in
numpy, on tests/covisibility_spec.py and tests/map_store_spec.py.

collect   local = [cur] ++ best(cur, max_covisible)                                   (local_ba_lm.rs:665-683)
          P     = the distinct live slots of local's tables in first-seen order       (:686-704)
          c(k)  = the features of keyframe k whose slot is in range, live and in P, repeats counted
          fixed = the keyframes outside local with c > 0, ascending                   (:707-726, derived from the tables)
          one BA_OBS32 per counted feature, observers local[0], local[1..], fixed[..] (:856-882)
"""
import numpy as np

import covisibility_spec as CS
import map_store_spec as MS

BA_OBS32 = np.dtype([("kf_idx", "<i4"), ("mp_idx", "<i4"), ("u", "<f4"), ("v", "<f4")])


def collect(tables, keypoints_xy, live, cur, max_covisible):
    """tables [n_kfs]: int32 arrays or None; keypoints_xy [n_kfs]: f32 [n_k, 2]; live u8 [capacity].
    -> dict(counts int32 [4] = (K, F, M, N), local_kf int32 [1 + max_covisible] (-1 padded), fixed_kf int32 [F - 1],
            list_slot int32 [M], obs32 BA_OBS32 [N], empty: M == 0)"""
    live = np.asarray(live)
    local, row = CS.local_keyframes(tables, live, cur, max_covisible)
    P = MS.select_keyframes([tables[k] for k in local], live)
    index = {int(s): i for i, s in enumerate(P.tolist())}

    def counted(k):
        t = tables[k]
        if t is None:
            return []
        return [(i, index[s]) for i, s in enumerate(np.asarray(t).tolist()) if 0 <= s < len(live) and live[s] and s in index]

    per_kf = [counted(k) for k in range(len(tables))]
    fixed = [k for k in range(len(tables)) if k not in local and per_kf[k]]
    rows = []
    for code, k in [(i - 1, k) for i, k in enumerate(local)] + [(-2 - j, k) for j, k in enumerate(fixed)]:
        xy = np.asarray(keypoints_xy[k], np.float32).reshape(-1, 2)
        rows += [(code, m, xy[i, 0], xy[i, 1]) for i, m in per_kf[k]]
    obs = np.array(rows, BA_OBS32) if rows else np.zeros(0, BA_OBS32)
    counts = np.array([len(local) - 1, 1 + len(fixed), len(P), len(obs)], np.int32)
    return dict(counts=counts, local_kf=row.astype(np.int32), fixed_kf=np.array(fixed, np.int32), list_slot=P.astype(np.int32), obs32=obs,
                empty=len(P) == 0)
