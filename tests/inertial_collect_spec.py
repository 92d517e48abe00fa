"""Specification of the INERTIAL local-BA window collected from the resident map (include/orbx.h, "local INERTIAL BA from the resident
map"), in numpy, on tests/map_store_spec.py.

collect   K     = len(chain); chain[0] is the anchor                                   (local_inertial_ba.rs:366-384, :973-978)
          P     = the distinct live slots of the chain's tables in first-seen order      (:387-403)
          c(k)  = the features of keyframe k whose slot is in range, live and in P, repeats counted
          fixed = the keyframes outside the chain with c > 0, ascending                  (:406-429, derived from the tables)
          one BA_OBS32 per counted feature, observers chain[0], chain[1..], fixed[..]: kf_idx i for chain[i] (i >= 1), -1 for the
          anchor, -2 - j for fixed[j]; mp_idx | STEREO where has_point[feature] != 0     (:996-1029)
widen     the BA_OBS form of such observations, the flag in _pad: orbx_ba_solve_inertial's argument
"""
import numpy as np

import map_store_spec as MS

BA_OBS32 = np.dtype([("kf_idx", "<i4"), ("mp_idx", "<i4"), ("u", "<f4"), ("v", "<f4")])
BA_OBS = np.dtype([("kf_idx", "<i4"), ("fixed_idx", "<i4"), ("mp_idx", "<i4"), ("_pad", "<i4"), ("u", "<f8"), ("v", "<f8")])
STEREO = 0x40000000


def collect(tables, keypoints_xy, has_point, live, chain):
    """tables [n_kfs]: int32 arrays or None; keypoints_xy [n_kfs]: f32 [n_k, 2]; has_point [n_kfs]: u8 [n_k] or None (a keyframe made
    without stereo points); live u8 [capacity]; chain: positions in tables, oldest first.
    -> None where len(chain) < 2, else dict(counts int32 [4] = (K, F, M, N), fixed_kf int32 [F - 1], list_slot int32 [M],
       obs32 BA_OBS32 [N], empty: M == 0)"""
    live = np.asarray(live)
    chain = [int(k) for k in chain]
    assert len(set(chain)) == len(chain) and all(0 <= k < len(tables) for k in chain)
    if len(chain) < 2:
        return None
    P = MS.select_keyframes([tables[k] for k in chain], live)
    index = {int(s): i for i, s in enumerate(P.tolist())}

    def counted(k):
        t = tables[k]
        if t is None:
            return []
        return [(i, index[s]) for i, s in enumerate(np.asarray(t).tolist()) if 0 <= s < len(live) and live[s] and s in index]

    per_kf = [counted(k) for k in range(len(tables))]
    fixed = [k for k in range(len(tables)) if k not in chain and per_kf[k]]
    rows = []
    for code, k in [(i if i else -1, k) for i, k in enumerate(chain)] + [(-2 - j, k) for j, k in enumerate(fixed)]:
        xy = np.asarray(keypoints_xy[k], np.float32).reshape(-1, 2)
        hp = has_point[k]
        rows += [(code, m | (STEREO if hp is not None and hp[i] else 0), xy[i, 0], xy[i, 1]) for i, m in per_kf[k]]
    obs = np.array(rows, BA_OBS32) if rows else np.zeros(0, BA_OBS32)
    counts = np.array([len(chain), 1 + len(fixed), len(P), len(obs)], np.int32)
    return dict(counts=counts, fixed_kf=np.array(fixed, np.int32), list_slot=P.astype(np.int32), obs32=obs, empty=len(P) == 0)


def widen(obs32, n_fixed):
    """BA_OBS32 with the stereo flag in mp_idx -> BA_OBS with it in _pad (fixed observer F = the identity pose: fixed_idx -1)"""
    o = np.zeros(len(obs32), BA_OBS)
    k = obs32["kf_idx"]
    o["kf_idx"] = np.where(k >= 0, k, -1)
    o["fixed_idx"] = np.where((k >= 0) | (-1 - k == n_fixed), -1, -1 - k)
    o["mp_idx"] = obs32["mp_idx"] & ~STEREO
    o["_pad"] = (obs32["mp_idx"] & STEREO) != 0
    o["u"] = obs32["u"]; o["v"] = obs32["v"]
    return o
