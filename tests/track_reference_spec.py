"""Specification of orbx_track_reference (include/orbx.h) in numpy: the numeric part of track_with_reference_kf
(tracker.rs:992-1064) up to and after PnP.

match()    BFMatcher(NORM_HAMMING, crossCheck = true).train_match(kf.descriptors, frame.descriptors): oracle.crosscheck_match, the
           reference of orbx_hamming_match_crosscheck (query = keyframe feature, train = frame feature);
dense_match()  the same rule stated independently on the full distance table (the CPU tests compare the two);
gather()   the matches whose keyframe feature has a live map point, in match order (:1024-1043);
finish()   status and the pose rule, given what PnP returned for the gathered arrays (:1051-1063).
PnP itself is not restated here: the GPU tests compose (PnP on these gathered arrays = what the fused call hands through).
A frame is (kp, desc, kf_desc, kf_positions, kf_valid, prior_wc).
"""
import numpy as np

OK, NO_MODEL, TOO_FEW_CORRESPONDENCES, TOO_FEW_INLIERS = 0, 1, 2, 3
PNP_NO_MODEL = 1
MIN_CORRESPONDENCES = 4                                                        # tracker.rs:1051
DMATCH = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("img_idx", "<i4"), ("distance", "<f4")])

_POP = np.array([bin(i).count("1") for i in range(256)], np.uint16)


def distance_table(q, t):
    """[nq, nt] uint16 Hamming distances of 32-byte rows"""
    q = np.asarray(q, np.uint8).reshape(-1, 32); t = np.asarray(t, np.uint8).reshape(-1, 32)
    out = np.zeros((len(q), len(t)), np.uint16)
    for i in range(0, len(q), 64):                                            # (in slabs: the xor table is nq x nt x 32 bytes)
        out[i:i + 64] = _POP[q[i:i + 64, None, :] ^ t[None, :, :]].sum(2, dtype=np.uint16)
    return out


def dense_match(kf_desc, desc):
    """mutual nearest neighbours from the full table: argmin over columns per row and over rows per column (np.argmin takes the
    first minimum = the lowest index wins a tie, in both directions), ascending row.  [spec] an empty side: no matches."""
    D = distance_table(kf_desc, desc)
    if D.shape[0] == 0 or D.shape[1] == 0:
        return np.zeros(0, DMATCH)
    fwd = D.argmin(1); bwd = D.argmin(0)
    rows = np.flatnonzero(bwd[fwd] == np.arange(len(fwd)))
    m = np.zeros(len(rows), DMATCH)
    m["query_idx"] = rows; m["train_idx"] = fwd[rows]; m["distance"] = D[rows, fwd[rows]].astype(np.float32)
    return m


def match(oracle, kf_desc, desc):
    m = oracle.crosscheck_match(kf_desc, desc)
    assert m.dtype == DMATCH
    return m


def gather(kp, kf_positions, kf_valid, matches):
    """the correspondences of one frame in match order = ascending keyframe-feature index"""
    pos = np.asarray(kf_positions, np.float64).reshape(-1, 3); valid = np.asarray(kf_valid, np.uint8).reshape(-1)
    q = matches["query_idx"]; t = matches["train_idx"]
    keep = valid[q] != 0 if len(q) else np.zeros(0, bool)
    kf_idx = q[keep].astype(np.int32); feat_idx = t[keep].astype(np.int32)
    pts2d = np.stack([kp["x"][feat_idx], kp["y"][feat_idx]], 1).astype(np.float32) if len(kf_idx) else np.zeros((0, 2), np.float32)
    return dict(kf_idx=kf_idx, feat_idx=feat_idx, points3d=pos[kf_idx].copy(), points2d=pts2d)


def finish(min_correspondences, n_matches, g, prior_wc, pnp_pose, pnp_status, pnp_n_inliers):
    """(record, pose): the rules behind PnP; there is no inlier guard on this path"""
    n_corr = len(g["kf_idx"])
    pose = np.asarray(pnp_pose, np.float64).copy()
    status, n_inl = OK, int(pnp_n_inliers)
    if n_corr < min_correspondences:
        status, n_inl = TOO_FEW_CORRESPONDENCES, 0
        pose = np.asarray(prior_wc, np.float64).copy()
    elif pnp_status == PNP_NO_MODEL:
        status = NO_MODEL
    return dict(status=status, n_matches=int(n_matches), n_correspondences=n_corr, n_inliers=n_inl), pose


def match_and_gather(oracle, frames):
    """frames [(kp, desc, kf_desc, kf_positions, kf_valid, prior_wc), ...] -> (offsets [B+1] int32, [matches], [gathered])"""
    ms, gs = [], []
    for kp, desc, kd, pos, valid, _ in frames:
        m = match(oracle, kd, desc)
        ms.append(m); gs.append(gather(kp, pos, valid, m))
    off = np.zeros(len(frames) + 1, np.int32)
    off[1:] = np.cumsum([len(g["kf_idx"]) for g in gs])
    return off, ms, gs
