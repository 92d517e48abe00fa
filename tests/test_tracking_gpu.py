"""orbx_track_frames[_device] on the GPU against tests/tracking_spec.py: exact equality everywhere.  The search, the gather, the
index arrays, matched and the records equal the spec; pose, inlier mask, errors and PnP's records equal, byte for byte, what
solve_pnp_ransac_batch_device returns for the spec's gathered arrays (composition, no tolerance)."""
import numpy as np
import pytest

import tracking_scenes as G
import tracking_spec as S

pytestmark = pytest.mark.gpu
CAM = G.CAMERA
NAMES = sorted(G.batches())


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.CameraModel(**CAM)


@pytest.fixture(scope="module")
def batches():
    return G.batches()


@pytest.fixture(scope="module")
def expected(oracle, batches):
    """(mode, name) -> (offsets, [match], [gathered]): computed once, never modified"""
    return {(mode, name): S.search_and_gather(oracle, CAM, S.default_config(mode), fr) for mode in (0, 1) for name, fr in batches.items()}


def _cfg(pkg, mode):
    return pkg.TrackConfig.for_mode(mode)


def _device_inputs(frames):
    import torch
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cat = lambda parts, empty: np.concatenate(parts) if sum(len(p) for p in parts) else empty
    kp = cat([f[0] for f in frames], np.zeros(1, G.KEYPOINT)).view(np.float32).reshape(-1, 7).copy()
    desc = cat([f[1] for f in frames], np.zeros((1, 32), np.uint8))
    pos = cat([f[2] for f in frames], np.zeros((1, 3)))
    md = cat([f[3] for f in frames], np.zeros((1, 32), np.uint8))
    fc = np.array([len(f[0]) for f in frames], np.int32)
    fs = (np.cumsum(fc) - fc).astype(np.int32)
    mo = np.zeros(len(frames) + 1, np.int32); mo[1:] = np.cumsum([len(f[2]) for f in frames])
    return dict(kp=d(kp), desc=d(desc), feat_start=d(fs), feat_count=d(fc), max_feat=int(fc.max()), positions=d(pos), mp_desc=d(md),
                mp_offsets=mo, search_poses_wc=d(np.stack([f[4] for f in frames])), priors_wc=d(np.stack([f[5] for f in frames])))


def _run_device(h, pkg, cam, frames, mode, **over):
    import torch
    a = _device_inputs(frames)
    a.update(over)
    o = h.track_frames_device(cam, cfg=_cfg(pkg, mode), **a)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in o.items()}
    r["pnp_results"] = r["pnp_results"].view(pkg.PNP_RESULT).reshape(-1)
    r["results"] = r["results"].view(pkg.TRACK_RESULT).reshape(-1)
    return r


def _frame_bytes_device(r, b, n_feat):
    """everything the call says about frame b, as bytes (offsets taken out: a frame alone starts at 0)"""
    s = slice(int(r["offsets"][b]), int(r["offsets"][b + 1]))
    assert (r["matched"][b, n_feat:] == -1).all()
    return tuple(np.ascontiguousarray(x).tobytes() for x in (r["points3d"][s], r["points2d"][s], r["mp_idx"][s], r["feat_idx"][s], r["poses"][b],
                                                              r["inlier"][s], r["err"][s], r["pnp_results"][b:b + 1], r["matched"][b, :n_feat],
                                                              r["results"][b:b + 1]))


def _frame_bytes_host(pkg, t):
    rec = np.zeros(1, pkg.TRACK_RESULT)
    rec[0] = (t.status, t.n_in_front, len(t.mp_idx), t.n_inliers)
    pr = np.zeros(1, pkg.PNP_RESULT)
    pr[0] = tuple(t.pnp_stats[k] for k in pkg.PNP_RESULT.names)
    return tuple(np.ascontiguousarray(x).tobytes() for x in (t.points3d, t.points2d, t.mp_idx, t.feat_idx, t.pose, t.inlier_mask.astype(np.uint8),
                                                              t.reproj_errors, pr, t.matched, rec))


def _pnp_reference(h, cam, off, gs, frames, max_n):
    """solve_pnp_ransac_batch_device on the spec's gathered arrays"""
    import torch
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    N = int(off[-1])
    p3 = np.concatenate([g["points3d"] for g in gs] + [np.zeros((1, 3))])          # (one spare row: an empty tensor has no address)
    p2 = np.concatenate([g["points2d"] for g in gs] + [np.zeros((1, 2), np.float32)])
    poses, inl, err, res = h.solve_pnp_ransac_batch_device(cam, d(off), d(p3), d(p2), d(np.stack([f[5] for f in frames])), max_n)
    torch.cuda.synchronize()
    return poses.cpu().numpy(), inl.cpu().numpy()[:N], err.cpu().numpy()[:N], res.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", [0, 1])
def test_equals_spec_and_pnp_composition(gpu_handle, pkg, cam, batches, expected, mode, name):
    frames = batches[name]
    off, ms, gs = expected[(mode, name)]
    r = _run_device(gpu_handle, pkg, cam, frames, mode)
    N = int(off[-1])
    assert r["offsets"].tolist() == off.tolist()
    cat = lambda k, empty: np.concatenate([g[k] for g in gs]) if N else empty
    assert r["mp_idx"][:N].tolist() == cat("mp_idx", np.zeros(0)).tolist() and r["feat_idx"][:N].tolist() == cat("feat_idx", np.zeros(0)).tolist()
    assert r["points3d"][:N].tobytes() == cat("points3d", np.zeros((0, 3))).tobytes()
    assert r["points2d"][:N].tobytes() == cat("points2d", np.zeros((0, 2), np.float32)).tobytes()
    max_n = max(len(f[2]) for f in frames)
    poses, inl, err, res = _pnp_reference(gpu_handle, cam, off, gs, frames, max_n)
    assert r["inlier"][:N].tobytes() == inl.tobytes() and r["err"][:N].tobytes() == err.tobytes()
    assert r["pnp_results"].tobytes() == res.tobytes()
    pres = res.view(pkg.PNP_RESULT).reshape(-1)
    cfg = S.default_config(mode)
    for b, f in enumerate(frames):
        s = slice(int(off[b]), int(off[b + 1]))
        rec, pose, matched = S.finish(cfg, len(f[0]), ms[b], gs[b], f[5], poses[b], inl[s], int(pres[b]["status"]), int(pres[b]["n_inliers"]))
        got = r["results"][b]
        assert {k: int(got[k]) for k in pkg.TRACK_RESULT.names} == rec, (name, b)
        assert r["poses"][b].tobytes() == pose.tobytes(), (name, b)
        assert r["matched"][b, :len(f[0])].tolist() == matched.tolist() and (r["matched"][b, len(f[0]):] == -1).all(), (name, b)


def test_scenes_reach_every_status(gpu_handle, pkg, cam, batches):
    """the named scenes end where their names say (the spec comparison above holds whatever they do)"""
    st = lambda name, mode: _run_device(gpu_handle, pkg, cam, batches[name], mode)["results"]["status"].tolist()
    assert st("corr_3_4", 1) == [pkg.TRACK_TOO_FEW_CORRESPONDENCES, pkg.TRACK_OK]
    assert st("corr_9_10", 0) == [pkg.TRACK_TOO_FEW_CORRESPONDENCES, pkg.TRACK_OK]
    assert st("no_model_next_to_good", 1) == [pkg.TRACK_NO_MODEL, pkg.TRACK_OK]
    assert st("no_model_next_to_good", 0) == [pkg.TRACK_TOO_FEW_INLIERS, pkg.TRACK_OK]
    r = _run_device(gpu_handle, pkg, cam, batches["duplicate_inliers"], 1)
    f = r["feat_idx"][:int(r["offsets"][1])]
    dup = [x for x in set(f.tolist()) if (f == x).sum() == 2]
    assert len(dup) == 1 and r["inlier"][:len(f)][f == dup[0]].all() and r["matched"][0, dup[0]] == 30      # both inliers: the later point stays
    assert st("b3", 1) == [pkg.TRACK_OK] * 3 and st("b3", 0) == [pkg.TRACK_OK] * 3


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", [0, 1])
def test_host_form_and_single_frames_equal_device_batch(gpu_handle, pkg, cam, batches, mode, name):
    frames = batches[name]
    r = _run_device(gpu_handle, pkg, cam, frames, mode)
    host = gpu_handle.track_frames(cam, frames, _cfg(pkg, mode))
    for b, f in enumerate(frames):
        want = _frame_bytes_device(r, b, len(f[0]))
        assert _frame_bytes_host(pkg, host[b]) == want, (name, b, "host form")
        if len(frames) > 1:
            one = _run_device(gpu_handle, pkg, cam, [f], mode)
            assert _frame_bytes_device(one, 0, len(f[0])) == want, (name, b, "frame alone")


@pytest.mark.parametrize("mode", [0, 1])
def test_feature_count_above_max_feat_is_not_read(gpu_handle, pkg, cam, batches, mode):
    import torch
    frames = batches["b3"]
    good = _run_device(gpu_handle, pkg, cam, frames, mode)
    a = _device_inputs(frames)
    fc = a["feat_count"].cpu().numpy().copy()
    fc[1] = a["max_feat"] + 1
    r = _run_device(gpu_handle, pkg, cam, frames, mode, feat_count=torch.from_numpy(fc).cuda())
    rec = r["results"][1]
    assert (int(rec["status"]), int(rec["n_correspondences"]), int(rec["n_inliers"])) == (pkg.TRACK_TOO_FEW_CORRESPONDENCES, 0, 0)
    assert int(rec["n_in_front"]) == int(good["results"][1]["n_in_front"])
    assert r["offsets"][1] == r["offsets"][2] and (r["matched"][1] == -1).all() and r["poses"][1].tobytes() == frames[1][5].tobytes()
    for b in (0, 2):
        assert _frame_bytes_device(r, b, len(frames[b][0])) == _frame_bytes_device(good, b, len(frames[b][0]))


def test_features_straight_from_the_extractor(gpu_handle, pkg, cam):
    """feat_count is a strided view of process_stereo_batch_device's device-side counts, read by the call's kernels on the handle's
    stream.  The counts are zeroed, the extraction is enqueued and the tracker is called with no synchronisation in between: were the
    counts read anywhere but behind the extraction, the frames would have no features and no correspondences.  The result equals the
    host form on the downloaded features."""
    import torch
    P = 8
    imgs = torch.from_numpy(np.stack([np.stack(pkg.synth.stereo_pair(5, k)) for k in range(P)])).cuda()
    cap = gpu_handle.orb_params.n_features + 2048
    out = gpu_handle.alloc_batch_outputs(P, cap)
    start, count = gpu_handle.track_feature_slots(out)                   # taken before anything is extracted: a view, nothing is read
    assert count.data_ptr() == out["nkp"].data_ptr() and count.stride(0) == 2 and start.tolist() == [2 * b * cap for b in range(P)]
    # a first extraction, downloaded, only to make map points that belong to the features
    gpu_handle.process_stereo_batch_device(imgs, out)
    gpu_handle.synchronize()
    nkp = out["nkp"].cpu().numpy()
    assert nkp[:, 0].min() > 300
    rng = np.random.default_rng(9)
    frames = []
    for b in range(P):
        n = int(nkp[b, 0])
        kp = out["kp"][b, 0, :n].cpu().numpy().view(G.KEYPOINT).reshape(-1)
        desc = out["desc"][b, 0, :n].cpu().numpy()
        T = G.pose(rng)
        pick = rng.choice(n, 200 + 20 * b, replace=False)
        X = G.backproject(T, np.stack([kp["x"][pick], kp["y"][pick]], 1).astype(np.float64) + rng.normal(0.0, 0.4, (len(pick), 2)), rng.uniform(2.0, 10.0, len(pick)))
        frames.append((kp, desc, X, desc[pick].copy(), T, G.perturb(rng, T)))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    mo = np.zeros(P + 1, np.int32); mo[1:] = np.cumsum([len(f[2]) for f in frames])
    pos, md = d(np.concatenate([f[2] for f in frames])), d(np.concatenate([f[3] for f in frames]))
    sp, pr = d(np.stack([f[4] for f in frames])), d(np.stack([f[5] for f in frames]))
    for mode in (0, 1):
        out["nkp"].zero_()                                              # stale counts say: no features
        gpu_handle.process_stereo_batch_device(imgs, out)               # asynchronous on the handle's stream
        o = gpu_handle.track_frames_device(cam, out["kp"].view(-1, 7), out["desc"].view(-1, 32), start, count, cap, pos, md, mo, sp, pr,
                                           cfg=_cfg(pkg, mode))
        gpu_handle.synchronize()
        r = {k: v.cpu().numpy() for k, v in o.items()}
        r["pnp_results"] = r["pnp_results"].view(pkg.PNP_RESULT).reshape(-1); r["results"] = r["results"].view(pkg.TRACK_RESULT).reshape(-1)
        host = gpu_handle.track_frames(cam, frames, _cfg(pkg, mode))
        for b in range(P):
            assert host[b].status == pkg.TRACK_OK and len(host[b].mp_idx) > 100
            assert _frame_bytes_host(pkg, host[b]) == _frame_bytes_device(r, b, len(frames[b][0])), (mode, b)


def test_outputs_feed_pose_inertial_on_the_device(gpu_handle, pkg, cam, batches):
    """offsets / points / poses of the fused call go into pose_inertial_optimization_batch_device as they are; the result equals the
    host-path call on the same correspondences."""
    import torch
    frames = batches["b3"]
    B = len(frames)
    a = _device_inputs(frames)
    o = gpu_handle.track_frames_device(cam, cfg=_cfg(pkg, 1), **a)
    M = int(a["mp_offsets"][-1])
    rng = np.random.default_rng(4)
    vel = rng.normal(0.0, 0.2, (B, 3)); bias = rng.normal(0.0, 0.01, (B, 6)); pvel = vel + rng.normal(0.0, 0.02, (B, 3))
    prev = np.stack([G.perturb(rng, f[4], 2.0, 0.05) for f in frames])
    preint = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.05]), (B, 1))
    stereo = (rng.uniform(size=M) < 0.5).astype(np.uint8)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    poses, v, bi, inl, res = gpu_handle.pose_inertial_optimization_batch_device(cam, o["offsets"], o["points3d"], o["points2d"], d(stereo), o["poses"],
                                                                                 d(vel), d(bias), d(prev), d(pvel), d(preint))
    torch.cuda.synchronize()
    off = o["offsets"].cpu().numpy()
    host_t = gpu_handle.track_frames(cam, frames, _cfg(pkg, 1))
    host = gpu_handle.pose_inertial_optimization_batch(
        cam, [(t.pose, vel[b], bias[b], prev[b], pvel[b], preint[b], t.points3d, t.points2d, stereo[off[b]:off[b + 1]]) for b, t in enumerate(host_t)])
    res = res.cpu().numpy().view(pkg.POSE_INERTIAL_RESULT).reshape(-1)
    poses, v, bi, inl = poses.cpu().numpy(), v.cpu().numpy(), bi.cpu().numpy(), inl.cpu().numpy()
    for b, hr in enumerate(host):
        assert (poses[b].tobytes(), v[b].tobytes(), bi[b].tobytes(), inl[off[b]:off[b + 1]].tobytes()) == \
               (hr.pose.tobytes(), hr.velocity.tobytes(), hr.bias.tobytes(), hr.inlier_mask.astype(np.uint8).tobytes()), b
        assert (int(res[b]["num_inliers"]), int(res[b]["num_observations"]), int(res[b]["iterations"]), int(res[b]["status"])) == \
               (hr.num_inliers, hr.num_observations, hr.iterations, hr.status) and hr.num_observations > 30


def test_invalid_arguments_are_refused(gpu_handle, pkg, cam, batches):
    frames = batches["b2"]
    a = _device_inputs(frames)
    bad = [dict(mp_offsets=np.array([0], np.int32)),                                  # n_frames = 0
           dict(mp_offsets=np.array([0, 150, 100], np.int32)),                         # not ascending
           dict(mp_offsets=np.array([1, 150, 220], np.int32))]                         # not from 0
    for over in bad:
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.track_frames_device(cam, cfg=_cfg(pkg, 1), **dict(a, **over))
        assert e.value.code == -1 and "orbx_track_frames_device" in str(e.value)
    for cfg in (pkg.TrackConfig(mode=2), pkg.TrackConfig(radius=-1.0), pkg.TrackConfig(img_w=0.0), pkg.TrackConfig(min_correspondences=3),
                pkg.TrackConfig(min_inliers=-1), pkg.TrackConfig(radius=float("nan"))):
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.track_frames_device(cam, cfg=cfg, **a)
        assert e.value.code == -1
        with pytest.raises(pkg.OrbxError):
            gpu_handle.track_frames(cam, frames, cfg)
    with pytest.raises(pkg.OrbxError):
        gpu_handle.track_frames(cam, [], _cfg(pkg, 1))
    # a PnP configuration out of range is refused by the tracker's own check, before anything is enqueued (PnP's check, behind the
    # first three launches, would name orbx_pnp_ransac_batch_device)
    with pytest.raises(pkg.OrbxError) as e:
        gpu_handle.track_frames_device(cam, cfg=_cfg(pkg, 1), pnp_cfg=pkg.PnPConfig(model_points=3), **a)
    assert e.value.code == -1 and "orbx_track_frames_device" in str(e.value)
    with pytest.raises(pkg.OrbxError):
        gpu_handle.track_frames(cam, frames, _cfg(pkg, 1), pkg.PnPConfig(max_iterations=0))
