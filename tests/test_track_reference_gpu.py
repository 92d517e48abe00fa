"""orbx_track_reference[_device] / orbx_keyframe_track_reference on the GPU against tests/track_reference_spec.py: exact equality
everywhere.  Matches, counts, offsets, the index arrays and the gathered points equal the spec; pose, inlier mask, errors and PnP's
records equal, byte for byte, what solve_pnp_ransac_batch_device returns for the spec's gathered arrays (composition, no tolerance)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import track_reference_scenes as R
import track_reference_spec as S
from test_track_reference_cpu import build_driver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(R.batches())


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.CameraModel(**R.CAMERA)


@pytest.fixture(scope="module")
def batches():
    return R.batches()


@pytest.fixture(scope="module")
def expected(oracle, batches):
    """name -> (offsets, [matches], [gathered]): computed once, never modified"""
    return {name: S.match_and_gather(oracle, fr) for name, fr in batches.items()}


def _d(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cat(parts, empty):
    return np.concatenate(parts) if sum(len(p) for p in parts) else empty


def _frame_inputs(frames):
    kp = _cat([f[0] for f in frames], np.zeros(1, R.KEYPOINT)).view(np.float32).reshape(-1, 7).copy()
    desc = _cat([f[1] for f in frames], np.zeros((1, 32), np.uint8))
    fc = np.array([len(f[0]) for f in frames], np.int32)
    fs = (np.cumsum(fc) - fc).astype(np.int32)
    return dict(kp=_d(kp), desc=_d(desc), feat_start=_d(fs), feat_count=_d(fc), max_feat=int(fc.max()), priors_wc=_d(np.stack([f[5] for f in frames])))


def _device_inputs(frames):
    a = _frame_inputs(frames)
    ko = np.zeros(len(frames) + 1, np.int32); ko[1:] = np.cumsum([len(f[2]) for f in frames])
    a.update(kf_desc=_d(_cat([f[2] for f in frames], np.zeros((1, 32), np.uint8))), kf_positions=_d(_cat([f[3] for f in frames], np.zeros((1, 3)))),
             kf_valid=_d(_cat([f[4] for f in frames], np.zeros(1, np.uint8))), kf_offsets=ko)
    return a


def _download(pkg, o):
    import torch
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in o.items()}
    r["pnp_results"] = r["pnp_results"].view(pkg.PNP_RESULT).reshape(-1)
    r["results"] = r["results"].view(pkg.TRACK_REF_RESULT).reshape(-1)
    r["matches"] = r["matches"].view(pkg.DMATCH).reshape(-1)
    return r


def _run_device(h, pkg, cam, frames, min_correspondences=4, **over):
    a = _device_inputs(frames)
    a.update(over)
    return _download(pkg, h.track_reference_device(cam, min_correspondences=min_correspondences, **a))


def _frame_bytes_device(r, b, k0):
    """everything the call says about frame b, as bytes (offsets taken out: a frame alone starts at 0); k0: where its keyframe's
    rows start in the packed arrays"""
    s = slice(int(r["offsets"][b]), int(r["offsets"][b + 1]))
    nm = int(r["results"][b]["n_matches"])
    return tuple(np.ascontiguousarray(x).tobytes() for x in (r["matches"][k0:k0 + nm], r["points3d"][s], r["points2d"][s], r["kf_idx"][s], r["feat_idx"][s],
                                                              r["poses"][b], r["inlier"][s], r["err"][s], r["pnp_results"][b:b + 1], r["results"][b:b + 1]))


def _frame_bytes_host(pkg, t):
    rec = np.zeros(1, pkg.TRACK_REF_RESULT)
    rec[0] = (t.status, len(t.matches), len(t.kf_idx), t.n_inliers)
    pr = np.zeros(1, pkg.PNP_RESULT)
    pr[0] = tuple(t.pnp_stats[k] for k in pkg.PNP_RESULT.names)
    return tuple(np.ascontiguousarray(x).tobytes() for x in (t.matches, t.points3d, t.points2d, t.kf_idx, t.feat_idx, t.pose, t.inlier_mask.astype(np.uint8),
                                                              t.reproj_errors, pr, rec))


def _kf_starts(frames):
    return (np.cumsum([len(f[2]) for f in frames]) - np.array([len(f[2]) for f in frames])).tolist()


def _pnp_reference(h, cam, off, gs, frames, max_n):
    """solve_pnp_ransac_batch_device on the spec's gathered arrays"""
    import torch
    N = int(off[-1])
    p3 = np.concatenate([g["points3d"] for g in gs] + [np.zeros((1, 3))])          # (one spare row: an empty tensor has no address)
    p2 = np.concatenate([g["points2d"] for g in gs] + [np.zeros((1, 2), np.float32)])
    poses, inl, err, res = h.solve_pnp_ransac_batch_device(cam, _d(off), _d(p3), _d(p2), _d(np.stack([f[5] for f in frames])), max_n)
    torch.cuda.synchronize()
    return poses.cpu().numpy(), inl.cpu().numpy()[:N], err.cpu().numpy()[:N], res.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_equals_spec_and_pnp_composition(gpu_handle, pkg, cam, batches, expected, name):
    frames = batches[name]
    off, ms, gs = expected[name]
    r = _run_device(gpu_handle, pkg, cam, frames)
    N = int(off[-1])
    assert r["offsets"].tolist() == off.tolist()
    for b, k0 in enumerate(_kf_starts(frames)):
        assert int(r["results"][b]["n_matches"]) == len(ms[b]), (name, b)
        assert r["matches"][k0:k0 + len(ms[b])].tobytes() == ms[b].tobytes(), (name, b)
    cat = lambda k, empty: np.concatenate([g[k] for g in gs]) if N else empty
    assert r["kf_idx"][:N].tolist() == cat("kf_idx", np.zeros(0)).tolist() and r["feat_idx"][:N].tolist() == cat("feat_idx", np.zeros(0)).tolist()
    assert r["points3d"][:N].tobytes() == cat("points3d", np.zeros((0, 3))).tobytes()
    assert r["points2d"][:N].tobytes() == cat("points2d", np.zeros((0, 2), np.float32)).tobytes()
    max_n = max(len(f[2]) for f in frames)
    poses, inl, err, res = _pnp_reference(gpu_handle, cam, off, gs, frames, max_n)
    assert r["inlier"][:N].tobytes() == inl.tobytes() and r["err"][:N].tobytes() == err.tobytes()
    assert r["pnp_results"].tobytes() == res.tobytes()
    pres = res.view(pkg.PNP_RESULT).reshape(-1)
    for b, f in enumerate(frames):
        rec, pose = S.finish(S.MIN_CORRESPONDENCES, len(ms[b]), gs[b], f[5], poses[b], int(pres[b]["status"]), int(pres[b]["n_inliers"]))
        got = r["results"][b]
        assert {k: int(got[k]) for k in pkg.TRACK_REF_RESULT.names} == rec, (name, b)
        assert r["poses"][b].tobytes() == pose.tobytes(), (name, b)


def test_scenes_reach_every_status(gpu_handle, pkg, cam, batches):
    """the named scenes end where their names say (the spec comparison above holds whatever they do)"""
    run = lambda name: _run_device(gpu_handle, pkg, cam, batches[name])
    st = lambda name: run(name)["results"]["status"].tolist()
    assert st("corr_3_4") == [pkg.TRACK_TOO_FEW_CORRESPONDENCES, pkg.TRACK_OK]
    assert st("no_model_next_to_good") == [pkg.TRACK_NO_MODEL, pkg.TRACK_OK]
    r = run("no_model_next_to_good")
    assert r["poses"][0].tobytes() == batches["no_model_next_to_good"][0][5].tobytes() and r["poses"][1].tobytes() != batches["no_model_next_to_good"][1][5].tobytes()
    r = run("valid_all_zero")
    rec = r["results"][0]
    assert (int(rec["status"]), int(rec["n_correspondences"]), int(rec["n_inliers"])) == (pkg.TRACK_TOO_FEW_CORRESPONDENCES, 0, 0) and int(rec["n_matches"]) >= 20
    assert r["poses"][0].tobytes() == batches["valid_all_zero"][0][5].tobytes()
    r = run("identical")
    assert r["matches"][:1].tolist() == [(0, 0, 0, 0.0)] and int(r["results"][0]["n_matches"]) == 1
    assert st("empty_sides") == [pkg.TRACK_TOO_FEW_CORRESPONDENCES, pkg.TRACK_TOO_FEW_CORRESPONDENCES, pkg.TRACK_OK]
    assert st("realistic") == [pkg.TRACK_OK] and st("b3_shared_keyframe") == [pkg.TRACK_OK] * 3
    # there is no inlier guard on this path: whatever PnP finds, TOO_FEW_INLIERS is never produced
    for name in ("ties", "thin", "small"):
        assert set(st(name)) <= {pkg.TRACK_OK, pkg.TRACK_NO_MODEL, pkg.TRACK_TOO_FEW_CORRESPONDENCES}


def test_min_correspondences_is_the_guard(gpu_handle, pkg, cam, batches):
    """four correspondences under min_correspondences = 5: PnP ran on them, the frame still ends TOO_FEW_CORRESPONDENCES with the prior"""
    frames = batches["corr_3_4"]
    r = _run_device(gpu_handle, pkg, cam, frames, min_correspondences=5)
    assert r["results"]["status"].tolist() == [pkg.TRACK_TOO_FEW_CORRESPONDENCES] * 2 and r["results"]["n_inliers"].tolist() == [0, 0]
    assert r["results"]["n_correspondences"].tolist() == [3, 4]
    assert r["poses"][1].tobytes() == frames[1][5].tobytes() and int(r["pnp_results"][1]["status"]) == pkg.PNP_OK


@pytest.mark.parametrize("name", NAMES)
def test_host_form_and_single_frames_equal_device_batch(gpu_handle, pkg, cam, batches, name):
    frames = batches[name]
    r = _run_device(gpu_handle, pkg, cam, frames)
    host = gpu_handle.track_reference(cam, frames)
    for b, (f, k0) in enumerate(zip(frames, _kf_starts(frames))):
        want = _frame_bytes_device(r, b, k0)
        assert _frame_bytes_host(pkg, host[b]) == want, (name, b, "host form")
        if len(frames) > 1:
            one = _run_device(gpu_handle, pkg, cam, [f])
            assert _frame_bytes_device(one, 0, 0) == want, (name, b, "frame alone")


def test_keyframe_handles_equal_packed_rows(gpu_handle, pkg, cam, batches):
    """frames 0 and 2 name the same resident keyframe (one handle listed twice); the packed form repeats its rows"""
    import torch
    frames = batches["b3_shared_keyframe"]
    packed = _run_device(gpu_handle, pkg, cam, frames)
    mk = lambda f: pkg.KeyFrame(gpu_handle, torch.zeros((max(len(f[2]), 1), 7), dtype=torch.float32, device="cuda"), _d(f[2]), len(f[2]))
    ka, kb = mk(frames[0]), mk(frames[1])
    try:
        a = _frame_inputs(frames)
        o = gpu_handle.keyframe_track_reference(cam, [ka, kb, ka], a["kp"], a["desc"], a["feat_start"], a["feat_count"], a["max_feat"], [f[3] for f in frames],
                                                [f[4] for f in frames], a["priors_wc"])
        r = _download(pkg, o)
        assert r["offsets"].tolist() == packed["offsets"].tolist()
        for b, k0 in enumerate(_kf_starts(frames)):
            assert _frame_bytes_device(r, b, k0) == _frame_bytes_device(packed, b, k0), b
        # a keyframe whose feature count disagrees with the rows given for it
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.keyframe_track_reference(cam, [ka, kb, kb], a["kp"], a["desc"], a["feat_start"], a["feat_count"], a["max_feat"], [f[3] for f in frames],
                                                [f[4] for f in frames], a["priors_wc"])
        assert e.value.code == -1 and "orbx_keyframe_track_reference" in str(e.value)
    finally:
        gpu_handle.synchronize()
        ka.close(); kb.close()


@pytest.mark.parametrize("bad", ["above", "negative"])
def test_feature_count_outside_bounds_is_not_read(gpu_handle, pkg, cam, batches, bad):
    frames = batches["b3_shared_keyframe"]
    good = _run_device(gpu_handle, pkg, cam, frames)
    a = _device_inputs(frames)
    fc = a["feat_count"].cpu().numpy().copy()
    fc[1] = a["max_feat"] + 1 if bad == "above" else -1
    r = _run_device(gpu_handle, pkg, cam, frames, feat_count=_d(fc))
    rec = r["results"][1]
    assert (int(rec["status"]), int(rec["n_matches"]), int(rec["n_correspondences"]), int(rec["n_inliers"])) == (pkg.TRACK_TOO_FEW_CORRESPONDENCES, 0, 0, 0)
    assert r["offsets"][1] == r["offsets"][2] and r["poses"][1].tobytes() == frames[1][5].tobytes()
    ks = _kf_starts(frames)
    for b in (0, 2):
        assert _frame_bytes_device(r, b, ks[b]) == _frame_bytes_device(good, b, ks[b])


def test_features_straight_from_the_extractor(gpu_handle, pkg, cam):
    """feat_count is a strided view of process_stereo_batch_device's device-side counts, read by the call's kernels on the handle's
    stream.  The counts are zeroed, the extraction is enqueued and the tracker is called with no synchronisation in between: were the
    counts read anywhere but behind the extraction, the frames would have no features and no matches.  Frame b is the left image of
    pair b, its reference keyframe the right image's features with a map point behind most of them.  The result equals the host
    form on the downloaded features."""
    import torch
    z = np.load(os.path.join(ROOT, "tests", "golden", "small_quota_320x240_n150_images.npz"))
    pairs = np.stack([np.stack([z["left"], z["right"]]), np.stack([z["right"], z["left"]])])
    P = len(pairs)
    imgs = torch.from_numpy(pairs).cuda()
    cap = gpu_handle.orb_params.n_features + 2048
    out = gpu_handle.alloc_batch_outputs(P, cap)
    start, count = gpu_handle.track_feature_slots(out)
    assert count.data_ptr() == out["nkp"].data_ptr() and count.stride(0) == 2 and start.tolist() == [2 * b * cap for b in range(P)]
    gpu_handle.process_stereo_batch_device(imgs, out)                    # a first extraction, downloaded, to build the keyframes
    gpu_handle.synchronize()
    nkp = out["nkp"].cpu().numpy()
    assert nkp.min() > 100
    rng = np.random.default_rng(9)
    frames = []
    for b in range(P):
        nl, nr = int(nkp[b, 0]), int(nkp[b, 1])
        kp = out["kp"][b, 0, :nl].cpu().numpy().view(R.KEYPOINT).reshape(-1)
        desc = out["desc"][b, 0, :nl].cpu().numpy()
        kkp = out["kp"][b, 1, :nr].cpu().numpy().view(R.KEYPOINT).reshape(-1)
        kd = out["desc"][b, 1, :nr].cpu().numpy()
        T = R.G.pose(rng)
        X = R.G.backproject(T, np.stack([kkp["x"], kkp["y"]], 1).astype(np.float64), rng.uniform(2.0, 10.0, nr))
        frames.append((kp, desc, kd, X, (rng.uniform(size=nr) < 0.8).astype(np.uint8), R.G.perturb(rng, T)))
    ko = np.zeros(P + 1, np.int32); ko[1:] = np.cumsum([len(f[2]) for f in frames])
    kd, pos, va = _d(np.concatenate([f[2] for f in frames])), _d(np.concatenate([f[3] for f in frames])), _d(np.concatenate([f[4] for f in frames]))
    pr = _d(np.stack([f[5] for f in frames]))
    out["nkp"].zero_()                                                  # stale counts say: no features
    gpu_handle.process_stereo_batch_device(imgs, out)                   # asynchronous on the handle's stream
    o = gpu_handle.track_reference_device(cam, out["kp"].view(-1, 7), out["desc"].view(-1, 32), start, count, cap, kd, pos, va, ko, pr)
    gpu_handle.synchronize()
    r = _download(pkg, o)
    host = gpu_handle.track_reference(cam, frames)
    for b in range(P):
        assert len(host[b].matches) > 20 and len(host[b].kf_idx) > 10
        assert _frame_bytes_host(pkg, host[b]) == _frame_bytes_device(r, b, int(ko[b])), b


def test_outputs_feed_pose_inertial_on_the_device(gpu_handle, pkg, cam, batches):
    """offsets / points / poses of the fused call go into pose_inertial_optimization_batch_device as they are; the result equals the
    host-path call on the same correspondences."""
    import torch
    frames = batches["b3_shared_keyframe"]
    B = len(frames)
    a = _device_inputs(frames)
    o = gpu_handle.track_reference_device(cam, **a)
    K = int(a["kf_offsets"][-1])
    rng = np.random.default_rng(4)
    vel = rng.normal(0.0, 0.2, (B, 3)); bias = rng.normal(0.0, 0.01, (B, 6)); pvel = vel + rng.normal(0.0, 0.02, (B, 3))
    prev = np.stack([R.G.perturb(rng, f[5], 2.0, 0.05) for f in frames])
    preint = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.05]), (B, 1))
    stereo = (rng.uniform(size=K) < 0.5).astype(np.uint8)
    poses, v, bi, inl, res = gpu_handle.pose_inertial_optimization_batch_device(cam, o["offsets"], o["points3d"], o["points2d"], _d(stereo), o["poses"],
                                                                                 _d(vel), _d(bias), _d(prev), _d(pvel), _d(preint))
    torch.cuda.synchronize()
    off = o["offsets"].cpu().numpy()
    host_t = gpu_handle.track_reference(cam, frames)
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
    import ctypes as C
    frames = batches["corr_3_4"]
    a = _device_inputs(frames)
    for mc in (3, 0, -1):
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.track_reference_device(cam, min_correspondences=mc, **a)
        assert e.value.code == -1 and "orbx_track_reference_device" in str(e.value)
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.track_reference(cam, frames, min_correspondences=mc)
        assert e.value.code == -1
    for over in (dict(kf_offsets=np.array([0, 6, 5], np.int32)), dict(kf_offsets=np.array([1, 6, 13], np.int32))):      # not ascending; not from 0
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.track_reference_device(cam, **dict(a, **over))
        assert e.value.code == -1
    with pytest.raises(pkg.OrbxError) as e:                          # a row minimum packs the frame feature into 22 bits
        gpu_handle.track_reference_device(cam, **dict(a, max_feat=(1 << 22) + 1))
    assert e.value.code == -1
    # a PnP configuration out of range is refused by the call's own check, before anything is enqueued
    with pytest.raises(pkg.OrbxError) as e:
        gpu_handle.track_reference_device(cam, pnp_cfg=pkg.PnPConfig(model_points=3), **a)
    assert e.value.code == -1 and "orbx_track_reference_device" in str(e.value)
    with pytest.raises(pkg.OrbxError):
        gpu_handle.track_reference(cam, frames, pnp_cfg=pkg.PnPConfig(max_iterations=0))
    # n_frames < 0 and a null handle, through the C ABI itself
    L = gpu_handle._L
    pc = pkg.PnPConfig()._c(); c = cam._c()
    tail = [None] * 19
    assert L.orbx_track_reference(gpu_handle._h, C.byref(c), C.byref(pc), C.c_int(4), C.c_int(-1), *tail) == -1
    assert L.orbx_track_reference_device(gpu_handle._h, C.byref(c), C.byref(pc), C.c_int(4), C.c_int(-1), None, None, None, None, C.c_int(1), C.c_int(0),
                                         *([None] * 16)) == -1
    assert L.orbx_keyframe_track_reference(gpu_handle._h, C.byref(c), C.byref(pc), C.c_int(4), C.c_int(-1), None, None, None, None, None, C.c_int(1),
                                           C.c_int(0), *([None] * 15)) == -1
    assert L.orbx_track_reference(None, C.byref(c), C.byref(pc), C.c_int(4), C.c_int(1), *tail) == -1
    assert L.orbx_track_reference_device(None, C.byref(c), C.byref(pc), C.c_int(4), C.c_int(1), None, None, None, None, C.c_int(1), C.c_int(0),
                                         *([None] * 16)) == -1
    assert L.orbx_keyframe_track_reference(None, C.byref(c), C.byref(pc), C.c_int(4), C.c_int(1), None, None, None, None, None, C.c_int(1), C.c_int(0),
                                           *([None] * 15)) == -1
    # no frames: nothing to do
    assert L.orbx_track_reference(gpu_handle._h, C.byref(c), C.byref(pc), C.c_int(4), C.c_int(0), *tail) == 0


class _Reader:
    def __init__(self, buf):
        self.buf, self.pos = buf, 0

    def take(self, dtype, n):
        a = np.frombuffer(self.buf, dtype, n, self.pos)
        self.pos += a.nbytes
        return a

    def vec(self, dtype):
        return self.take(dtype, int(self.take("<u8", 1)[0]))


def test_cpp_driver_equals_python_mirror(pkg, batches, tmp_path):
    """include/orbx.hpp: track_reference and track_with_reference_kf give the Python mirror's bytes"""
    tmp = str(tmp_path)
    exe = build_driver(tmp)
    frames = batches["corr_3_4"] + batches["b3_shared_keyframe"][:2]
    c = R.CAMERA
    with open(os.path.join(tmp, "tref_in.bin"), "wb") as f:
        f.write(struct.pack("<i5d", len(frames), c["fx"], c["fy"], c["cx"], c["cy"], c["baseline"]))
        for kp, desc, kd, pos, valid, pr in frames:
            f.write(struct.pack("<ii7d", len(kp), len(kd), *[float(v) for v in pr]))
            for a, t in ((kp, R.KEYPOINT), (desc, np.uint8), (kd, np.uint8), (pos, np.float64), (valid, np.uint8)):
                f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([exe, tmp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "TRACK_REFERENCE_DRIVER_OK" in r.stdout, (r.stdout, r.stderr)
    rd = _Reader(open(os.path.join(tmp, "tref_out.bin"), "rb").read())
    h = pkg.Handle(pkg.CameraModel(**c), 1000, device=0, max_w=752, max_h=480, max_batch=1)
    try:
        want = h.track_reference(pkg.CameraModel(**c), frames)
    finally:
        h.close()
    for t in want:
        rec = rd.take(pkg.TRACK_REF_RESULT, 1); pnp = rd.take(pkg.PNP_RESULT, 1); pose = rd.take("<f8", 7)
        ma, ki, fi, p3, p2, err, inl = rd.vec(pkg.DMATCH), rd.vec("<i4"), rd.vec("<i4"), rd.vec(("<f8", 3)), rd.vec(("<f4", 2)), rd.vec("<f8"), rd.vec("u1")
        assert (rec.tobytes(), pnp.tobytes(), ma.tobytes(), p3.tobytes(), p2.tobytes(), ki.tobytes(), fi.tobytes(), pose.tobytes(), inl.tobytes(),
                err.tobytes()) == tuple(_frame_bytes_host(pkg, t)[i] for i in (9, 8, 0, 1, 2, 3, 4, 5, 6, 7))
    for t in want:
        some = int(rd.take("u1", 1)[0]); pose = rd.take("<f8", 7)
        assert some == (0 if t.status == pkg.TRACK_TOO_FEW_CORRESPONDENCES else 1)
        if some:
            assert pose.tobytes() == t.pose.tobytes()
    assert int(rd.take("<i4", 1)[0]) == 1 and rd.pos == len(rd.buf)
    assert {t.status for t in want} >= {pkg.TRACK_OK, pkg.TRACK_TOO_FEW_CORRESPONDENCES}
