"""The host plumbing the batched forms share (orbx_internal.hpp: UploadRing, orbx_reserve_pinned, the host-call skeleton; DESIGN.md,
"Host staging"), through the entry points that use it.

Ring reuse: a device form copies its small host tables (mp_offsets, the item table, FeatureVector node ids, the keyframe form's
positions / valid) into one of two pinned slots before it returns, so the caller may reuse its arrays at once.  Three calls are
enqueued back to back on a fresh handle with nothing synchronised in between, each table overwritten as soon as its call has returned
(call 2's table is the largest, call 3 takes slot 0 again); every output must equal, byte for byte, the same call made alone on
another fresh handle.  The overwriting values are wrong but in range (offsets of zero, no node, no valid row): a library that read a
table late would give other bytes, not read out of bounds.  The resident map's ring carries the tables of every orbx_map_* device
form: three different forms share it in test_ring_map_device_forms.

Staging growth: a host form's pinned buffer and workspace grow between a small, a large and a small call; each result equals the
device form's on the same data.

Partial download: orbx_pose_inertial_batch copies the inlier flags back only when asked for them."""
import os
import struct
import subprocess

import numpy as np
import pytest

import loop_verify_scenes as Z
import track_reference_scenes as R
import tracking_scenes as G
import test_track_reference_gpu as TR
import test_tracking_gpu as TF
from test_pose_inertial_cpu import build_pose_inertial_driver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.CameraModel(**G.CAMERA)


def _fresh(pkg, cam):
    return pkg.Handle(cam, 1000, device=0, max_w=752, max_h=480, max_batch=1)


def _d(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(pkg, o, records):
    """a device form's dict of tensors as numpy arrays (after a synchronise), the record arrays viewed as their dtypes"""
    r = {k: v.cpu().numpy() for k, v in o.items()}
    for k, dt in records.items():
        r[k] = r[k].view(dt).reshape(-1)
    return r


def _back_to_back(pkg, cam, calls, enqueue, spoil, finish):
    """enqueue(handle, call) -> (outputs, host tables) for each call on one fresh handle, spoiling the tables as soon as the call has
    returned and synchronising once at the end; then every call alone on a handle of its own.  Returns ([together], [alone])."""
    h = _fresh(pkg, cam)
    try:
        outs = []
        for c in calls:
            o, tables = enqueue(h, c)
            for t in tables:
                spoil(t)
            outs.append(o)
        h.synchronize()
        together = [finish(o) for o in outs]
    finally:
        h.close()
    alone = []
    for c in calls:
        h = _fresh(pkg, cam)
        try:
            o, _ = enqueue(h, c)
            h.synchronize()
            alone.append(finish(o))
        finally:
            h.close()
    return together, alone


def _zero(t):
    assert t.flags["C_CONTIGUOUS"] and t.flags["WRITEABLE"]
    t[...] = 0


# ---- ring reuse ---------------------------------------------------------------------------------------------------------
# frames per call: 2, then 3 (the larger table), then 1 (slot 0 again)
def _track_calls():
    return [[G.frame(201, 40, 60), G.frame(202, 35, 55)], [G.frame(203, 40, 60), G.frame(204, 45, 64), G.frame(205, 30, 50)], [G.frame(206, 38, 58)]]


@pytest.fixture(scope="module")
def tref_calls():
    return [[R.ref_frame(211, 50, 60), R.ref_frame(212, 45, 55)], [R.ref_frame(213, 50, 60), R.ref_frame(214, 55, 64), R.ref_frame(215, 40, 50)],
            [R.ref_frame(216, 48, 58)]]


def _lv_calls():
    return [[Z.keyframe_pair(221 + 10 * n + k, 50, 34, with_nodes=True) for k in range(n)] for n in (2, 3, 1)]


def test_ring_track_frames_device(pkg, cam):
    def enqueue(h, frames):
        a = TF._device_inputs(frames)
        mo = a["mp_offsets"]
        assert mo.dtype == np.int32 and mo.flags["C_CONTIGUOUS"]
        return (h.track_frames_device(cam, cfg=pkg.TrackConfig.for_mode(1), **a), [len(f[0]) for f in frames]), [mo]

    def finish(x):
        o, nf = x
        r = _host(pkg, o, dict(pnp_results=pkg.PNP_RESULT, results=pkg.TRACK_RESULT))
        return [TF._frame_bytes_device(r, b, n) for b, n in enumerate(nf)] + [r["offsets"].tobytes()], r

    calls = _track_calls()
    together, alone = _back_to_back(pkg, cam, calls, enqueue, _zero, finish)
    for k, ((got, _), (want, r)) in enumerate(zip(together, alone)):
        assert int(r["offsets"][-1]) > 20 * len(calls[k]), k                      # the calls found their map points
        assert got == want, k


def _tref_finish(pkg, frames):
    def finish(o):
        r = _host(pkg, o, dict(pnp_results=pkg.PNP_RESULT, results=pkg.TRACK_REF_RESULT, matches=pkg.DMATCH))
        return [TR._frame_bytes_device(r, b, k0) for b, k0 in enumerate(TR._kf_starts(frames))] + [r["offsets"].tobytes()], r
    return finish


def test_ring_track_reference_device(pkg, cam, tref_calls):
    def enqueue(h, frames):
        a = TR._device_inputs(frames)
        ko = a["kf_offsets"]
        assert ko.dtype == np.int32 and ko.flags["C_CONTIGUOUS"]
        return (h.track_reference_device(cam, **a), frames), [ko]

    finish = lambda x: _tref_finish(pkg, x[1])(x[0])
    together, alone = _back_to_back(pkg, cam, tref_calls, enqueue, _zero, finish)
    for k, ((got, _), (want, r)) in enumerate(zip(together, alone)):
        assert int(r["results"]["n_matches"].min()) > 10, k
        assert got == want, k


def test_ring_keyframe_track_reference(pkg, cam, tref_calls):
    """The keyframe form's positions / valid are host arrays that travel through the ring with the item table.  Handle.keyframe_track_reference
    packs its per-frame lists into temporaries of its own, so the library is called here as that method calls it, with packed arrays
    the test owns and spoils."""
    import ctypes as C
    import torch
    from orb_slam3_rust_amd.api import _vp

    def enqueue(h, frames):
        feats = [(torch.zeros((max(len(f[2]), 1), 7), dtype=torch.float32, device="cuda"), _d(f[2])) for f in frames]    # alive until the synchronise
        kfs = [pkg.KeyFrame(h, kp, desc, len(desc)) for kp, desc in feats]
        a = TR._frame_inputs(frames)
        B = len(frames)
        ko = np.zeros(B + 1, np.int32); ko[1:] = np.cumsum([len(f[2]) for f in frames])
        po = np.ascontiguousarray(np.concatenate([f[3] for f in frames]), np.float64)
        va = np.ascontiguousarray(np.concatenate([f[4] for f in frames]), np.uint8)
        o = h._track_reference_outputs(B, int(ko[-1]), a["priors_wc"].device)
        pc = pkg.PnPConfig()._c(); c = cam._c()
        arr = (C.c_void_p * B)(*[k._p for k in kfs])
        h._after_torch(a["kp"], a["desc"], a["feat_start"], a["feat_count"], a["priors_wc"], *o.values())
        h._check(h._L.orbx_keyframe_track_reference(
            h._h, C.byref(c), C.byref(pc), C.c_int(4), C.c_int(B), arr, _vp(a["kp"]), _vp(a["desc"]), _vp(a["feat_start"]), _vp(a["feat_count"]),
            C.c_int(1), C.c_int(a["max_feat"]), _vp(po), _vp(va), _vp(ko), _vp(a["priors_wc"]), _vp(o["matches"]), _vp(o["offsets"]), _vp(o["points3d"]),
            _vp(o["points2d"]), _vp(o["kf_idx"]), _vp(o["feat_idx"]), _vp(o["poses"]), _vp(o["inlier"]), _vp(o["err"]), _vp(o["pnp_results"]),
            _vp(o["results"])))
        return (o, frames, kfs, feats), [ko, po, va]

    def finish(x):
        o, frames, kfs, _ = x
        for k in kfs:                                                                    # (after the handle's synchronise)
            k.close()
        return _tref_finish(pkg, frames)(o)

    together, alone = _back_to_back(pkg, cam, tref_calls, enqueue, _zero, finish)
    for k, ((got, _), (want, r)) in enumerate(zip(together, alone)):
        assert int(r["results"]["n_matches"].min()) > 10 and int(r["offsets"][-1]) > 10 * len(tref_calls[k]), k
        assert got == want, k
    # ... and the packed device form agrees, so the reference is not wrong in the same way
    h = _fresh(pkg, cam)
    try:
        r = TR._run_device(h, pkg, cam, tref_calls[1])
        assert [TR._frame_bytes_device(r, b, k0) for b, k0 in enumerate(TR._kf_starts(tref_calls[1]))] == alone[1][0][:-1]
    finally:
        h.close()


def test_ring_verify_loop_candidates_device_feature_vector(pkg, cam):
    def enqueue(h, pairs):
        a, cn, ln, co, lo, cp, lp = h._loop_verify_pack(pairs)
        assert cn.dtype == np.uint32 and ln.dtype == np.uint32 and co.dtype == np.int32 and lo.dtype == np.int32 and cp.dtype == np.float64
        assert all(t.flags["C_CONTIGUOUS"] for t in (cn, ln, co, lo, cp, lp))
        o = h.verify_loop_candidates_device(cam, _d(a["cur_desc"]), _d(a["cur_pts"]), _d(a["cur_has"]), co, cp,
                                            _d(a["loop_kp"].view(np.uint8).reshape(-1, 28)), _d(a["loop_desc"]), _d(a["loop_pts"]), _d(a["loop_has"]),
                                            lo, lp, cn, ln)
        return (o, co.copy(), h), [cn, ln, co, lo, cp, lp]

    def spoil(t):
        if t.dtype == np.uint32:
            t[...] = Z.S.NODE_NONE                                                       # in no node: nothing would match
        else:
            _zero(t)

    def finish(x):
        o, co, h = x
        r = _host(pkg, o, dict(results=pkg.LOOP_VERIFY_RESULT, matches=pkg.DMATCH))
        per_pair = h._loop_verify_unpack(len(co) - 1, co, r["matches"], r["feature_matches"], r["pts_current"], r["pts_loop"], r["inlier"], r["sim3"],
                                         r["results"])
        return [(p["status"], p["matches"].tobytes(), p["feature_matches"].tobytes(), p["pts_current"].tobytes(), p["pts_loop"].tobytes(),
                 p["inlier"].tobytes(), p["sim3"].tobytes(), p["record"].tobytes()) for p in per_pair], per_pair

    together, alone = _back_to_back(pkg, cam, _lv_calls(), enqueue, spoil, finish)
    for k, ((got, _), (want, per_pair)) in enumerate(zip(together, alone)):
        assert all(len(p["matches"]) >= 15 and len(p["feature_matches"]) >= 15 for p in per_pair), k      # matched by node, and Sim3 ran
        assert got == want, k


def _map_world(pkg, h):
    """a store of capacity 64 with 48 live points and four keyframes of 8-16 features whose slot tables name live slots, dead slots,
    -1 and repeats; made before the calls (set_map_point_slots waits for its copy)"""
    import torch
    rng = np.random.default_rng(231)
    mp = pkg.MapPointStore(h, 64)
    live = np.sort(rng.choice(64, 48, replace=False)).astype(np.int32)
    mp.set(live, rng.normal(0.0, 2.0, (48, 3)), rng.integers(0, 256, (48, 32), dtype=np.uint8))
    kfs = []
    for n in (8, 11, 14, 16):
        kfs.append(pkg.KeyFrame(h, torch.zeros((n, 7), dtype=torch.float32, device="cuda"), torch.zeros((n, 32), dtype=torch.uint8, device="cuda"), n))
        kfs[-1].set_map_point_slots(mp, rng.integers(-1, 64, n).astype(np.int32))
    return mp, kfs, live, _d(rng.integers(0, 64, 12).astype(np.int32))


def test_ring_map_device_forms(pkg, cam):
    """The resident map's ring (every orbx_map_* device form's tables go through it): covisibility (host table: queries), observations
    (slots, the largest table) and the slot-source selection (src_offsets), back to back with nothing synchronised in between."""
    def tables(live):
        return [("cov", np.array([2, 0], np.int32)), ("obs", live[::-1][:40].copy()), ("sel", np.array([0, 5, 12], np.int32))]

    def enqueue(h, world, kind, t):
        mp, kfs, _, d_src = world
        assert t.dtype == np.int32 and t.ndim == 1 and t.flags["C_CONTIGUOUS"]              # the wrapper hands the library this memory
        if kind == "cov":
            return h.map_covisibility_device(mp, kfs, t, n_best=2)
        if kind == "obs":
            return h.map_observations_device(mp, kfs, t)
        return h.map_select_points_device(mp, src_slots=d_src, src_offsets=t)

    def spoil(kind, t):                                                                      # wrong, and what the call accepts
        assert t.flags["WRITEABLE"]
        t[...] = {"cov": (t + 1) % 4, "obs": np.roll(t, 1), "sel": np.zeros_like(t)}[kind]

    def finish(kind, o):
        r = {k: v.cpu().numpy() for k, v in o.items()}
        if kind == "cov":
            assert int(r["weights"].sum()) > 0 and int(r["n_best"].min()) > 0
            return [r[k].tobytes() for k in ("weights", "best", "n_best")]
        if kind == "obs":
            n = int(r["obs_start"][-1])
            assert n > 20
            return [r["obs_start"].tobytes(), r["obs_kf"][:n].tobytes(), r["obs_feat"][:n].tobytes()]
        n = int(r["list_offsets"][-1])
        assert 0 < n < 12 and int(r["list_offsets"][1]) > 0                                  # some entries are dead, both frames have a list
        return [r["list_offsets"].tobytes()] + [r[k][:n].tobytes() for k in ("list_slot", "positions", "mp_desc")]

    def run(which):
        h = _fresh(pkg, cam)
        try:
            world = _map_world(pkg, h)
            h.synchronize()
            outs = []
            for kind, t in tables(world[2]):
                if which in (None, kind):
                    outs.append((kind, enqueue(h, world, kind, t)))
                    spoil(kind, t)
            h.synchronize()
            res = [finish(kind, o) for kind, o in outs]
            for k in world[1]:
                k.close()
            world[0].close()
            return res
        finally:
            h.close()

    together = run(None)
    assert len(together) == 3
    for k, kind in enumerate(("cov", "obs", "sel")):
        assert together[k] == run(kind)[0], kind


# ---- staging growth -----------------------------------------------------------------------------------------------------
BIG = 32768          # a problem whose blobs exceed the 1 MiB the first small call allocates


def test_pnp_host_staging_grows(pkg, cam):
    import torch
    small = pkg.synth.pnp_problem(31, 8, 0.0, 5.0, 0.1)
    big = pkg.synth.pnp_problem(32, BIG, 0.3, 5.0, 0.1)
    h = _fresh(pkg, cam)
    try:
        host = [h.solve_pnp_ransac_batch(cam, [(s["points3d"], s["points2d"], s["prior_wc"])])[0] for s in (small, big, small)]
        for s, g in zip((small, big, small), host):
            n = len(s["points3d"])
            poses, inl, err, res = h.solve_pnp_ransac_batch_device(cam, _d(np.array([0, n], np.int32)), _d(s["points3d"]),
                                                                   _d(np.ascontiguousarray(s["points2d"], np.float32)), _d(s["prior_wc"].reshape(1, 7)), n)
            torch.cuda.synchronize()
            rec = np.zeros(1, pkg.PNP_RESULT)
            rec[0] = tuple(g.stats[k] for k in pkg.PNP_RESULT.names)
            assert g.pose.tobytes() == poses.cpu().numpy()[0].tobytes(), n
            assert g.inlier_mask.astype(np.uint8).tobytes() == inl.cpu().numpy().tobytes() and g.reproj_errors.tobytes() == err.cpu().numpy().tobytes(), n
            assert rec.tobytes() == res.cpu().numpy().tobytes(), n
        assert host[1].stats["n_inliers"] > BIG // 2
        a, b = host[0], host[2]
        assert (a.pose.tobytes(), a.inlier_mask.tobytes(), a.reproj_errors.tobytes(), a.stats) == \
               (b.pose.tobytes(), b.inlier_mask.tobytes(), b.reproj_errors.tobytes(), b.stats)
    finally:
        h.close()


def test_sim3_host_staging_grows(pkg, cam):
    small = Z.sim3_points(41, 20, 0.0)[:2]
    big = Z.sim3_points(42, BIG, 0.3)[:2]
    h = _fresh(pkg, cam)
    try:
        host = [h.compute_sim3_ransac_batch([p]) for p in (small, big, small)]
        for (p1, p2), (sim3, inl, rec) in zip((small, big, small), host):
            n = len(p1)
            ds, di, dr = h.compute_sim3_ransac_batch_device(_d(np.array([0, n], np.int32)), _d(p1), _d(p2), n)
            h.synchronize()
            assert sim3.tobytes() == ds.cpu().numpy().tobytes() and inl[0].tobytes() == di.cpu().numpy().tobytes(), n
            assert rec.tobytes() == dr.cpu().numpy().tobytes(), n
            assert int(rec[0]["status"]) == 0, n
        assert int(host[1][2][0]["n_inliers"]) > BIG // 2
        assert [x.tobytes() for x in (host[0][0], host[0][1][0], host[0][2])] == [x.tobytes() for x in (host[2][0], host[2][1][0], host[2][2])]
    finally:
        h.close()


# ---- partial download ---------------------------------------------------------------------------------------------------
def test_pose_inertial_without_inlier_output(gpu_handle, pkg, tmp_path):
    """Handle.pose_inertial_optimization always asks for the inlier flags; the C++ mirror (include/orbx.hpp) passes NULL for them, so
    its driver is the call with the output omitted.  Poses, velocities, biases and records are the same bytes either way."""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA)                       # the driver's camera
    n = 200                                                               # (the generator's smaller scenes end TOO_FEW with every flag 0)
    s = pkg.synth.pose_inertial_problem(52, n, 0.2, 0.5, 2.0, 0.05, near_identity=True)
    exe = build_pose_inertial_driver(str(tmp_path))
    fin, fout = os.path.join(tmp_path, "in.bin"), os.path.join(tmp_path, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", n))
        for k in ("pose_wc", "velocity", "bias", "prev_kf_pose_wc", "prev_kf_velocity", "preint"):
            f.write(np.ascontiguousarray(s[k], np.float64).tobytes())
        f.write(np.ascontiguousarray(s["points3d"]).tobytes()); f.write(np.ascontiguousarray(s["points2d"]).tobytes())
        f.write(np.ascontiguousarray(s["is_stereo"], np.uint8).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    without = open(fout, "rb").read()
    g = gpu_handle.pose_inertial_optimization(cam, s["pose_wc"], s["velocity"], s["bias"], s["prev_kf_pose_wc"], s["prev_kf_velocity"], s["preint"],
                                              s["points3d"], s["points2d"], s["is_stereo"])
    assert g.status == pkg.POSE_INERTIAL_OK and 5 <= g.num_inliers == int(g.inlier_mask.sum()) < n      # the flags came back, some of them 0
    assert without == g.pose.tobytes() + g.velocity.tobytes() + g.bias.tobytes() + struct.pack("<3Q", g.num_inliers, g.num_observations, g.iterations)
