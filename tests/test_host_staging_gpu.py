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

Partial download: orbx_pose_inertial_batch copies the inlier flags back only when asked for them.

The single-problem host forms (the matchers, the triangulation and fuse searches, the pair loop, the BoW calls and the orbx_keyframe_*
searches) share one blob, one pinned buffer and one ring (IoWorkspaces, pin_io, ring_io): the last part of this file holds them to
their device forms through growth, to the ranges they may write, through empty sides, through ring reuse and through the nesting of a
host form around a device form that owns a workspace of its own."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import loop_verify_scenes as Z
import track_reference_scenes as R
import tracking_scenes as G
import triangulation_scenes as TS
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


# ---- the single-problem host forms ----------------------------------------------------------------------------------------
# Every form below is called as api.py calls it, with output arrays the test owns: filled with SENT before the call, so that what the
# call did not write still says so.  A form's answer is a list of (name, the bytes the call is to write); `spare` is what lies behind
# them in the same arrays.
SENT = 0xA5
BOWV_MAX = 8192                                                            # orbx_bow_vectors' limit (api.BOW_VECTORS_MAX)
FUSE_SCALE = 3.0 * (1.2 * (1.2 * 1.2) * ((1.2 * 1.2) * (1.2 * 1.2)))


def _vp(x):
    from orb_slam3_rust_amd.api import _vp as vp
    return vp(x)


def _sent(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = SENT
    return a


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENT).all())


def _kpt(kp):
    import torch
    return torch.from_numpy(np.ascontiguousarray(kp).view(np.float32).reshape(-1, 7).copy()).cuda()


def _dz(n, *tail, dtype=None):
    """an output tensor of the device forms, at least one row"""
    import torch
    return torch.zeros((max(int(n), 1),) + tail, dtype=dtype or torch.int32, device="cuda")


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def _keyframe(pkg, h, kp, desc, pts=None, has=None, pose=(1.0, 0, 0, 0, 0, 0, 0)):
    """a resident keyframe of host arrays; the tensors it is copied from stay alive until the handle's next synchronise"""
    n = len(kp)
    if n == 0:
        return pkg.KeyFrame(h, None, None, 0, None, None, pose_wc=pose)
    t = [_kpt(kp), _d(desc)] + ([_d(pts), _d(has)] if pts is not None else [None, None])
    h._after_torch(*[x for x in t if x is not None])
    return pkg.KeyFrame(h, t[0], t[1], n, t[2], t[3], pose_wc=pose)


class _handle_of:
    """a fresh handle for the block; its vocabulary, if one was made, goes first"""
    def __init__(self, pkg, cam):
        self.h = _fresh(pkg, cam)

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        v = _vocs.pop(id(self.h), None)
        if v:
            v[1].close()
        self.h.close()


class _Out:
    """what a call wrote (parts: name -> array cut to the range the call owns) and what it had to leave alone (spare)"""
    def __init__(self, parts, spare=()):
        self.parts, self.spare = parts, list(spare)

    def bytes(self):
        return [(k, np.ascontiguousarray(v).tobytes()) for k, v in self.parts.items()]


# -- stereo_match: d = (kpL, descL, kpR, descR)
def _stereo_host(pkg, h, cam, d):
    kpL, dL, kpR, dR = d
    nL, nR = len(kpL), len(kpR)
    m = _sent(max(nL, 1), pkg.DMATCH); pts = _sent((max(nL, 1), 3), np.float64); has = _sent(max(nL, 1), np.uint8); nm = C.c_int(-7)
    h._check(h._L.orbx_stereo_match(h._h, _vp(kpL), _vp(dL), C.c_int(nL), _vp(kpR), _vp(dR), C.c_int(nR), _vp(m), C.byref(nm), _vp(pts), _vp(has)))
    n = nm.value
    assert 0 <= n <= nL
    if nL == 0:
        return _Out(dict(n=np.int32(n)), [m, pts, has])
    return _Out(dict(n=np.int32(n), matches=m[:n], points=pts[:nL], has=has[:nL]), [m[n:], pts[nL:], has[nL:]])


def _stereo_device(pkg, h, cam, d):
    import torch
    kpL, dL, kpR, dR = d
    nL, nR = len(kpL), len(kpR)
    cap = max(nL, nR, 1)
    o = h.alloc_batch_outputs(1, cap)
    if nL:
        o["kp"][0, 0, :nL] = _kpt(kpL); o["desc"][0, 0, :nL] = _d(dL)
    if nR:
        o["kp"][0, 1, :nR] = _kpt(kpR); o["desc"][0, 1, :nR] = _d(dR)
    o["nkp"][0, 0] = nL; o["nkp"][0, 1] = nR
    torch.cuda.synchronize()
    h.stereo_match_batch_device(o, 1)
    h.synchronize()
    n = int(o["nmatches"][0].item())
    return _Out(dict(n=np.int32(n), matches=_np(o["matches"][0, :n]), points=_np(o["points"][0, :nL]), has=_np(o["has_point"][0, :nL])))


# -- hamming_match_crosscheck: d = (q, t)
def _cross_host(pkg, h, cam, d):
    q, t = d
    out = _sent(max(len(q), 1), pkg.DMATCH); n = C.c_int(-7)
    h._check(h._L.orbx_hamming_match_crosscheck(h._h, _vp(q), C.c_int(len(q)), _vp(t), C.c_int(len(t)), _vp(out), C.byref(n)))
    assert 0 <= n.value <= len(q)
    return _Out(dict(n=np.int32(n.value), matches=out[:n.value]), [out[n.value:]])


def _cross_device(pkg, h, cam, d):
    q, t = d
    tq, tt = _d(q), _d(t)
    out = _dz(len(q), 4); n = _dz(1)
    h._after_torch(tq, tt, out, n)
    h._check(h._L.orbx_hamming_match_crosscheck_device(h._h, _vp(tq), C.c_int(len(q)), _vp(tt), C.c_int(len(t)), _vp(out), _vp(n)))
    h.synchronize()
    k = int(n.item())
    return _Out(dict(n=np.int32(k), matches=_np(out[:k])))


# -- hamming_batch: d = (a, b)
def _hb_host(pkg, h, cam, d):
    out = _sent(max(len(d[0]), 1), np.uint32)
    h._check(h._L.orbx_hamming_batch(h._h, _vp(d[0]), _vp(d[1]), C.c_int(len(d[0])), _vp(out)))
    return _Out(dict(dist=out[:len(d[0])]), [out[len(d[0]):]])


def _hb_device(pkg, h, cam, d):
    a, b = _d(d[0]), _d(d[1])
    out = _dz(len(d[0]))
    h._after_torch(a, b, out)
    h._check(h._L.orbx_hamming_batch_device(h._h, _vp(a), _vp(b), C.c_int(len(d[0])), _vp(out)))
    h.synchronize()
    return _Out(dict(dist=_np(out[:len(d[0])])))


# -- guided_match and its keyframe form: d = (kp, desc, q_uv, q_desc)
def _gm_args(mode=1, radius=40.0):
    return C.c_double(752.0), C.c_double(480.0), C.c_double(radius), C.c_int(mode)


def _gm_host(pkg, h, cam, d, keyframe=False):
    kp, desc, uv, qd = d
    nq = len(uv)
    idx = _sent(max(nq, 1), np.int32); dist = _sent(max(nq, 1), np.uint32)
    w, hh, r, mode = _gm_args()
    if keyframe:
        kf = _keyframe(pkg, h, kp, desc)
        h._check(h._L.orbx_keyframe_guided_match(h._h, kf._p, w, hh, _vp(uv), _vp(qd), C.c_int(nq), r, mode, _vp(idx), _vp(dist)))
        kf.close()
    else:
        h._check(h._L.orbx_guided_match(h._h, _vp(kp), _vp(desc), C.c_int(len(kp)), w, hh, _vp(uv), _vp(qd), C.c_int(nq), r, mode, _vp(idx), _vp(dist)))
    return _Out(dict(idx=idx[:nq], dist=dist[:nq]), [idx[nq:], dist[nq:]])


def _gm_device(pkg, h, cam, d):
    kp, desc, uv, qd = d
    nq = len(uv)
    t = [_kpt(kp), _d(desc), _d(uv), _d(qd)]
    idx = _dz(nq); dist = _dz(nq)
    w, hh, r, mode = _gm_args()
    h._after_torch(*t, idx, dist)
    h._check(h._L.orbx_guided_match_device(h._h, _vp(t[0]), _vp(t[1]), C.c_int(len(kp)), w, hh, _vp(t[2]), _vp(t[3]), C.c_int(nq), r, mode, _vp(idx),
                                           _vp(dist)))
    h.synchronize()
    return _Out(dict(idx=_np(idx[:nq]), dist=_np(dist[:nq], np.uint32)))


# -- the triangulation searches: d = two_view_features' dict (node1 / node2: the FeatureVector form)
def _sft_keyframes(pkg, h, s):
    kfs = []
    for k in "12":
        n = len(s["kp" + k])
        kf = _keyframe(pkg, h, s["kp" + k], s["desc" + k], np.zeros((n, 3)), s["stereo1"] if k == "1" else np.zeros(n, np.uint8), s["pose" + k + "_wc"])
        kf.set_map_points([7 if m else None for m in s["mp" + k]])
        kfs.append(kf)
    return kfs


def _sft_host(pkg, h, cam, s, form="plain"):
    n1, n2 = len(s["kp1"]), len(s["kp2"])
    pairs = _sent((max(n1, 1), 2), np.int32); n = C.c_int(-7)
    c = cam._c()
    p1 = np.ascontiguousarray(s["pose1_wc"], np.float64); p2 = np.ascontiguousarray(s["pose2_wc"], np.float64)
    if form == "keyframe":
        kfs = _sft_keyframes(pkg, h, s)
        h._check(h._L.orbx_keyframe_search_for_triangulation(h._h, C.byref(c), kfs[0]._p, kfs[1]._p, C.c_uint(50), _vp(pairs), C.byref(n)))
        for k in kfs:
            k.close()
    elif form == "bow":
        h._check(h._L.orbx_search_for_triangulation_bow(h._h, C.byref(c), _vp(s["kp1"]), _vp(s["desc1"]), _vp(s["mp1"]), _vp(s["stereo1"]), _vp(s["node1"]),
                                                        C.c_int(n1), _vp(s["kp2"]), _vp(s["desc2"]), _vp(s["mp2"]), _vp(s["node2"]), C.c_int(n2), _vp(p1),
                                                        _vp(p2), C.c_uint(50), _vp(pairs), C.byref(n)))
    else:
        h._check(h._L.orbx_search_for_triangulation(h._h, C.byref(c), _vp(s["kp1"]), _vp(s["desc1"]), _vp(s["mp1"]), _vp(s["stereo1"]), C.c_int(n1),
                                                    _vp(s["kp2"]), _vp(s["desc2"]), _vp(s["mp2"]), C.c_int(n2), _vp(p1), _vp(p2), C.c_uint(50), _vp(pairs),
                                                    C.byref(n)))
    assert 0 <= n.value <= n1
    return _Out(dict(n=np.int32(n.value), pairs=pairs[:n.value]), [pairs[n.value:]])


def _sft_device(pkg, h, cam, s):
    pairs, cnt = h.search_for_triangulation_device(cam, _kpt(s["kp1"]), _d(s["desc1"]), _d(s["mp1"]), _d(s["stereo1"]), _kpt(s["kp2"]), _d(s["desc2"]),
                                                   _d(s["mp2"]), s["pose1_wc"], s["pose2_wc"])
    h.synchronize()
    n = int(cnt.item())
    return _Out(dict(n=np.int32(n), pairs=_np(pairs[:n])))


# -- the fuse searches: d = fuse_scene's dict
def _fuse_host(pkg, h, cam, f, keyframe=False):
    P_, T = len(f["positions"]), len(f["kf_poses_wc"])
    idx = _sent((max(P_, 1), max(T, 1)), np.int32); dist = _sent((max(P_, 1), max(T, 1)), np.uint32)
    c = cam._c()
    off = f["kf_feat_offset"]
    if keyframe:
        kfs = []
        for t in range(T):
            a, b = int(off[t]), int(off[t + 1])
            kfs.append(_keyframe(pkg, h, f["kps"][a:b], f["descs"][a:b], pose=f["kf_poses_wc"][t]))
        arr = (C.c_void_p * max(T, 1))(*[k._p for k in kfs])
        h._check(h._L.orbx_keyframe_fuse_search(h._h, C.byref(c), _vp(f["positions"]), _vp(f["mp_desc"]), C.c_int(P_), arr, C.c_int(T), C.c_double(FUSE_SCALE),
                                                C.c_uint(50), _vp(idx), _vp(dist)))
        for k in kfs:
            k.close()
    else:
        poses = np.ascontiguousarray(f["kf_poses_wc"], np.float64).reshape(-1, 7)
        h._check(h._L.orbx_fuse_search(h._h, C.byref(c), _vp(f["positions"]), _vp(f["mp_desc"]), C.c_int(P_), _vp(poses), _vp(off), _vp(f["kps"]),
                                       _vp(f["descs"]), C.c_int(T), C.c_double(FUSE_SCALE), C.c_uint(50), _vp(idx), _vp(dist)))
    if P_ == 0 or T == 0:
        return _Out({}, [idx, dist])
    return _Out(dict(idx=idx, dist=dist))


def _fuse_enqueue(h, cam, f, poses):
    """orbx_fuse_search_device with the host array `poses` handed over as it is; asynchronous"""
    return h.fuse_search_device(cam, _d(f["positions"]), _d(f["mp_desc"]), poses, _d(f["kf_feat_offset"]), _kpt(f["kps"]), _d(f["descs"]), FUSE_SCALE)


def _fuse_device(pkg, h, cam, f):
    idx, dist = _fuse_enqueue(h, cam, f, f["kf_poses_wc"])
    h.synchronize()
    return _Out(dict(idx=_np(idx), dist=_np(dist, np.uint32)))


def _fuse_cut(f, P_, T, n_feat=None):
    """the first P_ points and T keyframes of a fuse scene (n_feat: only that many features of each)"""
    off = f["kf_feat_offset"]
    rows = np.concatenate([np.arange(off[t], off[t + 1] if n_feat is None else min(off[t] + n_feat, off[t + 1])) for t in range(T)] + [np.zeros(0, np.int64)])
    new = np.zeros(T + 1, np.int32)
    new[1:] = np.cumsum([off[t + 1] - off[t] if n_feat is None else min(n_feat, off[t + 1] - off[t]) for t in range(T)])
    rows = rows.astype(np.int64)
    return dict(positions=np.ascontiguousarray(f["positions"][:P_]), mp_desc=np.ascontiguousarray(f["mp_desc"][:P_]),
                kf_poses_wc=np.ascontiguousarray(f["kf_poses_wc"][:T]).reshape(-1, 7), kf_feat_offset=new, kps=np.ascontiguousarray(f["kps"][rows]),
                descs=np.ascontiguousarray(f["descs"][rows]), camera=f["camera"])


# -- triangulate_pairs: d = (keyframe dict 1, keyframe dict 2, pairs [n,2])
def _tp_host(pkg, h, cam, d):
    k1, k2, pairs = d
    n = len(pairs)
    pts = _sent((max(n, 1), 3), np.float64); st = _sent(max(n, 1), np.uint16)
    c = cam._c(); cfg = pkg.TriangulationConfig()._c()
    h._check(h._L.orbx_triangulate_pairs(h._h, C.byref(c), C.byref(cfg), C.c_int(0), _vp(k1["kp"]), _vp(k1["pts"]), _vp(k1["has"]), C.c_int(len(k1["kp"])),
                                         _vp(np.ascontiguousarray(k1["pose"], np.float64)), _vp(k2["kp"]), _vp(k2["pts"]), _vp(k2["has"]),
                                         C.c_int(len(k2["kp"])), _vp(np.ascontiguousarray(k2["pose"], np.float64)), _vp(pairs), C.c_int(n), _vp(pts), _vp(st)))
    return _Out(dict(points=pts[:n], status=st[:n]), [pts[n:], st[n:]])


def _tp_device(pkg, h, cam, d):
    k1, k2, pairs = d
    pts, st = h.triangulate_pairs_device(cam, _kpt(k1["kp"]), _d(k1["pts"]), _d(k1["has"]), k1["pose"], _kpt(k2["kp"]), _d(k2["pts"]), _d(k2["has"]), k2["pose"],
                                         _d(pairs))
    h.synchronize()
    return _Out(dict(points=_np(pts), status=_np(st, np.uint16)))


# -- the BoW calls: d = (vocabulary arrays, descriptors)
_vocs = {}


def _voc(pkg, h, arrays):
    """one device vocabulary per handle (closed with it)"""
    if id(h) not in _vocs or _vocs[id(h)][0] is not h:
        _vocs[id(h)] = (h, pkg.OrbVocabulary.from_nodes(*arrays, k=10, l=3, handle=h))
    return _vocs[id(h)][1]


def _bt_host(pkg, h, cam, d):
    v = _voc(pkg, h, d[0]); n = len(d[1])
    word = _sent(max(n, 1), np.uint32); leaf = _sent(max(n, 1), np.uint32); node = _sent(max(n, 1), np.uint32); w = _sent(max(n, 1), np.float64)
    h._check(h._L.orbx_bow_transform(h._h, v._v, _vp(d[1]), C.c_int(n), C.c_int(1), _vp(word), _vp(leaf), _vp(node), _vp(w)))
    return _Out(dict(word=word[:n], leaf=leaf[:n], node=node[:n], weight=w[:n]), [word[n:], leaf[n:], node[n:], w[n:]])


def _bt_device(pkg, h, cam, d):
    import torch
    v = _voc(pkg, h, d[0]); n = len(d[1])
    dd = _d(d[1]); word = _dz(n); leaf = _dz(n); node = _dz(n); w = _dz(n, dtype=torch.float64)
    h._after_torch(dd, word, leaf, node, w)
    h._check(h._L.orbx_bow_transform_device(h._h, v._v, _vp(dd), C.c_int(n), C.c_int(1), _vp(word), _vp(leaf), _vp(node), _vp(w)))
    h.synchronize()
    return _Out(dict(word=_np(word[:n], np.uint32), leaf=_np(leaf[:n], np.uint32), node=_np(node[:n], np.uint32), weight=_np(w[:n])))


def _bv_host(pkg, h, cam, d):
    v = _voc(pkg, h, d[0]); n = len(d[1])
    bw = _sent(max(n, 1), np.uint32); bv = _sent(max(n, 1), np.float64); fn = _sent(max(n, 1), np.uint32); fs = _sent(n + 1, np.int32); fi = _sent(max(n, 1), np.int32)
    nb = C.c_int(-7); nf = C.c_int(-7)
    h._check(h._L.orbx_bow_vectors(h._h, v._v, _vp(d[1]), C.c_int(n), C.c_int(1), _vp(bw), _vp(bv), C.byref(nb), _vp(fn), _vp(fs), _vp(fi), C.byref(nf)))
    a, b = nb.value, nf.value
    assert 0 <= a <= n and 0 <= b <= n
    if n == 0:
        return _Out(dict(n_bow=np.int32(a), n_fv=np.int32(b)), [bw, bv, fn, fs, fi])
    return _Out(dict(n_bow=np.int32(a), n_fv=np.int32(b), bow_word=bw[:a], bow_weight=bv[:a], fv_node=fn[:b], fv_start=fs[:b + 1], fv_index=fi[:n]),
                [bw[a:], bv[a:], fn[b:], fs[b + 1:], fi[n:]])


def _bv_enqueue(pkg, h, d):
    return _voc(pkg, h, d[0]).vectors_device(_d(d[1]), len(d[1]), 1)


def _bv_finish(r, n):
    a, b = (int(x) for x in r["counts"].cpu().numpy())
    return _Out(dict(n_bow=np.int32(a), n_fv=np.int32(b), bow_word=_np(r["bow_word"][:a], np.uint32), bow_weight=_np(r["bow_weight"][:a]),
                     fv_node=_np(r["fv_node"][:b], np.uint32), fv_start=_np(r["fv_start"][:b + 1]), fv_index=_np(r["fv_index"][:n])))


def _bv_device(pkg, h, cam, d):
    r = _bv_enqueue(pkg, h, d)
    h.synchronize()
    return _bv_finish(r, len(d[1]))


# -- the neighbour loop: d = (scene of triangulation_scenes.make_scene, cap)
def _nb_keyframe(pkg, h, kf):
    k = _keyframe(pkg, h, kf["kp"], kf["desc"], kf["pts"], kf["has"], kf["pose"])
    if k.n == 0:
        return k
    k.set_map_points([7 if m else None for m in kf["mp"]])
    if kf.get("node") is not None:
        k.set_feature_nodes(kf["node"])
    return k


def _nb_host(pkg, h, cam, d):
    sc, cap = d
    cur = _nb_keyframe(pkg, h, sc["current"]); nbs = [_nb_keyframe(pkg, h, k) for k in sc["neighbours"]]
    T = len(nbs)
    arr = (C.c_void_p * max(T, 1))(*[k._p for k in nbs])
    nb = _sent(max(cap, 1), np.int32); i1 = _sent(max(cap, 1), np.int32); i2 = _sent(max(cap, 1), np.int32); pts = _sent((max(cap, 1), 3), np.float64)
    stats = _sent((max(T, 1), 4), np.int32); n = C.c_int(-7)
    c = cam._c(); cfg = pkg.TriangulationConfig()._c()
    h._check(h._L.orbx_keyframe_triangulate_from_neighbors(h._h, C.byref(c), C.byref(cfg), C.c_int(0), cur._p, arr, C.c_int(T), C.c_int(cap), _vp(nb), _vp(i1),
                                                           _vp(i2), _vp(pts), C.byref(n), _vp(stats)))
    for k in [cur] + nbs:
        k.close()
    m = min(n.value, cap)
    assert n.value >= 0
    return _Out(dict(n=np.int32(n.value), neighbour=nb[:m], idx1=i1[:m], idx2=i2[:m], points=pts[:m], stats=stats[:T]), [nb[m:], i1[m:], i2[m:], pts[m:], stats[T:]])


def _nb_cut(sc, n_feat, T):
    cut = lambda kf: {k: (v if k == "pose" or v is None else np.ascontiguousarray(v[:n_feat])) for k, v in kf.items()}
    return dict(camera=sc["camera"], current=cut(sc["current"]), neighbours=[cut(k) for k in sc["neighbours"][:T]])


@pytest.fixture(scope="module")
def io_data(pkg):
    """the large problem of every form, made once; the small ones are its first rows"""
    KP = pkg.KEYPOINT
    rng = np.random.default_rng(77)
    d = {}
    d["stereo"] = pkg.synth.matcher_features(61, 8200, 8000, KP)                                    # 161 B a feature: 1.3 MB
    q = rng.integers(0, 256, (16500, 32), dtype=np.uint8)
    t = q[rng.permutation(16500)[:16000]].copy(); t[:, 5] ^= rng.integers(0, 4, 16000, dtype=np.uint8)
    d["cross"] = (q, t)                                                                              # 80 B a query: 1.3 MB
    d["hamming"] = (rng.integers(0, 256, (20000, 32), dtype=np.uint8), rng.integers(0, 256, (20000, 32), dtype=np.uint8))   # 68 B a pair
    kpL, dL = d["stereo"][0], d["stereo"][1]
    sel = rng.integers(0, len(kpL), 20000)
    uv = np.stack([kpL["x"][sel], kpL["y"][sel]], 1).astype(np.float64) + rng.normal(0, 3, (20000, 2))
    qd = dL[sel].copy(); qd[:, 0] ^= rng.integers(0, 8, 20000, dtype=np.uint8)
    d["guided"] = (kpL, dL, np.ascontiguousarray(uv), qd)                                            # 56 B a query: 1.1 MB of queries alone
    voc = pkg.synth.vocabulary(21, k=10, depth=3)
    d["sft"] = _two_views(pkg, voc, 63, 9000)                                                        # ~131 B a feature pair: 1.2 MB
    d["sft_mid"] = _two_views(pkg, voc, 67, 1100)
    d["stereo_mid"] = pkg.synth.matcher_features(68, 900, 850, KP)
    # the keyframe form sends nothing up and 8 B a feature of keyframe 1 down: 140 k features (the small scene's, 70 times over)
    s2 = pkg.synth.two_view_features(64, 1900, KP)
    big = {k: (np.ascontiguousarray(np.concatenate([v] * 70)) if k.endswith("1") and not k.startswith("pose") else v) for k, v in s2.items()}
    d["sft_kf"] = big
    d["fuse"] = pkg.synth.fuse_scene(65, 8000, 10, 2000, KP)                                         # 56 B a point + 8 B a pair + 60 B a feature: 2.3 MB
    sc = TS.pair_scene()
    k1, k2 = sc["current"], sc["neighbours"][1]
    d["pairs"] = (k1, k2, np.ascontiguousarray(np.stack([rng.integers(0, len(k1["kp"]), 40000), rng.integers(0, len(k2["kp"]), 40000)], 1), np.int32))   # 34 B a pair
    d["voc"] = voc
    d["bow_desc"] = rng.integers(0, 256, (24000, 32), dtype=np.uint8)                                # orbx_bow_transform: 52 B a descriptor
    d["nb"] = TS.make_scene(66, n_points=7600, T=4, n_distract=400, nodes="all")                     # 36 B a slot, 4 x 8000 slots: 1.1 MB of lists
    return d


def _two_views(pkg, voc, seed, n):
    from oracle import oracle as O
    s = pkg.synth.two_view_features(seed, n, pkg.KEYPOINT, dup=0.3)
    ov = O.Vocabulary.from_arrays(*voc)
    s["node1"] = np.ascontiguousarray(ov.transform(s["desc1"], 1)[2], np.uint32); s["node2"] = np.ascontiguousarray(ov.transform(s["desc2"], 1)[2], np.uint32)
    return s


def _cut_view(s, n1, n2):
    return {k: (v if k.startswith("pose") or k == "camera" else np.ascontiguousarray(v[:n1] if k.endswith("1") else v[:n2])) for k, v in s.items()}


def _io_forms(d):
    """name -> (host form, device form or None, the problem at a size: a number of features, queries, pairs or points; 0 < size or None = all)"""
    rows = lambda arrs, n: tuple(np.ascontiguousarray(a[:n]) for a in arrs)
    mid = lambda n: n is not None and n >= 100                             # a problem of its own, not the first rows of the large one
    sft = lambda n: d["sft_mid"] if mid(n) else _cut_view(d["sft"], n, n)
    nb_mid = TS.fused_scene("t3_nodes")
    kf = lambda f: (lambda pkg, h, cam, x: f(pkg, h, cam, x, keyframe=True))
    return {
        "stereo_match": (_stereo_host, _stereo_device, lambda n: d["stereo_mid"] if mid(n) else rows(d["stereo"], n)),
        "hamming_match_crosscheck": (_cross_host, _cross_device, lambda n: rows(d["cross"], n)),
        "hamming_batch": (_hb_host, _hb_device, lambda n: rows(d["hamming"], n)),
        "guided_match": (_gm_host, _gm_device, lambda n: rows(d["guided"][:2], None if n is None else 40 * n) + rows(d["guided"][2:], n)),
        "search_for_triangulation": (_sft_host, _sft_device, sft),
        # (no device form: the reference is the same call alone on a fresh handle)
        "search_for_triangulation_bow": (lambda pkg, h, cam, s: _sft_host(pkg, h, cam, s, "bow"), None, sft),
        "fuse_search": (_fuse_host, _fuse_device, lambda n: d["fuse"] if n is None else _fuse_cut(d["fuse"], n, 2, n)),
        "triangulate_pairs": (_tp_host, _tp_device, lambda n: d["pairs"][:2] + (np.ascontiguousarray(d["pairs"][2][:n]),)),
        "bow_transform": (_bt_host, _bt_device, lambda n: (d["voc"], np.ascontiguousarray(d["bow_desc"][:n]))),
        # (orbx_bow_vectors takes at most 8192 descriptors, 56 B each: its blob stays inside the first 1 MiB step)
        "bow_vectors": (_bv_host, _bv_device, lambda n: (d["voc"], np.ascontiguousarray(d["bow_desc"][:BOWV_MAX if n is None else n]))),
        "keyframe_guided_match": (kf(_gm_host), _gm_device, lambda n: rows(d["guided"][:2], None if n is None else 40 * n) + rows(d["guided"][2:], n)),
        "keyframe_search_for_triangulation": (lambda pkg, h, cam, s: _sft_host(pkg, h, cam, s, "keyframe"), _sft_device,
                                              lambda n: d["sft_kf"] if n is None else sft(n)),
        "keyframe_fuse_search": (kf(_fuse_host), _fuse_device, lambda n: d["fuse"] if n is None else _fuse_cut(d["fuse"], n, 2, n)),
        # (no device form either; every slot has room: cap = 4 neighbours x the current keyframe's features)
        "keyframe_triangulate_from_neighbors": (_nb_host, None, lambda n: (d["nb"], 4 * len(d["nb"]["current"]["kp"])) if n is None else
                                                (nb_mid, 3 * len(nb_mid["current"]["kp"])) if n >= 20 else (_nb_cut(d["nb"], 40 * n, 2), 80 * n)),
    }


IO_FORMS = ["stereo_match", "hamming_match_crosscheck", "hamming_batch", "guided_match", "search_for_triangulation", "search_for_triangulation_bow",
            "fuse_search", "triangulate_pairs", "bow_transform", "bow_vectors", "keyframe_guided_match", "keyframe_search_for_triangulation",
            "keyframe_fuse_search", "keyframe_triangulate_from_neighbors"]


def _io_cam(pkg, name, d):
    return pkg.CameraModel(**(TS.CAMERA if name in ("triangulate_pairs", "keyframe_triangulate_from_neighbors") else pkg.synth.EUROC_CAMERA))


def _alone(pkg, cam, fn, c, x):
    with _handle_of(pkg, cam) as h:
        return fn(pkg, h, c, x)


@pytest.mark.parametrize("name", IO_FORMS)
def test_io_host_staging_grows(pkg, cam, io_data, name):
    """small, large, small on one fresh handle: the blob passes the first 1 MiB step of the pinned buffer and of the workspace in the
    large call (orbx_bow_vectors: as far as its 8192-descriptor limit goes).  Each result equals the device form's on the same data
    (the FeatureVector search and the neighbour loop have none: the same call alone on a fresh handle), and nothing is written behind it."""
    host, device, at = _io_forms(io_data)[name]
    c = _io_cam(pkg, name, io_data)
    with _handle_of(pkg, cam) as h:
        got = [(n, host(pkg, h, c, at(n))) for n in (3, None, 5)]
        for n, g in got:
            want = device(pkg, h, c, at(n)) if device else _alone(pkg, cam, host, c, at(n))
            assert g.bytes() == want.bytes(), (name, n)
            assert all(_untouched(a) for a in g.spare), (name, n)
        big = got[1][1].parts
        found = {k: int(v) for k, v in big.items() if k in ("n", "n_bow", "n_fv")}
        assert all(v > 50 for v in found.values()), found                      # the large call found something
        if "idx" in big:
            assert int((big["idx"] >= 0).sum()) > 50


WRITTEN = [("stereo_match", 900), ("hamming_match_crosscheck", 700), ("search_for_triangulation", 1100), ("search_for_triangulation_bow", 1100),
           ("keyframe_search_for_triangulation", 1100), ("bow_vectors", 1500), ("keyframe_triangulate_from_neighbors", 20)]


@pytest.mark.parametrize("name,n", WRITTEN)
def test_io_written_ranges(pkg, cam, io_data, name, n):
    """matches, pairs, the BoW vectors and the neighbour loop's lists: the rows before the returned count are the device form's, the
    rows behind it still hold what the caller put there.  The neighbour loop once more with room for fewer rows than it makes."""
    host, device, at = _io_forms(io_data)[name]
    c = _io_cam(pkg, name, io_data)
    with _handle_of(pkg, cam) as h:
        g = host(pkg, h, c, at(n))
        want = device(pkg, h, c, at(n)) if device else _alone(pkg, cam, host, c, at(n))
        counts = {k: int(v) for k, v in g.parts.items() if k in ("n", "n_bow", "n_fv")}
        assert all(v > 10 for v in counts.values()), counts
        assert g.bytes() == want.bytes()
        assert sum(a.size for a in g.spare) > 0 and all(_untouched(a) for a in g.spare)   # there were rows behind the count, and they are as they were
        if name == "keyframe_triangulate_from_neighbors":
            sc, cap = at(n)
            few = host(pkg, h, c, (sc, counts["n"] // 2))
            assert int(few.parts["n"]) == counts["n"] and len(few.parts["idx1"]) == counts["n"] // 2
            for k in ("neighbour", "idx1", "idx2", "points"):
                assert few.parts[k].tobytes() == g.parts[k][:counts["n"] // 2].tobytes(), k
            assert all(_untouched(a) for a in few.spare)


def test_io_empty_sides(pkg, cam, io_data):
    """nL, nR, nq, nt, n1, n2, P, T, n_pairs = 0 and a neighbour loop that searches no neighbour: ORBX_OK, a zero count, no output row
    written (nR = 0 alone still owes the left features their "no point" rows), and the next call on the handle is right."""
    forms = _io_forms(io_data)
    e = lambda a: np.ascontiguousarray(a[:0])
    with _handle_of(pkg, cam) as h:
        def run(name, x, zero=("n",), written=()):
            host, device, at = forms[name]
            c = _io_cam(pkg, name, io_data)
            g = host(pkg, h, c, x)
            for k in zero:
                assert int(g.parts[k]) == 0, (name, k)
            assert set(g.parts) <= set(zero) | set(written), (name, list(g.parts))
            assert all(_untouched(a) for a in g.spare), name
            after = host(pkg, h, c, at(300 if name != "keyframe_triangulate_from_neighbors" else 20))
            want = device(pkg, h, c, at(300)) if device else _alone(pkg, cam, host, c, at(20 if name == "keyframe_triangulate_from_neighbors" else 300))
            assert after.bytes() == want.bytes(), name
            return g

        kpL, dL, kpR, dR = forms["stereo_match"][2](300)
        run("stereo_match", (e(kpL), e(dL), kpR, dR))                                             # nL = 0
        g = run("stereo_match", (kpL, dL, e(kpR), e(dR)), written=("matches", "points", "has"))   # nR = 0
        assert len(g.parts["matches"]) == 0 and not g.parts["has"].any()
        q, t = forms["hamming_match_crosscheck"][2](300)
        run("hamming_match_crosscheck", (e(q), t), written=("matches",))                          # nq = 0
        run("hamming_match_crosscheck", (q, e(t)), written=("matches",))                          # nt = 0
        a, b = forms["hamming_batch"][2](300)
        run("hamming_batch", (e(a), e(b)), zero=(), written=("dist",))                            # n_pairs = 0
        for name in ("guided_match", "keyframe_guided_match"):
            kp, desc, uv, qd = forms[name][2](300)
            run(name, (kp, desc, e(uv), e(qd)), zero=(), written=("idx", "dist"))                 # nq = 0
        for name in ("search_for_triangulation", "search_for_triangulation_bow", "keyframe_search_for_triangulation"):
            s = forms[name][2](300)
            run(name, _cut_view(s, 0, 300), written=("pairs",))                                   # n1 = 0
            run(name, _cut_view(s, 300, 0), written=("pairs",))                                   # n2 = 0
        for name in ("fuse_search", "keyframe_fuse_search"):
            f = forms[name][2](300)
            run(name, _fuse_cut(f, 0, 2), zero=())                                                # P = 0
            run(name, _fuse_cut(f, 300, 0), zero=())                                              # T = 0
        k1, k2, pairs = forms["triangulate_pairs"][2](300)
        run("triangulate_pairs", (k1, k2, e(pairs)), zero=(), written=("points", "status"))       # n_pairs = 0
        voc, desc = forms["bow_transform"][2](300)
        run("bow_vectors", (voc, e(desc)), zero=("n_bow", "n_fv"))                                # n = 0
        # every neighbour where the current keyframe is: none is a baseline away, none is searched
        sc, cap = forms["keyframe_triangulate_from_neighbors"][2](20)
        near = dict(sc, neighbours=[dict(k, pose=sc["current"]["pose"]) for k in sc["neighbours"]])
        g = run("keyframe_triangulate_from_neighbors", (near, cap), written=("neighbour", "idx1", "idx2", "points", "stats"))
        assert len(g.parts["idx1"]) == 0 and not g.parts["stats"].any()
        g = run("keyframe_triangulate_from_neighbors", (dict(sc, neighbours=[]), cap), written=("neighbour", "idx1", "idx2", "points", "stats"))   # T = 0
        assert len(g.parts["idx1"]) == 0


def test_ring_fuse_search_device(pkg, cam, io_data):
    """T = 2, 3, 1 back to back, kf_poses_wc overwritten by identity poses as soon as each call has returned, one synchronise at the end."""
    f = io_data["fuse"]
    c = pkg.CameraModel(**f["camera"])

    def enqueue(h, T):
        x = _fuse_cut(f, 400, T)
        poses = x["kf_poses_wc"].copy()
        assert poses.dtype == np.float64 and poses.flags["C_CONTIGUOUS"]
        return _fuse_enqueue(h, c, x, poses), [poses]

    def spoil(p):
        assert p.flags["WRITEABLE"]
        p[...] = np.array([1.0, 0, 0, 0, 0, 0, 0])

    finish = lambda o: [_np(o[0]).tobytes(), _np(o[1]).tobytes(), int((_np(o[0]) >= 0).sum())]
    together, alone = _back_to_back(pkg, cam, [2, 3, 1], enqueue, spoil, finish)
    for k, (got, want) in enumerate(zip(together, alone)):
        assert want[2] > 100, k
        assert got == want, k


def test_io_nesting(pkg, cam, io_data):
    """orbx_keyframe_fuse_search and orbx_bow_vectors hold the host forms' blob while orbx_fuse_search_device and orbx_bow_vectors_device
    run inside them on workspaces of their own; here the four alternate on one handle, the device forms asynchronous, and each
    workspace grows in the middle: the blob and the gathered features past 1 MiB in the large keyframe call, the pose table in a
    device call with 20000 keyframes (orbx_bow_vectors_device's scratch cannot: 8192 descriptors are 160 kB).  Every output equals
    the same call alone on a fresh handle."""
    f = io_data["fuse"]
    c = pkg.CameraModel(**f["camera"])
    voc, desc = io_data["voc"], io_data["bow_desc"]
    many = _fuse_cut(f, 40, 1, 30)                                                                 # 20000 keyframes of one feature each
    T = 20000
    many = dict(many, kf_poses_wc=np.ascontiguousarray(np.repeat(many["kf_poses_wc"], T, 0)), kf_feat_offset=np.arange(T + 1, dtype=np.int32),
                kps=np.ascontiguousarray(np.resize(many["kps"], T)), descs=np.ascontiguousarray(np.resize(many["descs"], (T, 32))))
    kfs = lambda x: (lambda h: _fuse_host(pkg, h, c, x, keyframe=True))
    fsd = lambda x: (lambda h: _fuse_enqueue(h, c, x, x["kf_poses_wc"]))
    bv = lambda n: (lambda h: _bv_host(pkg, h, c, (voc, np.ascontiguousarray(desc[:n]))))
    bvd = lambda n: (lambda h: (_bv_enqueue(pkg, h, (voc, np.ascontiguousarray(desc[:n]))), n))
    calls = [kfs(_fuse_cut(f, 30, 2, 50)), fsd(_fuse_cut(f, 30, 3, 50)), bv(40), bvd(60), fsd(many), kfs(f), bvd(BOWV_MAX), bv(BOWV_MAX), fsd(_fuse_cut(f, 50, 2, 40)),
             kfs(_fuse_cut(f, 50, 3, 40)), bvd(30), bv(50)]

    def finish(o):
        if isinstance(o, _Out):
            return o.bytes()
        if isinstance(o[0], dict):
            return _bv_finish(o[0], o[1]).bytes()
        return [_np(o[0]).tobytes(), _np(o[1]).tobytes()]

    with _handle_of(pkg, cam) as h:
        outs = [call(h) for call in calls]
        h.synchronize()
        together = [finish(o) for o in outs]
    for k, call in enumerate(calls):
        with _handle_of(pkg, cam) as h:
            o = call(h)
            h.synchronize()
            assert together[k] == finish(o), k
