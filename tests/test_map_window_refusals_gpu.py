"""What the six BA-window entry points of the resident map refuse, pinned: orbx_map_collect_ba_window[_device], orbx_map_local_ba,
orbx_map_collect_inertial_window[_device], orbx_map_local_inertial_ba.  Every bad call of bad_calls() goes through the ctypes
library object (the Python mirror would refuse some of them first); its return code and its orbx_last_error text are compared
with tests/golden/map_window_refusals.json, which was recorded by running the same list on the commit before the two window
paths became one.  Calls that break two rules at once pin the precedence.  A refusal touches nothing: n_live, the slot tables
and the outputs of a following good call are what they were before.

record(path) writes the fixture (run it on a GPU from a script of your own; the test never writes)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_window_refusals.json")
CAPACITY, N_FEAT, MAX_COV = 16, 8, 2
LIST_BOUND, OBS_BOUND = 16, 24           # min(8 + 2 * 8, capacity) = min(3 * 8, capacity); the features of the three keyframes
INERTIAL_MAX_K = 51                      # BA_INERTIAL_MAX_K (orbx_internal.hpp)

# parameter names of the entry points, in the order of include/orbx.h
COLLECT_TAIL = ["list_cap", "obs_cap", "counts", "local_kf", "fixed_kf", "list_slot", "positions", "obs32"]
PARAMS = {
    "orbx_map_collect_ba_window_device": ["h", "mp", "n_kfs", "kfs", "cur", "max_covisible"] + COLLECT_TAIL,
    "orbx_map_collect_ba_window": ["h", "mp", "n_kfs", "kfs", "cur", "max_covisible"] + COLLECT_TAIL,
    "orbx_map_local_ba": ["h", "cam", "cfg", "mp", "n_kfs", "kfs", "cur", "should_stop", "user", "local_kf", "poses_out", "counts", "it", "e0", "e1"],
    "orbx_map_collect_inertial_window_device": ["h", "mp", "n_kfs", "kfs", "n_chain", "chain"] + [p for p in COLLECT_TAIL if p != "local_kf"],
    "orbx_map_collect_inertial_window": ["h", "mp", "n_kfs", "kfs", "n_chain", "chain"] + [p for p in COLLECT_TAIL if p != "local_kf"],
    "orbx_map_local_inertial_ba": ["h", "cam", "icfg", "mp", "n_kfs", "kfs", "n_chain", "chain", "vel", "bias", "E", "edge_kf", "preint", "should_stop", "user",
                                   "poses_out", "vel_out", "bias_out", "fixed_kf", "counts", "it", "e0", "e1"],
}
COLLECTS = [e for e in PARAMS if "collect" in e]
DEVICE = [e for e in PARAMS if e.endswith("_device")]
VISUAL = [e for e in PARAMS if "inertial" not in e]
INERTIAL = [e for e in PARAMS if "inertial" in e]
REQUIRED_OUT = {
    "orbx_map_collect_ba_window_device": ["counts", "local_kf", "fixed_kf", "list_slot", "positions", "obs32"],
    "orbx_map_collect_ba_window": ["counts", "local_kf", "fixed_kf", "list_slot", "positions", "obs32"],
    "orbx_map_local_ba": ["local_kf", "poses_out", "counts", "it", "e0", "e1"],
    "orbx_map_collect_inertial_window_device": ["counts", "fixed_kf", "list_slot", "positions", "obs32"],
    "orbx_map_collect_inertial_window": ["counts", "fixed_kf", "list_slot", "positions", "obs32"],
    "orbx_map_local_inertial_ba": ["poses_out", "vel_out", "bias_out", "fixed_kf", "counts", "it", "e0", "e1"],
}


def _project(cam, pose_wc, X):
    """pixel coordinates of world points X [n,3] in the camera at pose_wc (qw, qx, qy, qz, t)"""
    w, x, y, z = pose_wc[:4]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    Xc = (X - pose_wc[4:]) @ R                                               # R^T (X - t), row by row
    return np.stack([cam["fx"] * Xc[:, 0] / Xc[:, 2] + cam["cx"], cam["fy"] * Xc[:, 1] / Xc[:, 2] + cam["cy"]], 1)


class Scene:
    """One store of capacity 16 (slots 0..13 live), three keyframes of 8 features each with slot tables on a short inertial
    trajectory, one keyframe of a second store; and the six entry points' good arguments as ctypes values."""

    def __init__(self, pkg, h):
        import torch
        self.pkg, self.h, self.L, self.torch = pkg, h, pkg.load_library(), torch
        cam = dict(pkg.synth.EUROC_CAMERA)
        w = pkg.synth.inertial_window(5, 3, CAPACITY, pkg.BA_OBS, n_fixed=1, noise_px=0.0)
        rng = np.random.default_rng(77)
        self.live = np.arange(14, dtype=np.int32)
        self.positions = np.ascontiguousarray(w["points"][:14], np.float64)
        self.desc = rng.integers(0, 256, (14, 32), dtype=np.uint8)
        self.mp = pkg.MapPointStore(h, CAPACITY)
        self.mp2 = pkg.MapPointStore(h, CAPACITY)
        self.mp2.set(self.live[:4], self.positions[:4], self.desc[:4])
        self.reset()
        self.tables, self.kfs = [], []
        for k in range(3):                                                   # features: slots k, k+2, .. (one not live, one -1), keypoints their projections
            t = np.array([(k + 2 * i) % CAPACITY for i in range(N_FEAT - 1)] + [-1], np.int32)
            uv = _project(cam, w["gt_poses_wc"][k], w["gt_points"][np.maximum(t, 0)]) + rng.normal(0.0, 0.5, (N_FEAT, 2))
            self.tables.append(t)
            self.kfs.append(self._keyframe(uv, w["poses_wc"][k]))
            self.kfs[-1].set_map_point_slots(self.mp, t)
        self.other = self._keyframe(uv, w["poses_wc"][0])
        self.other.set_map_point_slots(self.mp2, np.array([0, 1, 2, 3, -1, -1, -1, -1], np.int32))
        self.all_kfs = self.kfs + [self.other]
        self.w = w
        self.keep = []                                                       # every array a call was handed stays alive

    def _keyframe(self, uv, pose):
        kp = np.zeros(N_FEAT, self.pkg.KEYPOINT)
        kp["x"] = uv[:, 0]; kp["y"] = uv[:, 1]; kp["size"] = 31.0
        d_kp = self.torch.from_numpy(kp.view(np.uint8).reshape(-1, kp.dtype.itemsize)).cuda()
        return self.pkg.KeyFrame(self.h, d_kp, self.torch.zeros((N_FEAT, 32), dtype=self.torch.uint8, device="cuda"), N_FEAT, pose_wc=pose)

    def reset(self):
        """the store as it was made (the local-BA calls write optimised positions back)"""
        self.mp.set(self.live, self.positions, self.desc)

    def close(self):
        for k in self.all_kfs:
            k.close()
        self.mp.close(); self.mp2.close()

    def kf_array(self, kfs):
        a = (C.c_void_p * max(len(kfs), 1))(*[k._p for k in kfs])
        self.keep.append(a)
        return a

    def good(self, entry):
        """the entry point's good arguments by name; the outputs by name too (zero-filled: rows past the counts compare equal)"""
        torch, pkg = self.torch, self.pkg
        dev = entry.endswith("_device")
        def out(shape, dt):
            return torch.zeros(shape, dtype=getattr(torch, dt), device="cuda") if dev else np.zeros(shape, dt)
        o = dict(counts=out(4, "int32"), local_kf=out(1 + MAX_COV, "int32"), fixed_kf=out(3, "int32"), list_slot=out(LIST_BOUND, "int32"),
                 positions=out((LIST_BOUND, 3), "float64"), obs32=out((OBS_BOUND, 16), "uint8"), poses_out=np.zeros((3, 7)), vel_out=np.zeros((3, 3)),
                 bias_out=np.zeros((3, 6)), it=C.c_int(), e0=C.c_double(), e1=C.c_double())
        cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA)._c()
        cfg = pkg.LocalBAConfigLM(max_covisible_keyframes=MAX_COV)._c()
        icfg = pkg.LocalInertialBAConfig()._c()
        chain = np.array([0, 1, 2], np.int32)
        w = self.w
        ins = dict(vel=np.ascontiguousarray(w["velocities"]), bias=np.ascontiguousarray(w["biases"]), edge_kf=np.ascontiguousarray(w["edge_kf"], np.int32),
                   preint=np.ascontiguousarray(w["preint"]), chain=chain)
        self.keep += [o, ins, cam, cfg, icfg]
        a = dict(h=self.h._h, mp=self.mp._p, n_kfs=C.c_int(3), kfs=self.kf_array(self.kfs), cur=C.c_int(0), max_covisible=C.c_int(MAX_COV),
                 list_cap=C.c_int(LIST_BOUND), obs_cap=C.c_int(OBS_BOUND), cam=C.byref(cam), cfg=C.byref(cfg), icfg=C.byref(icfg), n_chain=C.c_int(3),
                 E=C.c_int(len(ins["edge_kf"])), should_stop=C.cast(None, pkg.api.SHOULD_STOP_FN), user=None)
        for k, v in list(o.items()) + list(ins.items()):
            a[k] = C.byref(v) if k in ("it", "e0", "e1") else pkg.api._vp(v)
        return a, o

    def call(self, entry, **override):
        a, o = self.good(entry)
        for k, v in override.items():
            if k.startswith("_"):
                continue
            assert k in PARAMS[entry], (entry, k)
            if isinstance(v, np.ndarray):
                self.keep.append(v)
                v = self.pkg.api._vp(v)
            a[k] = v
        self.h._after_torch()
        rc = getattr(self.L, entry)(*[a[p] for p in PARAMS[entry]])
        return rc, o

    def good_round(self):
        """the six good calls on the store as it was made -> everything they answer, as bytes"""
        got = {}
        for entry in PARAMS:
            self.reset()
            rc, o = self.call(entry)
            self.torch.cuda.synchronize()
            got[entry] = [rc] + [(v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v.value if hasattr(v, "value") else v)).tobytes().hex()
                                 for k, v in sorted(o.items())]
        self.reset()
        return got

    def state(self):
        return dict(n_live=self.mp.info()["n_live"], n_live2=self.mp2.info()["n_live"], tables=[k.get_map_point_slots().tolist() for k in self.all_kfs])


def bad_calls(s):
    """[(name, entry, overrides)]: overrides by parameter name; "_hook": with an all-reduce hook set on the handle"""
    i32 = lambda *v: np.array(v, np.int32)
    null = C.c_void_p(None)
    kfs_other = s.kf_array([s.kfs[0], s.kfs[1], s.other])
    kfs_52 = s.kf_array([s.kfs[i % 3] for i in range(INERTIAL_MAX_K + 1)])
    chain_52 = np.arange(INERTIAL_MAX_K + 1, dtype=np.int32)
    calls = []
    for e in PARAMS:
        calls.append(("null store", e, dict(mp=null)))
        calls.append(("keyframe of another store", e, dict(kfs=kfs_other)))
        calls.append(("n_kfs = 0", e, dict(n_kfs=C.c_int(0), **({"n_chain": C.c_int(0)} if e in INERTIAL else {}))))
        for name in REQUIRED_OUT[e]:
            calls.append(("null " + name, e, {name: null}))
    for e in VISUAL:
        calls.append(("cur = n_kfs", e, dict(cur=C.c_int(3))))
        calls.append(("cur = -1", e, dict(cur=C.c_int(-1))))
    for e in ("orbx_map_collect_ba_window_device", "orbx_map_collect_ba_window"):
        calls.append(("max_covisible = -1", e, dict(max_covisible=C.c_int(-1))))
    cfg_neg = s.pkg.LocalBAConfigLM(max_covisible_keyframes=-1)._c()
    s.keep.append(cfg_neg)
    calls.append(("max_covisible = -1", "orbx_map_local_ba", dict(cfg=C.byref(cfg_neg))))
    for e in COLLECTS:
        calls.append(("list_cap one below the bound", e, dict(list_cap=C.c_int(LIST_BOUND - 1))))
        calls.append(("obs_cap one below the bound", e, dict(obs_cap=C.c_int(OBS_BOUND - 1))))
    for e in DEVICE:
        buf = s.torch.zeros((OBS_BOUND + 1, 16), dtype=s.torch.uint8, device="cuda")
        s.keep.append(buf)
        calls.append(("d_obs32 off by 8 bytes", e, dict(obs32=C.c_void_p(buf.data_ptr() + 8))))
    for e in INERTIAL:
        calls.append(("chain index out of range", e, dict(chain=i32(0, 3, 2))))
        calls.append(("chain index negative", e, dict(chain=i32(0, -1, 2))))
        calls.append(("chain entry twice", e, dict(chain=i32(0, 1, 1))))
        calls.append(("chain of one keyframe", e, dict(n_chain=C.c_int(1))))
    li = "orbx_map_local_inertial_ba"
    big = dict(n_kfs=C.c_int(INERTIAL_MAX_K + 1), kfs=kfs_52, n_chain=C.c_int(INERTIAL_MAX_K + 1), chain=chain_52,
               vel=np.zeros((INERTIAL_MAX_K + 1, 3)), bias=np.zeros((INERTIAL_MAX_K + 1, 6)), poses_out=np.zeros((INERTIAL_MAX_K + 1, 7)),
               vel_out=np.zeros((INERTIAL_MAX_K + 1, 3)), bias_out=np.zeros((INERTIAL_MAX_K + 1, 6)), fixed_kf=np.zeros(INERTIAL_MAX_K + 1, np.int32))
    calls.append(("n_chain = BA_INERTIAL_MAX_K + 1", li, big))
    calls.append(("IMU edge out of range", li, dict(edge_kf=i32(0, 1, 1, 3))))
    calls.append(("IMU edge negative", li, dict(edge_kf=i32(-1, 1, 1, 2))))
    calls.append(("IMU edge with equal ends", li, dict(edge_kf=i32(0, 1, 2, 2))))
    calls.append(("E = -1", li, dict(E=C.c_int(-1))))
    for e in ("orbx_map_local_ba", li):
        calls.append(("all-reduce hook set", e, dict(_hook=True)))
    # two rules at once: which one answers
    calls.append(("null store and cur outside", "orbx_map_collect_ba_window_device", dict(mp=null, cur=C.c_int(7))))
    calls.append(("keyframe of another store and chain entry twice", "orbx_map_collect_inertial_window", dict(kfs=kfs_other, chain=i32(0, 2, 2))))
    calls.append(("n_chain above the solver's and an IMU edge out of range", li, dict(big, edge_kf=i32(0, 1, 1, 60))))
    calls.append(("all-reduce hook set and a null output", li, dict(_hook=True, counts=null)))
    calls.append(("list_cap below the bound and a null output", "orbx_map_collect_ba_window", dict(list_cap=C.c_int(LIST_BOUND - 1), counts=null)))
    calls.append(("chain of one keyframe and keyframe of another store", "orbx_map_collect_inertial_window_device", dict(n_chain=C.c_int(1), kfs=kfs_other)))
    return calls


def run_bad_calls(s):
    """-> {"<entry>: <name>": [return code, orbx_last_error text]}"""
    got = {}
    for name, entry, ov in bad_calls(s):
        if ov.get("_hook"):
            s.h.set_allreduce(lambda ptr, n, stream: None)
        try:
            rc, _ = s.call(entry, **ov)
        finally:
            if ov.get("_hook"):
                s.h.set_allreduce(None)
        key = "%s: %s" % (entry, name)
        assert key not in got, key
        got[key] = [int(rc), s.L.orbx_last_error(s.h._h).decode()]
    return got


def record(path):
    """writes the fixture: what the library in use answers to bad_calls()"""
    import orb_slam3_rust_amd as pkg
    h = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), 2000, device=0, max_w=1920, max_h=1080, max_batch=8)
    s = Scene(pkg, h)
    got = run_bad_calls(s)
    assert all(rc != 0 for rc, _ in got.values()), [k for k, v in got.items() if v[0] == 0]
    with open(path, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    s.close(); h.close()
    return got


@pytest.mark.gpu
def test_refusals_keep_their_code_text_and_precedence_and_touch_nothing(pkg, gpu_handle):
    want = json.load(open(GOLDEN))
    s = Scene(pkg, gpu_handle)
    try:
        state, good = s.state(), s.good_round()
        assert all(v[0] == 0 for v in good.values()), {k: v[0] for k, v in good.items()}
        got = run_bad_calls(s)
        assert sorted(got) == sorted(want)
        wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
        assert not wrong, wrong
        assert all(rc != 0 for rc, _ in got.values())
        assert s.state() == state
        assert s.good_round() == good
    finally:
        s.close()
