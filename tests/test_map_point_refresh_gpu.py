"""orbx_refresh_map_points on the MI355X against its specification (tests/map_point_refresh_spec.py): phase 4 of search_in_neighbors
(search_in_neighbors.rs:139-150) — compute_distinctive_descriptors and update_map_point_normal_and_depth for a batch of map points.

Comparison.  Descriptor bytes, chosen, best_max_dist, n_desc, n_observers, the kept normals and the +inf / 0 depth ranges are exact.
min_distance / max_distance within 1e-14 relative: both sides feed bit-identical operands to one square root and one correctly rounded
multiply or divide, so a device sqrt within 1 ulp gives <= 2 ulp = 4.4e-16; the rest is margin.  Normal components within 1e-12
absolute: each of n <= 300 unit-vector terms carries <= 3 ulp = 3.3e-16, so the sum is off by <= 1e-13, and under the cone condition
(every point's observers inside a 60 degree cone, asserted on the scenes by tests/test_map_point_refresh_cpu.py) |sum| >= n / 2 >= 1,
so the division does not amplify it.  Every test prints its largest errors before it asserts."""
import numpy as np
import pytest

import map_point_refresh_scenes as G
import map_point_refresh_spec as S

pytestmark = pytest.mark.gpu

DEPTH_RTOL, NORMAL_ATOL = 1e-14, 1e-12
_cache = {}


def scene(name):
    """(scene, specification result), computed once and shared."""
    if name not in _cache:
        sc = G.golden_scene(G.golden_cases())[0] if name == "golden" else G.RANDOM_SCENES[name]()
        _cache[name] = (sc, S.refresh(sc))
    return _cache[name]


def host_form(h, sc):
    return h.refresh_map_points(sc["positions"], sc["obs_start"], sc["obs_kf"], sc["obs_feat"], sc["kf_poses_wc"], sc["kf_feat_offset"], sc["descs"],
                                sc["scale_range"], sc["mp_desc"], sc["normals"])


def compare(label, got, want):
    """got: api.MapPointRefresh, want: the specification's dict.  Prints the largest error of each kind, then asserts."""
    assert got.records.dtype == S.RECORD
    finite = np.isfinite(want["min_distance"])
    kept = np.array([a["normal_kept"] for a in want["aux"]], bool)
    rel = lambda g, w: float(np.max(np.abs(g - w) / np.abs(w), initial=0.0))
    e_min = rel(got.min_distance[finite], want["min_distance"][finite])
    e_max = rel(got.max_distance[finite], want["max_distance"][finite])
    e_nrm = float(np.max(np.abs(got.normals[~kept] - want["normals"][~kept]), initial=0.0))
    print("%s: %d points, largest error min_distance %.3e rel, max_distance %.3e rel, normal %.3e abs" % (label, len(kept), e_min, e_max, e_nrm))
    assert got.records.tobytes() == want["records"].tobytes(), np.flatnonzero(got.records != want["records"])[:10]
    assert np.array_equal(got.mp_desc, want["mp_desc"])
    assert np.array_equal(got.normals[kept], want["normals"][kept])                                   # kept normals: the input's bits
    assert np.array_equal(got.min_distance[~finite], want["min_distance"][~finite]) and np.array_equal(got.max_distance[~finite], want["max_distance"][~finite])
    assert e_min <= DEPTH_RTOL and e_max <= DEPTH_RTOL and e_nrm <= NORMAL_ATOL
    return e_min, e_max, e_nrm


def test_track_lengths_at_every_boundary(gpu_handle):
    """One point each with 0, 1, 2, 3, 63, 64, 65, 66, 130, 255, 256, 257, 300 observations; 5 keyframes of 300 features."""
    sc, want = scene("boundaries")
    assert np.diff(sc["obs_start"]).tolist() == G.BOUNDARY_LENGTHS
    compare("boundaries", host_form(gpu_handle, sc), want)


@pytest.mark.parametrize("variant", ["a", "b"])
def test_points_that_straddle_windows(gpu_handle, variant):
    """700 points of 0..12 observations over about 16 windows; points of 64 observations start at observation 255 and 511 (variant a) and
    at 256 and 511 (variant b: a point of 64 that starts at 255 covers 256, so the three starts need two lists); long points of 65 and
    200 observations are interleaved."""
    sc, want = scene("straddle_" + variant)
    compare("straddle " + variant, host_form(gpu_handle, sc), want)


def test_skipped_observations(gpu_handle):
    """obs_kf = -1 and = T, obs_feat = -1 and = n_features, a keyframe without features; points whose rows are all invalid while
    their observers exist are not updated, yet their normal and depth range are refreshed."""
    sc, want = scene("skips")
    got = host_form(gpu_handle, sc)
    compare("skips", got, want)
    for p in (1, 2, 6):                                                            # short and long: observers, no rows
        assert got.records["chosen"][p] == -1 and got.records["n_desc"][p] == 0 and got.records["n_observers"][p] > 0
        assert np.array_equal(got.mp_desc[p], sc["mp_desc"][p]) and not np.array_equal(got.normals[p], sc["normals"][p]) and np.isfinite(got.min_distance[p])
    assert got.records["n_observers"][3] == 0 and np.isinf(got.min_distance[3]) and got.max_distance[3] == 0.0


def test_ties_and_duplicates(gpu_handle):
    """Constructed equal maxima with n = 4 and n = 100: the earliest position wins in both kernels."""
    sc, want = scene("ties")
    assert not any(a["unique_min"] for a in want["aux"])                           # every point is a tie
    got = host_form(gpu_handle, sc)
    compare("ties", got, want)
    assert got.records["chosen"].tolist() == [1, 1, 2, 1, 1, 2] and (got.records["best_max_dist"] == 12).all()


def test_permuted_lists_choose_the_same_descriptor(gpu_handle):
    """Shuffling each point's list leaves the chosen descriptor's bytes unchanged and maps `chosen` through the permutation."""
    sc, want = scene("permutation")
    got = host_form(gpu_handle, sc)
    compare("permutation", got, want)
    sh, perm = G.shuffled(sc, 7)
    got2 = host_form(gpu_handle, sh)
    assert np.array_equal(got2.mp_desc, got.mp_desc)
    st = sc["obs_start"]
    assert all(perm[st[p] + got2.records["chosen"][p]] == got.records["chosen"][p] for p in range(len(st) - 1))
    for k in ("best_max_dist", "n_desc", "n_observers"):
        assert np.array_equal(got2.records[k], got.records[k])


def _resident(pkg, h, sc):
    import torch
    off = sc["kf_feat_offset"]
    kfs = []
    for t in range(len(off) - 1):
        n = int(off[t + 1] - off[t])
        d = torch.from_numpy(np.ascontiguousarray(sc["descs"][off[t]:off[t + 1]])).cuda() if n else torch.zeros((1, 32), dtype=torch.uint8, device="cuda")
        kp = torch.zeros((max(n, 1), pkg.KEYPOINT.itemsize), dtype=torch.uint8, device="cuda")
        kfs.append(pkg.KeyFrame(h, kp, d, n, keyframe_id=t, pose_wc=sc["kf_poses_wc"][t]))
    return kfs


@pytest.mark.parametrize("variant", ["a", "b"])
def test_the_three_forms_give_the_same_bytes(pkg, gpu_handle, variant):
    """Host arrays, device arrays and resident orbx_keyframes: the same bytes for every output.  A keyframe made by another handle
    is refused; M = 0 is OK."""
    import torch
    h = gpu_handle
    sc, want = scene("straddle_" + variant)
    a = host_form(h, sc)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_desc, d_nrm = dev(sc["mp_desc"]), dev(sc["normals"])
    o = h.refresh_map_points_device(dev(sc["positions"]), dev(sc["obs_start"]), dev(sc["obs_kf"]), dev(sc["obs_feat"]), int(sc["obs_start"][-1]),
                                    sc["kf_poses_wc"], sc["kf_feat_offset"], dev(sc["descs"]), sc["scale_range"], d_desc, d_nrm)
    h.synchronize()
    kfs = _resident(pkg, h, sc)
    c = pkg.KeyFrame.refresh_map_points(h, kfs, sc["positions"], sc["obs_start"], sc["obs_kf"], sc["obs_feat"], sc["scale_range"], sc["mp_desc"], sc["normals"])
    for name, b in (("device", (d_desc.cpu().numpy(), d_nrm.cpu().numpy(), o["min_distance"].cpu().numpy(), o["max_distance"].cpu().numpy(),
                                o["records"].cpu().numpy().view(pkg.MP_REFRESH_RECORD).reshape(-1))),
                    ("keyframes", (c.mp_desc, c.normals, c.min_distance, c.max_distance, c.records))):
        for x, y in zip((a.mp_desc, a.normals, a.min_distance, a.max_distance, a.records), b):
            assert x.tobytes() == y.tobytes(), name
    if variant == "a":
        other = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), 500, device=0, max_w=752, max_h=480, max_batch=1)
        try:
            foreign = _resident(pkg, other, sc)[:1]
            with pytest.raises(pkg.OrbxError):
                pkg.KeyFrame.refresh_map_points(h, kfs[:-1] + foreign, sc["positions"], sc["obs_start"], sc["obs_kf"], sc["obs_feat"], sc["scale_range"],
                                                sc["mp_desc"], sc["normals"])
            for k in foreign:
                k.close()
        finally:
            other.close()
        e = np.zeros((0, 3))
        r = h.refresh_map_points(e, [0], [], [], sc["kf_poses_wc"], sc["kf_feat_offset"], sc["descs"], sc["scale_range"], np.zeros((0, 32), np.uint8), e)
        assert len(r.records) == 0
        assert len(pkg.KeyFrame.refresh_map_points(h, kfs, e, [0], [], [], sc["scale_range"], np.zeros((0, 32), np.uint8), e).records) == 0
        with pytest.raises(pkg.OrbxError):                                          # obs_start must start at 0 and ascend
            bad = dict(sc); bad["obs_start"] = sc["obs_start"].copy(); bad["obs_start"][5] = bad["obs_start"][6] + 1
            host_form(h, bad)
    for k in kfs:
        k.close()


def test_golden_file_through_the_gpu(gpu_handle):
    """The hand-derived answers of tests/golden/map_point_refresh_known_answers.json: exact, every one."""
    sc, expect = G.golden_scene(G.golden_cases())
    got = host_form(gpu_handle, sc)
    for p, w in enumerate(expect):
        rec = got.records[p]
        assert (rec["chosen"], rec["best_max_dist"], rec["n_desc"], rec["n_observers"]) == (w["chosen"], w["best_max_dist"], w["n_desc"], w["n_observers"]), w["name"]
        assert np.array_equal(got.mp_desc[p], w["descriptor"]) and np.array_equal(got.normals[p], w["normal"]), w["name"]
        assert got.min_distance[p] == w["min_distance"] and got.max_distance[p] == w["max_distance"], w["name"]


def test_search_in_neighbors_shape(pkg, gpu_handle):
    """A current keyframe and 6 neighbours of 400 features (and two more observers): search_in_neighbors_affected ->
    collect_map_point_refresh -> KeyFrame.refresh_map_points on resident keyframes, against the specification."""
    arrays, cur, neighbours, descs = G.neighbourhood()
    snap = pkg.MapSnapshot(**arrays)
    affected = snap.search_in_neighbors_affected(cur, neighbours)
    d = snap.collect_map_point_refresh(affected + [31337])
    assert d.mp_ids == [m for m in affected if m in set(arrays["mp_ids"])] and len(d.mp_ids) > 500 and (d.obs_kf == -1).sum() <= 1
    T = len(d.kf_ids)
    rows = [descs[arrays["kf_ids"].index(k)] for k in d.kf_ids]
    rng = np.random.default_rng(1)
    sc = dict(positions=d.positions, obs_start=d.obs_start, obs_kf=d.obs_kf, obs_feat=d.obs_feat,
              kf_poses_wc=np.array([arrays["kf_pose_wc"][arrays["kf_ids"].index(k)] for k in d.kf_ids]),
              kf_feat_offset=np.arange(T + 1, dtype=np.int32) * 400, descs=np.concatenate(rows), scale_range=G.SCALE_RANGE,
              mp_desc=rng.integers(0, 256, (len(d.mp_ids), 32), dtype=np.uint8), normals=np.tile([0.0, 0.0, 1.0], (len(d.mp_ids), 1)))
    kfs = _resident(pkg, gpu_handle, sc)
    got = pkg.KeyFrame.refresh_map_points(gpu_handle, kfs, sc["positions"], sc["obs_start"], sc["obs_kf"], sc["obs_feat"], sc["scale_range"],
                                          sc["mp_desc"], sc["normals"])
    compare("search_in_neighbors", got, S.refresh(sc))
    assert got.num_descriptors_updated == int((got.records["n_desc"] > 0).sum()) > 500
    for k in kfs:
        k.close()
