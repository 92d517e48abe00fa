"""rank_select_kernel selects the kept keys of a level first (radix select on the response word, ties with the n-th kept) and
sorts only those; fast_kernel's survivor phases on inputs that load them.  Every case compares the GPU with the CPU specification
(oracle.orb_extract: keypoints, their order and the descriptors, byte for byte) and asserts, from the oracle's output alone, that the
input reaches the branch it is meant for — a case that stops exercising its branch fails instead of passing."""
import numpy as np
import pytest

from conftest import records_equal

pytestmark = pytest.mark.gpu

W, H = 752, 480


def _first_diff(a, b):
    if len(a) != len(b):
        return "%d vs %d keypoints" % (len(a), len(b))
    for name in a.dtype.names:
        bad = np.nonzero(a[name].view(np.uint32) != b[name].view(np.uint32))[0]
        if len(bad):
            return "%s differs at %d rows, first %d: %r vs %r" % (name, len(bad), bad[0], a[name][bad[0]], b[name][bad[0]])
    return "equal"


def _dots(period):
    """identical one-pixel blobs on a period x period grid: every FAST score and every Harris response of level 0 ties"""
    a = np.full((H, W), 20, np.uint8)
    a[8::period, 8::period] = 240
    return a


def _checker(c, lo=60, hi=180):
    y, x = np.mgrid[0:H, 0:W]
    return np.where(((y // c) + (x // c)) % 2 == 0, lo, hi).astype(np.uint8)


def _noise(seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def _sparse():
    a = np.full((H, W), 40, np.uint8)
    a[100:140, 100:140] = 200
    a[300:330, 500:560] = 220
    a[200:215, 300:315] = 10
    return a


def _check(pkg, oracle, img, n_features, **over):
    """GPU == oracle on `img`; returns (keypoints of the oracle, quota per level, kept count per level of the oracle)"""
    p = oracle.orb_params(n_features)
    for k, v in over.items():
        setattr(p, k, v)
    ok, od = oracle.orb_extract(img, p)
    T = oracle.orb_level_table(W, H, p)
    quota = [T.quota[l] for l in range(p.n_levels)]
    kept = np.bincount(ok["octave"].astype(int), minlength=p.n_levels).tolist()
    h = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), n_features, device=0, max_w=W, max_h=H, max_batch=1, orb_params=over or None)
    try:
        kp, d = h.process_stereo(img, img, cap_kp=len(ok) + 64)[:2]
    finally:
        h.close()
    assert records_equal(kp, ok), _first_diff(kp, ok)
    assert np.array_equal(d, od)
    return ok, quota, kept


@pytest.mark.parametrize("period", [24, 32])
def test_ties_at_the_quota(pkg, oracle, period):
    """Response ties at the quota-th key: all of them are kept, so the oracle returns more than n_features keypoints — on level 0
    more than the quota and no more than the 1024 keys the kernel sorts in LDS (the select-with-ties branch, not the rank sort)."""
    ok, quota, kept = _check(pkg, oracle, _dots(period), 500)
    assert len(ok) > 500
    assert quota[0] < kept[0] <= 1024


def test_level_with_fewer_candidates_than_its_quota(pkg, oracle):
    """M <= quota: nothing to select, every key is kept and sorted (a kept count below the quota means the level had no more candidates)"""
    ok, quota, kept = _check(pkg, oracle, _sparse(), 1000)
    assert any(0 < k < q for k, q in zip(kept, quota))
    ok, quota, kept = _check(pkg, oracle, _dots(24), 500)
    assert any(0 < k < q for k, q in zip(kept, quota)) and any(k > q for k, q in zip(kept, quota))


@pytest.mark.parametrize("kind,n_features", [("dots16", 1500), ("dots12", 300), ("synth", 5000), ("noise", 6000)])
def test_more_kept_than_the_lds_array(pkg, oracle, kind, n_features):
    """A level whose kept count is above 1024 (by heavy ties, or by its quota on a dense image): the rank-sort path"""
    img = {"dots16": lambda: _dots(16), "dots12": lambda: _dots(12), "synth": lambda: pkg.synth.stereo_pair(3, 1)[0], "noise": lambda: _noise(1)}[kind]()
    ok, quota, kept = _check(pkg, oracle, img, n_features)
    assert max(kept) > 1024
    if kind.startswith("dots"):
        assert len(ok) > n_features


@pytest.mark.parametrize("n_features,target", [(583, 127), (588, 128), (592, 129), (1172, 255), (1177, 256), (1182, 257),
                                               (2351, 511), (2356, 512), (2360, 513)])
def test_kept_counts_around_the_sort_sizes(pkg, oracle, n_features, target):
    """Level 0 keeps exactly `target` keys: one below, at and one above the padded sort sizes 128, 256 and 512"""
    ok, quota, kept = _check(pkg, oracle, pkg.synth.stereo_pair(3, 1)[0], n_features)
    assert quota[0] == target and kept[0] == target


@pytest.mark.parametrize("cell", [3, 4])
@pytest.mark.parametrize("thr", [7, 20])
def test_fine_checkerboards(pkg, oracle, cell, thr):
    """Fine checkerboards: ring pixels on both sides of the centre, so many pre-test survivors pass for both polarities; thousands of
    FAST corners on the first level that has any"""
    img = _checker(cell)
    p = oracle.orb_params(1500)
    p.fast_threshold = thr
    assert max(len(oracle.orb_fast_level(img, p, l)) for l in range(3)) > 5000
    ok, quota, kept = _check(pkg, oracle, img, 1500, fast_threshold=thr)
    assert len(ok) > 500


def test_noise_at_threshold_one(pkg, oracle):
    """Noise at FAST threshold 1: nearly every position survives the pre-test, more than half of a tile's position list"""
    img = _noise(2)
    p = oracle.orb_params(2000)
    p.fast_threshold = 1
    assert len(oracle.orb_fast_level(img, p, 0)) > 25000
    ok, quota, kept = _check(pkg, oracle, img, 2000, fast_threshold=1)
    assert kept[:3] == quota[:3]
