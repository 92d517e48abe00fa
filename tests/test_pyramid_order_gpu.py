"""The extractor's launches walk the image groups in alternating directions (XcdMap in orb_kernels.hip), the stereo matcher its pairs
likewise.  That may not change a byte: an image's keypoints, descriptors and counts do not depend on where in a batch it stands or on how
many images the batch holds (n = 7, 9, 17: the partial last group of 8 is the first one a reversed launch dispatches), and every pyramid
level of every image equals the CPU specification's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = (101, 77)            # the smallest size of test_extract_gpu.py's pyramid cases
N_FEATURES = 1000


def _images(pkg, n, w, h, seed):
    """n distinct images: the left and right views of ceil(n / 2) synthetic pairs."""
    return np.ascontiguousarray(pkg.synth.stereo_batch(seed, 0, (n + 1) // 2, w=w, h=h).reshape(-1, h, w)[:n])


def _extract(h, torch, imgs, cap):
    n = len(imgs)
    out = h.alloc_batch_outputs((n + 1) // 2, cap)
    h.extract_batch_device(torch.from_numpy(imgs).cuda(), out)
    h.synchronize()
    nkp = out["nkp"].cpu().numpy().reshape(-1)[:n]
    kp = out["kp"].cpu().numpy().reshape(-1, cap, 7)[:n].view(np.uint32)
    desc = out["desc"].cpu().numpy().reshape(-1, cap, 32)[:n]
    return nkp, kp, desc


@pytest.fixture(scope="module")
def handle(pkg):
    h = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), N_FEATURES, device=0, max_w=752, max_h=480, max_batch=9)
    yield h
    h.close()


@pytest.fixture(scope="module")
def alone(pkg, handle):
    """Every image of the two sets extracted in a call of its own (computed once)."""
    import torch
    cap = N_FEATURES + 64
    res = {}
    for (w, hh), n in ((SMALL, 17), ((752, 480), 9)):
        imgs = _images(pkg, n, w, hh, 90 + w)
        res[(w, hh)] = (imgs, [_extract(handle, torch, imgs[i:i + 1], cap) for i in range(n)])
    return res


@pytest.mark.parametrize("w,h,n", [SMALL + (1,), SMALL + (7,), SMALL + (8,), SMALL + (9,), SMALL + (17,), (752, 480, 9)])
def test_image_in_batch_equals_image_alone(handle, alone, w, h, n):
    import torch
    cap = N_FEATURES + 64
    imgs, single = alone[(w, h)]
    nkp, kp, desc = _extract(handle, torch, imgs[:n], cap)
    total = 0
    for i in range(n):
        n1, k1, d1 = single[i]
        assert nkp[i] == n1[0], "image %d of %d: %d keypoints in the batch, %d alone" % (i, n, nkp[i], n1[0])
        c = int(nkp[i])
        total += c
        assert np.array_equal(kp[i, :c], k1[0, :c]), "keypoints of image %d of %d" % (i, n)
        assert np.array_equal(desc[i, :c], d1[0, :c]), "descriptors of image %d of %d" % (i, n)
    if (w, h) == (752, 480):
        assert total > 500 * n


def test_pair_in_batch_equals_pair_alone(pkg, handle):
    """process_stereo_batch_device for 1, 3 and 9 pairs: the matcher's pair order follows the extractor's last launch."""
    import torch
    cap = N_FEATURES + 64
    pairs = pkg.synth.stereo_batch(93, 0, 9)

    def run(p):
        out = handle.alloc_batch_outputs(len(p), cap)
        handle.process_stereo_batch_device(torch.from_numpy(np.ascontiguousarray(p)).cuda(), out)
        handle.synchronize()
        return {k: out[k].cpu().numpy() for k in ("kp", "desc", "nkp", "matches", "nmatches", "points", "has_point")}

    single = [run(pairs[i:i + 1]) for i in range(9)]
    for b in (1, 3, 9):
        got = run(pairs[:b])
        for i in range(b):
            one = single[i]
            nm, nl = int(one["nmatches"][0]), int(one["nkp"][0, 0])
            assert np.array_equal(got["nkp"][i], one["nkp"][0]) and got["nmatches"][i] == nm, (b, i)
            assert nm > 100
            assert np.array_equal(got["matches"][i, :nm], one["matches"][0, :nm]), (b, i)
            assert np.array_equal(got["has_point"][i, :nl], one["has_point"][0, :nl]), (b, i)
            keep = one["has_point"][0, :nl] == 1
            assert np.array_equal(got["points"][i, :nl][keep].view(np.uint64), one["points"][0, :nl][keep].view(np.uint64)), (b, i)


@pytest.mark.parametrize("w,h,n", [(752, 480, 1), (752, 480, 9), (190, 150, 3)])
def test_every_level_of_every_image_in_a_batch(pkg, oracle, handle, w, h, n):
    """Levels 1..7 of every image of a batch against the oracle's pyramid, byte for byte: launch l+1 reads what launch l wrote while walking the
    images the other way round.  190 x 150: level 7 is 53 x 42, a single tile, and no level height is a multiple of the tile's 96 (or 32) rows."""
    import torch
    imgs = _images(pkg, n, w, h, 95)
    _extract(handle, torch, imgs, N_FEATURES + 64)
    p = oracle.orb_params(N_FEATURES)
    for i in range(n):
        for l in range(1, 8):
            want = oracle.orb_pyramid_level(imgs[i], p, l)
            got = handle.debug_level(i, l)
            assert got.shape == want.shape and np.array_equal(got, want), "%dx%d image %d of %d level %d: %d pixels differ" % (w, h, i, n, l, (got != want).sum())
