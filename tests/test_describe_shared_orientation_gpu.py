"""describe_tile_kernel with the orientation evaluated once per tile: the centroids of a tile's keypoints go through 16-byte LDS records, ONE wave
evaluates the angle and its sin / cos for up to 64 keypoints (one per lane), further rounds of 64 follow for denser tiles, and the tests read
the records back.  Keypoints and descriptors must be the bits of the CPU oracle and of the per-keypoint form (describe_fused_kernel).

320 x 240 is the smallest size at which eight levels keep a 64 x 64 window (level 7 is 89 x 67), so the tile form is admissible: 13 describe tiles
per image.  The scenes are chosen so that the oracle's keypoints put into single tiles: nothing, exactly one keypoint, a count that is no multiple
of 4 (nor of 16), more than 64 (a second evaluation round) and more than 128 (a third) — asserted below from the oracle's keypoints, with the
tile cut of orb_prepare_geometry restated here, so that the test cannot pass without those rounds."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, N_FEATURES, EDGE, DT_T_MAX = 320, 240, 2500, 31, 153
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cut(k):
    """orb_prepare_geometry's cut of k keypoint positions into n equal tiles of t: the n in n0 .. n0 + 4 that needs the fewest 48-px windows."""
    best, out, n0 = 1 << 30, None, (k + DT_T_MAX - 1) // DT_T_MAX
    for n in range(n0, n0 + 5):
        t = (k + n - 1) // n
        wins = n * ((t + 39 + 47) // 48)
        if wins < best:
            best, out = wins, (n, t)
    return out


def _tile_counts(O, kp, p):
    """Keypoints per describe tile, every level's tiles in one flat list."""
    T = O.orb_level_table(W, H, p)
    counts = []
    for l in range(T.n_levels):
        kw, kh = T.w[l] - 2 * EDGE, T.h[l] - 2 * EDGE
        assert T.w[l] >= 64 and T.h[l] >= 64 and kw > 0 and kh > 0
        (nx, tw), (ny, th) = _cut(kw), _cut(kh)
        c = np.zeros((ny, nx), int)
        k = kp[kp["octave"] == l]
        x = np.rint(k["x"] / np.float32(T.scale[l])).astype(int)
        y = np.rint(k["y"] / np.float32(T.scale[l])).astype(int)
        np.add.at(c, ((y - EDGE) // th, (x - EDGE) // tw), 1)
        counts += [int(v) for v in c.ravel()]
    return counts


def _blobs(seed, n):
    """A flat image with n bright rectangles: a few corners each, most tiles empty."""
    r = np.random.default_rng(seed)
    img = np.full((H, W), 100, np.uint8)
    for _ in range(n):
        x, y, a, b = int(r.integers(20, W - 30)), int(r.integers(20, H - 30)), int(r.integers(3, 9)), int(r.integers(3, 9))
        img[y:y + b, x:x + a] = int(r.integers(160, 255))
    return img


@pytest.fixture(scope="module")
def scenes(oracle):
    """name -> (image, oracle keypoints, oracle descriptors, keypoints per tile); computed once."""
    p = oracle.orb_params(N_FEATURES)
    imgs = {"sparse": _blobs(2, 10), "noise": np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8), "flat": np.full((H, W), 90, np.uint8)}
    out = {}
    for name, img in imgs.items():
        kp, d = oracle.orb_extract(img, p)
        out[name] = (img, kp, d, _tile_counts(oracle, kp, p))
    return out


def _extract(P, h, imgs, cap, slots=None):
    """extract_batch_device on a stack of images: (per image keypoint bytes, descriptors), the raw output tensors too."""
    import torch
    o = h.alloc_batch_outputs((max(slots or len(imgs), len(imgs)) + 1) // 2, cap)
    h.extract_batch_device(torch.from_numpy(np.stack(imgs)).cuda(), o)
    err = None
    try:
        h.check_status()
    except P.OrbxError as e:
        err = e
    nkp = o["nkp"].cpu().numpy().reshape(-1)
    kp = o["kp"].cpu().numpy().reshape(-1, cap, 7)
    desc = o["desc"].cpu().numpy().reshape(-1, cap, 32)
    return [(kp[i, :nkp[i]].tobytes(), desc[i, :nkp[i]].copy()) for i in range(len(imgs))], (nkp, kp, desc, err)


CAP = N_FEATURES + 2048


@pytest.fixture(scope="module")
def tile_form(pkg, scenes):
    """The tile form (forced for the suite: ORBX_DESC_TILE=1) on every scene alone and on a batch of the three scenes (one of them twice); one handle."""
    assert os.environ.get("ORBX_DESC_TILE") == "1"
    h = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), N_FEATURES, device=0, max_w=W, max_h=H, max_batch=2)
    h.set_profiling(True)
    res = {name: _extract(pkg, h, [s[0]], CAP)[0][0] for name, s in scenes.items()}
    assert "describe_tile_kernel" in h.kernel_times() and "describe_fused_kernel" not in h.kernel_times()
    h.set_profiling(False)
    res["batch"] = _extract(pkg, h, [scenes[n][0] for n in ("noise", "sparse", "flat", "sparse")], CAP)[0]
    yield h, res
    h.close()


@pytest.fixture(scope="module")
def per_keypoint_form(scenes, tmp_path_factory):
    """The same scenes through describe_fused_kernel: a child process, the switch is read when the geometry is prepared."""
    d = tmp_path_factory.mktemp("per_kp")
    np.savez(str(d / "in.npz"), **{n: s[0] for n, s in scenes.items()})
    script = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r)
        import torch
        import orb_slam3_rust_amd as P
        src = np.load(sys.argv[1]); out = {}
        h = P.Handle(P.CameraModel(**P.synth.EUROC_CAMERA), %d, device=0, max_w=%d, max_h=%d, max_batch=1)
        h.set_profiling(True)
        for n in src.files:
            o = h.alloc_batch_outputs(1, %d)
            h.extract_batch_device(torch.from_numpy(src[n][None]).cuda(), o)
            h.check_status()
            k = int(o["nkp"].cpu().numpy().reshape(-1)[0])
            out["k_" + n] = o["kp"].cpu().numpy().reshape(-1, 7)[:k].view(np.uint8).reshape(-1); out["d_" + n] = o["desc"].cpu().numpy().reshape(-1, 32)[:k]
        assert "describe_fused_kernel" in h.kernel_times() and "describe_tile_kernel" not in h.kernel_times()
        h.close()
        np.savez(sys.argv[2], **out)
    """ % (ROOT, N_FEATURES, W, H, CAP))
    subprocess.run([sys.executable, "-c", script, str(d / "in.npz"), str(d / "out.npz")], check=True, env=dict(os.environ, ORBX_DESC_TILE="0"), timeout=300)
    return np.load(str(d / "out.npz"))


def test_scenes_cover_every_round_count(scenes):
    """What the scenes are for, from the oracle's keypoints alone."""
    sparse, noise = scenes["sparse"][3], scenes["noise"][3]
    assert len(sparse) == len(noise) == 13
    print("keypoints per tile: sparse %s, noise %s" % (sparse, noise))
    assert 0 in sparse and 1 in sparse                                        # an empty tile, a tile with exactly one keypoint
    assert any(c % 4 and c % 16 and c > 4 for c in sparse)                    # partial groups of four past the first
    assert any(64 < c <= 128 for c in noise) and any(c > 128 for c in noise)  # a second and a third evaluation round
    assert any(c > 128 and c % 64 for c in noise) and 1 in noise              # the last round partial; one keypoint beside dense tiles
    assert all(c == 0 for c in scenes["flat"][3]) and len(scenes["flat"][1]) == 0


@pytest.mark.parametrize("name", ["sparse", "noise", "flat"])
def test_single_image_equals_oracle_and_per_keypoint_form(scenes, tile_form, per_keypoint_form, name):
    _, kp, d, _ = scenes[name]
    gk, gd = tile_form[1][name]
    assert len(gk) == kp.nbytes and gk == kp.tobytes(), "keypoints differ from the oracle"
    assert np.array_equal(gd, d), "descriptors differ from the oracle at rows %s" % np.nonzero((gd != d).any(1))[0][:8]
    assert per_keypoint_form["k_" + name].tobytes() == gk and np.array_equal(per_keypoint_form["d_" + name], gd)


def test_batch_of_different_scenes(scenes, tile_form):
    """Dense, sparse and empty images in one launch: a block's records and counts are its own tile's."""
    for (gk, gd), name in zip(tile_form[1]["batch"], ("noise", "sparse", "flat", "sparse")):
        _, kp, d, _ = scenes[name]
        assert gk == kp.tobytes() and np.array_equal(gd, d), name


def test_capacity_below_the_keypoint_count(pkg, scenes, tile_form):
    """cap_kp smaller than the count: the overflow is reported, the first cap_kp output slots are the oracle's, and the keypoints whose slot
    lies past the capacity write nothing — the slot of a second image behind stays zero."""
    _, kp, d, _ = scenes["noise"]
    cap = 1000
    assert len(kp) > cap + 1000
    _, (nkp, gk, gd, err) = _extract(pkg, tile_form[0], [scenes["noise"][0]], cap, slots=2)
    assert err is not None and err.code == -4
    assert nkp[0] == cap
    assert gk[0].tobytes() == kp[:cap].tobytes() and np.array_equal(gd[0], d[:cap])
    assert not gk[1].any() and not gd[1].any()
