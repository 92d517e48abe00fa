"""fast_kernel's block-wide corner list: phase 2 lists the positions that score above zero inside the tile and the border-filtered region a
second time (from the top of the survivor list's array downwards, one ballot and one returning LDS add per wave round, the border tests folded
into two unsigned compares), phase 3 walks that list and aggregates its appends per wave round.  The candidate order is free, so the
extractor's final output — and the sorted candidates of every level — are compared with the CPU oracle bit for bit.

Images: the 96 x 96 checkerboard of 3-px cells; an image without corners; an image whose only bright pixels sit in the NMS frame and on the
border-filter edge of tiles, a partial right / bottom tile among them; and a lattice of single bright pixels every 4 px.  (Under the oracle's
FAST-9 the 3-px checkerboard has NO corner — the ring of radius 3 changes colour every three pixels, no arc of 9 — but every one of its
positions survives the compass pre-test, so it is the densest survivor list with an empty corner list.  The densest strict maxima this
detector can produce are isolated pixels 4 apart, whose rings do not touch a neighbour: one corner per 4 x 4 positions, all above zero and all
listed; their values differ, so the NMS compares unequal scores.)"""
import numpy as np
import pytest

from conftest import records_equal

pytestmark = pytest.mark.gpu

EDGE, FT = 31, 62


def _checker():
    y, x = np.mgrid[0:96, 0:96]
    return np.where(((x // 3) + (y // 3)) % 2 == 0, 30, 220).astype(np.uint8)


def _lattice(w=158, h=158):
    """One whole 62 x 62 tile and partial tiles right of and below it; a bright pixel every 4 px, no two neighbours equal."""
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x % 4 == 0) & (y % 4 == 0), 120 + (7 * x + 13 * y) % 97, 20).astype(np.uint8)


def _frame_and_edge(w=144, h=130):
    """Single bright pixels on a flat image: level 0 is a whole tile and a 20-px partial one per row (columns 31..92, 93..112), the last
    admissible column / row is w - 32 / h - 32.  (x, y, value): on the edge; one past it (in the partial tile's NMS frame: scored, never a
    corner); pairs across the edge and across the boundary between two tiles, the stronger one inside and outside in turn."""
    img = np.full((h, w), 60, np.uint8)
    xe, ye, xt = w - EDGE - 1, h - EDGE - 1, EDGE + FT - 1
    dots = [(xe, 50, 200), (xe + 1, 60, 200), (50, ye, 200), (60, ye + 1, 200), (xe, ye, 210),
            (xe, 70, 150), (xe + 1, 71, 230), (xe, 90, 230), (xe + 1, 91, 150), (70, ye, 150), (71, ye + 1, 230),
            (EDGE, 40, 200), (EDGE - 1, 45, 200), (40, EDGE, 200), (45, EDGE - 1, 200),
            (xt, 80, 220), (xt + 1, 81, 180), (xt, 86, 180), (xt + 1, 87, 220)]
    for x, y, v in dots:
        img[y, x] = v
    return img, xe, ye, xt


IMAGES = {"checkerboard": _checker, "flat": lambda: np.full((96, 96), 77, np.uint8), "frame_and_edge": lambda: _frame_and_edge()[0], "lattice": _lattice}


@pytest.mark.parametrize("name", list(IMAGES))
def test_candidates_and_output_equal_oracle(pkg, oracle, name):
    img = IMAGES[name]()
    h_px, w_px = img.shape
    p = oracle.orb_params(2000)
    want = [np.sort(oracle.orb_fast_level(img, p, l)) for l in range(8)]
    xy0 = {(int(v) & 0xfff, (int(v) >> 12) & 0xfff) for v in want[0]}
    if name in ("checkerboard", "flat"):
        assert sum(len(c) for c in want) == 0
    elif name == "lattice":
        assert len(want[0]) == len(range(32, w_px - EDGE, 4)) ** 2 > 500          # every lattice pixel inside the border-filtered region
    else:
        _, xe, ye, xt = _frame_and_edge()
        assert {(xe, 50), (50, ye), (xe, ye), (xe, 90), (EDGE, 40), (40, EDGE), (xt, 80), (xt + 1, 87)} <= xy0   # on the edges; the stronger of a pair
        assert not xy0 & {(xe + 1, 60), (60, ye + 1), (EDGE - 1, 45), (45, EDGE - 1)}                              # past the edge
        assert not xy0 & {(xe, 70), (70, ye), (xt + 1, 81), (xt, 86)} and all(x <= xe and y <= ye for x, y in xy0)  # put down by a neighbour in the frame
    h = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), 2000, device=0, max_w=w_px, max_h=h_px, max_batch=1)
    try:
        ok, od = oracle.orb_extract(img, p)
        kpL, dL, kpR, dR = h.process_stereo(img, np.ascontiguousarray(img[::-1, ::-1]), cap_kp=len(ok) + 4096)[:4]
        for l in range(8):
            got = np.sort(h.debug_candidates(0, l))
            assert np.array_equal(got, want[l]), "FAST level %d: %d vs %d candidates" % (l, len(got), len(want[l]))
        assert records_equal(kpL, ok) and np.array_equal(dL, od)
        ok, od = oracle.orb_extract(np.ascontiguousarray(img[::-1, ::-1]), p)
        assert records_equal(kpR, ok) and np.array_equal(dR, od)
    finally:
        h.close()
