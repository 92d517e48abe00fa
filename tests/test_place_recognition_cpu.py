"""Place recognition without a GPU: the reference's unit values on the restatement (tests/place_recognition_spec.py), the restatement's
L1 score against orbx_bow_score (host code of the library) byte for byte, the usefulness of the parity scenes the GPU tests compare
on, the self-in-connected finding, the ConsistencyChecker, and the header's defaults."""
import ctypes as C
import struct

import numpy as np
import pytest

import place_recognition_scenes as SC
import place_recognition_spec as S


def bits(x):
    return struct.pack("<d", float(x))


def lib_bow_score(pkg, w1, v1, w2, v2):
    L = pkg.load_library()
    L.orbx_bow_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    w1 = np.ascontiguousarray(w1, np.uint32); w2 = np.ascontiguousarray(w2, np.uint32)
    v1 = np.ascontiguousarray(v1, np.float64); v2 = np.ascontiguousarray(v2, np.float64)
    out = C.c_double()
    rc = L.orbx_bow_score(w1.ctypes.data, v1.ctypes.data, len(w1), w2.ctypes.data, v2.ctypes.data, len(w2), C.byref(out))
    assert rc == 0
    return out.value


def random_bow(rng, n, n_words=1 << 32, normalise=True, negative=False):
    w = np.unique(rng.integers(0, n_words, n, dtype=np.uint64)).astype(np.uint32)
    while len(w) < n:                                                # top up after duplicates fell away
        w = np.unique(np.concatenate([w, rng.integers(0, n_words, n - len(w), dtype=np.uint64).astype(np.uint32)]))
    v = rng.uniform(-1.0 if negative else 0.01, 1.0, len(w))
    if normalise:
        v = v / np.abs(v).sum()
    return w, v


def edge_pairs():
    """The pairs of the byte-for-byte checks: random sizes, an empty vector on either side, disjoint and identical vectors, word ids 0
    and 2^32 - 1, unnormalised and negative weights, n = 8192."""
    rng = np.random.default_rng(20240)
    pairs = []
    for _ in range(40):
        n1, n2 = int(rng.integers(1, 1500)), int(rng.integers(1, 1500))
        nw = int(rng.choice([200, 3000, 100000, 1 << 32]))
        pairs.append((random_bow(rng, min(n1, nw // 2), nw), random_bow(rng, min(n2, nw // 2), nw)))
    a = random_bow(rng, 700, 5000); b = random_bow(rng, 900, 5000)
    e = (np.zeros(0, np.uint32), np.zeros(0, np.float64))
    pairs += [(e, a), (a, e), (e, e), (a, a)]
    pairs.append(((a[0][a[0] < 2500], a[1][a[0] < 2500]), (b[0][b[0] >= 2500], b[1][b[0] >= 2500])))     # disjoint
    lo = (np.array([0, 7, 0xFFFFFFFF], np.uint32), np.array([0.25, 0.5, 0.25]))
    hi = (np.array([0, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32), np.array([0.5, 0.125, 0.375]))
    pairs += [(lo, hi), (hi, lo), ((np.array([0xFFFFFFFF], np.uint32), np.array([1.0])), (np.array([0], np.uint32), np.array([1.0])))]
    pairs.append((random_bow(rng, 800, 4000, normalise=False, negative=True), random_bow(rng, 1000, 4000, normalise=False, negative=True)))
    pairs.append((random_bow(rng, 8192, 30000), random_bow(rng, 8192, 30000)))
    pairs.append((random_bow(rng, 8192, 1 << 32), random_bow(rng, 5, 100)))
    return pairs


def test_reference_unit_values():
    """detector.rs:457-480 (test_bow_score_identical / _different) on the DOT restatement, vocabulary/mod.rs:443-462 on L1."""
    w = np.array([1, 2, 3], np.uint32); v = np.array([0.5, 0.3, 0.2])
    for f in (S.dot_score, S.dot_score_merge):
        assert f(w, v, w, v) > 0.3
        assert f(np.array([1, 2], np.uint32), np.array([0.5, 0.5]), np.array([3, 4], np.uint32), np.array([0.5, 0.5])) == 0.0
    v1 = (np.array([0, 1], np.uint32), np.array([0.5, 0.5])); v3 = (np.array([2, 3], np.uint32), np.array([0.5, 0.5]))
    for f in (S.l1_score, S.l1_score_merge):
        assert abs(f(*v1, *v1) - 1.0) < 1e-10
        assert f(*v1, *v3) < 0.01


def test_restatement_l1_equals_orbx_bow_score_byte_for_byte(pkg):
    n_tree_differs = 0
    for (w1, v1), (w2, v2) in edge_pairs():
        want = lib_bow_score(pkg, w1, v1, w2, v2)
        assert bits(S.l1_score(w1, v1, w2, v2)) == bits(want), (len(w1), len(w2))
        if len(w1) + len(w2) <= 3000:                                # the plain-Python merge is the slow form
            assert bits(S.l1_score_merge(w1, v1, w2, v2)) == bits(want)
            assert bits(S.dot_score_merge(w1, v1, w2, v2)) == bits(S.dot_score(w1, v1, w2, v2))
        x, y, in1, in2 = S._dense(w1, v1, w2, v2)
        n_tree_differs += bits(1.0 - 0.5 * float(np.abs(x - y).sum())) != bits(want)
    assert n_tree_differs > 0          # a pairwise (tree) sum is another number: the order is part of the specification


def test_bow_score_rejects_unordered_words(pkg):
    L = pkg.load_library()
    w = np.array([3, 3], np.uint32); v = np.array([0.5, 0.5]); out = C.c_double()
    L.orbx_bow_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert L.orbx_bow_score(w.ctypes.data, v.ctypes.data, 2, w.ctypes.data, v.ctypes.data, 2, C.byref(out)) == -1


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_parity_scene_is_useful(pkg, name):
    """Over the scene's queries (default config, both scorings looked at, L1 asserted): at least half return a candidate; one returns
    none because too few connected keyframes were scored (threshold 0); one returns none although a threshold was computed; one has
    two ids with one score; one has more candidates than the cap."""
    d, queries = SC.load(pkg, name)
    db = SC.spec_database(d)
    with_cand = zero_thr = none_reach = tie = over_cap = 0
    for q in queries:
        thr, checked, cands = SC.outcome(db, d, q)
        with_cand += len(cands) > 0
        zero_thr += checked < S.DEFAULTS["min_covisibles_for_threshold"] and thr == 0.0 and not cands
        none_reach += thr >= 0.01 and not cands
        sc = [c[1] for c in cands]
        tie += len(set(sc)) < len(sc)
        over_cap += len(cands) > SC.CAP
    print(name, dict(queries=len(queries), with_cand=with_cand, zero_thr=zero_thr, none_reach=none_reach, tie=tie, over_cap=over_cap))
    assert 2 * with_cand >= len(queries)
    assert zero_thr >= 1 and none_reach >= 1 and tie >= 1 and over_cap >= 1
    # the relocalisation query finds something too, in more than one map
    w, v = d["words"][queries[0]], d["weights"][queries[0]]
    r = db.detect_candidates(w, v, None, 50)
    assert len(r) > SC.CAP and len({m for _i, m, _s in r}) == 2
    assert all(m != 1 for _i, m, _s in db.detect_candidates(w, v, 1, 50))


def test_self_in_connected_sets_threshold_to_ratio(pkg):
    """get_connected_keyframes inserts the current keyframe (detector.rs:234) and compute_min_score does not exclude it: with its own id
    among the first ten scored its self-score 1.0 makes the threshold 0.75; without, the threshold is the best neighbour's score * 0.75."""
    d, _ = SC.load(pkg, "loop_a")
    db = SC.spec_database(d)
    q = 104
    others = [c for c in d["connected"][q] if c != q and d["maps"][c] == d["maps"][q]]     # each of them is scored
    assert len(others) >= 10
    thr_self, n_self = db.min_score(q, [q] + others, S.DEFAULTS, S.L1)
    thr_late, n_late = db.min_score(q, others[:10] + [q], S.DEFAULTS, S.L1)       # the eleventh is never scored
    thr_none, _ = db.min_score(q, others, S.DEFAULTS, S.L1)
    assert n_self == n_late == 10
    assert thr_self == 0.75
    assert thr_late == thr_none and 0.01 < thr_late < 0.75
    assert len(db.detect_loop_candidates(q, others)) > len(db.detect_loop_candidates(q, [q] + others))


def _cand(pkg, cur, loop, score, cov=()):
    return pkg.LoopCandidate(cur, loop, score, list(cov))


def test_consistency_checker(pkg):
    """detector.rs:394-434"""
    ck = pkg.ConsistencyChecker(pkg.LoopDetectorConfig(consistency_threshold=3))
    assert ck.add_and_check(10, [_cand(pkg, 10, 1, 0.8, [2, 3])]) is None
    assert ck.add_and_check(11, [_cand(pkg, 11, 1, 0.85, [2])]) is None
    r = ck.add_and_check(12, [_cand(pkg, 12, 1, 0.9)])
    assert r is not None and r.loop_kf_id == 1
    assert len(ck.history) == 0 and ck.consistent_counts == {}      # cleared after a detection (:139-143)


def test_consistency_checker_no_match(pkg):
    """detector.rs:436-455"""
    ck = pkg.ConsistencyChecker(pkg.LoopDetectorConfig(consistency_threshold=3))
    for i in range(10, 15):
        assert ck.add_and_check(i, [_cand(pkg, i, i - 9, 0.8)]) is None
    assert len(ck.history) == 5                                      # threshold + 2 entries kept (:130-132)
    assert ck.add_and_check(15, []) is None and len(ck.history) == 5


def test_header_defaults_equal_reference(pkg):
    """orbx_default_loop_detector_config = LoopDetectorConfig::default() (detector.rs:36-46) = the Python dataclass."""
    from orb_slam3_rust_amd.api import _LoopDetectorConfig
    c = _LoopDetectorConfig()
    pkg.load_library().orbx_default_loop_detector_config(C.byref(c))
    got = (c.min_score_ratio, c.consistency_threshold, c.min_covisibles_for_threshold, c.max_covisibles_to_check, c.min_temporal_gap)
    assert got == (0.75, 3, 5, 10, 30)
    p = pkg.LoopDetectorConfig()
    assert got == (p.min_score_ratio, p.consistency_threshold, p.min_covisibles_for_threshold, p.max_covisibles_to_check, p.min_temporal_gap)
    assert got == tuple(S.DEFAULTS[k] for k in ("min_score_ratio", "consistency_threshold", "min_covisibles_for_threshold",
                                                "max_covisibles_to_check", "min_temporal_gap"))


def test_bow_database_shape(pkg):
    """synth.bow_database: neighbours share most words, the revisited stretch shares them with keyframes at least 30 ids back."""
    d = pkg.synth.bow_database(5, 120, words_per_kf=400, n_words=50000, revisit=(80, 30, 10))
    share = lambda i, j: len(np.intersect1d(d["words"][i], d["words"][j])) / len(d["words"][i])
    assert share(40, 41) > 0.6 and share(40, 70) < 0.05
    assert share(85, 15) > 0.6 and share(85, 50) < 0.05
    assert all(np.all(np.diff(w.astype(np.int64)) > 0) for w in d["words"])
    assert all(abs(v.sum() - 1.0) < 1e-12 for v in d["weights"])
    assert all(i in c for i, c in enumerate(d["connected"]))
