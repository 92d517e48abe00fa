"""The device-resident keyframe BoW database (orbx_kfdb_*, kfdb_kernels.hip) against orbx_bow_score and the restatement of
tests/place_recognition_spec.py: every score byte for byte, both searches in ids, order, counts and score bytes; batches, insertion
orders, erase / replace histories and repeated runs against each other; add_device fed by orbx_bow_vectors_device; each filter alone;
bad arguments; the compiled C++ caller against the Python class."""
import os
import struct
import subprocess

import numpy as np
import pytest

import place_recognition_scenes as SC
import place_recognition_spec as S
from test_place_recognition_cpu import lib_bow_score, random_bow

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam3-rust_amd")


def fill(pkg, h, d, order=None):
    db = pkg.KeyFrameDatabase(h)
    for i in (order if order is not None else range(len(d["ids"]))):
        db.add(d["ids"][i], (d["words"][i], d["weights"][i]), d["maps"][i], d["bad"][i])
    return db


def loop_bytes(db, d, queries, cfg=None, scoring=S.L1, cap=SC.CAP):
    """The single-call results of the queries as one byte string each."""
    out = []
    for q in queries:
        ids, sc, total = db.detect_loop_candidates(q, d["connected"][q], cfg, scoring, cap)
        out.append(struct.pack("<i", total) + ids.tobytes() + sc.tobytes())
    return out


def assert_loop_equals_spec(db, sdb, d, q, cfg_kw, scoring, cap, pkg):
    cfg = pkg.LoopDetectorConfig(**cfg_kw)
    ids, sc, total = db.detect_loop_candidates(q, d["connected"][q], cfg, scoring, cap)
    want = sdb.detect_loop_candidates(q, d["connected"][q], cfg_kw, scoring)
    where = (q, cfg_kw, scoring)
    assert total == len(want), where
    assert [int(i) for i in ids] == [w[0] for w in want[:cap]], where
    assert sc.tobytes() == np.array([w[1] for w in want[:cap]], np.float64).tobytes(), where
    return len(want)


# ---- scores -------------------------------------------------------------------------------------------------------------------------
def mixed_database(seed, N, n_words=20000):
    """N BowVectors of 0 to 8192 words in one database: mostly short, some empty, a few of the full 8192."""
    rng = np.random.default_rng([0x5C0, seed, N])
    sizes = np.minimum(rng.geometric(1.0 / 150.0, N), 3000)
    sizes[rng.random(N) < 0.03] = 0
    for j in rng.integers(0, max(N, 1), min(N, 3)):
        sizes[j] = 8192
    if N >= 63:
        sizes[:4] = [0, 1, 8192, 8191]
    return [random_bow(rng, int(n), n_words) for n in sizes]


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 1000, 20000])
def test_scores_equal_host_arithmetic_byte_for_byte(gpu_handle, pkg, N):
    bows = mixed_database(1, N)
    db = pkg.KeyFrameDatabase(gpu_handle)
    ids = np.random.default_rng(N).permutation(3 * N)[:N].astype(np.uint64) + np.uint64(1 << 40) * np.uint64(N % 2)    # ids beyond 32 bits too
    for i in range(N):
        db.add(ids[i], bows[i], i % 3)
    assert len(db) == N
    rng = np.random.default_rng(77)
    queries = [random_bow(rng, 1000, 20000)]
    if N in (65, 1000):
        queries += [random_bow(rng, 8192, 20000), (np.zeros(0, np.uint32), np.zeros(0)), random_bow(rng, 1, 20000)]
    order = np.argsort(ids)
    for qw, qv in queries:
        for scoring in (S.L1, S.DOT):
            gi, gs = db.score((qw, qv), scoring)
            assert np.array_equal(gi, ids[order])
            if scoring == S.L1:
                want = np.array([lib_bow_score(pkg, qw, qv, *bows[i]) for i in order], np.float64)
            else:
                want = np.array([S.dot_score(qw, qv, *bows[i]) for i in order], np.float64)
            bad = np.flatnonzero(gs.view(np.uint64) != want.view(np.uint64))
            assert len(bad) == 0, (N, scoring, len(qw), len(bad), bad[:5], gs[bad[:5]], want[bad[:5]])
    db.close()


# ---- the two searches ---------------------------------------------------------------------------------------------------------------
CONFIGS = [dict(), dict(min_score_ratio=0.5), dict(min_score_ratio=1.0), dict(min_covisibles_for_threshold=2), dict(max_covisibles_to_check=3),
           dict(max_covisibles_to_check=20, min_covisibles_for_threshold=12), dict(min_temporal_gap=5), dict(min_temporal_gap=0),
           dict(consistency_threshold=7)]


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_loop_candidates_equal_restatement(gpu_handle, pkg, name):
    d, queries = SC.load(pkg, name)
    db, sdb = fill(pkg, gpu_handle, d), SC.spec_database(d)
    found = 0
    for ci, cfg_kw in enumerate(CONFIGS):
        for q in (queries if ci == 0 else queries[::3]):
            for scoring in ((S.L1, S.DOT) if ci < 2 else (S.L1,)):
                found += assert_loop_equals_spec(db, sdb, d, q, cfg_kw, scoring, SC.CAP, pkg)
    assert found > 100
    for q in queries[:6]:                                               # a cap that holds every candidate, and none
        n = assert_loop_equals_spec(db, sdb, d, q, {}, S.L1, len(d["ids"]), pkg)
        ids, sc, total = db.detect_loop_candidates(q, d["connected"][q], cap=0)
        assert len(ids) == 0 and total == n
    db.close()


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_detect_candidates_equal_restatement(gpu_handle, pkg, name):
    d, queries = SC.load(pkg, name)
    db, sdb = fill(pkg, gpu_handle, d), SC.spec_database(d)
    N = len(d["ids"])
    nonempty = 0
    for q in queries[::4]:
        w, v = d["words"][q], d["weights"][q]
        for exclude in (None, 0, 1, 5):
            for max_results in (0, 1, 10, N + 7):
                ids, maps, sc = db.detect_candidates((w, v), exclude, max_results)
                want = sdb.detect_candidates(w, v, exclude, max_results)
                assert [int(i) for i in ids] == [c[0] for c in want], (q, exclude, max_results)
                assert [int(m) for m in maps] == [c[1] for c in want]
                assert sc.tobytes() == np.array([c[2] for c in want], np.float64).tobytes()
                nonempty += len(want) > 0
    assert nonempty > 20
    ids, _, _ = db.detect_candidates((np.zeros(0, np.uint32), np.zeros(0)), None, 10)      # an empty query shares no word
    assert len(ids) == 0
    db.close()


# ---- batches, insertion orders, histories -------------------------------------------------------------------------------------------
def test_batch_equals_single_calls(gpu_handle, pkg):
    d, queries = SC.load(pkg, "loop_b")
    db = fill(pkg, gpu_handle, d)
    single = loop_bytes(db, d, queries)
    assert sum(len(s) > 4 for s in single) > len(queries) // 2
    unknown = 10 ** 9
    for Q in (1, 7, 64):
        qs = [queries[(5 * i) % len(queries)] for i in range(Q)]
        if Q > 1:
            qs[1] = unknown                                            # an unknown current id inside a batch: no candidates, the others untouched
        ids, sc, cnt = db.detect_loop_candidates_batch(qs, [d["connected"][q] if q != unknown else [] for q in qs], cap=SC.CAP)
        for i, q in enumerate(qs):
            if q == unknown:
                assert cnt[i] == 0
                continue
            m = min(int(cnt[i]), SC.CAP)
            assert struct.pack("<i", int(cnt[i])) + ids[i, :m].tobytes() + sc[i, :m].tobytes() == single[queries.index(q)], (Q, i, q)
    for scoring in (S.L1, S.DOT):                                      # two runs give the same bytes
        assert loop_bytes(db, d, queries, None, scoring) == loop_bytes(db, d, queries, None, scoring)
    db.close()


def test_results_do_not_depend_on_how_the_database_was_filled(gpu_handle, pkg):
    d, queries = SC.load(pkg, "loop_a")
    N = len(d["ids"])
    base = fill(pkg, gpu_handle, d)
    want = loop_bytes(base, d, queries)
    want_dot = loop_bytes(base, d, queries, None, S.DOT)
    w0, v0 = d["words"][queries[0]], d["weights"][queries[0]]
    want_score = [a.tobytes() for a in base.score((w0, v0))]
    want_reloc = [a.tobytes() for a in base.detect_candidates((w0, v0), None, 25)]
    rng = np.random.default_rng(4)

    def check(db, what):
        assert loop_bytes(db, d, queries) == want, what
        assert loop_bytes(db, d, queries, None, S.DOT) == want_dot, what
        assert [a.tobytes() for a in db.score((w0, v0))] == want_score, what
        assert [a.tobytes() for a in db.detect_candidates((w0, v0), None, 25)] == want_reloc, what
        assert len(db) == N

    shuffled = fill(pkg, gpu_handle, d, rng.permutation(N))             # another insertion order
    check(shuffled, "shuffled")
    half = rng.permutation(N)[:N // 2]                                  # half erased and re-added (tombstones, then compaction at a query)
    for i in half:
        shuffled.erase(d["ids"][i])
    shuffled.erase(12345678)                                            # absent: not an error
    assert len(shuffled) == N - len(half) and shuffled.sizes()[1] == N
    for i in half[::-1]:
        shuffled.add(d["ids"][i], (d["words"][i], d["weights"][i]), d["maps"][i], d["bad"][i])
    check(shuffled, "erased and re-added")
    shuffled.compact()
    assert shuffled.sizes() == (N, N)
    check(shuffled, "compacted")
    junk = pkg.KeyFrameDatabase(gpu_handle)                             # every entry first added as something else, then replaced by add
    for i in range(N):
        j = (i + 37) % N
        junk.add(d["ids"][i], (d["words"][j], d["weights"][j]), 1 - d["maps"][i], not d["bad"][i])
    for i in rng.permutation(N):
        junk.add(d["ids"][i], (d["words"][i], d["weights"][i]), d["maps"][i], d["bad"][i])
    assert junk.sizes() == (N, 2 * N)
    check(junk, "replaced")
    flagged = fill(pkg, gpu_handle, dict(d, bad=np.zeros(N, bool)))     # the bad flag set afterwards
    for i in np.flatnonzero(d["bad"]):
        flagged.set_bad(d["ids"][i], True)
    check(flagged, "set_bad")
    for db in (base, shuffled, junk, flagged):
        db.close()


# ---- add_device ---------------------------------------------------------------------------------------------------------------------
def test_add_device_takes_bow_vectors_device_outputs(gpu_handle, pkg):
    import torch
    h = gpu_handle
    voc = pkg.synth.vocabulary(5, k=8, depth=3)
    gv = pkg.OrbVocabulary.from_nodes(*voc, 8, 3, handle=h)
    rng = np.random.default_rng(9)
    host_db, dev_db = pkg.KeyFrameDatabase(h), pkg.KeyFrameDatabase(h)
    sizes = [0, 1, 37, 500, 2000, 8192, 300]
    descs = []
    for kid, n in enumerate(sizes):
        base = voc[2][rng.integers(1, len(voc[2]), n)]                  # node descriptors with a few bits flipped
        desc = base ^ (rng.random((n, 32)) < 0.03).astype(np.uint8) if n else np.zeros((0, 32), np.uint8)
        descs.append(np.ascontiguousarray(desc, np.uint8))
        bw, bv, _fn, _fs, _fi = gv.vectors_arrays(descs[-1], 2)
        host_db.add(kid, (bw, bv), kid % 2, kid == 3)
    h._after_torch()
    for kid, n in enumerate(sizes):
        t = torch.from_numpy(descs[kid].reshape(-1, 32).copy() if n else np.zeros((1, 32), np.uint8)).to("cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(h._ext_stream):
            torch.cuda._sleep(50_000_000)                               # the handle's stream is busy while the two calls below are made
        r = gv.vectors_device(t, n, 2)
        dev_db.add_device(kid, r["bow_word"], r["bow_weight"], r["counts"], n, kid % 2, kid == 3)
        assert not h._ext_stream.query(), "add_device waited for the stream"
    h.synchronize()
    for kid in range(len(sizes)):
        a, b = host_db.download(kid), dev_db.download(kid)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2:] == b[2:], kid
        if sizes[kid] > 1:
            assert len(a[0]) > 1
    q = host_db.download(3)[:2]
    for scoring in (S.L1, S.DOT):
        assert [x.tobytes() for x in host_db.score(q, scoring)] == [x.tobytes() for x in dev_db.score(q, scoring)]
    conn = [[4, 6], [2]]
    cfg = pkg.LoopDetectorConfig(min_covisibles_for_threshold=1, min_temporal_gap=1)
    ra = host_db.detect_loop_candidates_batch([2, 4], conn, cfg, cap=8)
    rb = dev_db.detect_loop_candidates_batch([2, 4], conn, cfg, cap=8)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb))
    dev_db.add_device(1, r["bow_word"], r["bow_weight"], r["counts"], sizes[-1], 1, False)      # replace an entry from the device ...
    h.synchronize()
    assert dev_db.sizes() == (len(sizes), len(sizes) + 1)
    dev_db.compact()                                                    # ... and compact: every entry shrinks to its device-given size
    assert dev_db.sizes() == (len(sizes), len(sizes))
    for kid in range(len(sizes)):
        a, b = host_db.download(6 if kid == 1 else kid), dev_db.download(kid)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), kid
    host_db.close(); dev_db.close(); gv.close()


# ---- filters, each alone ------------------------------------------------------------------------------------------------------------
def small_scene():
    """Keyframes 0..79 that all hold nearly the same BowVector (every pair scores high), so that what a filter removes is visible."""
    rng = np.random.default_rng(8)
    w = np.arange(0, 400, 2, dtype=np.uint32)
    base = rng.uniform(0.5, 1.5, len(w))
    bows = []
    for _ in range(80):
        v = base * rng.uniform(0.97, 1.03, len(w))
        bows.append((w, v / v.sum()))
    return bows


def test_filters_each_alone(gpu_handle, pkg):
    bows = small_scene()
    cur, gap = 70, 30
    conn = [70, 69, 68, 67, 66, 71]
    cfg = pkg.LoopDetectorConfig()

    def run(mutate=None, connected=conn, current=cur, config=cfg):
        db, sdb = pkg.KeyFrameDatabase(gpu_handle), S.Database()
        maps, bad = [0] * 80, [False] * 80
        if mutate:
            mutate(maps, bad)
        for i, (w, v) in enumerate(bows):
            db.add(i, (w, v), maps[i], bad[i]); sdb.add(i, w, v, maps[i], bad[i])
        ids, sc, total = db.detect_loop_candidates(current, connected, config, cap=80)
        c = dict(S.DEFAULTS, min_temporal_gap=config.min_temporal_gap)
        want = sdb.detect_loop_candidates(current, connected, c)
        assert total == len(want) and [int(i) for i in ids] == [x[0] for x in want]
        assert sc.tobytes() == np.array([x[1] for x in want]).tobytes()
        db.close()
        return set(int(i) for i in ids)

    everything = run()
    assert everything == set(range(0, cur - gap + 1))                  # gap exactly min_temporal_gap is in, min_temporal_gap - 1 is out
    assert cur - gap in everything and cur - gap + 1 not in everything
    assert run(lambda m, b: b.__setitem__(7, True)) == everything - {7}                    # a bad entry
    assert run(lambda m, b: m.__setitem__(9, 1)) == everything - {9}                       # an entry of another map
    assert run(connected=conn + [11]) == everything - {11}                                 # a connected entry
    assert run(connected=[999] + conn) == everything                                       # an id in connected[] that is not an entry
    assert run(connected=[69, 69, 69, 69, 69]) == everything                               # duplicates count again: five scored -> a threshold
    assert run(connected=[69, 69, 69, 69]) == set()                                        # four scored: threshold 0
    assert run(current=500) == set()                                                       # the current id unknown
    assert run(config=pkg.LoopDetectorConfig(min_temporal_gap=31)) == everything - {40}
    # a bad keyframe and one of another map among connected[]: the bad one is scored for the threshold, the other is skipped
    assert run(lambda m, b: (b.__setitem__(69, True), m.__setitem__(68, 1)), connected=[69, 68, 67, 66, 65, 64]) == everything
    assert run(lambda m, b: m.__setitem__(68, 1), connected=[69, 68, 67, 66, 65]) == set()


def test_bad_arguments_leave_the_database_usable(gpu_handle, pkg):
    bows = small_scene()[:10]
    db = pkg.KeyFrameDatabase(gpu_handle)
    for i, b in enumerate(bows):
        db.add(i, b)
    before = [a.tobytes() for a in db.score(bows[0])]
    w, v = bows[0]
    bad_w = w.copy(); bad_w[5] = bad_w[4]
    cases = [lambda: db.add(3, (bad_w, v)), lambda: db.add(3, (w[::-1].copy(), v)), lambda: db.add(3, (w, v), map_idx=-1),
             lambda: db.add(3, (np.arange(8193, dtype=np.uint32), np.ones(8193))), lambda: db.score((bad_w, v)), lambda: db.score((w, v), 2),
             lambda: db.detect_candidates((bad_w, v)), lambda: db.detect_candidates((w, v), None, -1),
             lambda: db.detect_loop_candidates(0, [1, 2], cap=-1), lambda: db.detect_loop_candidates(0, [1, 2], scoring=7),
             lambda: db.detect_loop_candidates(0, [1, 2], pkg.LoopDetectorConfig(min_temporal_gap=-1)),
             lambda: db.detect_loop_candidates(0, [1, 2], pkg.LoopDetectorConfig(max_covisibles_to_check=-3)),
             lambda: db.detect_loop_candidates(0, [1, 2], pkg.LoopDetectorConfig(min_score_ratio=float("nan"))),
             lambda: db.set_bad(99), lambda: db.download(99), lambda: db.add_device(3, 0, 0, 0, 10)]
    for i, c in enumerate(cases):
        with pytest.raises(pkg.OrbxError) as e:
            c()
        assert e.value.code == -1, i
    L = pkg.load_library()
    off = np.array([0, 2, 1], np.int32); cur = np.zeros(2, np.uint64); conn = np.zeros(2, np.uint64)
    ids = np.zeros((2, 4), np.uint64); sc = np.zeros((2, 4)); cnt = np.zeros(2, np.int32)
    cfg = pkg.LoopDetectorConfig()._c()
    import ctypes as C
    args = lambda o: (db._p, C.byref(cfg), 0, 2, cur.ctypes.data, o.ctypes.data, conn.ctypes.data, 4, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data)
    assert L.orbx_kfdb_detect_loop_candidates_batch(*args(off)) == -1                       # offsets that do not ascend
    assert L.orbx_kfdb_detect_loop_candidates_batch(*args(np.array([1, 2, 2], np.int32))) == -1
    one = C.c_int()
    assert L.orbx_kfdb_score(db._p, 0, w.ctypes.data, v.ctypes.data, len(w), ids.ctypes.data, sc.ctypes.data, 3, C.byref(one)) == -4 and one.value == 10
    assert len(db) == 10 and [a.tobytes() for a in db.score(bows[0])] == before
    db.close()


# ---- the compiled caller ------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_equals_python(gpu_handle, pkg, tmp_path):
    exe = os.path.join(tmp_path, "kfdb_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "kfdb_driver.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lorbx_hip", "-Wl,-rpath," + LIBDIR], check=True)
    d, queries = SC.load(pkg, "loop_a")
    N = len(d["ids"])
    db = fill(pkg, gpu_handle, d)
    fin, fout = os.path.join(tmp_path, "in.bin"), os.path.join(tmp_path, "out.bin")
    reloc = [(None, 10, queries[0]), (1, 500, queries[1]), (0, 0, queries[2])]
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", N))
        for i in range(N):
            f.write(struct.pack("<Qiii", int(d["ids"][i]), int(d["maps"][i]), int(d["bad"][i]), len(d["words"][i])))
            f.write(d["words"][i].tobytes()); f.write(d["weights"][i].tobytes())
        f.write(struct.pack("<i", 2 * len(queries)))
        for scoring in (S.L1, S.DOT):
            for q in queries:
                f.write(struct.pack("<Qii", q, scoring, len(d["connected"][q]))); f.write(np.array(d["connected"][q], np.uint64).tobytes())
        f.write(struct.pack("<i", len(reloc)))
        for ex, mr, q in reloc:
            f.write(struct.pack("<iii", -1 if ex is None else ex, mr, len(d["words"][q]))); f.write(d["words"][q].tobytes()); f.write(d["weights"][q].tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=300)
    want = b""
    some = 0
    for scoring in (S.L1, S.DOT):
        for q in queries:
            ids, sc, total = db.detect_loop_candidates(q, d["connected"][q], None, scoring, cap=N)
            want += struct.pack("<i", total) + b"".join(struct.pack("<Qd", int(i), float(s)) for i, s in zip(ids, sc))
            some += total
    for ex, mr, q in reloc:
        ids, maps, sc = db.detect_candidates((d["words"][q], d["weights"][q]), ex, mr)
        want += struct.pack("<i", len(ids)) + b"".join(struct.pack("<Qid", int(i), int(m), float(s)) for i, m, s in zip(ids, maps, sc))
        some += len(ids)
    assert some > 50
    assert open(fout, "rb").read() == want + b"\x01"
    db.close()
