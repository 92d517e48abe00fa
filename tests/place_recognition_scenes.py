"""The parity scenes of the place-recognition tests: synth.bow_database trajectories with a revisited stretch, duplicates (score ties),
a second map, bad keyframes and keyframes with too few connected ones, and the queries asked of them.  test_place_recognition_cpu.py
proves on the restatement alone that each scene exercises every outcome; test_place_recognition_gpu.py compares the device with it."""
import place_recognition_spec as S

CAP = 3          # candidates returned per query on these scenes: small, so that some queries have more

SCENES = {
    # name: (bow_database arguments, queries)
    "loop_a": (dict(seed=3, n_keyframes=160, words_per_kf=160, n_words=5000, revisit=(100, 40, 20), n_duplicates=6, other_map_every=17,
                    bad_every=23, short_lists_every=9), list(range(100, 140)) + [0, 5, 50, 60, 99, 145, 150, 159]),
    "loop_b": (dict(seed=11, n_keyframes=220, words_per_kf=240, n_words=20000, revisit=(150, 60, 40), n_duplicates=9, other_map_every=13,
                    bad_every=19, short_lists_every=7, reach=7), list(range(150, 210)) + [1, 30, 90, 149, 215, 219]),
}


def load(pkg, name):
    args, queries = SCENES[name]
    d = pkg.synth.bow_database(**args)
    return d, queries


def spec_database(d, order=None):
    db = S.Database()
    for i in (order if order is not None else range(len(d["ids"]))):
        db.add(d["ids"][i], d["words"][i], d["weights"][i], d["maps"][i], d["bad"][i])
    return db


def outcome(db, d, q, cfg=None, scoring=S.L1):
    """What the restatement says about query q: (threshold, scored, ordered candidates)."""
    c = dict(S.DEFAULTS, **(cfg or {}))
    thr, checked = db.min_score(q, d["connected"][q], c, scoring)
    return thr, checked, db.detect_loop_candidates(q, d["connected"][q], c, scoring)
