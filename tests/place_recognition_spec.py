"""Independent restatement of the place-recognition specification (include/orbx.h: orbx_kfdb_*): the two BoW scorings,
KeyFrameDatabase::detect_candidates (reference src/atlas/keyframe_db.rs:58-94) and detect_loop_candidates
(src/loop_closing/detector.rs:185-368), step by step in numpy / plain Python.

Test infrastructure only: the product never imports it.  A BowVector is a pair (ascending u32 word ids, f64 weights).  Every sum is
one left-to-right f64 chain in ascending word id: the `_merge` forms walk the two lists as orbx_bow_score does, the vectorised forms
lay the terms out in union order and add them with np.cumsum (a sequential accumulation, unlike np.sum's pairwise tree); the CPU
tests hold the two forms equal byte for byte.
"""
import numpy as np

L1, DOT = 0, 1
DEFAULTS = dict(min_score_ratio=0.75, consistency_threshold=3, min_covisibles_for_threshold=5, max_covisibles_to_check=10,
                min_temporal_gap=30)          # detector.rs:36-46


def _chain(terms):
    """0.0 + t0 + t1 + ... one add after another"""
    return float(np.cumsum(np.concatenate([[0.0], np.asarray(terms, np.float64)]))[-1])


def l1_score_merge(w1, v1, w2, v2):
    """OrbVocabulary::score (vocabulary/mod.rs:357-374) as orbx_bow_score fixes it."""
    a = b = 0
    n1, n2 = len(w1), len(w2)
    diff = 0.0
    while a < n1 or b < n2:
        if b >= n2 or (a < n1 and int(w1[a]) < int(w2[b])):
            diff += abs(float(v1[a]) - 0.0); a += 1
        elif a >= n1 or int(w2[b]) < int(w1[a]):
            diff += abs(float(v2[b])); b += 1
        else:
            diff += abs(float(v1[a]) - float(v2[b])); a += 1; b += 1
    return 1.0 - 0.5 * diff


def dot_score_merge(w1, v1, w2, v2):
    """keyframe_db.rs:73-79 / detector.rs:380-386 over the common words in ascending word id: product, then add."""
    a = b = 0
    n1, n2 = len(w1), len(w2)
    score = 0.0
    while a < n1 and b < n2:
        if int(w1[a]) < int(w2[b]):
            a += 1
        elif int(w2[b]) < int(w1[a]):
            b += 1
        else:
            score += float(v1[a]) * float(v2[b]); a += 1; b += 1
    return score


def _dense(w1, v1, w2, v2):
    w1 = np.asarray(w1, np.uint32); w2 = np.asarray(w2, np.uint32)
    u = np.union1d(w1, w2)
    x = np.zeros(len(u)); y = np.zeros(len(u))
    in1 = np.zeros(len(u), bool); in2 = np.zeros(len(u), bool)
    i1 = np.searchsorted(u, w1); i2 = np.searchsorted(u, w2)
    x[i1] = v1; y[i2] = v2; in1[i1] = True; in2[i2] = True
    return x, y, in1, in2


def l1_score(w1, v1, w2, v2):
    x, y, in1, in2 = _dense(w1, v1, w2, v2)
    terms = np.where(in1 & in2, np.abs(x - y), np.where(in1, np.abs(x - 0.0), np.abs(y)))
    return 1.0 - 0.5 * _chain(terms)


def dot_score(w1, v1, w2, v2):
    x, y, in1, in2 = _dense(w1, v1, w2, v2)
    both = in1 & in2
    return _chain(x[both] * y[both])


def score(scoring, w1, v1, w2, v2):
    return l1_score(w1, v1, w2, v2) if scoring == L1 else dot_score(w1, v1, w2, v2)


def _ordered(cands):
    """score descending; equal scores by ascending keyframe id (SPEC CHOICE: the reference's stable sort leaves them in HashMap order)"""
    return sorted(cands, key=lambda c: (-c[-1], c[0]))


class Database:
    """KeyFrameDatabase (keyframe_db.rs:31-95) plus the map's view of its keyframes (map index, is_bad) that detect_loop_candidates reads."""

    def __init__(self):
        self.entries = {}                       # id -> (words, weights, map, bad)

    def add(self, kf_id, words, weights, map_idx=0, is_bad=False):
        self.entries[int(kf_id)] = (np.asarray(words, np.uint32), np.asarray(weights, np.float64), int(map_idx), bool(is_bad))   # :45-47

    def erase(self, kf_id):
        self.entries.pop(int(kf_id), None)      # :50-52

    def detect_candidates(self, qw, qv, exclude_map=None, max_results=10):
        """keyframe_db.rs:58-94 -> [(id, map, score)]"""
        cands = []
        for kid, (w, v, m, _bad) in self.entries.items():
            if exclude_map is not None and m == exclude_map:
                continue
            s = dot_score(qw, qv, w, v)
            if s > 0.0:
                cands.append((kid, m, s))
        return _ordered(cands)[:max_results]

    def min_score(self, cur, connected, cfg, scoring):
        """compute_min_score (detector.rs:265-298) -> (threshold, number scored).  connected[] is walked as given."""
        qw, qv, qmap, _ = self.entries[int(cur)]
        best, checked = 0.0, 0
        for cid in connected:
            if checked >= cfg["max_covisibles_to_check"]:
                break
            e = self.entries.get(int(cid))
            if e is None or e[2] != qmap:       # map.get_keyframe: the current keyframe's map
                continue
            s = score(scoring, qw, qv, e[0], e[1])
            if s > best:
                best = s
            checked += 1
        if checked < cfg["min_covisibles_for_threshold"]:
            return 0.0, checked
        return best * cfg["min_score_ratio"], checked

    def detect_loop_candidates(self, cur, connected, cfg=None, scoring=L1):
        """detector.rs:185-368 -> all candidates [(id, score)], ordered."""
        cfg = dict(DEFAULTS, **(cfg or {}))
        if int(cur) not in self.entries:        # :195-198
            return []
        thr, _ = self.min_score(cur, connected, cfg, scoring)
        if thr < 0.01:                          # :212-215
            return []
        qw, qv, qmap, _ = self.entries[int(cur)]
        conn = set(int(c) for c in connected)
        out = []
        for kid, (w, v, m, bad) in self.entries.items():
            if m != qmap or kid in conn:        # :315-320
                continue
            if abs(int(cur) - kid) < cfg["min_temporal_gap"]:   # :323-331
                continue
            if bad:                             # :334
                continue
            s = score(scoring, qw, qv, w, v)
            if s >= thr:                        # :347
                out.append((kid, s))
        return _ordered(out)
