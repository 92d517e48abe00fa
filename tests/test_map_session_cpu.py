"""The session model (tests/map_session_spec.py) over the session scenes (tests/map_session_scenes.py), without a GPU: invariants after
every call, the composed model against a dict-based host map driven by the literal replays the specifications ship, what a session
has to reach before it tests anything, and a forgetful model that shows recycling is exercised.  Prints per seed the per-step
counts, the chosen CAPACITY and how many fuse passes met map_fuse_spec.reference_replay's agreement conditions."""
import numpy as np
import pytest

import covisibility_spec as CS
import map_create_spec as MC
import map_fuse_spec as FS
import map_observations_spec as OSP
import map_session_scenes as W
import map_session_spec as S

_runs = {}


class HostMap:
    """kf_points[g] = {feature: map point} per keyframe of the session, driven beside the model by create_replay, remove_replay, a
    literal observer count for culling, associate_replay and cull_keyframes_replay; fuse is replayed by reference_replay at the
    passes that meet its agreement conditions and taken from the model elsewhere.  Checks the invariants after every call."""

    def __init__(self, n):
        self.kf_points = [{} for _ in range(n)]
        self.agreeing, self.passes, self.calls = 0, 0, 0

    def _tables(self, m, where=None):
        out = []
        for p in (range(len(m.listed)) if where is None else where):
            g = m.listed[p]
            t = np.full(m.counts[g], -1, np.int32)
            for i, s in self.kf_points[g].items():
                t[i] = s
            out.append(t)
        return out

    def _take(self, m, kp, where=None):
        for p, d in zip(range(len(m.listed)) if where is None else where, kp):
            self.kf_points[m.listed[p]] = dict(d)

    def track(self, m, want):
        assert want["record"]["n_correspondences"] == len(want["gathered"]["mp_idx"])

    def table(self, m, want):
        self.kf_points[want["g"]] = MC.tables_as_points([want["table"]], m.live)[0]

    def neighbours(self, m, want):
        t = self._tables(m)
        assert all(len(set(d.values())) == len(d) for d in (self.kf_points[g] for g in m.listed))      # every point once per keyframe: the replay applies
        assert CS.associate_replay(t, m.live)[want["cur"]].tobytes() == want["weights"].tobytes()

    def create(self, m, want):
        order = want["order"]
        cur, nbs = m._keyframe(m.listed[order[0]]), [m._keyframe(m.listed[i]) for i in order[1:]]
        kp = MC.create_replay(cur, nbs, self._tables(m, order), m.live, want["free_slots"], want["created_pairs"])
        assert kp == MC.tables_as_points(want["tables"], MC.live_after(m.live, want))
        assert not m.live[want["free_slots"]].any() and not set(want["free_slots"].tolist()) & {s for g in m.listed for s in self.kf_points[g].values()}
        self._take(m, kp, order)

    def cull(self, m, want):
        seen = {}
        for g in m.listed:
            for s in set(self.kf_points[g].values()):
                seen[s] = seen.get(s, 0) + 1
        culled = [int(s) for s in want["cand"] if seen.get(int(s), 0) < W.CULL_MIN_OBS]
        assert culled == want["culled"].tolist() and m.live[want["cand"]].all() and len(set(want["cand"].tolist())) == len(want["cand"])
        self._take(m, MC.remove_replay([self.kf_points[g] for g in m.listed], culled))

    def fuse(self, m, want):
        cur, nb = want["cur"], want["nb"]
        search = m.search()
        for r, before, src, tgt in ((want["a"], want["tables_before"], [cur], nb), (want["b"], FS.Tables(want["a"]["tables"], want["tables_before"].counts), nb, [cur])):
            self.passes += 1
            if S.agrees(r, len(tgt)):
                self.agreeing += 1
                tabs, removed, fused, added = FS.reference_replay(before, m.live, m.positions, m.desc, src, tgt, search)
                assert all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(r["tables"], tabs))
                assert sorted(removed) == r["goner"].tolist() and fused == r["counts"][3] and added == r["counts"][2]
        assert not OSP.n_observers(want["tables"], m.live)[np.concatenate([want["a"]["goner"], want["b"]["goner"]]).astype(np.int64)].any()
        self._take(m, MC.tables_as_points(want["tables"], want["live"]))

    def ba(self, m, want):
        pass

    def remove(self, m, want):
        self._take(m, MC.remove_replay([self.kf_points[g] for g in m.listed], want["slots"]))

    def redundancy(self, m, want):
        kf_points = {p: [self.kf_points[g].get(i) for i in range(m.counts[g])] for p, g in enumerate(m.listed)}
        observers = {}
        for p, ids in kf_points.items():
            for s in ids:
                if s is not None:
                    observers.setdefault(s, set()).add(p)
        got = OSP.cull_keyframes_replay(kf_points, observers, want["cand"].tolist(), W.KF_MIN_OBS, W.KF_THRESHOLD)
        assert [got[int(c)] for c in want["cand"]] == [(int(t), int(r), bool(c)) for t, r, c in zip(want["total"], want["redundant"], want["cull"])]

    def state(self, m, after):
        self.calls += 1
        assert [self.kf_points[g] for g in m.listed] == MC.tables_as_points(m.T(), m.live), after
        check_invariants(m)


def check_invariants(m):
    live = set(np.flatnonzero(m.live).tolist())
    free = set(m.free)
    assert len(free) == len(m.free) and not free & live and len(free) + len(live) == m.capacity
    named = {int(s) for g in m.listed if m.tables[g] is not None for s in m.tables[g].tolist() if s >= 0}
    assert not named & free
    assert len(live) == m.n_created - m.n_removed
    assert set(m.recent) <= live


def model_run(seed, oracle):
    """the model alone over a whole session with the host map beside it; computed once per seed -> (model, host map)"""
    if seed not in _runs:
        h = HostMap(W.N_KF)
        _runs[seed] = (S.run(W.session(seed), oracle, dev=h), h)
    return _runs[seed]


def _line(seed, g, st):
    return "seed %d step %d: created %d dropped %d culled %d goners %d reused %d near-gate %d of %d BA iterations %d" % (
        seed, g, st["created"], st["dropped"], st["culled"], st["goners"], st["reused"], st["near"], st["evaluated"], st["ba_iterations"])


@pytest.mark.parametrize("seed", W.SEEDS)
def test_model_equals_the_replays_and_keeps_its_invariants(oracle, seed):
    m, h = model_run(seed, oracle)
    for g in range(W.N_KF):
        print(_line(seed, g, m.stats[g]))
    print("seed %d: CAPACITY %d, %d of %d fuse passes met the agreement conditions and were replayed, %d states compared" % (seed, W.CAPACITY, h.agreeing, h.passes, h.calls))
    assert h.calls == 2 + 7 * (W.N_KF - 1) and h.passes == 2 * (W.N_KF - 1)
    sizes = [m.counts[g] for g in range(W.N_KF)]
    assert sizes[W.BIG] == 1100 and sizes[W.EMPTY] == 0 and all(250 <= n <= 400 for g, n in enumerate(sizes) if g not in (W.BIG, W.EMPTY))


@pytest.mark.parametrize("seed", W.SEEDS)
def test_session_reaches_the_hazards(oracle, seed):
    m, _ = model_run(seed, oracle)
    st = [m.stats[g] for g in range(W.N_KF)]
    assert sum(s["reused_after"]["cull"] for s in st) >= 1                  # culled, then handed out again by creation
    assert sum(s["reused_after"]["fuse"] for s in st) >= 1                  # a fuse goner handed out again
    assert sum(1 for s in st if s["dropped"] > 0) >= 1                      # the free list ran short
    for p in (0, 1):
        assert sum(1 for s in st if s["fuse_counts"] and s["fuse_counts"][p][3] > 0) >= 2, p
    assert sum(1 for s in st if s["ba_iterations"] > 0) >= 3
    assert all(s["near"] <= 0.01 * max(s["evaluated"], 1) for s in st)
    assert sum(1 for s in st if s["evaluated"] > 0) >= 4                    # the neighbour phase has pairs to judge
    # a keyframe was flagged, left out, and its old table names a slot that creation handed out again afterwards
    assert len(m.unlisted) == W.MAX_UNLISTED
    u = m.unlisted[0]
    at = next(g for g in range(W.N_KF) if u in [m.trace[g]["listed"][p] for p in m.trace[g].get("redundancy", {}).get("drop", [])])
    later = {int(s) for g in range(at + 1, W.N_KF) for s in m.trace[g]["create"]["new_slot"]}
    print("seed %d: keyframe %d flagged redundant at step %d and left out; its table still names %d slots that creation handed out again" % (
        seed, u, at, len(later & set(m.tables[u].tolist()))))
    assert at < W.N_KF - 1 and later & set(m.tables[u].tolist())
    assert max(len(m.trace[g]["listed"]) for g in range(W.N_KF)) >= 8 and len(m.trace[1]["listed"]) == 2
    assert any(m.trace[g]["ba"] is None for g in range(1, W.N_KF)) and any(m.trace[g]["ba"] is not None and m.trace[g]["ba"]["counts"][1] > 1 for g in range(1, W.N_KF))


@pytest.mark.parametrize("seed", W.SEEDS)
def test_a_forgetful_model_goes_wrong_within_two_steps_of_the_first_reuse(oracle, seed):
    m, _ = model_run(seed, oracle)
    first = next(g for g in range(W.N_KF) if m.stats[g]["reused"] > 0)
    f = S.run(W.session(seed), oracle, cls=S.ForgetfulModel, steps=min(first + 3, W.N_KF))
    differs = [g for g in range(min(first + 3, W.N_KF)) if not _same_state(m.snap[g], f.snap[g])]
    print("seed %d: first reuse at step %d, the forgetful model differs from step %d" % (seed, first, differs[0] if differs else -1))
    assert differs and differs[0] <= first + 2


def _same_state(a, b):
    """what a reader of the two maps sees: the live bytes and, per listed keyframe, {feature: live slot}"""
    ta, tb = ([None if g not in x["listed"] else x["tables"][g] for g in range(W.N_KF)] for x in (a, b))
    return a["live"].tobytes() == b["live"].tobytes() and MC.tables_as_points(ta, a["live"]) == MC.tables_as_points(tb, b["live"])
