"""The device line of ``heads.object_movement_mine_pairs`` (MSPA_TRACK_MINING=device) without a GPU: the switch, the draws made
from counts alone (``heads.plan_track_draws``) over a NumPy stand-in for the four K5d calls (tests/track_mining_util.py) against
the oracle's list-and-loop form and the host line, and every decline."""
import random

import numpy as np
import pytest

import track_mining_util as U
from mspa import _lib, engine, heads
from oracle import np_oracle as O

ARGSETS = ((1, 1, False, 0.3), (15, 30, True, 0.05), (5, 1e8, True, 1.0), (6, 3, True, 0.5))
BLOCKS = [(seed, T) for seed, T in zip(range(12), (3, 4, 5, 7, 9, 12, 16, 21, 27, 33, 38, 40))]


def distance_fn(world):
    def fn(points, frames):
        out = []
        for p, fr in zip(points, frames):
            ii, jj = np.triu_indices(len(fr), 1)
            out.append(np.linalg.norm(world[fr[jj], p] - world[fr[ii], p], axis=1))
        return out
    return fn


def key(s):
    return int(s["point_index"]), int(s["frame1"]), int(s["frame2"])


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(heads, "TRACK_MINING_BACKEND", U)
    monkeypatch.setenv("MSPA_TRACK_MINING", "device")
    return U


def host_line(monkeypatch, vis, groups, world, args, seed, **kw):
    with monkeypatch.context() as m:
        m.delenv("MSPA_TRACK_MINING", raising=False)
        rng = random.Random(seed)
        groups = [list(g) for g in groups]
        got = heads.object_movement_mine_pairs(vis, groups, distance_fn(world), *args, rng, **kw)
        assert heads.LAST_TRACK_MINING["path"] == "host"
    return got, rng.getstate(), groups


def test_the_switch(monkeypatch):
    monkeypatch.delenv("MSPA_TRACK_MINING", raising=False)
    assert engine.track_mining_backend() == "host"
    for value, want in (("device", "device"), (" Device ", "device"), ("host", "host"), ("", "host")):
        monkeypatch.setenv("MSPA_TRACK_MINING", value)
        assert engine.track_mining_backend() == want                      # read at every call
    for value in ("gpu", "1", "on"):
        monkeypatch.setenv("MSPA_TRACK_MINING", value)
        with pytest.raises(ValueError, match="MSPA_TRACK_MINING"):
            engine.track_mining_backend()
        with pytest.raises(ValueError, match="MSPA_TRACK_MINING"):
            heads.object_movement_mine_pairs(np.zeros((2, 1), bool), [[0]], None)


def test_library_has_the_four_entry_points():
    names = _lib.exported_symbols()
    for name in ("mspa_track_pair_stats", "mspa_track_pair_bin_counts", "mspa_track_pair_order", "mspa_track_pair_resolve"):
        assert name in names
    assert (_lib.TRACK_STAT_WORDS, _lib.TRACK_CLASS_STATIC, _lib.TRACK_MAX_FRAMES) == (6, heads.TRACK_CLASS_STATIC, heads.TRACK_MAX_FRAMES)
    assert engine.TRACK_MINING_BUDGET_BYTES == U.TRACK_MINING_BUDGET_BYTES == 1 << 30


def test_the_blocks_hold_their_hard_cases():
    world, vis, groups = U.make_block(5, 12)
    assert sorted(p for g in groups for p in g) == list(range(24)) and len(groups) == 3
    st = U.track_pair_stats(world, vis, np.arange(24))["stats"]
    assert st[1, 0] == 0 and st[2, 0] == 1                                # visible in 0 frames and in 1
    assert st[0, 1] > 0 and st[4, 2] == 0 and st[4, 1] == st[4, 0] * (st[4, 0] - 1) // 2
    assert st[3, 2] > 0 and st[3, 3] == st[3, 4]                          # every moving distance of point 3 is the same
    _f, _i, _j, d, _s, moving = U.point_pairs(world, vis, 7)
    assert len(np.unique(d[moving])) < moving.sum()                       # ties among moving pairs


@pytest.mark.parametrize("args", ARGSETS, ids=[str(a) for a in ARGSETS])
@pytest.mark.parametrize("seed,T", BLOCKS)
def test_device_line_equals_oracle_and_host_line(stand_in, monkeypatch, seed, T, args):
    world, vis, base = U.make_block(seed, T)
    want_rng, want_groups = random.Random(seed + 100), [list(g) for g in base]
    want = O.mine_frame_pairs(world, vis, want_groups, *args, want_rng)
    host, host_state, host_groups = host_line(monkeypatch, vis, base, world, args, seed + 100)
    rng, groups = random.Random(seed + 100), [list(g) for g in base]
    got = heads.object_movement_mine_pairs(vis, groups, None, *args, rng, world=world)
    assert heads.LAST_TRACK_MINING == {"path": "device", "reason": ""}
    assert [key(s) for s in got] == [key(s) for s in want] == [key(s) for s in host]
    assert rng.getstate() == want_rng.getstate() == host_state
    assert groups == want_groups == host_groups
    if T >= 5:
        assert len(got) > 0


def test_drop_test_and_thresholds_reach_the_device_line(stand_in, monkeypatch):
    world, vis, base = U.make_block(3, 30)
    kw = dict(object_not_moving_threshold=0.05, future_frame_windows=5.0)
    host, host_state, host_groups = host_line(monkeypatch, vis, base, world, (6, 3, True, 0.5), 7, **kw)
    _f, ii, _jj, d, static, moving = U.point_pairs(world, vis, 7, 0.05, 5.0)
    assert (static | moving).sum() < len(d)                               # the window drops pairs here
    rng, groups = random.Random(7), [list(g) for g in base]
    got = heads.object_movement_mine_pairs(vis, groups, None, 6, 3, True, 0.5, rng, world=world, **kw)
    assert heads.LAST_TRACK_MINING["path"] == "device"
    assert [key(s) for s in got] == [key(s) for s in host] and rng.getstate() == host_state and groups == host_groups


def test_plan_track_draws_makes_upstreams_calls_in_order():
    class Log(random.Random):
        def __init__(self):
            super().__init__(0)
            self.calls = []

        def shuffle(self, x):
            self.calls.append(("shuffle", len(x)))
            super().shuffle(x)

        def choice(self, seq):
            self.calls.append(("choice", len(seq)))
            return super().choice(seq)

        def sample(self, population, k, **kw):
            self.calls.append(("sample", len(population), k))
            return super().sample(population, k, **kw)

    stats = {0: (5, 3, [4, 0, 0, 0, 2, 0, 0, 0, 0, 4]), 1: (1, 0, [0] * 10), 2: (4, 0, [6] + [0] * 9), 3: (3, 3, [0] * 10)}
    rng = Log()
    groups = [[0, 1], [2, 3]]
    picks, swaps = heads.plan_track_draws(groups, stats, 2, 3, True, 0.5, rng)
    # point 0: bin 4 holds 2 -> npairs_per_bin = 2, carried over to point 2; bins of 4 and of 6 are sampled, the bin of 2 is not
    per_point = {0: [("choice", 3), ("sample", 4, 2), ("sample", 4, 2)], 1: [], 2: [("sample", 6, 1)], 3: [("choice", 3)]}
    want = []
    for g in groups:                                                      # as shuffled
        want.append(("shuffle", 2))
        for p in g:
            want.extend(per_point[p])
    # point 2 has an empty bin 4: npairs_per_bin = max(min(0, 2), 1) = 1
    assert rng.calls == want + [("sample", len(picks), len(picks) // 2)]
    assert sorted(c for p, c, _r in picks if p == 0) == [0, 0, 4, 4, 9, 9, 10] and len(swaps) == len(picks) // 2


DECLINES = ("T", "nonfinite", "budget", "empty", "empty lists", "no world")


@pytest.mark.parametrize("what", DECLINES)
def test_every_decline_runs_the_host_line_with_the_generator_untouched(stand_in, monkeypatch, what):
    world, vis, base = U.make_block(2, 14)
    given, text = world, None
    if what == "T":
        vis, base = np.zeros((65536, 2), bool), [[0, 1]]                  # nothing is visible: the host line computes no distance
        given = world = np.zeros((65536, 2, 3))
        text = "65535"
    elif what == "nonfinite":
        world[3, base[1][0]] = np.nan
        vis[3, base[1][0]] = vis[4, base[1][0]] = True
        text = "non-finite"
    elif what == "budget":
        monkeypatch.setattr(U, "TRACK_MINING_BUDGET_BYTES", 24 * 20)
        text = "budget"
    elif what == "empty":
        base, text = [], "empty groups"
    elif what == "empty lists":
        base, text = [[], []], "empty groups"
    else:
        given, text = None, "no device world"

    class Counting(random.Random):
        draws = 0

        def random(self):
            Counting.draws += 1
            return super().random()

        def getrandbits(self, k):
            Counting.draws += 1
            return super().getrandbits(k)

    seen = []
    real = heads._mine_pairs_device

    def watched(*a):
        before = Counting.draws
        r = real(*a)
        seen.append((r, Counting.draws - before))
        return r
    monkeypatch.setattr(heads, "_mine_pairs_device", watched)
    rng, groups = Counting(11), [list(g) for g in base]

    def run():
        return heads.object_movement_mine_pairs(vis, groups, distance_fn(world), 6, 3, True, 0.5, rng, world=given)
    if what == "nonfinite":                                               # upstream's histogram_bin_edges raises; so does the host line
        try:
            host_line(monkeypatch, vis, base, world, (6, 3, True, 0.5), 11)
            raised = None
        except ValueError as e:
            raised = e
        if raised is not None:
            with pytest.raises(ValueError):
                run()
            got = None
        else:
            got = run()
    else:
        got = run()
    assert heads.LAST_TRACK_MINING["path"] == "host" and text in heads.LAST_TRACK_MINING["reason"]
    if what != "no world":
        assert len(seen) == 1 and isinstance(seen[0][0], str) and seen[0][1] == 0      # declined, and no draw was consumed
    if got is not None:
        host, host_state, host_groups = host_line(monkeypatch, vis, base, world, (6, 3, True, 0.5), 11)
        assert [key(s) for s in got] == [key(s) for s in host] and rng.getstate() == host_state and groups == host_groups


def test_a_wrong_rank_is_refused_by_the_stand_in_as_by_the_library():
    world, vis, _ = U.make_block(1, 8)
    state = U.track_pair_stats(world, vis, np.array([5]))
    edges = np.stack([U.point_edges(r) for r in state["stats"]])
    counts = U.track_pair_bin_counts(state, edges)
    classes = np.concatenate([counts, state["stats"][:, 1:2]], axis=1)
    seg = np.array([0, state["stats"][0, 2]])
    _k, payload = U.track_pair_order(state, [0], seg, int(seg[1]))
    with pytest.raises(U.Refused):
        U.track_pair_resolve(state, counts, [0], seg, payload, [(0, 0, int(classes[0, 0]))], classes)
