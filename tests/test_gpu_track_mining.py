"""K5d on the MI355X (csrc/track_mining.hip) against its NumPy restatement (tests/track_mining_util.py): the statistics and the
bin counts, the segmented sort on its own, the resolve of every (class, rank), then ``heads.object_movement_mine_pairs`` with
MSPA_TRACK_MINING=device against the host line -- list, generator state, shuffled groups -- and the callers end to end."""
import importlib
import io
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_mining_util as U  # noqa: E402
from jpeg_util import content  # noqa: E402

from mspa import _lib, engine, heads, synth  # noqa: E402

DEV = "cuda"
ARGSETS = ((1, 1, False, 0.3), (15, 30, True, 0.05), (5, 1e8, True, 1.0), (6, 3, True, 0.5))
VISIBLE = (0, 1, 2, 63, 64, 65, 257)
THRESHOLD_POINT, P = 23, 24


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stats_block(T, seed):
    """P = 24 points seen in 0, 1, 2, 63, 64, 65, 257 frames (as far as T allows), coordinates rounded to 0.01 (ties); the last
    point sits at the origin and, in its last visible frame, exactly 0.01 along x: a distance EQUAL to the threshold."""
    rng = np.random.default_rng(seed)
    world = np.round(np.cumsum(rng.normal(0, 0.03, (T, P, 3)), axis=0), 2)
    vis = np.zeros((T, P), dtype=bool)
    wanted = [v for v in VISIBLE if v <= T]
    for p in range(P):
        vis[rng.choice(T, wanted[p % len(wanted)], replace=False), p] = True
    world[:, THRESHOLD_POINT] = 0.0
    world[T - 1, THRESHOLD_POINT] = (0.01, 0.0, 0.0)
    vis[:, THRESHOLD_POINT] = False
    vis[[0, min(1, T - 1), T - 1], THRESHOLD_POINT] = True
    return world, vis


def device_stats(world, vis, points, thr, window):
    state = engine.track_pair_stats(dev(world), dev(vis.astype(np.uint8)), dev(np.asarray(points, dtype=np.int32)), thr, window)
    stats = state["stats"].cpu().numpy()
    edges = np.stack([U.point_edges(r) for r in stats])
    counts = engine.track_pair_bin_counts(state, dev(edges), thr, window)
    return state, stats, edges, counts


@pytest.mark.parametrize("T,window", [(2, 1e8), (3, 1e8), (64, 1e8), (65, 1e8), (130, 1e8), (300, 1e8), (65, 5.0)])
def test_statistics_and_bin_counts_equal_the_restatement(T, window):
    world, vis = stats_block(T, 100 + T)
    points = np.arange(P)
    state, stats, edges, counts = device_stats(world, vis, points, 0.01, window)
    want = U.track_pair_stats(world, vis, points, 0.01, window)
    assert np.array_equal(stats, want["stats"])                           # counts, and min / max as bits
    assert sorted(set(stats[:, 0].tolist())) == sorted(set(v for v in VISIBLE if v <= T) | {min(3, T)})
    frames = state["frames"].cpu().numpy()
    positions = state["positions"].cpu().numpy()
    for r in range(P):
        V = stats[r, 0]
        assert np.array_equal(frames[r, :V], want["frames"][r, :V])
        assert np.array_equal(positions[r, :V], world[want["frames"][r, :V], r])
    counts = counts.cpu().numpy()
    assert np.array_equal(counts, U.track_pair_bin_counts(want, edges, 0.01, window))
    assert np.array_equal(counts.sum(axis=1), stats[:, 2])
    # d == threshold is MOVING: (0, last) and, from T = 3 on, (1, last) of the point at the origin; (0, 1) is static
    t = stats[THRESHOLD_POINT]
    if window == 1e8:
        assert (t[1], t[2]) == ((1, 2) if T >= 3 else (0, 1))
        assert t[3] == t[4] == np.float64(0.01).view(np.int64)
    several = stats[:, 3] != stats[:, 4]
    several &= stats[:, 2] > 0
    assert (counts[several, 0] > 0).all() and (counts[several, 9] > 0).all()      # d == dmin in bin 0, d == dmax in bin 9
    if T >= 64:
        assert several.sum() >= 3
    if window != 1e8:
        n_pairs = stats[:, 0] * (stats[:, 0] - 1) // 2
        assert (stats[:, 1] + stats[:, 2] < n_pairs).any()                # the frame-window test fired


SEGMENTS = (0, 1, 2, 255, 256, 257, 4097, 44850, 130816)


def sort_keys(kind, n, rng):
    if kind == "seven values":
        return rng.choice(rng.random(7).view(np.uint64), n)
    if kind == "lowest bit":
        return np.float64(0.37).view(np.uint64) | rng.integers(0, 2, n, dtype=np.uint64)
    if kind == "exponent":
        return (rng.integers(1000, 1040, n, dtype=np.uint64) << np.uint64(52)) | np.uint64(0x000fedcba9876543)
    if kind == "equal":
        return np.full(n, np.float64(1.25).view(np.uint64))
    return rng.random(n).view(np.uint64)                                  # "random": every key byte varies


@pytest.mark.parametrize("kind,ordered", [("seven values", False), ("lowest bit", False), ("exponent", False), ("equal", False),
                                          ("random", False), ("seven values", True)])
def test_segmented_sort_alone(kind, ordered):
    rng = np.random.default_rng(len(kind))
    seg = np.zeros(len(SEGMENTS) + 1, dtype=np.int64)
    np.cumsum(SEGMENTS, out=seg[1:])
    N = int(seg[-1])
    keys = np.zeros((2, N), dtype=np.uint64)
    payload = np.zeros((2, N), dtype=np.uint32)
    for s, n in enumerate(SEGMENTS):
        keys[0, seg[s]:seg[s + 1]] = sort_keys(kind, n, rng)
        pl = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        payload[0, seg[s]:seg[s + 1]] = np.sort(pl) if ordered else pl
    k_dev, p_dev = dev(keys.view(np.int64)), dev(payload.view(np.int32))
    engine.track_pair_sort(k_dev, p_dev, dev(seg), payload_ordered=ordered)
    got_k, got_p = k_dev.cpu().numpy().view(np.uint64)[0], p_dev.cpu().numpy().view(np.uint32)[0]
    for s in range(len(SEGMENTS)):
        a, b = seg[s], seg[s + 1]
        order = np.lexsort((payload[0, a:b], keys[0, a:b]))
        assert np.array_equal(got_k[a:b], keys[0, a:b][order]), (kind, SEGMENTS[s])
        assert np.array_equal(got_p[a:b], payload[0, a:b][order]), (kind, SEGMENTS[s])


def test_resolve_every_class_and_rank():
    world, vis, _ = U.make_block(4, 40)
    points = [7, 0, 3]                                                    # a moving point, a nearly static one, the two-valued one
    state, stats, edges, counts_dev = device_stats(world, vis, points, 0.01, 1e8)
    want_state = U.track_pair_stats(world, vis, np.asarray(points))
    counts = counts_dev.cpu().numpy()
    assert stats[1, 1] > 0 and stats[0, 2] > 100 and (counts[2] > 0).sum() == 1
    rows = np.arange(3, dtype=np.int32)
    seg = np.zeros(4, dtype=np.int64)
    np.cumsum(stats[:, 2], out=seg[1:])
    classes = np.concatenate([counts, stats[:, 1:2]], axis=1).astype(np.int32)
    picks = np.asarray([(s, c, r) for s in range(3) for c in range(11) for r in range(classes[s, c])], dtype=np.int32)
    assert len(picks) == stats[:, 1:3].sum()
    rows_dev, seg_dev = dev(rows), dev(seg)
    keys, payload = engine.track_pair_order(state, rows_dev, seg_dev, int(seg[-1]))
    want_keys, want_payload = U.track_pair_order(want_state, rows, seg, int(seg[-1]))
    assert np.array_equal(keys.cpu().numpy()[0], want_keys[0]) and np.array_equal(payload.cpu().numpy()[0], want_payload[0])
    got = engine.track_pair_resolve(state, counts_dev, rows_dev, seg_dev, payload, picks, classes).cpu().numpy()
    want = U.track_pair_resolve(want_state, counts, rows, seg, want_payload, picks, classes)
    assert np.array_equal(got, want) and (got[:, 0] < got[:, 1]).all()
    for s, c in ((0, 0), (1, 10), (2, 5)):                                # a rank equal to the class count: refused, no launch
        with pytest.raises(_lib.MspaError, match="rank") as e:
            engine.track_pair_resolve(state, counts_dev, rows_dev, seg_dev, payload, np.array([[s, c, classes[s, c]]]), classes)
        assert e.value.code == _lib.MSPA_EINVAL
    with pytest.raises(_lib.MspaError) as e:
        engine.track_pair_resolve(state, counts_dev, rows_dev, seg_dev, payload, np.array([[3, 0, 0]]), classes)
    assert e.value.code == _lib.MSPA_EINVAL


def key(s):
    return int(s["point_index"]), int(s["frame1"]), int(s["frame2"])


@pytest.fixture(scope="module")
def block():
    tr = synth.make_tracks(52, T=120, P=64, n_groups=4)
    rng = np.random.default_rng(8)
    vis = tr.visibility & (rng.random(tr.visibility.shape) > 0.25)        # a quarter of the visibility cleared
    c2w = torch.from_numpy(np.linalg.inv(tr.extrinsics_w2c).reshape(-1, 16)).to(DEV)
    world = engine.track_to_world(dev(tr.tracks_XYZ), c2w, tr.fx_fy_cx_cy, tr.image_hw, ("world",))["world"]
    order = rng.permutation(64)
    return world, vis, [sorted(int(p) for p in order[g::4]) for g in range(4)]


def both_lines(monkeypatch, world, vis, base, args, seed):
    out = {}
    for mode in ("host", "device"):
        monkeypatch.setenv("MSPA_TRACK_MINING", mode)
        rng, groups = random.Random(seed), [list(g) for g in base]
        try:
            got = heads.object_movement_mine_pairs(vis, groups, lambda p, f: engine.track_pair_distances(world, p, f), *args, rng,
                                                   world=world)
        except ValueError as e:
            got = str(e)
        out[mode] = (got if isinstance(got, str) else [key(s) for s in got], rng.getstate(), groups, dict(heads.LAST_TRACK_MINING))
    return out["host"], out["device"]


@pytest.mark.parametrize("args", ARGSETS, ids=[str(a) for a in ARGSETS])
def test_mine_pairs_device_equals_host(block, monkeypatch, args):
    world, vis, base = block
    host, device = both_lines(monkeypatch, world, vis, base, args, 31)
    assert device[0] == host[0] and len(host[0]) > 0                      # the list
    assert device[1] == host[1]                                           # rng.getstate()
    assert device[2] == host[2] != base                                   # the groups, shuffled alike
    assert host[3]["path"] == "host" and device[3] == {"path": "device", "reason": ""}


def test_a_nan_track_declines_to_the_host_line(block, monkeypatch):
    world, vis, base = block
    world = world.clone()
    world[5, base[2][3]] = float("nan")
    vis = vis.copy()
    vis[[5, 6, 9], base[2][3]] = True
    host, device = both_lines(monkeypatch, world, vis, base, (15, 30, True, 0.05), 31)
    assert device[:3] == host[:3]                                         # the host line's behaviour, whatever it is
    assert device[3]["path"] == "host" and "non-finite" in device[3]["reason"]


PKG_ROOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-spatialmllm_amd")


def facade(module):
    """The product's ``spatial_engine`` module of that name, whatever an earlier test imported under the package's name."""
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(PKG_ROOT):
            del sys.modules[name]
    if sys.path[0] != PKG_ROOT:
        sys.path.insert(0, PKG_ROOT)
    return importlib.import_module(module)


def _tree(d):
    files = {}
    for root, _, names in os.walk(d):
        for n in names:
            with open(os.path.join(root, n), "rb") as f:
                files[os.path.relpath(os.path.join(root, n), d)] = f.read()
    return files


@pytest.mark.parametrize("which", ["coord", "dot"])
def test_scene_level_callers_are_byte_identical(tmp_path, monkeypatch, which):
    from PIL import Image
    from mspa.annotate import PillowAnnotator
    tr = synth.make_tracks(35, T=60, P=64, n_groups=4)
    H, W = tr.image_hw
    payloads = []
    for t in range(tr.tracks_XYZ.shape[0]):
        b = io.BytesIO()
        Image.fromarray(content(H, W, t % 5)).save(b, "JPEG", quality=85)
        payloads.append(b.getvalue())
    (tmp_path / "src").mkdir()
    path = str(tmp_path / "src" / f"{tr.scene_id}.npz")
    np.savez(path, images_jpeg_bytes=np.array(payloads, dtype=object), tracks_XYZ=tr.tracks_XYZ, visibility=tr.visibility,
             fx_fy_cx_cy=tr.fx_fy_cx_cy, extrinsics_w2c=tr.extrinsics_w2c)
    OM = facade("spatial_engine.object_movement.single_object_movement_engine_coord")      # imported first: the modules seed ``random``
    OMD = facade("spatial_engine.object_movement.single_object_movement_engine_dot")
    results = {}
    for mode in ("host", "device"):
        if mode == "host":
            monkeypatch.delenv("MSPA_TRACK_MINING", raising=False)       # the switch unset
        else:
            monkeypatch.setenv("MSPA_TRACK_MINING", "device")
        img = str(tmp_path / mode / "img")
        random.seed(71)
        if which == "coord":
            eng = OM.TwoFrameVideoQAEngine("tapvid3d_displacement_vector", "adt")
            recs = eng.generate_qa_training_single_scene(path, 6, 5, img, True, 0.5)
        else:
            eng = OMD.TwoFrameVideoQAEngineDot("tapvid3d_total_distance", "adt")
            eng.annotator = PillowAnnotator()
            recs = eng.generate_qa_training_single_scene(path, str(tmp_path / mode / "base"), 6, 5, img, True, 0.5)
        assert heads.LAST_TRACK_MINING["path"] == mode
        results[mode] = (json.dumps(recs).replace(str(tmp_path / mode), "<dir>"), random.getstate(), _tree(str(tmp_path / mode)))
    assert results["host"][0] == results["device"][0] and len(json.loads(results["host"][0])) > 10
    assert results["host"][1] == results["device"][1]
    assert results["host"][2] == results["device"][2] and len(results["host"][2]) > 10


def test_pipeline_track_stage_is_byte_identical(tmp_path, monkeypatch):
    from mspa import pipeline
    scenes = [synth.make_scene(7100, n_points=1500, n_frames=4, color_hw=(96, 128), depth_hw=(96, 128), invalid_pose_frac=0.0,
                               with_color=False)]
    tracks = [synth.make_tracks(400 + k, T=100, P=64, n_groups=3) for k in range(2)]
    out, paths = {}, {}
    for mode in ("host", "device"):
        if mode == "host":
            monkeypatch.delenv("MSPA_TRACK_MINING", raising=False)
        else:
            monkeypatch.setenv("MSPA_TRACK_MINING", "device")
        counts = pipeline.run(scenes, str(tmp_path / mode), None, DEV, seed=3, n_camera=4, n_correspondence=4,
                              depth_images_per_scene=1, object_perception=False, tracks=tracks)
        paths[mode] = heads.LAST_TRACK_MINING.get("path")
        names = sorted(n for n in counts if n.startswith("object_movement_"))
        assert len(names) == 2 and all(counts[n] > 0 for n in names)
        out[mode] = {n: open(str(tmp_path / mode / f"{n}.jsonl"), "rb").read() for n in names}
    assert out["host"] == out["device"] and paths == {"host": "host", "device": "device"}
