"""Upload slots (mspa/upload.py) are pooled per process and outlive a ScenePrefetcher.  A slot that staged a scene decoded on the
device holds that decode (``pending_decode``: the packed frames and their count) until the consumer finishes it; whatever ends
an iteration early -- the consumer leaving, a staging error after the decode was enqueued -- must not hand such a slot to the
next prefetcher, which would otherwise look at the old scene's status, write the old scene's host-decoded frames over its own
depth and keep the old pinned buffer from its pool.  Scenes are built directly: synthetic frames written as 16-bit PNGs, one
frame per packed scene an 8-bit PNG that the packer declines and the host reader fills in."""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HW_A, HW_B = (48, 64), (60, 80)


@pytest.fixture
def slot_pool(monkeypatch):
    """A slot pool of the test's own, so that the second prefetcher of a test reuses exactly the first one's slots."""
    from mspa import upload
    pool = {}
    monkeypatch.setattr(upload, "_SLOT_POOL", pool)
    return pool


def _scene(tmp_path, seed, hw, pool=None, n_frames=4):
    """(HostScene, the host reader's frames).  With ``pool``: the frames as PNG files packed for the device decode (frame 1 an
    8-bit PNG); without: decoded frames in host memory."""
    from PIL import Image
    from mspa import ingest, sweep, synth
    from spatial_engine.utils.scannet_utils.handler import _images
    sc = synth.make_scene(seed, n_points=600, n_frames=n_frames, color_hw=hw, depth_hw=hw, invalid_pose_frac=0.0, with_color=False)
    ids = list(sc.valid_image_ids)
    assert len(ids) == n_frames
    E = {i: sc.E[i].copy() for i in ids}
    if pool is None:
        want = np.stack([sc.depth[i] for i in ids])
        return sweep.HostScene(f"h{seed}", sc.K, sc.A, E, {i: want[k] for k, i in enumerate(ids)}, hw, sc.points), want
    paths = []
    for k, i in enumerate(ids):
        p = str(tmp_path / f"{seed}_{i}.png")
        Image.fromarray((sc.depth[i] >> 8).astype(np.uint8) if k == 1 else sc.depth[i]).save(p, compress_level=1)
        paths.append(p)
    want = ingest.read_depth_frames(paths, 2, general_reader=_images.read_depth)
    assert np.array_equal(want[1], sc.depth[ids[1]] >> 8) and np.array_equal(want[2], sc.depth[ids[2]])
    packed = ingest.pack_scene_depth(paths, 2, pool=pool)
    assert packed is not None and (packed.status != 0).tolist() == [k == 1 for k in range(n_frames)]
    return sweep.HostScene(f"p{seed}", sc.K, sc.A, E, {}, hw, sc.points, packed=packed, depth_ids=ids), want


def _depth(scene):
    return scene.depth.cpu().numpy().view(np.uint16).copy()


def _check_slots_clean(slot_pool, bytes_pool, packs, n_slots=2):
    slots = [s for v in slot_pool.values() for s in v]
    assert len(slots) == n_slots
    assert [s.pending_decode for s in slots] == [None] * n_slots
    assert [getattr(s, "in_flight_frames", 0) for s in slots] == [0] * n_slots
    assert [p.buf is None for p in packs] == [True] * len(packs)          # every packed buffer went back to the test's pool
    assert len(bytes_pool._free) == len(packs)


def _host_pass_is_exact(tmp_path, threaded, seeds=(901, 902, 903)):
    """Host-decoded scenes of the same depth shape through the same two slots: each scene's depth is its own frames."""
    from mspa import upload
    hosts = [_scene(tmp_path, s, HW_A) for s in seeds]
    got = [_depth(s) for s in upload.ScenePrefetcher([h for h, _ in hosts], "cuda", slots=2, threaded=threaded)]
    assert len(got) == len(hosts)
    for k, (g, (_, want)) in enumerate(zip(got, hosts)):
        assert np.array_equal(g, want), (k, np.argwhere((g != want).any(axis=(1, 2))).ravel())


@pytest.mark.parametrize("threaded", [False, True])
def test_abandoned_iteration_leaves_no_pending_decode(threaded, tmp_path, slot_pool):
    """The consumer takes the first scene and closes the iteration while the second one's decode is staged in the other slot."""
    from mspa import ingest, upload
    pool = ingest.PinnedBytesPool()
    (a, want_a), (b, _) = _scene(tmp_path, 501, HW_A, pool), _scene(tmp_path, 502, HW_A, pool)
    past_b = threading.Event()

    def scenes():
        yield a
        yield b
        past_b.set()                       # the producer asks for a third scene only after b is staged
    it = iter(upload.ScenePrefetcher(scenes(), "cuda", slots=2, threaded=threaded, decode_on_device=True))
    first = next(it)
    assert np.array_equal(_depth(first), want_a)
    if threaded:
        assert past_b.wait(120)
    it.close()
    _check_slots_clean(slot_pool, pool, [a.packed, b.packed])
    _host_pass_is_exact(tmp_path, threaded)


@pytest.mark.parametrize("threaded", [False, True])
def test_staging_error_after_the_decode_was_enqueued(threaded, tmp_path, slot_pool):
    """A packed scene whose pose is not affine: its decode is on the slot's stream before the pose tables fail.  The
    ValueError reaches the consumer; no slot keeps the failed scene's decode (nor, unthreaded, the unconsumed first scene's)."""
    from mspa import ingest, upload
    pool = ingest.PinnedBytesPool()
    (a, _), (bad, _) = _scene(tmp_path, 511, HW_A, pool), _scene(tmp_path, 512, HW_A, pool)
    bad.E[list(bad.E)[2]][3, 1] = 1e-3
    with pytest.raises(ValueError, match="last row"):
        for _scene_on_device in upload.ScenePrefetcher([a, bad], "cuda", slots=2, threaded=threaded, decode_on_device=True):
            pass
    _check_slots_clean(slot_pool, pool, [a.packed, bad.packed])
    _host_pass_is_exact(tmp_path, threaded)


@pytest.mark.parametrize("threaded", [False, True])
def test_depth_shape_changing_in_one_slot(threaded, tmp_path, slot_pool):
    """Packed scenes of 48 x 64 and 60 x 80 frames (scanline pitch 6 400 and 9 728 bytes) and a host-decoded scene, through two
    slots: each slot decodes both shapes in turn, so its scanline scratch is reallocated for a new pitch (``_ensure_decode``).
    Every scene's depth equals the host reader's.  The decode stream must wait for the allocating stream after such a
    reallocation; a missing wait is a race this test cannot provoke deterministically -- it checks the results, not the wait."""
    from mspa import ingest, upload
    pool = ingest.PinnedBytesPool()
    specs = [(HW_A, 4, True), (HW_B, 5, True), (HW_B, 3, True), (HW_A, 4, False), (HW_A, 5, True), (HW_B, 4, True), (HW_A, 3, True)]
    scenes = [_scene(tmp_path, 700 + k, hw, pool if packed else None, n) for k, (hw, n, packed) in enumerate(specs)]
    got = [_depth(s) for s in upload.ScenePrefetcher([s for s, _ in scenes], "cuda", slots=2, threaded=threaded, decode_on_device=True)]
    assert len(got) == len(scenes)
    for k, (g, (_, want)) in enumerate(zip(got, scenes)):
        assert g.shape == want.shape and np.array_equal(g, want), k
    packs = [s.packed for s, _ in scenes if s.packed is not None]
    _check_slots_clean(slot_pool, pool, packs)
