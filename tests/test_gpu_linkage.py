"""K7b on the MI355X: engine.track_linkage against SciPy bit for bit (Z) and value for value (labels), batched and single, and
engine.track_rigid_groups / the MSPA_LINKAGE=device switch against the SciPy path they replace.  Every generated case is
compared in full: no tolerance, nothing excluded on tie grounds."""
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linkage_util as LU  # noqa: E402

from mspa import _lib, engine, synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG_ROOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-spatialmllm_amd")

# one below, at and one above a wave; across a wave-pair boundary; past one 256-lane pass
SIZES = (2, 3, 63, 64, 65, 130, 257)


def _run(mats, threshold):
    """mats [B, P, P] (NumPy) through one launch -> (Z, labels, status) on the host; the input tensor must come back unchanged."""
    dev = torch.from_numpy(np.ascontiguousarray(mats)).to(DEV)
    keep = dev.clone()
    Z, labels, status = engine.track_linkage(dev, threshold)
    torch.cuda.synchronize()
    assert torch.equal(dev.view(torch.int64), keep.view(torch.int64)), "track_linkage wrote its input"
    return Z.cpu().numpy(), labels.cpu().numpy(), status.cpu().numpy()


def _assert_block(m, threshold, Z, labels, status, what):
    want_Z, want_labels = LU.scipy_answer(m, threshold)
    assert status == 0, (what, int(status))
    assert Z.dtype == np.float64 and Z.shape == want_Z.shape and Z.tobytes() == want_Z.tobytes(), what
    assert labels.dtype == np.int32 and np.array_equal(labels, want_labels), what


@pytest.mark.parametrize("P", SIZES)
def test_equals_scipy(P):
    for kind in LU.KINDS:
        for B in (1, 5):                              # 5: ragged across the CUs, every block different
            mats = np.stack([LU.matrix(kind, P, 100 + b) for b in range(B)])
            for t in LU.thresholds(mats[0]):
                Z, labels, status = _run(mats, t)
                assert Z.shape == (B, P - 1, 4) and labels.shape == (B, P) and status.shape == (B,)
                for b in range(B):
                    _assert_block(mats[b], t, Z[b], labels[b], status[b], (kind, P, B, b, t))
        m = LU.matrix(kind, P, 100)                   # the [P, P] form
        dev = torch.from_numpy(m).to(DEV)
        Z, labels, status = engine.track_linkage(dev)
        assert Z.shape == (P - 1, 4) and labels.shape == (P,) and status.shape == ()
        _assert_block(m, 0.1, Z.cpu().numpy(), labels.cpu().numpy(), int(status), (kind, P, "single"))


def test_special_matrices():
    for m, t in [(np.zeros((65, 65)), 0.1), (np.zeros((65, 65)), 0.0), (LU.duplicate_rows(), 0.1), (LU.on_threshold(), 0.1),
                 (LU.on_threshold(), 0.05)]:
        Z, labels, status = _run(m[None], t)
        _assert_block(m, t, Z[0], labels[0], status[0], (m.shape, t))
    Z, labels, _ = _run(LU.on_threshold()[None], 0.1)
    assert Z[0, -1, 2] == 0.1 and labels[0].tolist() == [1, 1, 1, 1]


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_one_non_finite_block_in_a_batch(value):
    P, B, hit = 65, 5, 3
    mats = np.stack([LU.matrix("half_zero", P, 200 + b) for b in range(B)])
    good = mats[hit].copy()
    mats[hit, 7, 40] = mats[hit, 40, 7] = value
    Z, labels, status = _run(mats, 0.1)
    assert status.tolist() == [0, 0, 0, _lib.LINKAGE_NONFINITE, 0]
    assert not Z[hit].any() and not labels[hit].any()
    for b in range(B):
        if b != hit:
            _assert_block(mats[b], 0.1, Z[b], labels[b], status[b], b)
    mats[hit] = good
    assert _run(mats, 0.1)[2].tolist() == [0] * B


def test_trivial_sizes_and_limits():
    Z, labels, status = engine.track_linkage(torch.zeros((3, 1, 1), dtype=torch.float64, device=DEV))
    assert Z.shape == (3, 0, 4) and labels.tolist() == [[1]] * 3 and status.tolist() == [0, 0, 0]
    Z, labels, status = engine.track_linkage(torch.zeros((0, 0), dtype=torch.float64, device=DEV))
    assert Z.shape == (0, 4) and labels.shape == (0,) and int(status) == 0
    Z, labels, status = engine.track_linkage(torch.zeros((0, 9, 9), dtype=torch.float64, device=DEV))
    assert Z.shape == (0, 8, 4) and labels.shape == (0, 9) and status.shape == (0,)
    with pytest.raises(_lib.MspaError):
        engine.track_linkage(torch.zeros((_lib.LINKAGE_MAX_POINTS + 1,) * 2, dtype=torch.float64, device=DEV))


def _golden_tracks():
    from golden_util import GOLDEN_DIR
    z = np.load(os.path.join(GOLDEN_DIR, "tracks.npz"))
    return z["tracks_XYZ"], json.loads(str(z["groups_json"]))


def test_rigid_groups_on_the_golden_tracks():
    pts, groups = _golden_tracks()
    assert engine.track_rigid_groups(torch.from_numpy(np.ascontiguousarray(pts)).to(DEV)) == groups


def test_rigid_groups_two_bodies_plus_noise():
    """40 frames x 130 points: two rigid bodies (a translating one, a rotating one) and free points.  The device groups are
    SciPy's of the downloaded K7 matrix, and the batched K7 is the single K7 per block."""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    rng = np.random.default_rng(77)
    T, P = 40, 130
    base = rng.normal(size=(P, 3)) * 0.5
    xyz = np.empty((T, P, 3))
    for t in range(T):
        a = 0.03 * t
        R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        xyz[t, :50] = base[:50] + np.array([0.05 * t, 0.0, 2.0])
        xyz[t, 50:100] = base[50:100] @ R.T + np.array([0.0, 1.0, 3.0])
        xyz[t, 100:] = base[100:] + rng.normal(size=(P - 100, 3)) * 0.2 + np.array([0.0, -1.0, 2.5])
    dev = torch.from_numpy(xyz).to(DEV)
    loss = engine.track_rigidity_loss(dev).cpu().numpy()
    want = LU.groups_of(fcluster(linkage(squareform(loss, checks=False), method="average"), 0.1, criterion="distance"))
    assert sorted(map(len, want))[-2:] == [50, 50] and len(want) > 2
    assert engine.track_rigid_groups(dev) == want
    other = np.ascontiguousarray(xyz[:, ::-1])
    batch = engine.track_rigidity_loss_batch(torch.from_numpy(np.stack([xyz, other])).to(DEV)).cpu().numpy()
    assert np.array_equal(batch[0], loss)
    assert np.array_equal(batch[1], engine.track_rigidity_loss(torch.from_numpy(other).to(DEV)).cpu().numpy())
    bad = xyz.copy()
    bad[3, 5, 1] = np.inf                             # an infinite distance change (a NaN one fails `> smoothing` and counts as 0)
    bad_dev = torch.from_numpy(bad).to(DEV)
    with pytest.raises(ValueError, match="only finite values"):
        linkage(squareform(engine.track_rigidity_loss(bad_dev).cpu().numpy(), checks=False), method="average")
    with pytest.raises(ValueError, match="only finite values"):
        engine.track_rigid_groups(bad_dev)
    with pytest.raises(ValueError):
        engine.track_rigid_groups(dev[:, :1].contiguous())


def _facade_om():
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not getattr(sys.modules[name], "__file__", "").startswith(PKG_ROOT):
            del sys.modules[name]
    if sys.path[0] != PKG_ROOT:
        sys.path.insert(0, PKG_ROOT)
    OM = importlib.import_module("spatial_engine.object_movement.single_object_movement_engine_coord")
    assert OM.__file__.startswith(PKG_ROOT)
    return OM


def test_switch_in_rigid_body_segmentation(monkeypatch):
    OM = _facade_om()
    pts, groups = _golden_tracks()
    monkeypatch.delenv("MSPA_LINKAGE", raising=False)
    assert engine.linkage_backend() == "scipy"
    host = OM.rigid_body_segmentation(pts)
    calls = []
    real = engine.track_rigid_groups
    monkeypatch.setattr(engine, "track_rigid_groups", lambda *a, **k: calls.append(1) or real(*a, **k))
    assert OM.rigid_body_segmentation(pts) == host and not calls
    monkeypatch.setenv("MSPA_LINKAGE", "device")
    assert OM.rigid_body_segmentation(pts) == host == groups and calls == [1]
    monkeypatch.setenv("MSPA_LINKAGE", "gpu")
    with pytest.raises(ValueError, match="MSPA_LINKAGE"):
        OM.rigid_body_segmentation(pts)


def test_switch_in_the_pipeline_gives_the_same_files(tmp_path, monkeypatch):
    """Object-movement JSONL of mspa.pipeline on the track blocks the pipeline tests use: byte-identical with the switch on."""
    from mspa import pipeline
    scenes = [synth.make_scene(7100, n_points=1500, n_frames=4, color_hw=(96, 128), depth_hw=(96, 128), invalid_pose_frac=0.0,
                               with_color=False)]
    tracks = [synth.make_tracks(400 + k, T=100, P=64, n_groups=3) for k in range(3)]
    out = {}
    for mode in ("scipy", "device"):
        monkeypatch.setenv("MSPA_LINKAGE", mode)
        counts = pipeline.run(scenes, str(tmp_path / mode), None, DEV, seed=3, n_camera=4, n_correspondence=4,
                              depth_images_per_scene=1, object_perception=False, tracks=tracks)
        names = sorted(n for n in counts if n.startswith("object_movement_"))
        assert len(names) == 2 and all(counts[n] > 0 for n in names)
        out[mode] = {n: open(str(tmp_path / mode / f"{n}.jsonl"), "rb").read() for n in names}
    assert out["scipy"] == out["device"]
