"""SceneInfoHandler.instance_clouds on the scene of tests/golden/instance_clouds.npz, written to a temporary ScanNet layout with
Pillow (8-bit ``L`` masks and 16-bit depth as files; the colour frames registered in ``_images.MEMORY`` so that both paths see the
same RGB): against the reference's frozen per-object clouds, against the existing façade composition ``get_instance_mask`` +
``project_image_to_3d_with_mask`` for every (image, target), chunked, downstream of ``remove_statistical_outliers``, and through
each fallback."""
import os

import numpy as np
import pytest

from golden_util import same_f64
from test_gpu_facade import facade

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance_clouds.npz")
SID = "scene0950_00"


def _layout(ns, g, root, masks=None, mask_mode="L"):
    """The golden's scene under ``root``; ``masks`` replaces the label images (any dtype / shape Pillow can write)."""
    from PIL import Image
    posed, scans = os.path.join(root, "posed_images"), os.path.join(root, "scans")
    os.makedirs(os.path.join(posed, SID), exist_ok=True)
    os.makedirs(os.path.join(scans, SID, "instance-filt"), exist_ok=True)
    ids = [str(i) for i in g["image_ids"]]
    masks = g["labels"] if masks is None else masks
    for k, i in enumerate(ids):
        Image.fromarray(np.ascontiguousarray(g["depth"][k], dtype=np.uint16)).save(os.path.join(posed, SID, f"{i}.png"))
        ns.IMG.register(os.path.join(posed, SID, f"{i}.jpg"), np.ascontiguousarray(g["color"][k]))
        m = np.ascontiguousarray(masks[k])
        (Image.fromarray(m, mode="L") if mask_mode == "L" else Image.fromarray(m.astype(np.uint16))).save(
            os.path.join(scans, SID, "instance-filt", f"{int(i)}.png"))
    infos = {SID: {"num_posed_images": len(ids), "intrinsic_matrix": g["K"], "axis_align_matrix": g["A"], "num_objects": 8,
                   "images_info": {i: {"extrinsic_matrix": g["E"][k]} for k, i in enumerate(ids)}}}
    return ns.IH.SceneInfoHandler(infos, posed_images_root=posed, instance_data_root=os.path.join(root, "inst"), mask_image_root=scans), ids


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def scene(golden, tmp_path_factory):
    """(façade, golden, handler, image ids, the composition's result per (image, target, with_color)): computed once, shared."""
    ns = facade()
    h, ids = _layout(ns, golden, str(tmp_path_factory.mktemp("instance_clouds")))
    comp = {}
    for i in ids:
        for t in range(8):
            mask = h.get_instance_mask(SID, i, t)
            for c in (False, True):
                comp[i, t, c] = h.project_image_to_3d_with_mask(SID, i, mask, with_color=c)
    return ns, golden, h, ids, comp


def _equal(clouds, comp, ids, with_color):
    for i in ids:
        for t in range(8):
            got, want = clouds.cloud(i, t), comp[i, t, with_color]
            assert got.is_cuda and got.dtype.is_floating_point and tuple(got.shape) == want.shape, (i, t, got.shape, want.shape)
            assert same_f64(got.cpu().numpy(), want), (i, t)
            assert clouds.count(i, t) == len(want)
        assert clouds.present(i) == [t for t in range(8) if len(comp[i, t, with_color])]


@pytest.mark.parametrize("with_color", [False, True])
def test_equals_the_golden_and_the_composition(scene, with_color):
    from mspa import instances
    ns, g, h, ids, comp = scene
    clouds = h.instance_clouds(SID, with_color=with_color)
    assert instances.LAST_INSTANCE_CLOUDS == {"path": "device", "reason": ""}
    assert isinstance(clouds, instances.InstanceClouds) and clouds.rows.is_cuda and clouds.rows.shape[1] == (6 if with_color else 3)
    for k, i in enumerate(ids):
        for t in range(8):
            got = clouds.cloud(i, t).cpu().numpy()
            want = g[f"xyz_{k}_{t}"] if not with_color else np.hstack((g[f"xyz_{k}_{t}"], g[f"rgb_{k}_{t}"]))
            assert got.shape == want.shape, (i, t)
            if len(want) == 1:                                # the one-pixel object: BLAS's vector path in the reference
                print("one-pixel object", i, "bit-identical to the golden" if same_f64(got, want) else f"differs: {got - want}")
                assert np.allclose(got, want, rtol=1e-12, atol=0)
                continue
            assert same_f64(got, want), (i, t, np.abs(got - want).max() if len(want) else 0)
            if len(want):
                assert same_f64(clouds.aabb(i, t).cpu().numpy(), g[f"aabb_{k}_{t}"]), (i, t)
                assert same_f64(clouds.aabb(i, t).cpu().numpy(), ns.OPS.calculate_aabb(clouds.cloud(i, t)).cpu().numpy())
    _equal(clouds, comp, ids, with_color)                     # the one-pixel and the empty objects included
    with pytest.raises(ValueError):
        clouds.aabb(ids[0], 4)
    for t in (0, 4, 5, 7):
        want = np.vstack([comp[i, t, with_color] for i in ids])
        assert same_f64(clouds.object_cloud(t).cpu().numpy(), want), t
    # the pixel indices are the masks' np.where order
    pix = clouds.pixel.cpu().numpy()
    a, b = clouds.offsets[1 * 256 + 3], clouds.offsets[1 * 256 + 4]
    idx = np.flatnonzero(g["labels"][1].reshape(-1) == 3)
    assert np.all(np.diff(pix[a:b]) > 0) and set(pix[a:b].tolist()) <= set(idx.tolist())


def test_subset_of_images_and_chunking(scene):
    ns, g, h, ids, comp = scene
    whole = h.instance_clouds(SID, with_color=True)
    one = h.instance_clouds(SID, with_color=True, max_dense_bytes=1)           # one frame per chunk
    assert np.array_equal(one.counts, whole.counts) and np.array_equal(one.offsets, whole.offsets)
    for name in ("rows", "pixel", "lo", "hi", "rgb"):
        assert getattr(one, name).cpu().numpy().tobytes() == getattr(whole, name).cpu().numpy().tobytes(), name
    sub = h.instance_clouds(SID, image_ids=[ids[2], ids[0]])
    assert sub.image_ids == [ids[2], ids[0]]
    _equal(sub, comp, [ids[2], ids[0]], False)
    assert same_f64(sub.object_cloud(1).cpu().numpy(), np.vstack([comp[ids[2], 1, False], comp[ids[0], 1, False]]))


def test_outlier_removal_stays_on_the_device(scene):
    ns, g, h, ids, comp = scene
    clouds = h.instance_clouds(SID)
    for t in (1, 3):
        got = ns.OPS.remove_statistical_outliers(clouds.cloud(ids[1], t))
        want = ns.OPS.remove_statistical_outliers(comp[ids[1], t, False])
        assert got.is_cuda and 0 < len(want) < len(comp[ids[1], t, False]) and same_f64(got.cpu().numpy(), want), t


def test_non_finite_pose_is_left_out(scene, capsys):
    ns, g, h, ids, comp = scene
    infos = {SID: dict(h.infos[SID])}
    infos[SID]["images_info"] = dict(infos[SID]["images_info"])
    infos[SID]["images_info"][ids[1]] = {"extrinsic_matrix": np.full((4, 4), -np.inf)}
    h2 = ns.IH.SceneInfoHandler(infos, posed_images_root=h.posed_images_root, instance_data_root=h.instance_data_root,
                                mask_image_root=h.mask_image_root)
    clouds = h2.instance_clouds(SID)
    assert "contains inf or nan" in capsys.readouterr().out
    assert clouds.present(ids[1]) == [] and tuple(clouds.cloud(ids[1], 0).shape) == (0, 3)
    _equal(clouds, comp, [ids[0], ids[2]], False)


@pytest.mark.parametrize("case", ["sixteen_bit", "label_300", "other_size"])
def test_fallbacks(golden, tmp_path, case):
    """A 16-bit mask file with labels <= 255 goes through the general reader and still takes the device split; a label of 300 and
    a mask of another size build the same object from the per-object composition, the reason recorded."""
    from mspa import instances
    ns, g = facade(), golden
    masks = g["labels"].astype(np.uint16)
    if case == "label_300":
        masks = masks.copy()
        masks[masks == 3] = 300
    if case == "other_size":
        masks = masks[:, :120, :160]
    h, ids = _layout(ns, g, str(tmp_path), masks=masks, mask_mode="I;16")
    clouds = h.instance_clouds(SID, with_color=(case != "other_size"))
    wc = case != "other_size"
    if case == "sixteen_bit":
        assert instances.LAST_INSTANCE_CLOUDS == {"path": "device", "reason": ""}
    else:
        assert instances.LAST_INSTANCE_CLOUDS["path"] == "host" and instances.LAST_INSTANCE_CLOUDS["reason"]
        print(case, "->", instances.LAST_INSTANCE_CLOUDS["reason"])
    targets = list(range(8)) + ([299] if case == "label_300" else [])
    for i in ids:
        for t in targets:
            want = h.project_image_to_3d_with_mask(SID, i, h.get_instance_mask(SID, i, t), with_color=wc)
            got = clouds.cloud(i, t)
            assert got.is_cuda and tuple(got.shape) == want.shape and same_f64(got.cpu().numpy(), want), (case, i, t)
    if case == "label_300":
        assert clouds.count(ids[0], 299) > 0 and clouds.count(ids[0], 2) == 0 and 299 in clouds.present(ids[0])


def test_missing_mask_file_raises(golden, tmp_path):
    ns = facade()
    h, ids = _layout(ns, golden, str(tmp_path))
    path = os.path.join(h.mask_image_root, SID, "instance-filt", f"{int(ids[1])}.png")
    os.remove(path)
    with pytest.raises(FileNotFoundError, match="Mask image not found at path: "):
        h.instance_clouds(SID)
    with pytest.raises(FileNotFoundError, match="Mask image not found at path: "):
        h.get_instance_mask(SID, ids[1], 0)
