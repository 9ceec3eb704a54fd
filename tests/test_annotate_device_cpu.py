"""The host side of mspa.annotate.DeviceAnnotator: span packing, the label-mask cache, and the NumPy statement of the mask
blend against ``ImageDraw.text`` on the labels, colours and border positions the dot heads produce."""
import numpy as np
import pytest

from mspa import annotate
from mspa.annotate import LabelMasks, PillowAnnotator, blend_mask_numpy, default_annotator, pack_spans, rgb24


def test_pack_spans_groups_by_image_and_row_keeping_paint_order():
    spans = [(1, [(5, 0, 3, 0xAA), (2, 1, 1, 0xBB)]), (0, [(5, 2, 9, 0xCC)]), (1, [(5, 1, 4, 0xDD)])]
    got = pack_spans(spans)
    assert got.dtype == np.int32 and got.shape == (4, 5)
    assert got.tolist() == [[0, 5, 2, 9, 0xCC], [1, 2, 1, 1, 0xBB], [1, 5, 0, 3, 0xAA], [1, 5, 1, 4, 0xDD]]
    assert pack_spans([]).shape == (0, 5)
    assert rgb24((1, 2, 3)) == 0x030201


def test_label_masks_are_cached_per_text():
    lm = LabelMasks()
    a = lm.get("A")
    assert lm.get("A") is a and a[0].dtype == np.uint8 and a[0].size > 0
    assert lm.get("B") is not a
    assert lm.get("")[0].size == 0


@pytest.mark.parametrize("label", ["A", "B", "C", "D", "E", "1", "12"])
def test_mask_blend_equals_imagedraw_text(label):
    from PIL import Image, ImageDraw
    lm = LabelMasks()
    mask, dx, dy = lm.get(label)
    h, w = 60, 80
    rng = np.random.default_rng(len(label) + ord(label[0]))
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    colours = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 0, 0), (255, 255, 255), (17, 200, 99)]
    positions = [(30, 30), (-10, 20), (w - 5, 20), (20, -25), (20, h - 3), (-40, -40), (w + 5, h + 5), (0, 0)]
    for colour in colours:
        for (x, y) in positions:
            im = Image.fromarray(base.copy())
            ImageDraw.Draw(im).text((x, y), label, fill=colour, font=PillowAnnotator._font())
            got = base.copy()
            blend_mask_numpy(got, mask, x + dx, y + dy, colour)
            assert np.array_equal(np.asarray(im), got), (label, colour, x, y)


def test_default_annotator_without_the_variable_is_pillow(monkeypatch):
    monkeypatch.delenv("MSPA_ANNOTATE", raising=False)
    assert type(default_annotator()) is PillowAnnotator
    monkeypatch.setenv("MSPA_ANNOTATE", "pillow")
    assert type(default_annotator()) is PillowAnnotator


def test_flush_annotator_ignores_annotators_without_flush():
    annotate.flush_annotator(PillowAnnotator())
    annotate.flush_annotator(None)
