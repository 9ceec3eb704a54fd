"""The reference the device un-filter is compared with (tests/png_raw.py): scanlines wrapped in a PNG and decoded by Pillow give
back the image they were filtered from, agree with PNG 9.2 written out byte by byte on arbitrary filtered bytes, and the GPU
tests' width list reaches all three code paths and every remainder of the pair pipeline's unrolled loop."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from png_raw import (BYTES, EASY_FILTER_KINDS, FILTER_KINDS, HARD_FILTER_KINDS, HEIGHTS, PAIRS, ROWS, WIDTHS,  # noqa: E402
                     pair_remainder, pillow_unfilter, png_from_scanlines, row_filters, scanlines, scanlines_of,
                     unfilter_path, unfilter_reference)
from test_sweep_cpu import _png_gray16  # noqa: E402


@pytest.mark.parametrize("h,w", [(1, 1), (1, 2), (2, 3), (37, 53), (65, 130), (3, 1026)])
def test_wrapped_scanlines_decode_to_the_image_they_came_from(h, w):
    rng = np.random.default_rng(h * 131 + w)
    images = [rng.integers(0, 65536, (h, w), dtype=np.uint16),
              np.add.outer(np.arange(h), np.arange(w)).astype(np.uint16) * 257,
              rng.choice(np.array([0, 1, 0x7F80, 0x8000, 0xFFFF], np.uint16), (h, w))]
    for a in images:
        for filters in ([0], [1], [2], [3], [4], [0, 1, 2, 3, 4], [4, 3, 2, 1], [3, 4, 4]):
            raw = scanlines_of(_png_gray16(a, filters, 1))
            assert len(raw) == h * (2 * w + 1)
            assert [raw[y * (2 * w + 1)] for y in range(h)] == [filters[y % len(filters)] for y in range(h)]
            assert np.array_equal(pillow_unfilter(raw, h, w), a), (filters, a.dtype)
            assert np.array_equal(pillow_unfilter(scanlines_of(png_from_scanlines(raw, h, w, 9)), h, w), a)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (5, 3), (9, 8), (66, 5)])
def test_pillow_agrees_with_the_filter_definition_on_arbitrary_bytes(h, w):
    """Random filtered bytes (not the output of an encoder): Pillow's decode equals PNG 9.2 byte by byte, for every pattern the
    GPU tests use -- first rows that are Up / Average / Paeth (their row above is zeros) among them."""
    rng = np.random.default_rng(h * 7 + w)
    for kind in FILTER_KINDS:
        for content in ("random", "low", "flat"):
            raw = scanlines(row_filters(kind, h, rng), w, content, rng)
            assert len(raw) == h * (2 * w + 1)
            assert np.array_equal(pillow_unfilter(raw, h, w), unfilter_reference(raw, h, w)), (kind, content)


def test_case_lists_reach_every_path_and_remainder():
    rng = np.random.default_rng(0)
    seen = set()
    for w in WIDTHS:
        for kind in FILTER_KINDS:
            seen.add(unfilter_path(w, row_filters(kind, 65, rng)))
    assert seen == {ROWS, PAIRS, BYTES}
    pair_widths = [w for w in WIDTHS if unfilter_path(w, [4]) == PAIRS]
    assert {pair_remainder(w) for w in pair_widths} == set(range(8))
    assert {1, 2, 63, 64, 65, 130} <= set(HEIGHTS)
    # the dispatch at its edges: nd = 9 leaves the rows path, w = 2 has no pair path, 4 098 leaves the pair pipeline
    easy = [0, 1, 2]
    assert unfilter_path(1024, easy) == ROWS and unfilter_path(1026, easy) == PAIRS and unfilter_path(1025, easy) == BYTES
    assert unfilter_path(2, easy) == ROWS and unfilter_path(2, [4]) == BYTES and unfilter_path(4, [4]) == PAIRS
    assert unfilter_path(4096, [3]) == PAIRS and unfilter_path(4098, [3]) == BYTES and unfilter_path(4098, easy) == BYTES
    assert unfilter_path(128, easy, out_aligned=False) == BYTES and unfilter_path(128, [4], out_aligned=False) == BYTES
    for kind in EASY_FILTER_KINDS:
        assert row_filters(kind, 130, rng).max() <= 2
    for kind in HARD_FILTER_KINDS:
        assert row_filters(kind, 130, rng).max() >= 3
