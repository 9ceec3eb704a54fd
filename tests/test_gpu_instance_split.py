"""engine.instance_split (mspa_instance_split_count / _scatter) against the NumPy restatement of tests/instance_split_util.py, bit
for bit: counts, offsets, xyz, rgb, pixel, lo / hi.  Pixel counts around a wave and a tile and one ScanNet-shaped frame (162 x 121),
one and three frames, the label patterns that stress the ranking (64 distinct labels per wave, a label only in the last partial
wave, a label with no valid pixel, no selection at all).  Every case runs twice and must give identical bytes: the order of the
rows must not depend on how the workgroups were scheduled."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from instance_split_util import FRAMES, PATTERNS, SIZES, assert_same, hw_of, make_case, numpy_split  # noqa: E402


def _run(labels, valid, xyz, rgb):
    import torch
    from mspa import engine
    got = engine.instance_split(torch.from_numpy(labels).cuda(), torch.from_numpy(valid).cuda(), torch.from_numpy(xyz).cuda(),
                                None if rgb is None else torch.from_numpy(rgb).cuda())
    torch.cuda.synchronize()
    return tuple(g.cpu().numpy() if isinstance(g, torch.Tensor) else g for g in got)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("F", FRAMES)
def test_split_equals_numpy_and_repeats(F, pattern):
    for P in SIZES:
        labels, valid, xyz, rgb = make_case(F, P, pattern, seed=F * 1000 + P)        # the CPU test's inputs
        want = numpy_split(labels, valid, xyz, rgb)
        first = _run(labels, valid, xyz, rgb)
        assert_same(first, want, (F, P, pattern))
        assert_same(_run(labels, valid, xyz, rgb), first, (F, P, pattern, "second run"))
        if P in (65, 4097):
            assert_same(_run(labels, valid, xyz, None), numpy_split(labels, valid, xyz, None), (F, P, pattern, "no rgb"))


def test_arguments_are_checked():
    import torch
    from mspa import engine
    labels, valid, xyz, rgb = make_case(2, 65, "blocky", 1)
    H, W = hw_of(65)
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    with pytest.raises(ValueError):
        engine.instance_split(t(labels), t(valid[:1]), t(xyz), None)
    with pytest.raises(ValueError):
        engine.instance_split(t(labels), t(valid), t(xyz.astype(np.float32)), None)
    with pytest.raises(ValueError):
        engine.instance_split(t(labels), t(valid), t(xyz), t(rgb[:, :, :W - 1]))
    with pytest.raises(ValueError):
        engine.instance_split(t(labels.astype(np.int16)), t(valid), t(xyz), None)
    with pytest.raises(ValueError):
        engine.instance_split(labels, t(valid), t(xyz), None)
