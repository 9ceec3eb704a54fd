"""The instance split's rule and decomposition on the CPU: mspa_instance_split_host walks csrc/instance_split_core.h -- tile
histograms, their scan, ballot ranks inside a wave, the waves' counts of a round -- exactly as the kernels do, and must give the
NumPy restatement ``np.flatnonzero((labels == v) & valid)`` per label, byte for byte.  Walking the tiles and the waves in the
opposite order must not change a byte: that is the stability argument (no term of a row's position depends on execution order)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from instance_split_util import FRAMES, PATTERNS, SIZES, assert_same, make_case, numpy_split  # noqa: E402


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("F", FRAMES)
def test_host_split_equals_numpy_in_either_order(F, pattern):
    from mspa import engine
    for P in SIZES:
        labels, valid, xyz, rgb = make_case(F, P, pattern, seed=F * 1000 + P)
        want = numpy_split(labels, valid, xyz, rgb)
        for rev in (False, True):
            assert_same(engine.instance_split_host(labels, valid, xyz, rgb, reversed_order=rev), want, (F, P, pattern, rev))
        assert_same(engine.instance_split_host(labels, valid, xyz, None), numpy_split(labels, valid, xyz, None), (F, P, pattern, "no rgb"))


def test_case_list_reaches_the_edges():
    """The patterns do what their names say at the sizes used: 64 distinct labels in a wave, a label confined to the last partial
    wave, a label with no valid pixel, an empty selection."""
    labels, valid, _, _ = make_case(1, 4097, "round_robin", 1)
    assert len(set(labels.reshape(-1)[:64].tolist())) == 64 and labels.min() == 1 and labels.max() == 255
    labels, valid, xyz, _ = make_case(3, 4097, "last_wave", 2)
    assert (np.argwhere(labels.reshape(3, -1) == 9)[:, 1] == 4096).all()
    assert numpy_split(labels, valid, xyz)[0][:, 9].tolist() == [1, 1, 1]
    labels, valid, xyz, _ = make_case(1, 4096, "all_invalid", 3)
    c = numpy_split(labels, valid, xyz)[0]
    assert (labels == 5).any() and c[0, 5] == 0 and c[0, 4] > 0 and c[0, 6] > 0
    labels, valid, xyz, _ = make_case(3, 65, "zero", 4)
    assert numpy_split(labels, valid, xyz)[1][-1] == 0


def test_workspace_bytes_and_argument_checks():
    from mspa import _lib
    lib = _lib.load()
    assert lib.mspa_instance_split_workspace_bytes(3, 4097) == 3 * 2 * 256 * 4
    assert lib.mspa_instance_split_workspace_bytes(1, 0) == 16
    assert lib.mspa_instance_split_workspace_bytes(65536, 10) == -1 and lib.mspa_instance_split_workspace_bytes(1, 2 ** 31) == -1
    assert lib.mspa_instance_split_host(None, None, None, None, 1, 5, None, None, None, None, None, None, None, None, 0) == _lib.MSPA_EINVAL
