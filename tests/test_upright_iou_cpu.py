"""The upright IoU without a GPU: the host twin (csrc/upright_iou_core.h through mspa_upright_iou_host) against an exact oracle in
``fractions.Fraction`` that shares no code with it (tests/upright_iou_util.py):

  * the twin's footprint area and IoU lie within the header's ``area_bound`` and ``iou_bound`` of the exact values for every accepted
    pair of the batch; the worst observed ratios are printed;
  * 0 <= IoU <= 1, refused pairs are NaN, iou(a, b) and iou(b, a) are the same bytes, identical boxes give exactly 1.0, disjoint pairs
    exactly 0.0, axis-aligned pairs agree with ``ops.calculate_iou_3d``, a 70-box matrix equals its transpose byte for byte;
  * the matrix form against the pairs form, one box against many, empty shapes, the C entry points' MSPA_EINVALs, the ValueErrors;
  * the frozen results of tests/golden/upright_iou.npz are a fresh run's;
  * the header once more as a stand-alone g++ program under AddressSanitizer + UBSan."""
import os
import shutil
import struct
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upright_iou_util as U  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")
fold = lambda text: " ".join(text.split())                                   # noqa: E731


def _ops():
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(ROOT):
            del sys.modules[name]                   # the reference's modules of the same names, left by another test
    from spatial_engine.utils.scannet_utils.handler import ops
    return ops


def _exact(x):
    return Fraction(float(x))


def test_the_batch_is_what_its_docstring_says_and_the_random_pairs_overlap_and_miss_by_the_oracle_alone():
    a, b, names = U.batch()
    assert a.shape == b.shape == (len(names), 8) and len(names) <= 3000 and len(set(names)) == len(names)
    oracle = U.batch_oracle()
    assert [n for n, o in zip(names, oracle) if o is None] == list(U.REFUSED)
    random = [o for n, o in zip(names, oracle) if n.startswith("random-")]
    assert len(random) == U.N_RANDOM
    positive, zero = sum(o[2] is not None and o[2] > 0 for o in random), sum(o[2] == 0 for o in random)
    assert positive >= 0.2 * len(random) and zero >= 0.2 * len(random), (positive, zero)
    area, _dz, iou = oracle[U.index_of("octagon")]
    assert abs(float(area) - 2 * (np.sqrt(2.0) - 1)) < 1e-15
    assert oracle[U.index_of("identical")][2] == 1 and oracle[U.index_of("identical-turned")][2] == 1
    for name in U.ZERO_EXACTLY + ("touch-edge", "touch-corner", "zero-width", "zero-height"):
        assert oracle[U.index_of(name)][2] == 0, name
    assert oracle[U.index_of("both-degenerate")][2] is None
    assert oracle[U.index_of("touch-edge")][0] == 0 and oracle[U.index_of("touch-corner")][0] == 0
    _area, _dz, rect = oracle[U.index_of("rect30")]
    c, s = np.cos(np.deg2rad(30.0)), np.sin(np.deg2rad(30.0))
    assert abs(float(rect) - 1.6 / ((2.0 * c + 0.8 * s) * (2.0 * s + 0.8 * c))) < 1e-14


def test_area_and_iou_are_within_the_headers_bounds_of_the_exact_values_for_every_accepted_pair(capsys):
    from mspa import cloud_segments as CS
    a, b, names = U.batch()
    iou, parts = U.batch_twin()
    area_bound, iou_bound = CS.upright_iou_bound_host(a, b)
    worst_area, worst_iou = (0.0, ""), (0.0, "")
    for i, (name, exact) in enumerate(zip(names, U.batch_oracle())):
        if exact is None:
            assert np.isnan(iou[i]) and np.isnan(parts[i]).all() and np.isnan(area_bound[i]) and np.isnan(iou_bound[i]), name
            continue
        area, dz, value = exact
        error = abs(_exact(parts[i, 0]) - area)
        assert error <= _exact(area_bound[i]), (name, float(error), area_bound[i])
        if error:
            worst_area = max(worst_area, (float(error / _exact(area_bound[i])), name))
        assert (parts[i, 1] > 0) == (dz > 0) or abs(float(dz)) < 1e-9, name
        if value is None:
            assert np.isnan(iou[i]) and np.isnan(iou_bound[i]), name
            continue
        assert 0.0 <= iou[i] <= 1.0, (name, iou[i])
        error = abs(_exact(iou[i]) - value)
        assert error <= _exact(iou_bound[i]), (name, float(error), iou_bound[i])
        if error:
            worst_iou = max(worst_iou, (float(error / _exact(iou_bound[i])), name))
    with capsys.disabled():
        print(f"\nupright IoU, {len(names)} pairs: worst |area - exact| / area_bound = {worst_area[0]:.3g} ({worst_area[1]}), "
              f"worst |iou - exact| / iou_bound = {worst_iou[0]:.3g} ({worst_iou[1]})")
    assert worst_area[0] <= 1.0 and worst_iou[0] <= 1.0


def test_symmetry_identical_disjoint_and_refused_pairs():
    from mspa import cloud_segments as CS
    a, b, names = U.batch()
    iou, parts = U.batch_twin()
    back, back_parts = CS.upright_iou_host(b, a, want_parts=True)
    assert iou.tobytes() == back.tobytes() and parts.tobytes() == back_parts.tobytes()
    assert CS.upright_iou_host(a, b).tobytes() == iou.tobytes()                                  # with and without the second output
    for name in ("identical", "identical-turned"):
        assert iou[U.index_of(name)].tobytes() == np.float64(1.0).tobytes(), name
    for name in U.ZERO_EXACTLY + ("zero-width", "zero-height"):
        assert iou[U.index_of(name)].tobytes() == np.float64(0.0).tobytes(), name
    apart = [i for i, o in enumerate(U.batch_oracle()) if o is not None and o[2] == 0 and names[i].startswith("random-")]
    assert len(apart) > 400 and all(iou[i].tobytes() == np.float64(0.0).tobytes() for i in apart)
    for name in U.REFUSED + ("both-degenerate",):
        assert np.isnan(iou[U.index_of(name)]), name
    assert np.isnan(parts[[U.index_of(n) for n in U.REFUSED]]).all()
    zero_volume = np.array([[1, 2, 3, 2, 1, 0, 1, 0]], dtype=np.float64)                         # identical, volume 0: the 0 / 0
    assert np.isnan(CS.upright_iou_host(zero_volume, zero_volume)[0])
    minus = a[U.index_of("near")].copy()
    minus[2] = 0.0
    plus = minus.copy()
    minus[2] = -0.0                                                                               # a negative zero is the positive one
    other = b[U.index_of("near")]
    assert CS.upright_iou_host(minus, other).tobytes() == CS.upright_iou_host(plus, other).tobytes()
    assert CS.upright_iou_host(minus, plus).tobytes() == np.float64(1.0).tobytes()
    far, near = U.index_of("far"), U.index_of("near")
    # the centres leave by one subtraction: what 10^6 costs is the rounding of the moved centres themselves (2^-34 each), no more
    assert np.abs(parts[far] - parts[near]).max() < 1e-9 and abs(iou[far] - iou[near]) < 1e-9


def test_axis_aligned_pairs_agree_with_calculate_iou_3d_within_the_bound():
    from mspa import cloud_segments as CS
    ops = _ops()
    a6, b6 = U.aabb_pairs()
    a, b = U.aabb_to_upright(a6), U.aabb_to_upright(b6)
    got = CS.upright_iou_host(a, b)
    _area_bound, iou_bound = CS.upright_iou_bound_host(a, b)
    want = np.array([ops.calculate_iou_3d(x, y) for x, y in zip(a6, b6)])
    assert (want > 0).sum() > 100 and (np.abs(got - want) <= iou_bound + 8 * 2.0 ** -53).all()   # (calculate_iou_3d's own few roundings)
    first = U.index_of("aabb-0")
    assert U.batch_twin()[0][first:first + U.N_AABB].tobytes() == got.tobytes()
    assert isinstance(ops.calculate_iou_upright(a[0], b[0]), float) and ops.calculate_iou_upright(a[0], b[0]) == got[0]
    assert ops.calculate_iou_upright(a[0], b[0]) == ops.calculate_iou_upright(b[0], a[0])
    assert "No reference counterpart" in fold(ops.calculate_iou_upright.__doc__) and "calculate_iou_upright" not in ops.__all__
    import torch
    on_host = ops.calculate_iou_upright(torch.from_numpy(a[1].copy()), torch.from_numpy(b[1].copy()))
    assert on_host == got[1]


def test_the_matrix_is_the_pairs_entry_by_entry_and_a_set_against_itself_is_symmetric_as_bytes():
    from mspa import cloud_segments as CS
    boxes = U.matrix_boxes()
    matrix, parts = U.matrix_twin()
    n = len(boxes)
    assert matrix.shape == (n, n) and parts.shape == (n, n, 2)
    assert matrix.tobytes() == np.ascontiguousarray(matrix.T).tobytes()
    assert parts.tobytes() == np.ascontiguousarray(parts.transpose(1, 0, 2)).tobytes()
    diagonal = np.diag(matrix)
    assert np.isnan(diagonal[11]) and (np.delete(diagonal, 11) == 1.0).all() and matrix[3, 7] == 1.0
    assert np.isnan(matrix[11]).all() and np.isfinite(np.delete(np.delete(matrix, 11, 0), 11, 1)).all()
    rows, cols = np.divmod(np.arange(n * n), n)
    pairs, pair_parts = CS.upright_iou_host(boxes[rows], boxes[cols], want_parts=True)
    assert pairs.tobytes() == matrix.tobytes() and pair_parts.tobytes() == parts.tobytes()
    a, b, _names = U.batch()
    grouped = CS.upright_iou_matrix_host(a[:6].reshape(2, 3, 8), b[:10].reshape(2, 5, 8))        # [2, 3, 8] against [2, 5, 8]
    assert grouped.shape == (2, 3, 5)
    for g in range(2):
        for i in range(3):
            assert grouped[g, i].tobytes() == CS.upright_iou_host(a[3 * g + i], b[5 * g:5 * g + 5]).tobytes()


def test_one_box_against_many_and_the_empty_shapes():
    from mspa import cloud_segments as CS
    a, b, _names = U.batch()
    iou, _parts = U.batch_twin()
    one = a[U.index_of("near")]
    many = CS.upright_iou_host(one, b[:65])
    assert many.shape == (65,) and many.tobytes() == CS.upright_iou_host(np.broadcast_to(one, (65, 8)), b[:65]).tobytes()
    assert CS.upright_iou_host(b[:65], one.reshape(1, 8)).tobytes() == many.tobytes()
    assert CS.upright_iou_host(one, b[5]).shape == () and CS.upright_iou_host(a[5:6], b[5:6]).shape == (1,)
    assert CS.upright_iou_host(a[:12].reshape(3, 4, 8), b[:12].reshape(3, 4, 8)).tobytes() == iou[:12].tobytes()
    empty = np.zeros((0, 8))
    out, parts = CS.upright_iou_host(empty, empty, want_parts=True)
    assert out.shape == (0,) and parts.shape == (0, 2)
    assert CS.upright_iou_host(one, empty).shape == (0,)
    assert CS.upright_iou_matrix_host(empty, b[:4]).shape == (0, 4) and CS.upright_iou_matrix_host(a[:4], empty).shape == (4, 0)
    assert CS.upright_iou_matrix_host(np.zeros((2, 0, 8)), np.zeros((2, 3, 8))).shape == (2, 0, 3)
    area_bound, iou_bound = CS.upright_iou_bound_host(empty, empty)
    assert area_bound.shape == iou_bound.shape == (0,)


def test_the_python_functions_refuse_wrong_shapes_and_dtypes():
    from mspa import cloud_segments as CS
    a, b, _names = U.batch()
    for call in (CS.upright_iou_host, CS.upright_iou_matrix_host):
        with pytest.raises(ValueError):
            call(a[:4].astype(np.float32), b[:4])
        with pytest.raises(ValueError):
            call(a[:4, :6], b[:4, :6])
        with pytest.raises(ValueError):
            call(a[:4], b[:4].astype(np.float32))
    with pytest.raises(ValueError):
        CS.upright_iou_host(a[:4], b[:5])
    with pytest.raises(ValueError):
        CS.upright_iou_host(a[:4].reshape(2, 2, 8), b[:4])
    with pytest.raises(ValueError):
        CS.upright_iou_matrix_host(a[:8].reshape(2, 4, 8), b[:9].reshape(3, 3, 8))
    with pytest.raises(ValueError):
        CS.upright_iou_matrix_host(a[0], b[:4])
    with pytest.raises(ValueError):
        CS.upright_iou_bound_host(a[:4], b[:5])
    for call in (CS.upright_iou, CS.upright_iou_matrix):
        with pytest.raises((ValueError, RuntimeError)):
            call(a[:4], b[:4])                                               # NumPy boxes have no device: no quiet fallback
    sentence = "Enqueue only: one launch on the current stream and nothing is read back."
    assert sentence in fold(CS.upright_iou.__doc__) and sentence in fold(CS.upright_iou_matrix.__doc__)
    assert "Enqueue only" in fold(CS.upright_of_aabb.__doc__)
    assert "not a fallback" in fold(CS.upright_iou_host.__doc__) and "not a fallback" in fold(CS.upright_iou_matrix_host.__doc__)


def test_upright_of_aabb_on_the_host_is_the_numpy_restatement():
    import torch
    from mspa import cloud_segments as CS
    a6, _b6 = U.aabb_pairs()
    boxes = np.concatenate([a6, [[0, 0, 0, 1, 1, 2], [1, 2, 3, 0.5, 2, 1], [np.nan] * 6, [0, 0, 0, 1, np.nan, 1]]])
    got = CS.upright_of_aabb(torch.from_numpy(boxes)).numpy()
    assert got.tobytes() == U.aabb_to_upright(boxes).tobytes()
    assert got[-4].tolist() == [0, 0, 0, 1, 1, 2, 1, 0] and got[-3].tolist() == [1, 2, 3, 2, 0.5, 1, 0, 1]
    assert np.isnan(got[-2:]).all()
    assert CS.upright_of_aabb(torch.from_numpy(boxes.reshape(2, -1, 6))).shape == (2, len(boxes) // 2, 8)


def test_the_c_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    """Every refusal below returns MSPA_EINVAL from the argument checks; none of the pointers is a device pointer, and none is ever
    dereferenced as one (the checks come before the launch)."""
    from mspa import _lib
    lib = _lib.load()
    a, b = np.zeros((6, 8)), np.zeros((6, 8))
    out, parts = np.zeros(36), np.zeros((36, 2))
    p = lambda x: x.ctypes.data                                              # noqa: E731
    PAIRS, MATRIX = _lib.UPRIGHT_IOU_PAIRS, _lib.UPRIGHT_IOU_MATRIX

    def device(pa=6, pb=6, g=0, ra=0, rb=0, mode=PAIRS, a_p=p(a), b_p=p(b), out_p=p(out), parts_p=p(parts)):
        return lib.mspa_upright_iou_device(a_p, pa, b_p, pb, g, ra, rb, mode, out_p, parts_p, None)

    def host(pa=6, pb=6, g=0, ra=0, rb=0, mode=PAIRS, a_p=p(a), b_p=p(b), out_p=p(out), parts_p=p(parts)):
        return lib.mspa_upright_iou_host(a_p, pa, b_p, pb, g, ra, rb, mode, out_p, parts_p)

    refused = {}
    for name, call in (("device", device), ("host", host)):
        refused.update({
            f"{name}: negative Pa": call(pa=-1), f"{name}: negative Pb": call(pb=-1), f"{name}: Pa != Pb": call(pa=6, pb=5),
            f"{name}: pairs with G": call(g=1), f"{name}: pairs with A": call(ra=6), f"{name}: pairs with B": call(rb=6),
            f"{name}: matrix, Pa != G A": call(g=2, ra=2, rb=3, mode=MATRIX), f"{name}: matrix, Pb != G B": call(g=2, ra=3, rb=2, mode=MATRIX),
            f"{name}: matrix, negative G": call(g=-2, ra=-3, rb=-3, mode=MATRIX), f"{name}: matrix, negative B": call(g=2, ra=3, rb=-3, mode=MATRIX),
            f"{name}: unknown mode": call(mode=2), f"{name}: more than 2^31 pairs": call(pa=(1 << 31) + 1, pb=(1 << 31) + 1),
            f"{name}: more than 2^31 cells": call(pa=1 << 20, pb=1 << 20, g=1, ra=1 << 20, rb=1 << 20, mode=MATRIX),
            f"{name}: cells that overflow": call(pa=1 << 62, pb=1 << 62, g=1 << 31, ra=1 << 31, rb=1 << 31, mode=MATRIX),
            f"{name}: null a": call(a_p=None), f"{name}: null b": call(b_p=None), f"{name}: null out": call(out_p=None),
            f"{name}: a at 4 mod 8": call(a_p=p(a) + 4), f"{name}: b at 4 mod 8": call(b_p=p(b) + 4),
            f"{name}: out at 4 mod 8": call(out_p=p(out) + 4), f"{name}: parts at 4 mod 8": call(parts_p=p(parts) + 4)})
    bounds = np.zeros((2, 6))
    refused.update({"bound: negative P": lib.mspa_upright_iou_bound_host(p(a), p(b), -1, p(bounds[0]), p(bounds[1])),
                    "bound: null a": lib.mspa_upright_iou_bound_host(None, p(b), 6, p(bounds[0]), p(bounds[1])),
                    "bound: null out": lib.mspa_upright_iou_bound_host(p(a), p(b), 6, p(bounds[0]), None)})
    assert {k: v for k, v in refused.items() if v != _lib.MSPA_EINVAL} == {}
    assert b"mspa_upright_iou_bound_host" in lib.mspa_last_error_string()
    # zero outputs: nothing is enqueued, and the pointers of the empty sides may be null
    assert device(pa=0, pb=0, a_p=None, b_p=None, out_p=None, parts_p=None) == 0
    assert device(pa=1, pb=0, b_p=None, out_p=None, parts_p=None) == 0
    assert device(pa=0, pb=0, g=0, ra=3, rb=4, mode=MATRIX, a_p=None, b_p=None, out_p=None, parts_p=None) == 0
    assert device(pa=6, pb=0, g=2, ra=3, rb=0, mode=MATRIX, b_p=None, out_p=None, parts_p=None) == 0
    assert host() == 0 and host(parts_p=None) == 0 and host(pa=1) == 0 and host(g=2, ra=3, rb=3, mode=MATRIX) == 0      # the good arguments are good


def test_the_frozen_results_are_a_fresh_runs():
    frozen = U.golden()
    iou, parts = U.batch_twin()
    matrix, matrix_parts = U.matrix_twin()
    assert frozen["iou"].tobytes() == iou.tobytes() and frozen["parts"].tobytes() == parts.tobytes()
    assert frozen["matrix"].tobytes() == matrix.tobytes() and frozen["matrix_parts"].tobytes() == matrix_parts.tobytes()
    assert os.path.getsize(U.GOLDEN) < 1 << 20


# One record: int64 P, P * 8 float64 a, P * 8 float64 b -> P float64 iou, P * 2 float64 parts, P float64 area bounds, P float64 IoU
# bounds; then the P x P matrix of a against b (P * P float64).  Every buffer is a heap block of exactly its size.
DRIVER = r"""
#include "upright_iou_core.h"
#include <cstdio>
#include <cstdlib>
template <typename T> static T *block(int64_t n) { return (T *)malloc((size_t)(n > 0 ? n : 1) * sizeof(T)); }
int main() {
    int64_t P;
    while (fread(&P, 8, 1, stdin) == 1) {
        double *a = block<double>(P * 8), *b = block<double>(P * 8), *iou = block<double>(P), *parts = block<double>(P * 2);
        double *area_bound = block<double>(P), *iou_bound = block<double>(P), *matrix = block<double>(P * P);
        if (fread(a, 8, (size_t)(P * 8), stdin) != (size_t)(P * 8) || fread(b, 8, (size_t)(P * 8), stdin) != (size_t)(P * 8)) return 4;
        const mspa::uiou::Shape pairs = mspa::uiou::shape_of(P, P, 0, 0, 0, mspa::uiou::kPairs);
        const mspa::uiou::Shape cells = mspa::uiou::shape_of(P, P, 1, P, P, mspa::uiou::kMatrix);
        if (pairs.outputs != P || cells.outputs != P * P) return 5;
        mspa::uiou::iou_all(a, b, pairs, iou, parts);
        mspa::uiou::iou_all(a, b, cells, matrix, nullptr);
        for (int64_t i = 0; i < P; ++i) mspa::uiou::pair_bounds(a + 8 * i, b + 8 * i, area_bound[i], iou_bound[i]);
        fwrite(iou, 8, (size_t)P, stdout);
        fwrite(parts, 8, (size_t)(P * 2), stdout);
        fwrite(area_bound, 8, (size_t)P, stdout);
        fwrite(iou_bound, 8, (size_t)P, stdout);
        fwrite(matrix, 8, (size_t)(P * P), stdout);
        void *all[] = {a, b, iou, parts, area_bound, iou_bound, matrix};
        for (void *p : all) free(p);
    }
    return 0;
}
"""


def test_the_header_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    from mspa import cloud_segments as CS
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, str(tmp_path / "driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    a, b, _names = U.batch()
    boxes = U.matrix_boxes()
    records = [(a[:300], b[:300]), (boxes, boxes), (np.zeros((0, 8)), np.zeros((0, 8)))]
    inp = b"".join(struct.pack("<q", len(x)) + np.asarray(x, dtype="<f8").tobytes() + np.asarray(y, dtype="<f8").tobytes() for x, y in records)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    at = 0

    def take(count):
        nonlocal at
        got = np.frombuffer(run.stdout, dtype="<f8", count=count, offset=at)
        at += got.nbytes
        return got

    for x, y in records:
        P = len(x)
        iou, parts, area_bound, iou_bound, matrix = take(P), take(2 * P), take(P), take(P), take(P * P)
        want, want_parts = CS.upright_iou_host(x, y, want_parts=True)
        assert iou.tobytes() == want.tobytes() and parts.tobytes() == want_parts.tobytes()
        bounds = CS.upright_iou_bound_host(x, y)
        assert area_bound.tobytes() == bounds[0].tobytes() and iou_bound.tobytes() == bounds[1].tobytes()
        assert matrix.tobytes() == CS.upright_iou_matrix_host(x, y).tobytes()
    assert at == len(run.stdout)
