#!/usr/bin/env python
"""Freeze the upright IoUs of the batch of tests/upright_iou_util.py into tests/golden/upright_iou.npz.  Recorded results only: the
host twin's IoU and (area, dz) of every pair of the batch and of the 70-box matrix, plus the batch's pair count and a checksum of its
boxes, which the loader compares with the batch it builds.  Before anything is written the twin is held to the exact oracle of the
same utilities: every accepted pair's area and IoU must lie within the header's bounds of the exact values.

    python tools/gen_upright_iou_golden.py        # needs the built library (its host twin); rewrites the file
"""
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "multi-spatialmllm_amd"))
import upright_iou_util as U  # noqa: E402


def main():
    from mspa import cloud_segments as CS
    a, b, names = U.batch()
    iou, parts = U.batch_twin()
    area_bound, iou_bound = CS.upright_iou_bound_host(a, b)
    for i, (name, exact) in enumerate(zip(names, U.batch_oracle())):
        if exact is None or exact[2] is None:
            assert np.isnan(iou[i]), name
            continue
        assert abs(Fraction(float(parts[i, 0])) - exact[0]) <= Fraction(float(area_bound[i])), name
        assert abs(Fraction(float(iou[i])) - exact[2]) <= Fraction(float(iou_bound[i])), name
    matrix, matrix_parts = U.matrix_twin()
    os.makedirs(os.path.dirname(U.GOLDEN), exist_ok=True)
    np.savez_compressed(U.GOLDEN, pairs=np.int64(len(a)), a_sum=np.float64(np.nansum(a)), iou=iou, parts=parts, matrix=matrix,
                        matrix_parts=matrix_parts)
    print(U.GOLDEN, os.path.getsize(U.GOLDEN), "bytes;", len(a), "pairs,", matrix.shape, "matrix")


if __name__ == "__main__":
    main()
