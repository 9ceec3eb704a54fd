#!/usr/bin/env python3
"""Writes tests/golden/cloud_distance.npz: the brute-force oracle's outputs (tests/cloud_distance_util.py: NumPy alone, no code of the
library) for the pairs of the test batch from the identity pair of segment 8 on -- ``distance``, ``index`` and ``offsets`` -- and the
NumPy restatement of the six per-pair summaries at ``TAU`` for them.  The batch itself is seeded and rebuilt by the tests.
    python tools/gen_cloud_distance_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cloud_distance_util as U  # noqa: E402

FIRST_PAIR = 8


def frozen():
    t, t_off, q, q_off, pairs = U.batch()
    distance, index, offsets = U.oracle(t, t_off, q, q_off, pairs[FIRST_PAIR:])
    out = {"first_pair": np.int64(FIRST_PAIR), "distance": distance, "index": index, "offsets": offsets}
    out.update({"fit_" + k: v for k, v in U.fit_oracle(distance, offsets, U.TAU).items()})
    return out


if __name__ == "__main__":
    os.makedirs(os.path.dirname(U.GOLDEN), exist_ok=True)
    np.savez_compressed(U.GOLDEN, **frozen())
    print(U.GOLDEN, os.path.getsize(U.GOLDEN), "bytes")
