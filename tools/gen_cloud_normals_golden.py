#!/usr/bin/env python3
"""Writes tests/golden/cloud_normals.npz: the host twin's outputs (mspa.cloud_segments.normals_segments_host and knn_segments_host,
through csrc/cloud_normals_core.h) for the fixture segments of tests/cloud_normals_util.py -- the normals with viewpoints at K, the
counts and statuses under the cap, and a neighbour table at k = 3.  No reference can give these bits, so the fixture freezes the
twin's: a compiler, a flag or an edit that moves one bit of the rule shows up against it, on the host and, through
tests/test_gpu_cloud_normals.py, on the device.  The batch itself is seeded and rebuilt by the tests.  Arrays only.
    python tools/gen_cloud_normals_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "multi-spatialmllm_amd"))
import cloud_normals_util as U  # noqa: E402

TABLE_K = 3
PLANE_KEYS = ("R", "t", "status", "used", "converged_at", "fitness", "inlier_rmse")
STEP_KEYS = ("R", "t", "status", "used", "rmse")


def frozen():
    from mspa import cloud_segments as CS
    xyz, off, views = U.fixture_batch()
    out = {"viewed_" + k: v for k, v in CS.normals_segments_host(xyz, off, U.K, None, views).items()}
    capped = CS.normals_segments_host(xyz, off, U.K, U.CAP)
    out.update(capped_used=capped["used"], capped_status=capped["status"])
    index, distance = CS.knn_segments_host(xyz, off, TABLE_K)
    out.update(table_index=index.astype(np.int32), table_distance=distance)
    q, q_off, t, t_off, _truth, normals = U.plane_batch()             # the point-to-plane loop on the ICP batch, and its first step alone
    reg = CS.register_segments_host(q, q_off, t, t_off, max_distance=0.05, iterations=U.PLANE_ITERATIONS, estimation="point_to_plane", normals=normals)
    out.update({"plane_" + k: reg[k] for k in PLANE_KEYS})
    found = CS.nearest_segments_host(q, q_off, t, t_off, None, 0.05)
    step = CS.plane_fit_segments_host(q, q_off, t, normals, found["index"])
    out.update({"step_" + k: step[k] for k in STEP_KEYS})
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


if __name__ == "__main__":
    os.makedirs(os.path.dirname(U.GOLDEN), exist_ok=True)
    np.savez_compressed(U.GOLDEN, **frozen())
    print(U.GOLDEN, os.path.getsize(U.GOLDEN), "bytes")
