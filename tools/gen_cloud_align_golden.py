#!/usr/bin/env python3
"""Writes tests/golden/cloud_align.npz: the host twin's outputs (mspa.cloud_segments.rigid_fit_segments_host and
register_segments_host, through csrc/cloud_align_core.h) for the seeded batches of tests/cloud_align_util.py -- the Kabsch batch, its
variant with unmatched rows and shared segments, and the ICP batch at both caps with its history.  No reference can give these bits,
so the fixture freezes the twin's: a compiler, a flag or an edit that moves one bit of the rule shows up against it, on the host and,
through tests/test_gpu_cloud_align.py, on the device.  The batches themselves are seeded and rebuilt by the tests.
    python tools/gen_cloud_align_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "multi-spatialmllm_amd"))
import cloud_align_util as U  # noqa: E402

FIT_KEYS = ("R", "t", "used", "status", "eigen")
ICP_KEYS = ("R", "t", "status", "used", "converged_at", "fitness", "inlier_rmse", "history_used", "history_rmse")


def frozen():
    from mspa import cloud_segments as CS
    q, p, off, _cases = U.kabsch()
    out = {"kabsch_" + k: v for k, v in CS.rigid_fit_segments_host(q, off, p, np.arange(len(q), dtype=np.int64), want_parts=True).items() if k in FIT_KEYS}
    vq, vq_off, vp, pairs, index, _out_off = U.kabsch_variant()
    out.update({"variant_" + k: v for k, v in CS.rigid_fit_segments_host(vq, vq_off, vp, index, pairs, want_parts=True).items() if k in FIT_KEYS})
    iq, iq_off, it, it_off, _truth = U.icp()
    for cap in sorted(U.CAPS.values()):
        reg = CS.register_segments_host(iq, iq_off, it, it_off, max_distance=cap, iterations=12, want_history=True)
        out.update({f"icp{int(cap * 100)}_" + k: reg[k] for k in ICP_KEYS})
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


if __name__ == "__main__":
    os.makedirs(os.path.dirname(U.GOLDEN), exist_ok=True)
    np.savez_compressed(U.GOLDEN, **frozen())
    print(U.GOLDEN, os.path.getsize(U.GOLDEN), "bytes")
