#!/usr/bin/env python
"""Freeze scikit-learn's DBSCAN labels for the batch of tests/dbscan_segments_util.py into tests/golden/dbscan_labels.npz, so that
the device can be held to scikit-learn on a machine that has none.  Recorded results only: per parameter set (eps, min_points) of
``GOLDEN_PARAMETERS`` the labels [N] int32 of ``sklearn.cluster.DBSCAN(eps, min_samples=min_points, algorithm="kd_tree")`` run per
segment, plus the batch's row count and offsets, which the loader compares with the batch it builds.

    python tools/gen_dbscan_golden.py            # needs scikit-learn; rewrites the file
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dbscan_segments_util as D  # noqa: E402


def main():
    import sklearn
    rows, offsets, _names, _eps = D.batch()
    out = {"rows": np.int64(len(rows)), "offsets": offsets, "parameters": np.array(D.GOLDEN_PARAMETERS, dtype=np.float64),
           "sklearn_version": np.array(sklearn.__version__)}
    for k, (eps, min_points) in enumerate(D.GOLDEN_PARAMETERS):
        labels, clusters = D.sklearn_labels(rows, offsets, eps, min_points)
        out[f"labels_{k}"] = labels
        print(f"eps {eps} min_points {min_points}: {int(clusters.sum())} clusters, {int((labels < 0).sum())} noise rows of {len(rows)}")
    os.makedirs(os.path.dirname(D.GOLDEN), exist_ok=True)
    np.savez_compressed(D.GOLDEN, **out)
    print(D.GOLDEN, os.path.getsize(D.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
