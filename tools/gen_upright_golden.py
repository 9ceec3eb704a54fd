#!/usr/bin/env python
"""Freeze the upright boxes of the batch of tests/upright_box_util.py into tests/golden/upright_boxes.npz.  Recorded results only:
the host twin's hull indices, hull offsets, chosen edges and boxes, plus the batch's row count and offsets, which the loader
compares with the batch it builds.  Before anything is written the twin is held to the exact oracle of the same utilities: its hull
must be the oracle's vertex for vertex, and the exact m of every chosen edge must lie within the header's bound of the exact minimum.

    python tools/gen_upright_golden.py            # needs the built library (its host twin); rewrites the file
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "multi-spatialmllm_amd"))
import upright_box_util as B  # noqa: E402


def main():
    rows, offsets, names = B.batch()
    boxes, index, hull_offsets, edges = B.batch_twin()
    for s, (name, hull, exact) in enumerate(zip(names, B.batch_oracle(), B.batch_measures())):
        assert index[hull_offsets[s]:hull_offsets[s + 1]].tolist() == hull, name
        if exact is not None:
            m, diagonal_sq = exact
            assert m[int(edges[s])] - min(m) <= B.RECT_BOUND * diagonal_sq, name
        print(f"{name:20s} rows {offsets[s + 1] - offsets[s]:6d} hull {len(hull):5d} edge {int(edges[s]):5d}")
    os.makedirs(os.path.dirname(B.GOLDEN), exist_ok=True)
    np.savez_compressed(B.GOLDEN, rows=np.int64(len(rows)), offsets=offsets, boxes=boxes, hull_index=index, hull_offsets=hull_offsets,
                        edges=edges)
    print(B.GOLDEN, os.path.getsize(B.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
