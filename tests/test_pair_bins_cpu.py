"""The sampler's bin rule of csrc/pair_bins_core.h on the CPU: a g++ build of the header (plain, and a second time under
AddressSanitizer + UBSan, a stand-alone program with exactly sized heap buffers) and the library's host entry point
(mspa_pair_bin_codes_host) against the host line's own means -- the ``== 0`` split, ``pd.cut(x, edges, include_lowest=True)``,
``dropna`` -- on every edge, one ulp on either side of each, +-0, NaN, +-inf and values outside the range."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairtable_util as PU  # noqa: E402

from mspa import _lib, engine  # noqa: E402

pytest.importorskip("pandas")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")

# Records until the input ends: int64 n, int64 n_edges, edges (float64), x (float64) -> n codes (uint8), 256 counts (int64).
# edges, x and the outputs are heap blocks of exactly their sizes: a read or a write outside them is the sanitizer's to report.
DRIVER = r"""
#include "pair_bins_core.h"
#include <cstdio>
#include <cstdlib>
using namespace mspa::pair_bins;
int main() {
    int64_t head[2];
    while (fread(head, 8, 2, stdin) == 2) {
        const int64_t n = head[0], ne = head[1];
        double *edges = (double *)malloc((size_t)ne * 8), *x = (double *)malloc((size_t)n * 8);
        uint8_t *codes = (uint8_t *)malloc((size_t)n);
        int64_t *counts = (int64_t *)malloc((size_t)kClasses * 8);
        if (fread(edges, 8, (size_t)ne, stdin) != (size_t)ne) return 4;
        if (n && fread(x, 8, (size_t)n, stdin) != (size_t)n) return 4;
        classify_all(x, n, edges, (int32_t)ne, codes, counts);
        if (n) fwrite(codes, 1, (size_t)n, stdout);
        fwrite(counts, 8, (size_t)kClasses, stdout);
        free(edges);
        free(x);
        free(codes);
        free(counts);
    }
    return 0;
}
"""


def _build(tmp_path_factory, name, flags):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp(name)
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, str(d / "driver.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "pair_bins_driver", ["-O2"])


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    return _build(tmp_path_factory, "pair_bins_driver_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, cases):
    """cases: [(x, edges)] -> [(codes, counts)], one run."""
    inp = b"".join(struct.pack("<qq", len(x), len(e)) + np.asarray(e, dtype="<f8").tobytes() + np.asarray(x, dtype="<f8").tobytes()
                   for x, e in cases)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    out, o = [], 0
    for x, _e in cases:
        codes = np.frombuffer(run.stdout, dtype=np.uint8, count=len(x), offset=o)
        counts = np.frombuffer(run.stdout, dtype="<i8", count=256, offset=o + len(x))
        out.append((codes, counts))
        o += len(x) + 256 * 8
    assert o == len(run.stdout)
    return out


@pytest.fixture(scope="module")
def cases():
    """(x, edges as the sampler makes them, the classes pd.cut gives) per edge set; x shared."""
    x = np.concatenate([PU.edge_values(), PU.overlap_column(4000, 3)])
    return [(x, PU.edges_of(*s), PU.cut_reference(x, PU.edges_of(*s))) for s in PU.EDGE_SETS]


def _check(results, cases):
    for (codes, counts), (x, edges, want) in zip(results, cases):
        assert np.array_equal(codes, want), (edges[:3], x[codes != want][:8], codes[codes != want][:8], want[codes != want][:8])
        assert np.array_equal(counts, np.bincount(want, minlength=256))


def test_the_header_agrees_with_pd_cut(driver, cases):
    _check(_run(driver, [(x, e) for x, e, _w in cases]), cases)
    # every class occurs: each bin of each set, the zero part, the dropped rows
    for _x, edges, want in cases:
        assert set(want.tolist()) == set(range(len(edges) - 1)) | {_lib.PAIR_CLASS_ZERO, _lib.PAIR_CLASS_DROPPED}


def test_the_header_under_sanitizers(sanitized_driver, cases):
    small = [(x[:700], e, w[:700]) for x, e, w in cases] + [(x[:0], e, w[:0]) for x, e, w in cases[:1]]
    _check(_run(sanitized_driver, [(x, e) for x, e, _w in small]), small)


def test_the_library_and_the_numpy_restatement_agree(cases):
    for x, edges, want in cases:
        codes, counts = engine.pair_bin_codes_host(x, edges)
        assert np.array_equal(codes, want) and np.array_equal(counts, np.bincount(want, minlength=256))
        assert np.array_equal(PU.classify_numpy(x, edges.astype(np.float64)), want)


def test_the_host_entry_refuses_what_it_cannot_take():
    x = np.zeros(4)
    for edges in ([1.0], [1.0, 1.0], [2.0, 1.0], [0.0, np.nan], np.arange(0.0, 252.0)):
        with pytest.raises(_lib.MspaError):
            engine.pair_bin_codes_host(x, edges)
    codes, counts = engine.pair_bin_codes_host(np.zeros(0), [0.0, 1.0])
    assert len(codes) == 0 and counts.sum() == 0
