"""Average linkage + fcluster (csrc/linkage_core.h) on the CPU, against SciPy: a g++ build of the header over seeded matrices of
the three kinds that exercise the tie rules, the special matrices (all zeros, duplicate rows, a merge exactly on the threshold,
non-finite entries), and the argument checks of the C entry points.  Z is compared byte for byte, the labels value for value;
no case is excluded on tie grounds."""
import ctypes
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linkage_util as LU  # noqa: E402

from mspa import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")

# Reads records (int32 n, int32 pad, float64 threshold, n * n float64) until the input ends; writes per record int32 status,
# int32 n, Z [n - 1, 4] float64, labels [n] int32.  The input matrix is checked to be unchanged (exit 7).
DRIVER = r"""
#include "linkage_core.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace mspa::linkage;
int main() {
    int32_t head[2];
    double thr;
    while (fread(head, 4, 2, stdin) == 2) {
        const int n = head[0];
        if (fread(&thr, 8, 1, stdin) != 1) return 3;
        std::vector<double> m((size_t)n * n), Z((size_t)(n - 1) * 4, -1.0);
        if (fread(m.data(), 8, m.size(), stdin) != m.size()) return 4;
        const std::vector<double> before(m);
        std::vector<int32_t> labels((size_t)n, -1);
        const int32_t out[2] = {block_host(m.data(), n, thr, Z.data(), labels.data()), n};
        if (memcmp(before.data(), m.data(), m.size() * 8) != 0) return 7;
        fwrite(out, 4, 2, stdout);
        fwrite(Z.data(), 8, Z.size(), stdout);
        fwrite(labels.data(), 4, labels.size(), stdout);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("linkage_driver")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    build = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, str(d / "driver.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def _run(exe, jobs):
    """jobs: [(matrix [n, n], threshold)] -> [(status, Z, labels)], one driver run."""
    inp = b"".join(struct.pack("<iid", m.shape[0], 0, t) + np.ascontiguousarray(m, dtype=np.float64).tobytes() for m, t in jobs)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=600)
    assert run.returncode == 0, run.returncode
    out, o = [], 0
    for m, _ in jobs:
        n = m.shape[0]
        status, n_out = struct.unpack_from("<ii", run.stdout, o)
        assert n_out == n
        o += 8
        Z = np.frombuffer(run.stdout, np.float64, (n - 1) * 4, o).reshape(n - 1, 4)
        o += (n - 1) * 32
        labels = np.frombuffer(run.stdout, np.int32, n, o)
        o += n * 4
        out.append((status, Z, labels))
    assert o == len(run.stdout)
    return out


def _check(exe, jobs):
    differing = []
    for (m, t), (status, Z, labels) in zip(jobs, _run(exe, jobs)):
        want_Z, want_labels = LU.scipy_answer(m, t)
        if status != 0 or Z.tobytes() != want_Z.tobytes() or not np.array_equal(labels, want_labels):
            differing.append((m.shape[0], t, status))
    assert not differing, differing[:20]


def test_equals_scipy_on_seeded_matrices(driver):
    jobs = []
    for n in range(2, 65):
        for kind in LU.KINDS:
            for seed in (0, 1):
                m = LU.matrix(kind, n, seed)
                jobs += [(m, t) for t in LU.thresholds(m)]
    assert len(jobs) > 63 * 3 * 2
    _check(driver, jobs)


def test_special_matrices(driver):
    zeros = [np.zeros((n, n)) for n in (2, 3, 17, 64)]
    dup = LU.duplicate_rows()
    edge = LU.on_threshold()
    _check(driver, [(m, 0.1) for m in zeros] + [(m, 0.0) for m in zeros] + [(dup, 0.1), (dup, 0.0), (edge, 0.1), (edge, 0.05)])
    (status, Z, labels), = _run(driver, [(edge, 0.1)])
    assert status == 0 and Z[-1, 2] == 0.1 and labels.tolist() == [1, 1, 1, 1]          # exactly on the threshold: one cluster
    (_, _, labels), = _run(driver, [(edge, np.nextafter(0.1, 0.0))])
    assert labels.tolist() == [1, 1, 2, 2]


def test_non_finite_gives_status_1(driver):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    for value in (np.nan, np.inf, -np.inf):
        for n, (i, j) in ((2, (0, 1)), (9, (3, 7)), (33, (0, 32))):
            m = LU.matrix("continuous", n, 11)
            m[i, j] = m[j, i] = value
            with pytest.raises(ValueError, match="only finite values"):
                linkage(squareform(m, checks=False), method="average")
            (status, Z, labels), = _run(driver, [(m, 0.1)])
            assert status == _lib.LINKAGE_NONFINITE and not Z.any() and not labels.any()


def test_entry_points_validate_before_launching():
    """Bad sizes, null pointers, too many points and a short or misaligned workspace come back as MSPA_EINVAL, empty inputs as
    MSPA_OK -- no HIP call either way."""
    lib = _lib.load()
    dummy = ctypes.c_void_p(64)
    big = 1 << 40
    P_max = _lib.LINKAGE_MAX_POINTS
    assert P_max >= 2048
    call = lib.mspa_track_linkage
    assert call(dummy, -1, 8, 0.1, dummy, dummy, dummy, dummy, big, None) == _lib.MSPA_EINVAL
    assert call(dummy, 1, -8, 0.1, dummy, dummy, dummy, dummy, big, None) == _lib.MSPA_EINVAL
    assert call(dummy, 1, 8, 0.1, dummy, dummy, dummy, dummy, -1, None) == _lib.MSPA_EINVAL
    assert call(dummy, 1, P_max + 1, 0.1, dummy, dummy, dummy, dummy, big, None) == _lib.MSPA_EINVAL
    assert b"MSPA_LINKAGE_MAX_POINTS" in lib.mspa_last_error_string()
    for hole in range(5):
        args = [dummy] * 5
        args[hole] = None
        assert call(args[0], 1, 8, 0.1, args[1], args[2], args[3], args[4], big, None) == _lib.MSPA_EINVAL
        assert b"null pointer" in lib.mspa_last_error_string()
    need = lib.mspa_track_linkage_workspace_bytes(3, 8)
    assert need >= 3 * 8 * 8 * 8 and need % 16 == 0
    assert call(dummy, 3, 8, 0.1, dummy, dummy, dummy, dummy, need - 1, None) == _lib.MSPA_EINVAL
    assert b"workspace smaller" in lib.mspa_last_error_string()
    assert call(dummy, 3, 8, 0.1, dummy, dummy, dummy, ctypes.c_void_p(72), need, None) == _lib.MSPA_EINVAL
    assert call(None, 0, 8, 0.1, None, None, None, None, 0, None) == _lib.MSPA_OK            # no block
    assert call(None, 4, 0, 0.1, None, None, None, None, 0, None) == _lib.MSPA_OK            # no point
    assert call(None, 4, 1, 0.1, None, None, None, None, 0, None) == _lib.MSPA_OK            # one point: no merge
    assert lib.mspa_track_linkage_workspace_bytes(0, 8) == 0 and lib.mspa_track_linkage_workspace_bytes(4, 1) == 0
    assert lib.mspa_track_linkage_workspace_bytes(-1, 8) == -1 and lib.mspa_track_linkage_workspace_bytes(1, -1) == -1
    assert lib.mspa_track_linkage_workspace_bytes(1, P_max + 1) == -1
    assert lib.mspa_track_linkage_workspace_bytes(1, P_max) >= P_max * P_max * 8

    batch = lib.mspa_track_rigidity_loss_batch
    assert batch(dummy, -1, 3, 4, 0.01, dummy, None) == _lib.MSPA_EINVAL
    assert batch(dummy, 2, -1, 4, 0.01, dummy, None) == _lib.MSPA_EINVAL
    assert batch(None, 2, 3, 4, 0.01, dummy, None) == _lib.MSPA_EINVAL
    assert batch(dummy, 2, 3, 4, 0.01, None, None) == _lib.MSPA_EINVAL
    assert batch(dummy, 70000, 3, 4, 0.01, dummy, None) == _lib.MSPA_EINVAL
    assert batch(None, 0, 3, 4, 0.01, None, None) == _lib.MSPA_OK
    assert batch(None, 2, 3, 0, 0.01, None, None) == _lib.MSPA_OK
