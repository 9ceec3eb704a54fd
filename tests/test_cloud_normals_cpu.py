"""The k nearest rows and the normals of a ragged batch without a GPU: the host twin (csrc/cloud_normals_core.h through
mspa_cloud_normals_host) against references that share no code with it (tests/cloud_normals_util.py: a brute-force search over the
full d2 matrix, an mpmath oracle at 60 digits, ``numpy.linalg.eigh`` as the yardstick, exact rationals for signs and norms):

  * ``knn_segments_host`` equals the brute force bit for bit, indices and distances, on every segment, the tie-heavy lattices among
    them, with and without the cap and at k = 1, K, 30 and 64;
  * identities, by bytes: the lattice plane z = 3 has the normal (0, 0, 1) and the curvature 0.0 exactly; two runs give the same
    bits; the rows of a tie-free segment permuted give the same bits at the permuted places; float32 rows are their widened values;
  * statuses where the geometry puts them, NaN exactly where the status is not OK;
  * accuracy: per class the angle between the twin's normal and the oracle's eigenvector of the same neighbour set is at most 8 x
    ``eigh``'s worst on that class (at least one unit roundoff is allowed), the curvature by the same rule; | |n|^2 - 1 | in exact
    rational arithmetic is within the header's derived bound; every oriented normal has a positive exact dot with (v - p);
  * the ValueErrors and MSPA_EINVALs, empty shapes, the frozen fixture against a fresh run, the header as a stand-alone g++ program
    under AddressSanitizer + UBSan.

Measured here (host twin, x86-64), worst angle per class, twin (eigh): near 1.9e-16 (9.4e-16), far 7.2e-16 (1.5e-15), small 3.5e-17
(1.5e-16), large 7.2e-17 (3.9e-16), sphere 5.2e-16 (2.1e-15), lattice 0 (0): ratios of 0.19 to 0.48 against the 8 allowed.  Worst
curvature error 1.6e-16 (eigh 2.2e-16).  Worst | |n|^2 - 1 | 4.0 u against the bound of 8 u."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_normals_util as U  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")
fold = lambda text: " ".join(text.split())                                   # noqa: E731
_CACHE = {}


def CS():
    from mspa import cloud_segments
    return cloud_segments


def _twin(views=True, cap=None, k=U.K):
    """The twin on the batch, once per variant, with the neighbour table."""
    key = (views, cap, k)
    if key not in _CACHE:
        xyz, off, _names = U.batch()
        _CACHE[key] = CS().normals_segments_host(xyz, off, k, cap, U.viewpoints() if views else None, want_neighbours=True)
    return _CACHE[key]


# ---- neighbours -----------------------------------------------------------------------------------------------------------------

def test_the_constants_are_the_headers():
    from mspa import _lib
    header = open(os.path.join(CSRC, "cloud_normals_core.h")).read()
    assert f"kSweeps = {_lib.CLOUD_NORMALS_SWEEPS};" in header and f"kGapExponent = {_lib.CLOUD_NORMALS_GAP_EXPONENT};" in header
    assert "kUnitBound = 8.0 / 9007199254740992.0" in header and _lib.CLOUD_NORMALS_UNIT_BOUND == 8 * U.U
    assert (_lib.CLOUD_NORMALS_OK, _lib.CLOUD_NORMALS_FEW, _lib.CLOUD_NORMALS_DEGENERATE) == (U.OK, U.FEW, U.DEGENERATE)
    assert CS().NORMALS_STATUS == {"ok": U.OK, "few": U.FEW, "degenerate": U.DEGENERATE}


@pytest.mark.parametrize("cap", [None, U.CAP], ids=["no cap", "cap"])
@pytest.mark.parametrize("k", [1, U.K, 30, 64])
def test_the_neighbours_are_the_brute_forces_bit_for_bit(k, cap):
    xyz, off, names = U.batch()
    want_index, want_distance, want_used = U.brute(cap, k)
    index, distance = CS().knn_segments_host(xyz, off, k, cap)
    assert index.dtype == np.int64 and index.shape == (len(xyz), k) and distance.dtype == np.float64
    for name in names:
        _s, a, b = U.segment(name)
        assert np.array_equal(index[a:b], want_index[a:b]), name
        assert distance[a:b].tobytes() == want_distance[a:b].tobytes(), name
    out = CS().normals_segments_host(xyz, off, k, cap, want_neighbours=True)
    assert np.array_equal(out["used"], want_used) and out["used"].dtype == np.int32
    assert out["index"].tobytes() == index.tobytes() and out["distance"].tobytes() == distance.tobytes()      # one walk, two outputs
    assert (index[:, 0] == np.arange(len(xyz))).sum() >= len(xyz) - 225 and (distance[:, 0] == 0.0).all()    # the row itself, but for coincident twins
    assert ((index == -1) == (np.arange(k)[None] >= want_used[:, None])).all() and (np.isinf(distance) == (index == -1)).all()


# ---- identities -----------------------------------------------------------------------------------------------------------------

def test_a_lattice_plane_has_the_normal_0_0_1_and_the_curvature_0_exactly():
    out = _twin(views=False)
    for name in ("lattice", "lattice twice"):
        _s, a, b = U.segment(name)
        assert (out["status"][a:b] == U.OK).all()
        assert out["normal"][a:b].tobytes() == np.tile([0.0, 0.0, 1.0], (b - a, 1)).tobytes(), name
        assert out["curvature"][a:b].tobytes() == np.zeros((b - a,)).tobytes(), name
    for k in (5, 30, 64):                                                    # whatever the neighbourhood's size (3 are collinear along an edge)
        xyz, off, _names = U.batch()
        _s, a, b = U.segment("lattice")
        got = CS().normals_segments_host(xyz[a:b], [0, b - a], k)
        assert got["normal"].tobytes() == np.tile([0.0, 0.0, 1.0], (b - a, 1)).tobytes() and not got["curvature"].any() and not got["status"].any()


def test_the_same_input_gives_the_same_bits():
    xyz, off, _names = U.batch()
    again = CS().normals_segments_host(xyz, off, U.K, None, U.viewpoints(), want_neighbours=True)
    for key, value in _twin().items():
        assert again[key].tobytes() == value.tobytes(), key
    alone = CS().normals_segments_host(xyz[off[8]:off[9]], [0, off[9] - off[8]], U.K)       # a segment does not see its batch
    assert alone["normal"].tobytes() == _twin(views=False)["normal"][off[8]:off[9]].tobytes()


def test_permuted_rows_give_the_same_bits_at_the_permuted_places():
    assert U.tie_free_checked()
    xyz, off, _names = U.batch()
    rng = np.random.default_rng(5)
    moved, place = xyz.copy(), np.arange(len(xyz))
    for name in U.TIE_FREE:
        _s, a, b = U.segment(name)
        perm = a + rng.permutation(b - a)
        moved[a:b], place[a:b] = xyz[perm], perm
    got = CS().normals_segments_host(moved, off, U.K, None, U.viewpoints(), want_neighbours=True)
    want = _twin()
    for key in ("normal", "curvature", "used", "status", "distance"):
        assert got[key].tobytes() == want[key][place].tobytes(), key
    for name in U.TIE_FREE:                                                  # the table names the same rows under their new numbers
        _s, a, b = U.segment(name)
        assert np.array_equal(place[got["index"][a:b]], want["index"][place[a:b]]), name


def test_float32_rows_are_their_widened_values():
    _xyz, off, _names = U.batch()
    narrow = U.float32_rows()
    a, b = CS().normals_segments_host(narrow, off, U.K), CS().normals_segments_host(narrow.astype(np.float64), off, U.K)
    assert a["normal"].tobytes() == b["normal"].tobytes() and a["normal"].dtype == np.float64 and (a["status"] == U.OK).sum() > 3000


# ---- statuses -------------------------------------------------------------------------------------------------------------------

def test_the_statuses_are_the_geometrys_and_nan_stands_exactly_where_a_row_is_not_ok():
    _xyz, _off, names = U.batch()
    for out in (_twin(), _twin(views=False), _twin(cap=U.CAP)):
        bad = out["status"] != U.OK
        assert (np.isnan(out["normal"]).all(axis=1) == bad).all() and (np.isnan(out["normal"]).any(axis=1) == bad).all()
        assert (np.isnan(out["curvature"]) == bad).all() and ((out["used"] < 3) == (out["status"] == U.FEW)).all()
    out = _twin()
    for name in names:
        _s, a, b = U.segment(name)
        want = U.FEW if b - a < 3 else U.DEGENERATE if name == "line" else U.OK
        assert (out["status"][a:b] == want).all(), name
        assert (out["used"][a:b] == min(U.K, b - a)).all(), name
    capped, used = _twin(cap=U.CAP), U.brute(U.CAP)[2]
    assert np.array_equal(capped["used"], used) and (capped["status"] == U.FEW).any() and ((capped["status"] == U.OK) & (used < U.K)).any()
    coincident = CS().normals_segments_host(np.tile([[0.5, 1.5, -2.0]], (12, 1)), [0, 12], 5)
    assert (coincident["status"] == U.DEGENERATE).all() and (coincident["used"] == 5).all()
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)] + [[0, 0, 0]], dtype=np.float64)
    assert CS().normals_segments_host(corners, [0, 9], 9)["status"][8] == U.DEGENERATE      # isotropic: l0 = l1 = l2


# ---- accuracy -------------------------------------------------------------------------------------------------------------------

def test_the_accuracy_rule_per_class_against_the_mpmath_oracle(capsys):
    out = _twin(views=False)
    for cls, rows in U.references().items():
        worst = max(U.angle(out["normal"][i], n) for i, n, *_ in rows)
        yard = max(r[3] for r in rows)
        curv = max(abs(out["curvature"][i] - c) for i, _n, c, *_ in rows)
        curv_yard = max(r[4] for r in rows)
        with capsys.disabled():
            print(f"\n{cls}: {len(rows)} rows, angle {worst:.3g} (eigh {yard:.3g}), curvature {curv:.3g} (eigh {curv_yard:.3g})", end="")
        assert all(out["status"][i] == U.OK for i, *_ in rows), cls
        assert U.within_rule(worst, yard), (cls, worst, yard)
        assert U.within_rule(curv, curv_yard), (cls, curv, curv_yard)


def test_every_normal_is_a_unit_vector_within_the_derived_bound(capsys):
    from mspa import _lib
    worst = 0.0
    for out in (_twin(), _twin(cap=U.CAP)):
        ok = np.nonzero(out["status"] == U.OK)[0]
        worst = max([worst] + [U.exact_unit_defect(out["normal"][i]) for i in ok[::3]])
    with capsys.disabled():
        print(f"\nworst | |n|^2 - 1 | = {worst / U.U:.2f} u", end="")
    assert worst <= _lib.CLOUD_NORMALS_UNIT_BOUND


def test_the_orientation_is_the_sign_of_the_exact_dot():
    xyz, _off, _names = U.batch()
    viewed, plain = _twin(), _twin(views=False)
    flipped = 0
    for i, v in U.oriented_rows():
        assert U.exact_dot(v, xyz[i], viewed["normal"][i]) > 0, i
        same = viewed["normal"][i].tobytes() == plain["normal"][i].tobytes()
        assert same or viewed["normal"][i].tobytes() == (-plain["normal"][i]).tobytes(), i
        flipped += not same
    assert 0 < flipped < len(U.oriented_rows())
    s, a, b = U.segment("sphere in")                                         # towards the centre; from far outside, the near side points out
    assert (np.einsum("ij,ij->i", viewed["normal"][a:b], xyz[a:b]) < 0).all()
    s, a, b = U.segment("sphere out")
    outward = np.einsum("ij,ij->i", viewed["normal"][a:b], xyz[a:b] - [4.0, 0.0, 0.0]) > 0
    assert outward.any() and not outward.all()
    s, a, b = U.segment("slab 1025")                                         # a NaN viewpoint row: the canonical sign
    assert viewed["normal"][a:b].tobytes() == plain["normal"][a:b].tobytes()
    lead = plain["normal"][plain["status"] == U.OK]
    first = np.where(lead[:, 0] != 0, lead[:, 0], np.where(lead[:, 1] != 0, lead[:, 1], lead[:, 2]))
    assert (first > 0).all()


# ---- the rest -------------------------------------------------------------------------------------------------------------------

def test_the_value_errors():
    xyz, off, names = U.batch()
    for kw in ({"k": 0}, {"k": 65}, {"max_distance": 0.0}, {"max_distance": -1.0}, {"max_distance": np.inf}, {"max_distance": np.nan},
               {"viewpoints": np.zeros((3, 3))}, {"viewpoints": np.zeros((len(names), 2))}):
        with pytest.raises(ValueError):
            CS().normals_segments_host(xyz, off, **kw)
    with pytest.raises(ValueError):
        CS().knn_segments_host(xyz[:, :2], off, 3)
    with pytest.raises(ValueError):
        CS().knn_segments_host(xyz, off[:-2], 3)                             # offsets that stop short of the rows
    bad = xyz.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="finite coordinates"):
        CS().normals_segments_host(bad, off)


def test_the_entry_points_refuse_bad_arguments_before_anything_runs():
    from mspa import _lib
    lib = _lib.load()
    xyz, off, names = U.batch()
    N, S, k = len(xyz), len(names), 4
    normal, curvature, used, status = np.zeros((N, 3)), np.zeros((N,)), np.zeros((N,), dtype=np.int32), np.zeros((N,), dtype=np.uint8)
    index, distance = np.zeros((N, k), dtype=np.int64), np.zeros((N, k))
    p = lambda a: a.ctypes.data                                               # noqa: E731
    descending = off.copy()
    descending[3] = descending[2] - 1
    not_a_number = xyz.copy()
    not_a_number[5, 2] = np.inf

    def host(x=p(xyz), o=off, k=k, cap=np.inf, n=p(normal), c=p(curvature), u=p(used), s=p(status), i=p(index), d=p(distance)):
        return lib.mspa_cloud_normals_host(x, p(o), len(o) - 1, k, cap, None, n, c, u, s, i, d)

    assert host() == 0 and host(n=None, c=None, s=None) == 0 and host(i=None, d=None) == 0
    for rc in (host(o=descending), host(k=0), host(k=65), host(cap=0.0), host(cap=-2.0), host(cap=np.nan), host(x=None), host(u=None), host(c=None),
               host(d=None), host(n=None, c=None, s=None, i=None, d=None), host(x=p(not_a_number))):
        assert rc == _lib.MSPA_EINVAL
    assert b"non-finite coordinate" in (host(x=p(not_a_number)), lib.mspa_last_error_string())[1]
    # the device entry checks the same host tables first: no GPU is touched for a refusal or for nothing to do
    dummy = 4096
    grids, base = np.zeros((S, _lib.KNN_GRID_BYTES), dtype=np.uint8), np.zeros((S + 1,), dtype=np.int64)
    lo, hi = np.zeros((S, 3)), np.zeros((S, 3))
    for s in range(S):
        if off[s + 1] > off[s]:
            lo[s], hi[s] = xyz[off[s]:off[s + 1]].min(0), xyz[off[s]:off[s + 1]].max(0)
    assert lib.mspa_knn_segments_grids_host(p(lo), p(hi), p(off), S, k, p(grids)) == 0 and lib.mspa_knn_segments_tables_host(p(off), S, k, p(base)) == 0
    slots = int(base[S]) + S

    def device(o=off, k=k, cap=np.inf, g=p(grids), slots=slots, pts=dummy, views=None, n=dummy, c=dummy, u=dummy, s=dummy, i=dummy, d=dummy):
        return lib.mspa_cloud_normals_device(pts, dummy, slots, dummy, p(o), len(o) - 1, k, g, dummy, dummy, dummy, cap, views, n, c, u, s, i, d, None)

    for rc in (device(o=descending), device(k=0), device(k=65), device(cap=0.0), device(cap=np.nan), device(pts=None), device(u=None), device(c=None),
               device(i=None), device(n=None, c=None, s=None, i=None, d=None), device(g=None), device(g=p(np.zeros_like(grids))), device(slots=slots - 1), device(pts=dummy + 4), device(views=dummy + 2), device(n=dummy + 1), device(u=dummy + 2), device(d=dummy + 4)):
        assert rc == _lib.MSPA_EINVAL
    assert b"starts_dev holds fewer slots" in (device(slots=slots - 1), lib.mspa_last_error_string())[1]
    none = np.zeros((1,), dtype=np.int64)
    assert lib.mspa_cloud_normals_device(None, None, 0, None, p(none), 0, k, None, None, None, None, np.inf, None, None, None, None, None, dummy, dummy, None) == 0
    assert lib.mspa_cloud_normals_host(None, p(none), 0, k, np.inf, None, None, None, None, None, dummy, dummy) == 0


def test_empty_shapes():
    none = np.zeros((0, 3))
    for offsets in ([0], [0, 0, 0]):
        out = CS().normals_segments_host(none, offsets, 7, want_neighbours=True)
        assert out["normal"].shape == (0, 3) and out["curvature"].shape == (0,) and out["used"].shape == (0,) and out["status"].shape == (0,)
        assert out["index"].shape == (0, 7) and out["distance"].shape == (0, 7)
    index, distance = CS().knn_segments_host(np.array([[1.0, 2.0, 3.0]]), [0, 0, 1, 1], 2, 0.5)
    assert index.tolist() == [[0, -1]] and distance.tolist() == [[0.0, np.inf]]


def test_the_frozen_results_are_a_fresh_runs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_cloud_normals_golden as G
    frozen, fresh = U.golden(), G.frozen()
    assert sorted(frozen) == sorted(fresh)
    for key in fresh:
        assert frozen[key].dtype == np.asarray(fresh[key]).dtype and frozen[key].tobytes() == np.asarray(fresh[key]).tobytes(), key
    assert os.path.getsize(U.GOLDEN) < 100_000
    xyz, off, _views = U.fixture_batch()                                     # the fixture's segments are the batch's, alone
    for name, a in zip(U.FIXTURE, off[:-1]):
        _s, b0, b1 = U.segment(name)
        assert frozen["viewed_normal"][a:a + b1 - b0].tobytes() == _twin()["normal"][b0:b1].tobytes(), name


def test_the_docstrings_say_what_they_must():
    for f in (CS().knn_segments, CS().normals_segments):
        assert "One read-back per call, whatever S is" in fold(f.__doc__)
    assert "(0, 0, 1) and 0.0 exactly" in fold(CS().normals_segments.__doc__) and "hybrid search" in fold(CS().knn_segments.__doc__)


# One record: int64 S, k, has_views; float64 cap; then offsets [S + 1] (int64), xyz [N, 3], viewpoints [S, 3] where has_views (float64) ->
# normal [N, 3] f64, curvature [N] f64, used [N] i32, status [N] u8, index [N, k] i64, distance [N, k] f64.  Every buffer is a heap block
# of exactly its size.
DRIVER = r"""
#include "cloud_normals_core.h"
#include <cstdio>
#include <cstdlib>
template <typename T> static T *block(int64_t n) { return (T *)malloc((size_t)(n > 0 ? n : 1) * sizeof(T)); }
template <typename T> static bool get(T *p, int64_t n) { return fread(p, sizeof(T), (size_t)n, stdin) == (size_t)n; }
template <typename T> static void put(const T *p, int64_t n) { fwrite(p, sizeof(T), (size_t)n, stdout); }
int main() {
    int64_t head[3];
    double cap;
    while (fread(head, 8, 3, stdin) == 3 && fread(&cap, 8, 1, stdin) == 1) {
        const int64_t S = head[0], k = head[1];
        int64_t *off = block<int64_t>(S + 1);
        if (!get(off, S + 1)) return 5;
        const int64_t N = mspa::segs::batch_rows(off, S);
        if (N < 0) return 6;
        double *xyz = block<double>(3 * N), *views = block<double>(3 * S), *normal = block<double>(3 * N), *curvature = block<double>(N);
        double *distance = block<double>(N * k);
        int64_t *index = block<int64_t>(N * k);
        int32_t *used = block<int32_t>(N);
        uint8_t *status = block<uint8_t>(N);
        if (!get(xyz, 3 * N) || (head[2] && !get(views, 3 * S))) return 7;
        if (!mspa::cnorm::normals_all(xyz, off, S, (int32_t)k, mspa::cdist::cap2_of(cap), head[2] ? views : nullptr, normal, curvature, used, status,
                                      index, distance))
            return 8;
        put(normal, 3 * N), put(curvature, N), put(used, N), put(status, N), put(index, N * k), put(distance, N * k);
        void *all[] = {off, xyz, views, normal, curvature, distance, index, used, status};
        for (void *p : all) free(p);
    }
    return 0;
}
"""


def test_the_header_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, str(tmp_path / "driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    xyz, off, _names = U.batch()
    records = [(xyz, off, U.K, None, U.viewpoints()), (xyz, off, 64, U.CAP, None), (xyz, off, 1, None, None),
               (np.zeros((0, 3)), np.array([0, 0]), 3, None, None)]
    i8 = lambda x: np.asarray(x, dtype="<i8").tobytes()                      # noqa: E731
    f8 = lambda x: np.asarray(x, dtype="<f8").tobytes()                      # noqa: E731
    inp = b"".join(struct.pack("<qqqd", len(o) - 1, k, views is not None, np.inf if cap is None else cap) + i8(o) + f8(x) +
                   (f8(views) if views is not None else b"") for x, o, k, cap, views in records)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    at = 0

    def take(count, dtype):
        nonlocal at
        got = np.frombuffer(run.stdout, dtype=dtype, count=count, offset=at)
        at += got.nbytes
        return got

    for x, o, k, cap, views in records:
        N = len(x)
        got = {"normal": take(3 * N, "<f8"), "curvature": take(N, "<f8"), "used": take(N, "<i4"), "status": take(N, "u1"), "index": take(N * k, "<i8"),
               "distance": take(N * k, "<f8")}
        twin = CS().normals_segments_host(x, o, k, cap, views, want_neighbours=True)
        for key, value in got.items():
            assert value.tobytes() == twin[key].tobytes(), (key, k, cap)
    assert at == len(run.stdout)


# ---- point-to-plane (csrc/cloud_align_plane_core.h) ---------------------------------------------------------------------------------
#
# Measured here (host twin, x86-64): after 30 iterations on the 1 degree / 5 mm pair max |R - R_true| 1.1e-16; worst max |R^T R - I|
# after 1, 10 and 50 iterations at both caps 4.4 u against the bound of 32 u.

def _plane(cap=0.05, **kw):
    q, q_off, t, t_off, _truth, normals = U.plane_batch()
    return CS().register_segments_host(q, q_off, t, t_off, max_distance=cap, estimation="point_to_plane", normals=normals, **kw)


def test_plane_a_cloud_against_itself_with_its_own_normals_is_the_identity_exactly():
    _q, _q_off, t, t_off, _truth, normals = U.plane_batch()
    reg = CS().register_segments_host(t, t_off, t, t_off, max_distance=0.05, iterations=3, estimation="point_to_plane", normals=normals)
    live = np.diff(t_off) >= 6
    assert (reg["status"][live] == U.OK).all() and (reg["converged_at"] == 0).all()
    assert reg["R"].tobytes() == np.tile(np.eye(3), (len(live), 1, 1)).tobytes() and reg["t"].tobytes() == np.zeros((len(live), 3)).tobytes()
    step = CS().plane_fit_segments_host(t, t_off, t, normals, np.arange(len(t), dtype=np.int64))
    assert step["R"].tobytes() == reg["R"].tobytes() and not step["t"].any() and (step["rmse"][live] == 0.0).all()


def test_plane_every_rotation_is_orthonormal_within_the_bound_after_1_10_and_50_iterations(capsys):
    import cloud_align_util as A
    from mspa import _lib
    worst = 0.0
    for cap in (0.05, 0.08):
        for iterations in (1, 10, 50):
            reg = _plane(cap, iterations=iterations)
            for p in (A.EASY, A.HARD):
                assert reg["status"][p] == U.OK
                worst = max(worst, A.exact_ortho_defect(reg["R"][p]))
                assert np.linalg.det(reg["R"][p]) > 0
    with capsys.disabled():
        print(f"\nworst max |R^T R - I| = {worst / U.U:.2f} u", end="")
    assert worst <= _lib.CLOUD_ALIGN_ORTHO_BOUND


def test_plane_the_twins_correspondences_and_transform_are_the_numpy_point_to_plane_icps():
    import cloud_align_util as A
    _q, q_off, _t, t_off, truth, _normals = U.plane_batch()
    ref = U.numpy_plane_icp(A.EASY, 0.05)
    reg = _plane(iterations=U.PLANE_ITERATIONS, want_index=True)
    a, b = q_off[A.EASY], q_off[A.EASY + 1]
    for k in range(U.PLANE_ITERATIONS):
        got = reg["history_index"][k, a:b]
        assert np.array_equal(np.where(got >= 0, got - t_off[A.EASY], -1), ref["index"][k]), k
    R_true, t_true = truth[A.EASY]
    scale = 0.3
    err = (np.abs(reg["R"][A.EASY] - R_true).max(), np.abs(reg["t"][A.EASY] - t_true).max() / scale)
    yard = (np.abs(ref["R"] - R_true).max(), np.abs(ref["t"] - t_true).max() / scale)
    assert U.within_rule(err[0], yard[0]) and U.within_rule(err[1], yard[1]), (err, yard)
    assert reg["fitness"][A.EASY] == 1.0 and reg["inlier_rmse"][A.EASY] < 1e-15


def test_plane_a_flat_target_is_degenerate_and_few_below_six_rows_both_keep_init():
    q, t, normals = U.flat_case()
    rng = np.random.default_rng(11)
    init = np.concatenate([np.eye(3), rng.random((3, 1)) * 0.01], axis=1)[None]
    index = np.arange(len(q), dtype=np.int64)
    out = CS().plane_fit_segments_host(q, [0, len(q)], t, normals, index, init=init)
    assert out["status"].tolist() == [U.DEGENERATE] and out["used"].tolist() == [len(q)] and np.isfinite(out["rmse"]).all()
    assert out["R"].tobytes() == init[:, :, :3].tobytes() and out["t"].tobytes() == np.ascontiguousarray(init[:, :, 3]).tobytes()
    reg = CS().register_segments_host(q, [0, len(q)], t, [0, len(t)], max_distance=0.5, iterations=4, init=init, estimation="point_to_plane", normals=normals)
    assert reg["status"].tolist() == [U.DEGENERATE] and reg["R"].tobytes() == init[:, :, :3].tobytes() and reg["converged_at"].tolist() == [0]
    _q, _q_off, tt, _t_off, _truth, nn = U.plane_batch()
    few = CS().plane_fit_segments_host(tt[:5] + 0.001, [0, 5], tt, nn, np.arange(5, dtype=np.int64), init=init)
    assert few["status"].tolist() == [U.FEW] and few["used"].tolist() == [5] and few["R"].tobytes() == init[:, :, :3].tobytes()
    six = CS().plane_fit_segments_host(tt[:6] + 0.001, [0, 6], tt, nn, np.arange(6, dtype=np.int64))
    assert six["status"][0] != U.FEW and six["used"].tolist() == [6]
    blind = nn.copy()
    blind[:3] = np.nan                                                       # a NaN normal constrains nothing: the row is not used
    assert CS().plane_fit_segments_host(tt[:8] + 0.001, [0, 8], tt, blind, np.arange(8, dtype=np.int64))["status"].tolist() == [U.FEW]


def test_plane_point_to_point_by_keyword_is_the_call_without_it_by_bytes():
    q, q_off, t, t_off, _truth, _normals = U.plane_batch()
    a = CS().register_segments_host(q, q_off, t, t_off, max_distance=0.05, iterations=6, want_history=True)
    b = CS().register_segments_host(q, q_off, t, t_off, max_distance=0.05, iterations=6, want_history=True, estimation="point_to_point")
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
    from spatial_engine.utils.scannet_utils.handler import ops
    import cloud_align_util as A
    src, tgt = q[q_off[A.EASY]:q_off[A.EASY + 1]], t[t_off[A.EASY]:t_off[A.EASY + 1]]
    plain, keyed = ops.registration_icp(src, tgt, 0.05, max_iteration=5), ops.registration_icp(src, tgt, 0.05, max_iteration=5, estimation="point_to_point")
    assert plain["transformation"].tobytes() == keyed["transformation"].tobytes()
    plane = ops.registration_icp(src, tgt, 0.05, max_iteration=U.PLANE_ITERATIONS, estimation="point_to_plane")       # the normals estimated at k = 30
    reg = _plane(iterations=U.PLANE_ITERATIONS)
    assert plane["transformation"][:3, :3].tobytes() == reg["R"][A.EASY].tobytes() and plane["transformation"][:3, 3].tobytes() == reg["t"][A.EASY].tobytes()
    assert "TransformationEstimationPointToPlane" in fold(ops.registration_icp.__doc__)


def test_plane_sync_every_the_value_errors_the_einvals_and_the_empty_shapes():
    from mspa import _lib
    q, q_off, t, t_off, _truth, normals = U.plane_batch()
    full, synced = _plane(iterations=6), _plane(iterations=6, sync_every=2)
    assert not synced["all_converged"] and synced["R"].tobytes() == full["R"].tobytes() and synced["t"].tobytes() == full["t"].tobytes()
    reg = lambda **kw: CS().register_segments_host(q, q_off, t, t_off, max_distance=0.05, **kw)      # noqa: E731
    for kw in ({"estimation": "plane"}, {"estimation": "point_to_plane"}, {"normals": normals}, {"estimation": "point_to_plane", "normals": normals[:-1]},
               {"estimation": "point_to_plane", "normals": normals[:, :2]}):
        with pytest.raises(ValueError):
            reg(**kw)
    with pytest.raises(ValueError):
        CS().plane_fit_segments_host(q, q_off, t, normals, np.zeros((3,), dtype=np.int64))
    with pytest.raises(ValueError):
        CS().plane_fit_segments_host(q, q_off, t, normals[:5], np.zeros((len(q),), dtype=np.int64))
    lib = _lib.load()
    p = lambda a: a.ctypes.data                                               # noqa: E731
    P, M = len(q_off) - 1, len(q)
    index, init = np.zeros((M,), dtype=np.int64), np.tile(np.eye(3, 4).reshape(-1), (P, 1))
    T, used, status = np.zeros((P, 12)), np.zeros((P,), dtype=np.int64), np.zeros((P,), dtype=np.int32)
    bad_out = q_off.copy()
    bad_out[1] += 1

    def host(out_off=q_off, Nt=len(t), n_ptr=p(normals), iteration=0, init_ptr=p(init)):
        return lib.mspa_cloud_align_plane_fit_host(p(q), p(q_off), P, p(t), n_ptr, Nt, P, None, P, p(out_off), p(index), init_ptr, iteration, p(T), p(used),
                                                   p(status), None, None)

    assert host() == 0
    for rc in (host(out_off=bad_out), host(Nt=-1), host(n_ptr=None), host(iteration=-1), host(init_ptr=None)):
        assert rc == _lib.MSPA_EINVAL
    dummy = 4096

    def device(out_off=q_off, n_ptr=dummy, moments=dummy + 8, status_ptr=dummy, T_ptr=dummy):      # refused on the host: no GPU is touched
        return lib.mspa_cloud_align_plane_fit_device(dummy, p(q_off), P, dummy, dummy, n_ptr, len(t), P, None, None, P, p(out_off), dummy, dummy, dummy, 0,
                                                     moments, T_ptr, dummy, status_ptr, None, None, None)

    for rc in (device(out_off=bad_out), device(n_ptr=None), device(n_ptr=dummy + 4), device(moments=dummy), device(moments=None), device(status_ptr=dummy + 2),
               device(T_ptr=None)):
        assert rc == _lib.MSPA_EINVAL
    none = np.zeros((1,), dtype=np.int64)
    assert lib.mspa_cloud_align_plane_fit_device(None, p(none), 0, None, None, None, 0, 0, None, None, 0, p(none), None, None, None, 0, None, None, None, None,
                                                 None, None, None) == 0
    empty = np.zeros((0, 3))
    out = CS().plane_fit_segments_host(empty, [0, 0, 0], empty, empty, np.zeros((0,), dtype=np.int64))
    assert out["status"].tolist() == [U.FEW, U.FEW] and out["R"].tobytes() == np.tile(np.eye(3), (2, 1, 1)).tobytes() and np.isnan(out["rmse"]).all()
    assert CS().plane_fit_segments_host(empty, [0], empty, empty, np.zeros((0,), dtype=np.int64))["R"].shape == (0, 3, 3)
    assert "32 * 2^-53" in fold(CS().plane_fit_segments.__doc__) and "need not ever reproduce" in fold(CS().TargetIndex.register.__doc__)


# One record: int64 Sq, P, Nt; then q_offsets [Sq + 1], index [M] (int64), q_xyz [Nq, 3], t_xyz [Nt, 3], normals [Nt, 3], init [P, 12] (float64); pair s is
# (s, s) -> transform [P, 12] f64, used [P] i64, status [P] i32, rmse [P] f64.  Every buffer is a heap block of exactly its size.
PLANE_DRIVER = r"""
#include "cloud_align_plane_core.h"
#include <cstdio>
#include <cstdlib>
template <typename T> static T *block(int64_t n) { return (T *)malloc((size_t)(n > 0 ? n : 1) * sizeof(T)); }
template <typename T> static bool get(T *p, int64_t n) { return fread(p, sizeof(T), (size_t)n, stdin) == (size_t)n; }
template <typename T> static void put(const T *p, int64_t n) { fwrite(p, sizeof(T), (size_t)n, stdout); }
int main() {
    int64_t head[3];
    while (fread(head, 8, 3, stdin) == 3) {
        const int64_t Sq = head[0], P = head[1], Nt = head[2];
        int64_t *q_off = block<int64_t>(Sq + 1);
        if (P != Sq || !get(q_off, Sq + 1)) return 5;
        const int64_t Nq = mspa::segs::batch_rows(q_off, Sq);
        if (Nq < 0) return 6;
        int64_t *index = block<int64_t>(Nq), *used = block<int64_t>(P);
        double *q = block<double>(3 * Nq), *t = block<double>(3 * Nt), *n = block<double>(3 * Nt), *init = block<double>(12 * P), *T = block<double>(12 * P);
        double *rmse = block<double>(P);
        int32_t *status = block<int32_t>(P);
        if (!get(index, Nq) || !get(q, 3 * Nq) || !get(t, 3 * Nt) || !get(n, 3 * Nt) || !get(init, 12 * P)) return 7;
        mspa::cplane::fit_all(q, q_off, t, n, Nt, nullptr, P, q_off, index, init, 0, T, used, status, rmse, nullptr);
        put(T, 12 * P), put(used, P), put(status, P), put(rmse, P);
        void *all[] = {q_off, index, used, q, t, n, init, T, rmse, status};
        for (void *p : all) free(p);
    }
    return 0;
}
"""


def test_plane_the_header_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    (tmp_path / "driver.cpp").write_text(PLANE_DRIVER)
    exe = str(tmp_path / "driver")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, str(tmp_path / "driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    q, q_off, t, t_off, _truth, normals = U.plane_batch()
    found = CS().nearest_segments_host(q, q_off, t, t_off, None, 0.05)["index"]
    wild = found.copy()
    wild[::5] = 1 << 50                                                       # far outside the targets: clamped
    fq, ft, fn = U.flat_case()
    eye = lambda n: np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), (n, 1))      # noqa: E731  (R row-major, then t)
    records = [(q, q_off, found, t, normals), (q, q_off, wild, t, normals), (fq, np.array([0, len(fq)]), np.arange(len(fq)), ft, fn),
               (q, q_off, found, np.zeros((0, 3)), np.zeros((0, 3)))]
    i8 = lambda x: np.asarray(x, dtype="<i8").tobytes()                      # noqa: E731
    f8 = lambda x: np.asarray(x, dtype="<f8").tobytes()                      # noqa: E731
    inp = b"".join(struct.pack("<qqq", len(o) - 1, len(o) - 1, len(tx)) + i8(o) + i8(ix) + f8(x) + f8(tx) + f8(nx) + f8(eye(len(o) - 1))
                   for x, o, ix, tx, nx in records)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    at = 0
    for x, o, ix, tx, nx in records:
        P = len(o) - 1
        twin = CS().plane_fit_segments_host(x, o, tx, nx, np.asarray(ix, dtype=np.int64))
        for key, dtype, count in (("T", "<f8", 12 * P), ("used", "<i8", P), ("status", "<i4", P), ("rmse", "<f8", P)):
            got = np.frombuffer(run.stdout, dtype=dtype, count=count, offset=at)
            at += got.nbytes
            want = np.concatenate([twin["R"].reshape(P, 9), twin["t"]], axis=1) if key == "T" else twin[key]
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), key
    assert at == len(run.stdout)
