"""K3's launch decision (csrc/pair_route.h) on the CPU: a g++ build of the header, its route() against an independent
restatement of the launch rules over a sweep of shapes, output sets, pointer alignment and flags; cases pinned by hand; the
argument errors; and closure -- the keys route() returns are exactly the instantiations the header lists (and
pair_reproject.hip compiles).  The size query of the built library is checked against the same restatement."""
import os
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_route_cases as C  # noqa: E402
from pair_route_cases import Key  # noqa: E402

from mspa import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")

# Writes the header's tables -- kNumKeys, the keys (7 int32 each), the four error texts (128 bytes each) -- then reads records
# (dh, dw, H, W, outputs, aligned, flags) as int32 until the input ends and writes route()'s answer, 15 int32 each.
DRIVER = r"""
#include "pair_route.h"
#include <cstdio>
#include <cstring>
using namespace mspa;
static void put_key(const Key &k) {
    const int32_t v[7] = {(int32_t)k.kernel, (int32_t)k.set, k.ident, k.whole_tiles, k.linear, k.scaled, k.stream};
    fwrite(v, 4, 7, stdout);
}
static_assert(route(480, 640, 480, 640, kSetCorr, true, MSPA_PAIR_FAST).family == MSPA_KERNEL_PAIR_FAST_TIGHT, "constexpr route()");
static_assert(tight_rows_of(kSetCompact, true) == MSPA_CORR_TILE_H && tight_rows_of(kSetCompact) == MSPA_CORR_TILE_H, "API tile");
int main() {
    const int32_t n = kNumKeys;
    fwrite(&n, 4, 1, stdout);
    for (int i = 0; i < kNumKeys; ++i) put_key(kKeys[i]);
    for (int e = kRouteBadSize; e <= kRouteNeedsTight; ++e) {
        char text[128] = {};
        strncpy(text, route_error_text((RouteError)e), sizeof text - 1);
        fwrite(text, 1, sizeof text, stdout);
    }
    int32_t a[7];
    while (fread(a, 4, 7, stdin) == 7) {
        const Route r = route(a[0], a[1], a[2], a[3], (uint32_t)a[4], a[5] != 0, (uint32_t)a[6]);
        const int32_t head[2] = {(int32_t)r.err, r.family}, tail[6] = {r.rows, r.waves, r.threads, r.n_stripes, r.n_tiles, r.groups};
        fwrite(head, 4, 2, stdout);
        put_key(r.key);
        fwrite(tail, 4, 6, stdout);
        if (!r.err && (key_index(r.key) < 0 || !(kKeys[key_index(r.key)] == r.key))) return 3;
    }
    return 0;
}
"""

SIZES = (2, 16, 47, 48, 64, 96, 100, 128, 150, 480, 640, 968, 1296)
UNNAMED = (C.bits(C.SETS["bytes"]), C.bits(C.SETS["bits_bytes"]), C.O_VIS_BITS | C.O_PIX, C.CORR | C.O_XYZ64)
MASKS = tuple(C.NAMED.values()) + UNNAMED
FLAGS = (0, C.FAST, C.FAST | C.STREAM, C.FAST | C.WORD_STRIPES)


def depth_grids(H, W):
    return ((H, W), (H // 2, W // 2), (480, 640), (H + 1, W + 1))


def sweep():
    return [(dh, dw, H, W, m, al, f) for H in SIZES for W in SIZES for dh, dw in depth_grids(H, W) for m in MASKS
            for al in (1, 0) for f in FLAGS]


class Header:
    def __init__(self, exe):
        self.exe = exe
        self.keys, self.texts, _ = self._run([])

    def _run(self, records):
        blob = b"".join(struct.pack("<7i", *r) for r in records)
        out = subprocess.run([self.exe], input=blob, capture_output=True, check=True).stdout
        n = struct.unpack_from("<i", out)[0]
        keys = [self._key(struct.unpack_from("<7i", out, 4 + 28 * i)) for i in range(n)]
        off = 4 + 28 * n
        texts = [out[off + 128 * i:off + 128 * (i + 1)].rstrip(b"\0").decode() for i in range(4)]
        off += 512
        assert len(out) == off + 60 * len(records)
        routes = []
        for i in range(len(records)):
            v = struct.unpack_from("<15i", out, off + 60 * i)
            routes.append(C.Route(v[0], 0, None, 0, 0, 0, 0, 0, 0) if v[0] else C.Route(0, v[1], self._key(v[2:9]), *v[9:]))
        return keys, texts, routes

    @staticmethod
    def _key(v):
        return Key(v[0], v[1], *map(bool, v[2:]))

    def route(self, records):
        return self._run(records)[2]


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("route_driver")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    build = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(d / "driver.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return Header(exe)


@pytest.fixture(scope="module")
def swept(header):
    records = sweep()
    return records, header.route(records)


def test_route_equals_the_restated_launch_rules_over_the_sweep(swept):
    records, routes = swept
    assert len(records) == 13 * 13 * 4 * 9 * 2 * 4
    families = set()
    for rec, got in zip(records, routes):
        assert got == C.parent_route(*rec), rec
        families.add(got.family)
    assert families == {0, C.EXACT_FAMILY, C.FAST_FAMILY, C.LINEAR_FAMILY, C.TIGHT_FAMILY, C.RECT_FAMILY}   # 0: the error routes


def test_workspace_answer_agrees_with_the_compacted_sets_route(swept):
    """0 bytes exactly where the compacted set gets a (fused) kernel with aligned pointers, n * H * W * 4 otherwise -- from the
    restatement, from route() and from the built library's mspa_pair_correspondences_workspace_bytes; and the fused branch of
    mspa_pair_correspondences (route() without error for the pointers it was given) is the earlier code's `no workspace needed
    and depth 4-byte aligned`, so "the fused compacted set needs the tight kernel" cannot come out of that entry point: the
    launch code asks route() the same question with the same arguments."""
    records, routes = swept
    lib = _lib.load()
    n = 0
    for (dh, dw, H, W, m, al, f), got in zip(records, routes):
        if m != C.COMPACT:
            continue
        want = C.parent_workspace_bytes(3, dh, dw, H, W, f)
        if al:
            assert lib.mspa_pair_correspondences_workspace_bytes(3, dh, dw, H, W, f) == want
            n += 1
        if got.err == C.ERR_SIZE:
            continue                                      # a one-row depth grid: every launch refuses it, whatever the query said
        assert got.err == (0 if want == 0 and al else C.ERR_NEEDS_TIGHT), (dh, dw, H, W, al, f)
        assert got.err or got.family in (C.TIGHT_FAMILY, C.RECT_FAMILY)
    assert n > 1000
    # the dense route's own launch carries no O_CPIX: it cannot raise that error either
    assert all(r.err != C.ERR_NEEDS_TIGHT for rec, r in zip(records, routes) if not rec[4] & C.O_CPIX)


PIN = [   # (hw, dhw, outputs, aligned, flags) -> family, key, rows, waves, threads, stripes, tiles, groups; worked out by hand
    ((480, 640), None, C.CORR, 1, C.FAST, C.TIGHT_FAMILY, Key(C.K_TIGHT, C.CORR, 0, 0, 0, 0, 0), 48, 4, 256, 10, 100, 25),
    ((480, 640), None, C.MINIMAL, 1, C.FAST, C.TIGHT_FAMILY, Key(C.K_TIGHT, C.MINIMAL, 0, 0, 0, 0, 0), 48, 2, 128, 10, 100, 50),
    ((480, 640), None, C.COMPACT, 1, C.FAST, C.TIGHT_FAMILY, Key(C.K_TIGHT, C.COMPACT, 0, 0, 0, 0, 0), 48, 2, 128, 10, 100, 50),
    ((480, 640), None, C.DENSE, 1, C.FAST, C.TIGHT_FAMILY, Key(C.K_TIGHT, C.DENSE, 0, 0, 0, 0, 0), 32, 4, 256, 10, 150, 38),
    ((480, 640), None, C.DENSE_XYZ, 1, C.FAST, C.TIGHT_FAMILY, Key(C.K_TIGHT, C.DENSE_XYZ, 0, 0, 0, 0, 0), 32, 8, 512, 10, 150, 19),
    ((480, 640), None, C.CORR, 0, C.FAST, C.FAST_FAMILY, Key(C.K_FAST, C.CORR, 1, 1, 0, 0, 0), 16, 4, 256, 10, 300, 75),
    ((48, 128), None, C.DENSE, 1, C.FAST, C.FAST_FAMILY, Key(C.K_FAST, C.DENSE, 1, 1, 0, 0, 0), 16, 4, 256, 2, 6, 2),
    ((64, 128), None, C.CORR, 1, C.FAST, C.RECT_FAMILY, Key(C.K_TIGHT, C.CORR, 0, 0, 0, 1, 0), 48, 4, 256, 2, 4, 1),
    ((968, 1296), (480, 640), C.CORR, 1, C.FAST, C.RECT_FAMILY, Key(C.K_TIGHT, C.CORR, 0, 0, 0, 1, 0), 48, 4, 256, 21, 441, 111),
    ((968, 1296), (480, 640), C.MINIMAL, 1, C.FAST, C.RECT_FAMILY, Key(C.K_TIGHT, C.MINIMAL, 0, 0, 0, 1, 0), 64, 4, 256, 21, 336, 84),
    ((968, 1296), (480, 640), C.COMPACT, 1, C.FAST, C.RECT_FAMILY, Key(C.K_TIGHT, C.COMPACT, 0, 0, 0, 1, 0), 48, 4, 256, 21, 441, 111),
    ((968, 1296), (480, 640), UNNAMED[0], 1, C.FAST, C.FAST_FAMILY, Key(C.K_FAST, 0, 0, 0, 0, 0, 0), 16, 4, 256, 21, 1281, 321),
    ((968, 1296), (480, 640), UNNAMED[1], 1, C.FAST, C.LINEAR_FAMILY, Key(C.K_FAST, 0, 0, 0, 1, 0, 0), 16, 4, 256, None, 1226, 307),
    ((100, 150), None, C.CORR, 1, C.FAST, C.LINEAR_FAMILY, Key(C.K_FAST, C.CORR, 1, 0, 1, 0, 0), 16, 4, 256, None, 15, 4),
    ((100, 150), None, UNNAMED[0], 1, C.FAST, C.FAST_FAMILY, Key(C.K_FAST, 0, 1, 0, 0, 0, 0), 16, 4, 256, 3, 21, 6),
]


@pytest.mark.parametrize("pin", PIN, ids=lambda p: f"{p[0][1]}x{p[0][0]}{'_over_depth' if p[1] else ''}_{p[2]}_{'aligned' if p[3] else 'misaligned'}")
def test_pinned_routes(header, pin):
    hw, dhw, mask, al, flags, family, key, rows, waves, threads, stripes, tiles, groups = pin
    r, rs = header.route([(*(dhw or hw), *hw, mask, al, flags), (*(dhw or hw), *hw, mask, al, flags | C.STREAM)])
    assert (r.family, r.key, r.rows, r.waves, r.threads, r.n_tiles, r.groups) == (family, Key(*key), rows, waves, threads, tiles, groups)
    assert stripes is None or r.n_stripes == stripes
    # MSPA_PAIR_STREAM sets the key's `stream` for the tight kernel's two families and changes nothing else anywhere
    assert rs == r._replace(key=r.key._replace(stream=family in (C.TIGHT_FAMILY, C.RECT_FAMILY)))


def test_pinned_exact_routes(header):
    """Without MSPA_PAIR_FAST, with a float64 output, and under a depth grid larger than the colour grid: the exact kernel, a
    workgroup per 4096 pixels."""
    recs = [(H, W, H, W, m, al, 0) for H, W in ((480, 640), (100, 150), (2, 2), (968, 1296)) for m in MASKS[:4] + UNNAMED for al in (0, 1)]
    recs += [(480, 640, 480, 640, m | f64, 1, C.FAST) for m in (C.CORR, C.MINIMAL, C.DENSE) for f64 in (C.O_XYZ64, C.O_UV64, C.O_DEPTH64)]
    recs += [(dh, dw, 480, 640, C.CORR, 1, C.FAST | C.STREAM) for dh, dw in ((481, 640), (480, 641), (960, 1280))]
    for rec, r in zip(recs, header.route(recs)):
        ident = rec[:2] == rec[2:4]
        assert (r.err, r.family, r.key, r.threads, r.groups) == (0, C.EXACT_FAMILY, Key(C.K_EXACT, 0, ident, False, False, False, False),
                                                                  256, -(-rec[2] * rec[3] // 4096)), rec


def test_argument_errors(header):
    texts = dict(zip((C.ERR_SIZE, C.ERR_TOO_LARGE, C.ERR_FLAG, C.ERR_NEEDS_TIGHT), header.texts))
    assert texts == {C.ERR_SIZE: "mspa_pair_reproject: image size out of range [2, 32767]",
                     C.ERR_TOO_LARGE: "mspa_pair_reproject: H*W*W must be < 2^32",
                     C.ERR_FLAG: "mspa_pair_reproject: unknown flag",
                     C.ERR_NEEDS_TIGHT: "pair_reproject_impl: the fused compacted set needs the tight kernel and a tile-count table"}
    cases = [((100, 150, 100, 150, C.COMPACT, 1, C.FAST), C.ERR_NEEDS_TIGHT),        # neither whole tiles nor W % 16 == 0
             ((60, 81, 121, 162, C.COMPACT, 1, C.FAST), C.ERR_NEEDS_TIGHT),
             ((480, 640, 480, 640, C.COMPACT, 0, C.FAST), C.ERR_NEEDS_TIGHT),        # misaligned pointers
             ((480, 640, 480, 640, C.COMPACT, 1, 0), C.ERR_NEEDS_TIGHT),             # reference-order mode
             ((480, 640, 480, 640, C.CORR, 1, C.FAST | 4), C.ERR_FLAG),
             ((480, 640, 480, 640, C.CORR, 1, 0x100), C.ERR_FLAG),
             ((1, 640, 480, 640, C.CORR, 1, C.FAST), C.ERR_SIZE), ((480, 1, 480, 640, C.CORR, 1, 0), C.ERR_SIZE),
             ((480, 640, 1, 640, C.CORR, 1, C.FAST), C.ERR_SIZE), ((480, 640, 480, 32768, C.CORR, 1, 0), C.ERR_SIZE),
             ((32768, 640, 480, 640, C.CORR, 1, 0), C.ERR_SIZE), ((480, 640, 480, -64, C.CORR, 1, C.FAST), C.ERR_SIZE),
             ((1024, 2048, 1024, 2048, C.CORR, 1, C.FAST), C.ERR_TOO_LARGE),         # H W W == 2^32
             ((480, 640, 32767, 32767, C.MINIMAL, 1, 0), C.ERR_TOO_LARGE)]
    for (rec, want), r in zip(cases, header.route([c[0] for c in cases])):
        assert r.err == want, rec
    ok = header.route([(1023, 2048, 1023, 2048, C.CORR, 1, C.FAST), (2, 2, 2, 2, C.CORR, 1, C.FAST)])
    assert [r.err for r in ok] == [0, 0]


def test_keys_are_closed_under_route(header, swept):
    """Every instantiation the header lists is reached by some call of the sweep, and route() names no other."""
    listed = header.keys
    assert len(listed) == len(set(listed)) == 30
    reached = {r.key for r in swept[1] if not r.err}
    assert reached == set(listed)


def test_walk_covers_every_instantiation(header):
    """The GPU walk (tests/test_gpu_route_walk.py) launches each listed instantiation exactly once, where route() says so."""
    routes = header.route([C.walk_route_inputs(c) for c in C.WALK])
    assert [r.key for r in routes] == [c.key for c in C.WALK]
    assert sorted(c.key for c in C.WALK) == sorted(header.keys)
    assert header.route([C.walk_route_inputs(C.DENSE_ROUTE)])[0].key == C.DENSE_ROUTE.key
    assert header.route([(*C.DENSE_ROUTE.dhw, *C.DENSE_ROUTE.hw, C.COMPACT, 1, C.FAST)])[0].err == C.ERR_NEEDS_TIGHT
