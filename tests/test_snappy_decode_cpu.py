"""The Snappy decoder of csrc/snappy_core.h on the CPU: a g++ build of the header (plain, and a second time under
AddressSanitizer + UBSan, a stand-alone program with exactly sized heap buffers) and the library's host entry point, over both
writers' streams of the shared set, hand-built element forms and corrupt streams (tests/visindex_decode_util.py)."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visindex_decode_util as VU  # noqa: E402

from mspa import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")

# Records until the input ends: int64 src_len, int64 expected, src bytes -> int64 return value, `expected` bytes of dst.  src and
# dst are heap blocks of exactly src_len / expected bytes: a read or a write outside them is the sanitizer's to report.  dst is
# filled with 0xAB first.  The source must be unchanged afterwards (exit 7).
DRIVER = r"""
#include "snappy_core.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace mspa::snappy;
int main() {
    int64_t head[2];
    while (fread(head, 8, 2, stdin) == 2) {
        const int64_t n = head[0], expected = head[1];
        uint8_t *src = (uint8_t *)malloc((size_t)n), *keep = (uint8_t *)malloc((size_t)n), *dst = (uint8_t *)malloc((size_t)expected);
        if (n && fread(src, 1, (size_t)n, stdin) != (size_t)n) return 4;
        if (n) memcpy(keep, src, (size_t)n);
        if (expected) memset(dst, 0xAB, (size_t)expected);
        const int64_t rc = decompress(src, n, dst, expected);
        if (n && memcmp(keep, src, (size_t)n) != 0) return 7;
        fwrite(&rc, 8, 1, stdout);
        if (expected) fwrite(dst, 1, (size_t)expected, stdout);
        free(src);
        free(keep);
        free(dst);
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
    return _build(tmp_path_factory, "snappy_decode_driver", ["-O2"])


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    return _build(tmp_path_factory, "snappy_decode_driver_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, cases):
    """cases: [(stream, expected)] -> [(return value, dst bytes)], one run."""
    inp = b"".join(struct.pack("<qq", len(s), e) + s for s, e in cases)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    out, o = [], 0
    for _s, e in cases:
        (rc,) = struct.unpack_from("<q", run.stdout, o)
        out.append((rc, run.stdout[o + 8:o + 8 + e]))
        o += 8 + e
    assert o == len(run.stdout)
    return out


def _check_valid(results):
    for (name, _stream, data), (rc, got) in zip(VU.valid_streams(), results):
        assert rc == len(data) and got == data, name


def _check_corrupt(results):
    for (name, _stream, _expected, code), (rc, _got) in zip(VU.corrupt_streams(), results):
        assert rc == code, (name, rc, code)


def test_both_writers_streams_and_the_hand_built_forms_decode_through_the_driver(driver):
    valid = VU.valid_streams()
    assert len(valid) >= 2 * 62 and max(len(d) for _, _, d in valid) == 131079
    _check_valid(_run(driver, [(s, len(d)) for _, s, d in valid]))


def test_library_host_entry_point_decodes_the_same(driver):
    lib = _lib.load()
    for name, stream, data in VU.valid_streams():
        rc, got = VU.decompress_host(lib, stream, len(data))
        assert rc == len(data) and got == data, name
    dst = np.empty(64, dtype=np.uint8)
    assert lib.mspa_snappy_decompress_host(None, 4, dst.ctypes.data, 4) == _lib.MSPA_EINVAL
    assert lib.mspa_snappy_decompress_host(dst.ctypes.data, 4, None, 4) == _lib.MSPA_EINVAL
    assert lib.mspa_snappy_decompress_host(dst.ctypes.data, -1, dst.ctypes.data, 4) == _lib.MSPA_EINVAL
    assert lib.mspa_snappy_decompress_host(dst.ctypes.data, 4, dst.ctypes.data, 2 ** 31) == _lib.MSPA_EINVAL
    assert (_lib.SNAPPY_EPREAMBLE, _lib.SNAPPY_ETRUNCATED, _lib.SNAPPY_EOVERRUN, _lib.SNAPPY_EOFFSET, _lib.SNAPPY_ETRAILING,
            _lib.SNAPPY_ESHORT) == (VU.E_PREAMBLE, VU.E_TRUNCATED, VU.E_OVERRUN, VU.E_OFFSET, VU.E_TRAILING, VU.E_SHORT)


def test_hand_built_element_forms():
    by_name = {n: (s, d) for n, s, d in VU.valid_streams()}
    lib = _lib.load()
    assert by_name["hand_empty"] == (b"\x00", b"")
    s, d = by_name["hand_copy4"]
    assert s[10] & 3 == 3 and VU.decompress_host(lib, s, len(d)) == (len(d), d)           # a copy-4 tag behind the 8-byte literal
    s, d = by_name["hand_offset1_len64"]
    assert s == b"\x41\x00x" + bytes([2 | 63 << 2, 1, 0]) and d == b"x" * 65
    for extra, n in ((1, 100), (2, 1000), (3, 70000)):
        s, d = by_name[f"hand_lit{extra}_{n}"]
        p = len(VU.SU.encode_varint(len(d)))
        assert s[p] >> 2 == 59 + extra and int.from_bytes(s[p + 1:p + 1 + extra], "little") == n - 1


def test_every_corrupt_stream_is_declined_with_its_code_and_nothing_is_written_outside_dst(driver):
    lib = _lib.load()
    corrupt = VU.corrupt_streams()
    assert sum(1 for c in corrupt if c[0].startswith("cut")) == len(VU.SHORT)                 # truncated at every position
    assert {c[3] for c in corrupt} == {VU.E_PREAMBLE, VU.E_TRUNCATED, VU.E_OVERRUN, VU.E_OFFSET, VU.E_TRAILING, VU.E_SHORT}
    _check_corrupt(_run(driver, [(s, e) for _, s, e, _ in corrupt]))
    for name, stream, expected, code in corrupt:
        rc, _ = VU.decompress_host(lib, stream, expected)                                      # guard bands checked inside
        assert rc == code, (name, rc, code)


def test_sanitized_driver_runs_clean_over_the_corrupt_and_the_valid_sets(sanitized_driver):
    """AddressSanitizer + UBSan on exactly sized heap blocks: no read outside src, no write outside dst, no undefined shift or
    overflow, for any stream of either set -- and the same results."""
    _check_corrupt(_run(sanitized_driver, [(s, e) for _, s, e, _ in VU.corrupt_streams()]))
    _check_valid(_run(sanitized_driver, [(s, len(d)) for _, s, d in VU.valid_streams()]))
