"""The Snappy compressor and the page geometry of csrc/snappy_core.h on the CPU: a g++ build of the header over the shared stream
set (tests/snappy_util.py), with pyarrow's Snappy decoder as the independent oracle, and the library's host entry points against
the driver's bytes."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snappy_util as SU  # noqa: E402

from mspa import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")

# Records until the input ends.  'S', int64 n, n bytes -> int64 m, m stream bytes (the input is checked to be unchanged: exit 7;
# a stream longer than its capacity: exit 8).  'C', int64 rows, int64 page_bytes, rows + 1 int32 -> int64 pages, pages + 1 int64.
DRIVER = r"""
#include "snappy_core.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace mspa::snappy;
int main() {
    int kind;
    while ((kind = getchar()) != EOF) {
        int64_t head[2];
        if (kind == 'S') {
            if (fread(head, 8, 1, stdin) != 1) return 3;
            const int64_t n = head[0];
            std::vector<uint8_t> src((size_t)n), dst((size_t)capacity(n) + 64, 0xAB);
            if (n && fread(src.data(), 1, (size_t)n, stdin) != (size_t)n) return 4;
            const std::vector<uint8_t> before(src);
            const int64_t m = compress_host(src.data(), n, dst.data());
            if (before != src) return 7;
            if (m > capacity(n)) return 8;
            for (int64_t i = capacity(n); i < capacity(n) + 64; ++i) if (dst[(size_t)i] != 0xAB) return 9;
            fwrite(&m, 8, 1, stdout);
            fwrite(dst.data(), 1, (size_t)m, stdout);
        } else if (kind == 'C') {
            if (fread(head, 8, 2, stdin) != 2) return 5;
            const int64_t rows = head[0];
            std::vector<int32_t> offsets((size_t)rows + 1);
            if (fread(offsets.data(), 4, offsets.size(), stdin) != offsets.size()) return 6;
            std::vector<int64_t> cuts((size_t)rows + 1, -1);
            const int64_t pages = page_cuts(offsets.data(), rows, head[1], cuts.data(), rows + 1);
            if (pages < 0 || pages != page_cuts(offsets.data(), rows, head[1], nullptr, 0)) return 10;
            fwrite(&pages, 8, 1, stdout);
            fwrite(cuts.data(), 8, (size_t)pages + 1, stdout);
        } else {
            return 2;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("snappy_driver")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    build = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(d / "driver.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


@pytest.fixture(scope="module")
def compressed(driver):
    """{name: (data, stream)} of the whole stream set, one driver run."""
    cases = SU.streams()
    inp = b"".join(b"S" + struct.pack("<q", len(d)) + d for _, d in cases)
    run = subprocess.run([driver], input=inp, capture_output=True, timeout=120)
    assert run.returncode == 0, run.returncode
    out, o = {}, 0
    for name, d in cases:
        (m,) = struct.unpack_from("<q", run.stdout, o)
        out[name] = (d, run.stdout[o + 8:o + 8 + m])
        o += 8 + m
    assert o == len(run.stdout) and len(out) == len(cases)
    return out


def _copies(blocks):
    return [(e[1], e[3]) for els in blocks for e in els if e[0] == "copy"]


def test_every_stream_round_trips_through_pyarrow_within_capacity_block_by_block(compressed):
    lib = _lib.load()
    for name, (data, stream) in compressed.items():
        SU.check_stream(name, data, stream, lib.mspa_snappy_capacity(len(data)))


def test_library_host_entry_point_returns_the_drivers_bytes(compressed):
    lib = _lib.load()
    for name, (data, stream) in compressed.items():
        assert SU.compress_host(lib, data) == stream, name
    assert lib.mspa_snappy_capacity(-1) == -1 and lib.mspa_snappy_capacity(2 ** 31) == -1 and lib.mspa_snappy_capacity(6000) == 7032
    dst = np.empty(64, dtype=np.uint8)
    assert lib.mspa_snappy_compress_host(dst.ctypes.data, 100, dst.ctypes.data, 64) == _lib.MSPA_EINVAL          # dst too small
    assert lib.mspa_snappy_compress_host(None, 4, dst.ctypes.data, 64) == _lib.MSPA_EINVAL
    assert lib.mspa_snappy_compress_host(dst.ctypes.data, -1, dst.ctypes.data, 64) == _lib.MSPA_EINVAL


def test_zeros_overlap_at_offset_one_in_64_byte_pieces_with_the_60_byte_tail_rule(compressed):
    for n, pieces in ((66, [60, 5]), (67, [60, 6]), (68, [60, 7]), (69, [64, 4]), (65, [64]), (64, [63]), (5, [4])):
        data, stream = compressed[f"zeros{n}"]
        els = SU.split_blocks(stream)[1][0]
        assert els[0][:2] == ("lit", 1) and [e[1:] for e in els[1:]] == [(2 if sum(pieces) > 11 else 1, 1, k) for k in pieces], n
    data, stream = compressed["zeros65536"]
    els = SU.split_blocks(stream)[1][0]                    # 65 535 = 1023 * 64 + 63
    assert [e[3] for e in els[1:]] == [64] * 1023 + [63] and len(stream) == 3 + 2 + 3 * 1024
    for n in (0, 1, 3, 4):                                  # nothing to hash: one literal, or nothing
        data, stream = compressed[f"zeros{n}"]
        assert stream == SU.encode_varint(n) + (bytes([(n - 1) << 2]) + data if n else b"")


def test_noise_is_one_literal_per_block_and_identical_halves_do_not_reach_across_the_boundary(compressed):
    data, stream = compressed["noise65536"]
    assert stream == SU.encode_varint(65536) + bytes([61 << 2, 0xFF, 0xFF]) + data
    data, stream = compressed["halves"]
    n, blocks = SU.split_blocks(stream)
    assert n == 2 * SU.BLOCK and [[e[:2] for e in els] for els in blocks] == [[("lit", SU.BLOCK)]] * 2
    data, stream = compressed["noise65537"]
    assert [[e[:2] for e in els] for els in SU.split_blocks(stream)[1]] == [[("lit", SU.BLOCK)], [("lit", 1)]]


def test_periodic_digit_text_is_found_inside_a_chunk(compressed):
    # the lists repeat at distances 7 - 9: the first period is a literal, everything after it one copy at that distance
    for period in (7, 9):
        data, stream = compressed[f"p{period}_65536"]
        els = SU.split_blocks(stream)[1][0]
        assert els[0][:2] == ("lit", period) and {e[2] for e in els[1:]} == {period}
        assert sum(e[3] for e in els[1:]) == SU.BLOCK - period and len(stream) < 3200


def test_copy_lengths_forms_and_a_far_match(compressed):
    for k in SU.COPY_LENGTHS:
        data, stream = compressed[f"copy{k}"]
        copies = _copies(SU.split_blocks(stream)[1])
        want = SU.COPY_PIECES[k]
        assert any(copies[i:i + len(want)] == want for i in range(len(copies))), (k, copies)
    data, stream = compressed["far"]
    far = [e for e in SU.split_blocks(stream)[1][0] if e[0] == "copy" and e[2] >= 2048]
    assert far and far[0][1:] == (2, 3000, 40)             # 40 bytes from 3 000 back: the 3-byte form whatever the length
    data, stream = compressed["json"]
    import pyarrow as pa
    theirs = len(pa.Codec("snappy").compress(data))
    print(f"json lists: {len(data)} -> {len(stream)} bytes, pyarrow's Snappy {theirs}")
    assert len(stream) <= 1.10 * theirs                    # the cap of tests/test_parquet_assemble_cpu.py, on sparser lists


def test_page_cut_rule(driver):
    lib = _lib.load()
    cases = [
        ([0], 4096),                                                         # no rows: no pages
        ([0, 10], 4096),                                                     # one short row: one page
        ([0, 10, 20, 30], 14),                                               # every row lands exactly on the threshold
        ([0, 10, 20, 30], 15),                                               # ... and one byte short of it: pairs
        ([0, 5, 5000, 5004, 5008, 5008, 5010], 100),                         # one value larger than page_bytes; empty strings
        ([0, 96, 192, 288], 200),                                            # 100 + 100 reaches 200 exactly
        (list(range(0, 4000, 4)), 4096),                                     # 8 bytes per value: 512 values per page
    ]
    want = [[0], [0, 1], [0, 1, 2, 3], [0, 2, 3], [0, 2, 6], [0, 2, 3], [0, 512, 999]]
    inp = b"".join(b"C" + struct.pack("<qq", len(o) - 1, pb) + np.asarray(o, np.int32).tobytes() for o, pb in cases)
    run = subprocess.run([driver], input=inp, capture_output=True, timeout=60)
    assert run.returncode == 0, run.returncode
    o = 0
    for (offsets, pb), cuts in zip(cases, want):
        (pages,) = struct.unpack_from("<q", run.stdout, o)
        got = list(struct.unpack_from(f"<{pages + 1}q", run.stdout, o + 8))
        o += 8 * (pages + 2)
        assert got == cuts, (offsets, pb, got)
        assert SU.page_cuts_host(lib, offsets, pb).tolist() == cuts
    assert o == len(run.stdout)
    bad = np.array([0, 5, 3], dtype=np.int32)
    cuts = np.empty(3, dtype=np.int64)
    assert lib.mspa_parquet_page_cuts_host(bad.ctypes.data, 2, 100, cuts.ctypes.data, 3) == _lib.MSPA_EINVAL       # decreasing
    assert lib.mspa_parquet_page_cuts_host(bad.ctypes.data, 1, 0, cuts.ctypes.data, 3) == _lib.MSPA_EINVAL
    assert lib.mspa_parquet_page_cuts_host(bad.ctypes.data, 1, 1, cuts.ctypes.data, 1) == _lib.MSPA_EINVAL         # cuts too small


def test_page_payload_is_levels_then_plain_values():
    lib = _lib.load()
    offsets = np.array([0, 3, 3, 8], dtype=np.int32)
    data = np.frombuffer(b"abcdefgh", dtype=np.uint8)
    assert SU.page_payload_host(lib, offsets, data, 0, 3) == (b"\x02\x00\x00\x00" + b"\x06\x01" + b"\x03\x00\x00\x00abc" + b"\x00\x00\x00\x00"
                                                              + b"\x05\x00\x00\x00defgh")
    assert SU.page_payload_host(lib, offsets, data, 2, 3) == b"\x02\x00\x00\x00" + b"\x02\x01" + b"\x05\x00\x00\x00defgh"
    many = np.arange(0, 101, dtype=np.int32)                                # 100 values: varint(200) takes two bytes
    assert SU.page_payload_host(lib, many, np.zeros(100, np.uint8), 0, 100)[:7] == b"\x03\x00\x00\x00\xc8\x01\x01"
