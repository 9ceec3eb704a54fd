"""csrc/snappy_core.h's block_starts and decompress_block on the CPU: a g++ build of the header with a stand-alone driver (plain,
and a second time under AddressSanitizer + UBSan with exactly sized heap buffers) and the library's host entry point, over both
writers' streams, hand-built streams that are and are not blockwise, the segment shapes of the device scan and the corrupt set
(tests/snappy_blocks_util.py)."""
import os
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snappy_blocks_util as BU  # noqa: E402
import snappy_util as SU  # noqa: E402

from mspa import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")

# Records until the input ends: int64 src_len, int64 expected, src bytes -> int64 decompress's return value, int64 block_starts'
# return value, ceil(expected / 65536) + 1 starts (int64, -7 where nothing was written), int64 blocks whose decompress_block
# returned their size, and -- when block_starts returned a count > 0 -- the `expected` bytes the blocks decoded to.  Every buffer
# is a heap block of exactly its size (each block decodes into one of exactly ITS size): a read or a write outside is the
# sanitizer's to report.  The source must be unchanged afterwards (exit 7).
DRIVER = r"""
#include "snappy_core.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace mspa::snappy;
int main() {
    int64_t head[2];
    while (fread(head, 8, 2, stdin) == 2) {
        const int64_t n = head[0], expected = head[1], cap = block_count(expected) + 1;
        uint8_t *src = (uint8_t *)malloc((size_t)n), *keep = (uint8_t *)malloc((size_t)n), *dst = (uint8_t *)malloc((size_t)expected);
        int64_t *starts = (int64_t *)malloc((size_t)cap * 8);
        if (n && fread(src, 1, (size_t)n, stdin) != (size_t)n) return 4;
        if (n) memcpy(keep, src, (size_t)n);
        for (int64_t b = 0; b < cap; ++b) starts[b] = -7;
        const int64_t rc = decompress(src, n, dst, expected);
        const int64_t blocks = block_starts(src, n, expected, starts, cap);
        fwrite(&rc, 8, 1, stdout);
        fwrite(&blocks, 8, 1, stdout);
        fwrite(starts, 8, (size_t)cap, stdout);
        int64_t good = 0;
        if (blocks > 0) {
            uint8_t *all = (uint8_t *)malloc((size_t)expected);
            for (int64_t b = 0; b < blocks; ++b) {
                const int64_t nb = expected - b * kBlock < kBlock ? expected - b * kBlock : kBlock;
                uint8_t *one = (uint8_t *)malloc((size_t)nb);
                memset(one, 0xAB, (size_t)nb);
                if (decompress_block(src, starts[b], starts[b + 1], one, nb) == nb) ++good;
                memcpy(all + b * kBlock, one, (size_t)nb);
                free(one);
            }
            fwrite(&good, 8, 1, stdout);
            fwrite(all, 1, (size_t)expected, stdout);
            free(all);
        } else {
            fwrite(&good, 8, 1, stdout);
        }
        if (n && memcmp(keep, src, (size_t)n) != 0) return 7;
        free(src);
        free(keep);
        free(dst);
        free(starts);
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
    return _build(tmp_path_factory, "snappy_blocks_driver", ["-O2"])


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    return _build(tmp_path_factory, "snappy_blocks_driver_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, cases):
    """cases: [(stream, expected)] -> [(decompress rc, block_starts rc, starts, good blocks, block bytes or None)], one run."""
    inp = b"".join(struct.pack("<qq", len(s), e) + s for s, e in cases)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    out, o = [], 0
    for _s, e in cases:
        cap = BU.block_count(e) + 1
        vals = struct.unpack_from(f"<{cap + 3}q", run.stdout, o)
        o += 8 * (cap + 3)
        data = None
        if vals[1] > 0:
            data = run.stdout[o:o + e]
            o += e
        out.append((vals[0], vals[1], list(vals[2:2 + cap]), vals[2 + cap], data))
    assert o == len(run.stdout)
    return out


def _valid():
    """[(name, stream, data, blockwise)]: every valid stream of the three sets."""
    return ([(n, s, d, True) for n, s, d in BU.writer_streams()] + list(BU.hand_streams()) +
            [(n, s, d, True) for n, s, d in BU.segment_streams()])


def _check_valid(results):
    for (name, stream, data, blockwise), (rc, blocks, starts, good, got) in zip(_valid(), results):
        assert rc == len(data), name                                              # decompress still decodes every one of them
        want, want_starts = BU.py_block_starts(stream, len(data))
        assert blocks == want, (name, blocks, want)
        if not blockwise:
            assert blocks == BU.NOT_BLOCKWISE, name
            continue
        assert blocks == BU.block_count(len(data)) and starts == want_starts, name
        if blocks:
            assert good == blocks and got == data, name                           # each block alone, and their concatenation


def _check_corrupt(results):
    for (name, _stream, _expected), (rc, blocks, _starts, _good, _got) in zip(BU.corrupt_streams(), results):
        assert rc < 0 and blocks == rc, (name, rc, blocks)                          # decompress's code, whatever else is the matter


def test_both_writers_streams_are_blockwise_and_every_block_decodes_alone(driver):
    valid = _valid()
    names = [n for n, *_ in valid]
    assert {"pa_lists5", "own_lists5", "pa_mix3", "own_mix3", "pa_noise131079", "own_zeros131079"} <= set(names)
    assert BU.block_count(len(BU.list_text())) >= 5 and max(len(s) for _, s, _, _ in valid) <= 400_000
    _check_valid(_run(driver, [(s, len(d)) for _, s, d, _ in valid]))
    # the walk of the elements agrees with tests/snappy_util.py's element reader on what a block holds
    for name, stream, data in BU.writer_streams():
        if name in ("pa_lists5", "own_lists5", "pa_mix3", "own_mix3"):
            _, starts = BU.py_block_starts(stream, len(data))
            for b in range(len(starts) - 1):
                assert SU.decode_elements(SU.elements(stream[starts[b]:starts[b + 1]])) == data[b * BU.BLOCK:(b + 1) * BU.BLOCK], (name, b)


def test_hand_built_streams_not_blockwise_and_blockwise():
    lib = _lib.load()
    by_name = {n: (s, d, bw) for n, s, d, bw in BU.hand_streams()}
    assert [n for n, v in by_name.items() if not v[2]] == ["nb_literal_70000", "nb_copy_into_block0", "nb_copy2_crosses"]
    for name, (s, d, bw) in by_name.items():
        rc, starts = BU.block_starts_host(lib, s, len(d))
        if bw:
            assert (rc, starts) == BU.py_block_starts(s, len(d)), name
        else:
            assert rc == BU.NOT_BLOCKWISE == _lib.SNAPPY_NOT_BLOCKWISE, (name, rc)
    s, d, _ = by_name["bw_copy4_literal_heads"]
    p = len(SU.encode_varint(len(d)))
    assert s[p] == 60 << 2 and s.count(BU.copy4(60000, 64)) == 8 and BU.lit(b"xyz", 4) in s and len(d) > BU.BLOCK


def test_library_host_entry_point(driver):
    lib = _lib.load()
    for name, stream, data, blockwise in _valid():
        rc, starts = BU.block_starts_host(lib, stream, len(data))
        want, want_starts = BU.py_block_starts(stream, len(data))
        assert rc == want and (not blockwise or starts == want_starts), name
    import numpy as np
    buf = np.zeros(8, dtype=np.int64)
    src = np.zeros(8, dtype=np.uint8)
    assert lib.mspa_snappy_block_starts_host(None, 4, 4, buf.ctypes.data, 8) == _lib.MSPA_EINVAL
    assert lib.mspa_snappy_block_starts_host(src.ctypes.data, 4, 4, None, 8) == _lib.MSPA_EINVAL
    assert lib.mspa_snappy_block_starts_host(src.ctypes.data, 4, 65537, buf.ctypes.data, 2) == _lib.MSPA_EINVAL      # three entries needed
    assert lib.mspa_snappy_block_starts_host(src.ctypes.data, -1, 4, buf.ctypes.data, 8) == _lib.MSPA_EINVAL
    assert lib.mspa_snappy_blocks_workspace_bytes(-1, 1, 1) == -1 and lib.mspa_snappy_blocks_workspace_bytes(1000, 2, 3) >= 8 * 1000
    for args in ((None, 0, None, None, 1, None, None, 0, 0, None, 0, None, None, None),):
        assert lib.mspa_snappy_block_starts_device(*args) == _lib.MSPA_EINVAL                                         # before anything is enqueued
    assert lib.mspa_snappy_decompress_blocks_device(None, 0, None, None, 1, None, 0, None, None, None, 0, 0, None, 0, None, None,
                                                    None) == _lib.MSPA_EINVAL
    assert lib.mspa_snappy_decompress_blocks_device(None, -1, None, None, 0, None, 0, None, None, None, 0, 0, None, 0, None, None,
                                                    None) == _lib.MSPA_EINVAL


def test_corrupt_streams_get_the_decoders_code(driver):
    lib = _lib.load()
    corrupt = BU.corrupt_streams()
    assert sum(1 for c in corrupt if c[0].startswith("cut_block1_")) == 16
    results = _run(driver, [(s, e) for _, s, e in corrupt])
    _check_corrupt(results)
    for (name, stream, expected), (rc, *_rest) in zip(corrupt, results):
        assert BU.block_starts_host(lib, stream, expected)[0] == rc, name


def test_sanitized_driver_runs_clean_over_the_corrupt_and_the_valid_sets(sanitized_driver):
    """AddressSanitizer + UBSan on exactly sized heap blocks: no read outside src, no write outside a block's own bytes or the
    starts table, for any stream of either set -- and the same results."""
    _check_corrupt(_run(sanitized_driver, [(s, e) for _, s, e in BU.corrupt_streams()]))
    _check_valid(_run(sanitized_driver, [(s, len(d)) for _, s, d, _ in _valid()]))
