"""Parquet's RLE / bit-packed hybrid of csrc/rle_hybrid_core.h on the CPU: the library's host entry point
(mspa_rle_hybrid_take_host) and a g++ build of the header (plain, and a second time under AddressSanitizer + UBSan, a stand-alone
program with exactly sized heap buffers) against a pure-Python model, over streams from a Python encoder, the indices of real
pages pyarrow wrote, every decline code and every truncation of a valid stream (tests/rle_hybrid_util.py)."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rle_hybrid_util as RU  # noqa: E402

from mspa import _lib, engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")

# Records until the input ends: int64 src_len, int64 bit_width, int64 n_values, int64 n_rows, src bytes, rows (int64) -> int64
# return value, n_rows int32 of out.  src, rows and out are heap blocks of exactly their sizes: a read or a write outside them
# is the sanitizer's to report.  out is filled with -77 first.  The source must be unchanged afterwards (exit 7).
DRIVER = r"""
#include "rle_hybrid_core.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace mspa::rle_hybrid;
int main() {
    int64_t head[4];
    while (fread(head, 8, 4, stdin) == 4) {
        const int64_t n = head[0], bw = head[1], nv = head[2], nr = head[3];
        uint8_t *src = (uint8_t *)malloc((size_t)n), *keep = (uint8_t *)malloc((size_t)n);
        int64_t *rows = (int64_t *)malloc((size_t)nr * 8);
        int32_t *out = (int32_t *)malloc((size_t)nr * 4);
        if (n && fread(src, 1, (size_t)n, stdin) != (size_t)n) return 4;
        if (nr && fread(rows, 8, (size_t)nr, stdin) != (size_t)nr) return 4;
        if (n) memcpy(keep, src, (size_t)n);
        for (int64_t i = 0; i < nr; ++i) out[i] = -77;
        const int64_t rc = take(src, n, (int32_t)bw, nv, rows, nr, out);
        if (n && memcmp(keep, src, (size_t)n) != 0) return 7;
        fwrite(&rc, 8, 1, stdout);
        if (nr) fwrite(out, 4, (size_t)nr, stdout);
        free(src);
        free(keep);
        free(rows);
        free(out);
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
    return _build(tmp_path_factory, "rle_hybrid_driver", ["-O2"])


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    return _build(tmp_path_factory, "rle_hybrid_driver_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, cases):
    """cases: [(stream, bit width, n_values, rows)] -> [(return value, out)], one run."""
    inp = b"".join(struct.pack("<qqqq", len(s), bw, nv, len(rows)) + bytes(s) + struct.pack(f"<{len(rows)}q", *rows) for s, bw, nv, rows in cases)
    run = subprocess.run([exe], input=inp, capture_output=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:].decode(errors="replace"))
    out, o = [], 0
    for _s, _bw, _nv, rows in cases:
        (rc,) = struct.unpack_from("<q", run.stdout, o)
        out.append((rc, list(struct.unpack_from(f"<{len(rows)}i", run.stdout, o + 8))))
        o += 8 + 4 * len(rows)
    assert o == len(run.stdout)
    return out


def _against_the_model(cases, results):
    """Every result is the model's: its values, or the code it declines with (the rows in front of the one that met it may be
    written, the others are not)."""
    for (name, stream, bw, nv, rows), (rc, got) in zip(cases, results):
        want = RU.py_take(stream, bw, nv, rows)
        if isinstance(want, int):
            assert rc == want, (name, rc, want)
        else:
            assert rc == 0 and got == want, (name, rc)


def _all_cases():
    return ([c[:5] for c in RU.valid_cases()] + [c[:5] for c in RU.corrupt_cases()] + RU.truncation_cases())


def test_the_encoders_streams_decode_as_the_model_says():
    lib = _lib.load()
    valid = RU.valid_cases()
    assert {c[2] for c in valid} == set(RU.BIT_WIDTHS) and len(valid) == 7 * len(RU.BIT_WIDTHS)
    for name, stream, bw, nv, rows, want in valid:
        assert RU.take_host(lib, stream, bw, nv, rows) == (0, want), name
        rc, got = engine.rle_hybrid_take_host(stream, bw, nv, rows)
        assert rc == 0 and got.dtype == np.int32 and got.tolist() == want, name


def _dictionary_pages(path):
    """[(stream behind the bit width, bit width, n_values, the page's indices by the model)] of the file's dictionary-coded pages."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mspa import parquet_splice as PS
    col = pq.ParquetFile(path).metadata.row_group(0).column(1)
    with open(path, "rb") as f:
        f.seek(col.dictionary_page_offset)
        chunk = f.read(col.total_compressed_size)
    out, p = [], 0
    while p < len(chunk):
        r = PS._Reader(chunk, p)
        h = r.struct()
        p = r.p + PS._get(h, 3)
        v1 = PS._get(h, 5)
        if v1 is None or PS._get(v1, 2) not in (2, 8):
            continue
        body = pa.Codec("snappy").decompress(chunk[r.p:p], decompressed_size=PS._get(h, 2)).to_pybytes()
        (L,) = struct.unpack_from("<I", body, 0)
        out.append((body[4 + L + 1:], body[4 + L], PS._get(v1, 1)))
    return out


@pytest.mark.parametrize("name", ["one_entry", "duplicates", "runs_and_noise"])
def test_real_pages_indices_equal_pyarrows(tmp_path, name):
    """The indices of pages pyarrow wrote against the indices pyarrow reads back (``read_dictionary``): a one-entry dictionary
    (bit width 0 or 1: one RLE run), a table with duplicate values, and long runs between noise over several pages."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    lib = _lib.load()
    rng = np.random.default_rng(8)
    values = {"one_entry": ["[1, 2, 3]"] * 100,
              "duplicates": [f"[{k % 37}]" for k in range(1000)],
              "runs_and_noise": [f"[{k}]" for k in np.concatenate([rng.integers(0, 300, 700), np.full(900, 7), rng.integers(0, 300, 500),
                                                                   np.full(77, 5), rng.integers(0, 2, 300)])]}[name]
    path = str(tmp_path / f"{name}.parquet")
    table = pa.table({"key": pa.array([f"s:k:{k}" for k in range(len(values))], pa.string()), "values": pa.array(values, pa.string())})
    pq.write_table(table, path, **({} if name == "one_entry" else dict(data_page_size=64, write_batch_size=100)))
    back = pq.read_table(path, read_dictionary=["values"]).column("values")
    want = np.concatenate([c.indices.to_numpy() for c in back.chunks]).tolist()
    dictionary = back.chunk(0).dictionary.to_pylist()
    assert all(c.dictionary.to_pylist() == dictionary for c in back.chunks) and [dictionary[k] for k in want] == values
    assert (len(dictionary) == 1) == (name == "one_entry")
    pages = _dictionary_pages(path)
    assert sum(nv for _, _, nv in pages) == len(values) and (len(pages) > 1) == (name != "one_entry")
    first = 0
    for stream, bw, nv in pages:
        rows = list(range(nv))
        assert RU.take_host(lib, stream, bw, nv, rows) == (0, want[first:first + nv])
        some = rows[::7] + ([rows[-1]] if (nv - 1) % 7 else [])
        assert RU.take_host(lib, stream, bw, nv, some) == (0, [want[first + r] for r in some])
        first += nv


def test_every_decline_code_and_the_rows_check():
    lib = _lib.load()
    corrupt = RU.corrupt_cases()
    assert {c[5] for c in corrupt} == {RU.E_INVAL, RU.E_BITWIDTH, RU.E_HEADER, RU.E_ZERORUN, RU.E_TRUNCATED, RU.E_SHORT}
    assert (_lib.MSPA_EINVAL, _lib.RLE_EBITWIDTH, _lib.RLE_EHEADER, _lib.RLE_EZERORUN, _lib.RLE_ETRUNCATED, _lib.RLE_ESHORT) == \
        (RU.E_INVAL, RU.E_BITWIDTH, RU.E_HEADER, RU.E_ZERORUN, RU.E_TRUNCATED, RU.E_SHORT)
    snappy_and_own = {_lib.MSPA_EINVAL, _lib.MSPA_EHIP, _lib.MSPA_EUNSUPPORTED} | set(range(-22, -15))
    assert not ({RU.E_BITWIDTH, RU.E_HEADER, RU.E_ZERORUN, RU.E_TRUNCATED, RU.E_SHORT} & snappy_and_own)
    for name, stream, bw, nv, rows, code in corrupt:
        assert RU.take_host(lib, stream, bw, nv, rows)[0] == code, name
        if code == RU.E_INVAL:
            with pytest.raises(_lib.MspaError):
                engine.rle_hybrid_take_host(stream, bw, nv, rows)
        else:
            assert engine.rle_hybrid_take_host(stream, bw, nv, rows)[0] == code, name
    out = np.zeros(4, dtype=np.int32)
    rows = np.arange(4, dtype=np.int64)
    assert lib.mspa_rle_hybrid_take_host(None, 4, 3, 4, rows.ctypes.data, 4, out.ctypes.data) == _lib.MSPA_EINVAL
    assert lib.mspa_rle_hybrid_take_host(out.ctypes.data, 4, 3, 4, None, 4, out.ctypes.data) == _lib.MSPA_EINVAL
    assert lib.mspa_rle_hybrid_take_host(out.ctypes.data, 4, 3, 4, rows.ctypes.data, 4, None) == _lib.MSPA_EINVAL
    assert lib.mspa_rle_hybrid_take_host(out.ctypes.data, -1, 3, 4, rows.ctypes.data, 4, out.ctypes.data) == _lib.MSPA_EINVAL
    assert lib.mspa_rle_hybrid_take_host(out.ctypes.data, 2 ** 31, 3, 4, rows.ctypes.data, 4, out.ctypes.data) == _lib.MSPA_EINVAL


def test_every_truncation_gives_the_models_values_or_a_decline():
    """Cut at every position, the stream either still holds the needed rows -- then the values are the model's -- or is
    declined; the walk stops at the last needed row, so rows in front of the cut still come out."""
    lib = _lib.load()
    cuts = RU.truncation_cases()
    full = RU.py_take(*cuts[-1][1:])
    declined = 0
    for name, stream, bw, nv, rows in cuts:
        rc, got = RU.take_host(lib, stream, bw, nv, rows)
        want = RU.py_take(stream, bw, nv, rows)
        if isinstance(want, int):
            assert rc == want and rc in (RU.E_HEADER, RU.E_TRUNCATED, RU.E_SHORT), (name, rc, want)
            declined += 1
        else:
            assert rc == 0 and got == want == full, name
    assert declined == len(cuts) - 1                  # the last row lies in the last run, and a run is checked whole
    stream = cuts[-1][1]
    assert RU.take_host(lib, stream[:4], 9, cuts[-1][3], [0, 199]) == (0, full[:2])        # what lies behind is never looked at


def test_the_header_build_equals_the_model_on_every_case(driver):
    cases = _all_cases()
    _against_the_model(cases, _run(driver, [c[1:] for c in cases]))


def test_sanitized_driver_runs_clean_over_the_valid_the_corrupt_and_the_truncated_sets(sanitized_driver):
    """AddressSanitizer + UBSan on exactly sized heap blocks: no read outside src or rows, no write outside out, no undefined
    shift or overflow, for any case -- and the same results."""
    cases = _all_cases()
    _against_the_model(cases, _run(sanitized_driver, [c[1:] for c in cases]))
