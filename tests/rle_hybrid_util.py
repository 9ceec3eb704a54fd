"""What the tests of the dictionary-coded and v2 pages share (tests/test_rle_hybrid_cpu.py, tests/test_visindex_encoded_pages_cpu.py,
tests/test_gpu_visindex_encoded_pages.py): a Python encoder of parquet's RLE / bit-packed hybrid, a pure-Python model of
csrc/rle_hybrid_core.h's rules, the index files in the layouts pyarrow gives and a pure-Python walk of a values chunk with
pages of every kind the device path takes."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snappy_util as SU  # noqa: E402

E_INVAL, E_BITWIDTH, E_HEADER, E_ZERORUN, E_TRUNCATED, E_SHORT = -1, -32, -33, -34, -35, -36
BIT_WIDTHS = (0, 1, 7, 8, 9, 16, 17, 32)


# ------------------------------------------------------------------------------------------------------------------- the encoder
def uleb(v):
    return SU.encode_varint(v)


def rle_run(count, value, bit_width):
    """``count`` times ``value``: the header, then the value in ceil(bit_width / 8) bytes."""
    return uleb(count << 1) + int(value).to_bytes((bit_width + 7) // 8, "little")


def packed_run(values, bit_width):
    """The values in groups of 8, LSB first, the last group padded with zeros -> (bytes, the values with the padding)."""
    values = list(values) + [0] * (-len(values) % 8)
    acc = 0
    for k, v in enumerate(values):
        assert 0 <= v < (1 << bit_width) or (bit_width == 0 and v == 0)
        acc |= v << (k * bit_width)
    return uleb((len(values) // 8) << 1 | 1) + acc.to_bytes(len(values) // 8 * bit_width, "little"), values


def encode(runs, bit_width):
    """runs: [("rle", count, value) | ("packed", [values])] -> (stream, every value the runs stand for, [(first value, end)] per run)."""
    out, flat, spans = b"", [], []
    for run in runs:
        first = len(flat)
        if run[0] == "rle":
            out += rle_run(run[1], run[2], bit_width)
            flat += [run[2]] * run[1]
        else:
            b, vals = packed_run(run[1], bit_width)
            out += b
            flat += vals
        spans.append((first, len(flat)))
    return out, flat, spans


def int32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


# --------------------------------------------------------------------------------------------------------------------- the model
def py_take(stream, bit_width, n_values, rows):
    """csrc/rle_hybrid_core.h's rules restated: the int32 values of ``rows``, or the code the call is declined with."""
    if not 0 <= bit_width <= 32:
        return E_BITWIDTH
    p = v0 = v1 = q = 0
    packed, last, out = False, -1, []
    for t in rows:
        if t <= last or t >= n_values:
            return E_INVAL
        last = t
        while t >= v1:
            if p >= len(stream):
                return E_SHORT
            h = k = 0
            while True:
                if k == 5 or p + k >= len(stream):
                    return E_HEADER
                c = stream[p + k]
                h |= (c & 127) << (7 * k)
                k += 1
                if c < 128:
                    break
            m = h >> 1
            packed = bool(h & 1)
            count, nbytes = (m * 8, m * bit_width) if packed else (m, (bit_width + 7) // 8)
            if m == 0:
                return E_ZERORUN
            if nbytes > len(stream) - p - k:
                return E_TRUNCATED
            q = p + k
            v0, v1, p = v1, v1 + count, q + nbytes
        if packed:
            out.append(int32(int.from_bytes(stream[q:q + (v1 - v0) // 8 * bit_width], "little") >> ((t - v0) * bit_width) & ((1 << bit_width) - 1)))
        else:
            out.append(int32(int.from_bytes(stream[q:q + (bit_width + 7) // 8], "little")))
    return out


def take_host(lib, stream, bit_width, n_values, rows, guard=16):
    """mspa_rle_hybrid_take_host on an exactly sized copy of the stream, ``out`` between two guard bands: (return value, out)."""
    src = np.frombuffer(bytes(stream), dtype=np.uint8).copy() if len(stream) else np.zeros(1, np.uint8)
    rows = np.asarray(rows, dtype=np.int64)
    out = np.full(len(rows) + 2 * guard, -77, dtype=np.int32)
    rc = lib.mspa_rle_hybrid_take_host(src.ctypes.data if len(stream) else None, len(stream), bit_width, n_values,
                                       rows.ctypes.data if len(rows) else None, len(rows), out.ctypes.data + 4 * guard if len(rows) else None)
    assert (out[:guard] == -77).all() and (out[guard + len(rows):] == -77).all(), "a write outside out"
    return int(rc), out[guard:guard + len(rows)].tolist()


def valid_cases():
    """[(name, stream, bit width, n_values, rows, expected values)]: every bit width of BIT_WIDTHS with RLE runs of 1 and of more
    than 127 values (a 2-byte header), bit-packed runs of 1 and of 64 groups (a 2-byte header), the kinds alternating; rows on
    the first and the last value of every run, inside the padded last group, all of them, one alone, none."""
    rng = np.random.default_rng(5)
    out = []
    for bw in BIT_WIDTHS:
        top = (1 << bw) - 1

        def vals(n):
            return [int(x) for x in rng.integers(0, top + 1, size=n, dtype=np.uint64)] if bw else [0] * n

        runs = [("rle", 1, vals(1)[0]), ("packed", vals(8)), ("rle", 300, top), ("packed", vals(512)), ("rle", 128, vals(1)[0]),
                ("packed", vals(16)), ("rle", 2, 0), ("packed", vals(5))]          # the last group: 5 values and 3 of padding
        stream, flat, spans = encode(runs, bw)
        n_values = len(flat) - 3
        assert len(uleb(300 << 1)) == 2 and len(uleb(64 << 1 | 1)) == 2
        edges = sorted({a for a, _ in spans} | {min(b, n_values) - 1 for _, b in spans})
        for name, rows in (("edges", edges), ("all", list(range(n_values))), ("last", [n_values - 1]), ("first", [0]), ("none", []),
                           ("some", sorted(set(int(x) for x in rng.integers(0, n_values, size=40))))):
            out.append((f"bw{bw}_{name}", stream, bw, n_values, rows, [int32(flat[r]) for r in rows]))
        # with the padding counted as values, a row may lie in it
        out.append((f"bw{bw}_padding", stream, bw, len(flat), [len(flat) - 3, len(flat) - 1], [0, 0]))
    for name, stream, bw, n, rows, want in out:
        assert py_take(stream, bw, n, rows) == want, name
    return out


def corrupt_cases():
    """[(name, stream, bit width, n_values, rows, code)]: every decline code, and MSPA_EINVAL for the rows."""
    good, flat, _ = encode([("rle", 10, 3), ("packed", list(range(8)))], 3)
    out = [
        ("bit_width_33", good, 33, 18, [0], E_BITWIDTH),
        ("bit_width_negative", good, -1, 18, [0], E_BITWIDTH),
        ("bit_width_33_no_rows", good, 33, 18, [], E_BITWIDTH),
        ("header_6_bytes", b"\x80\x80\x80\x80\x80\x01\x03", 3, 18, [0], E_HEADER),
        ("header_past_input", b"\x94", 3, 18, [0], E_HEADER),
        ("header_past_input_second_run", rle_run(10, 3, 3) + b"\x80\x80", 3, 18, [12], E_HEADER),
        ("zero_rle_run", b"\x00\x03", 3, 18, [0], E_ZERORUN),
        ("zero_packed_run", b"\x01", 3, 18, [0], E_ZERORUN),
        ("rle_value_cut", uleb(10 << 1), 3, 18, [0], E_TRUNCATED),
        ("rle_value_cut_2_bytes", uleb(10 << 1) + b"\x01", 9, 18, [0], E_TRUNCATED),
        ("packed_cut", good[:-1], 3, 18, [17], E_TRUNCATED),
        ("packed_cut_not_needed_yet", good[:-1], 3, 18, [12], E_TRUNCATED),
        ("runs_end_early", rle_run(10, 3, 3), 3, 18, [9, 10], E_SHORT),
        ("empty_input", b"", 3, 18, [0], E_SHORT),
        ("rows_descend", good, 3, 18, [5, 4], E_INVAL),
        ("rows_repeat", good, 3, 18, [5, 5], E_INVAL),
        ("row_negative", good, 3, 18, [-1], E_INVAL),
        ("row_beyond", good, 3, 18, [18], E_INVAL),
    ]
    for name, stream, bw, n, rows, code in out:
        assert py_take(stream, bw, n, rows) == code, (name, py_take(stream, bw, n, rows))
    return out


def truncation_cases():
    """Every prefix of a valid stream, with the rows that need all of it -> [(name, stream, bit width, n_values, rows)]."""
    stream, flat, _ = encode([("rle", 200, 257), ("packed", [k * 37 % 512 for k in range(24)]), ("rle", 3, 1), ("packed", [5, 6, 7])], 9)
    n = len(flat) - 5
    rows = [0, 199, 200, 223, 224, 226, 227, n - 1]
    assert py_take(stream, 9, n, rows) == [int32(flat[r]) for r in rows]
    return [(f"cut{k}", stream[:k], 9, n, rows) for k in range(len(stream) + 1)]


# ------------------------------------------------------------------------------------------------------------------- index files
SCENE = "scene0000_00"
N_POINTS = 5000


def _write(table, path, **options):
    import pyarrow.parquet as pq
    pq.write_table(table, path, **options)
    return path


SMALL = dict(dictionary_pagesize_limit=4096, write_batch_size=8, data_page_size=4096)
LAYOUTS = {
    "defaults": {},
    "version_1_0": dict(version="1.0"),
    "small_dictionary": SMALL,
    "small_dictionary_v2": dict(SMALL, data_page_version="2.0"),
    "v2_plain": dict(use_dictionary=False, data_page_version="2.0"),
    "v2_uncompressed": dict(data_page_version="2.0", compression="none"),
    # six image rows are dictionary-coded, the fallback comes inside the next batch: the last two image rows are PLAIN
    "straddle": dict(dictionary_pagesize_limit=50000, write_batch_size=3, data_page_size=4096),
}


def index_files(directory):
    """{name: path}: SU.index_table() (8 image rows of ~9 KB, then 5 000 short rows) in every layout of LAYOUTS."""
    one = SU.index_table()
    return {name: _write(one, os.path.join(str(directory), f"{name}.parquet"), **options) for name, options in LAYOUTS.items()}


def plain_values(body, n):
    out, q = [], 0
    for _ in range(n):
        (m,) = struct.unpack_from("<I", body, q)
        out.append(body[q + 4:q + 4 + m])
        q += 4 + m
    assert q == len(body)
    return out


def walk(path, group=0):
    """A pure-Python walk of row group ``group``'s values chunk, pages of every kind: a list of dicts -- ``type``, ``encoding``,
    ``first_row``, ``values`` (the page's values as bytes: a data page's rows, a dictionary page's entries), ``indices`` (a
    dictionary-coded page's), and where the stream the device decompresses lies: ``stream_pos`` (in the chunk), ``stream_bytes``,
    ``stream_uncompressed``, ``compressed`` (whether it is a Snappy stream)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mspa import parquet_splice as PS
    md = pq.ParquetFile(path).metadata
    col = md.row_group(group).column(1)
    start = col.dictionary_page_offset if col.has_dictionary_page else col.data_page_offset
    with open(path, "rb") as f:
        f.seek(start)
        chunk = f.read(col.total_compressed_size)
    optional = md.schema.column(1).max_definition_level > 0
    snappy = col.compression == "SNAPPY"
    assert snappy or col.compression == "UNCOMPRESSED"

    def inflate(body, size, compressed):
        return pa.Codec("snappy").decompress(body, decompressed_size=size).to_pybytes() if compressed and size else bytes(body)

    out, p, row, dictionary = [], 0, 0, None
    while p < len(chunk):
        r = PS._Reader(chunk, p)
        h = r.struct()
        p = r.p
        ptype, unc, comp = PS._get(h, 1), PS._get(h, 2), PS._get(h, 3)
        v1, dic, v2 = PS._get(h, 5), PS._get(h, 7), PS._get(h, 8)
        page = {"type": ptype, "first_row": row, "stream_pos": p, "stream_bytes": comp, "stream_uncompressed": unc, "compressed": snappy}
        if ptype == 2:
            page["encoding"] = PS._get(dic, 2)
            page["values"] = dictionary = plain_values(inflate(chunk[p:p + comp], unc, snappy), PS._get(dic, 1))
        else:
            nv = PS._get(v1 or v2, 1)
            page["encoding"] = PS._get(v1, 2) if v1 else PS._get(v2, 4)
            if v1:
                body = inflate(chunk[p:p + comp], unc, snappy)
                if optional:
                    (L,) = struct.unpack_from("<I", body, 0)
                    assert body[4:4 + L] == uleb(nv << 1) + b"\x01"
                    body = body[4 + L:]
            else:
                lev = PS._get(v2, 5) + PS._get(v2, 6)
                assert PS._get(v2, 2) == 0 and PS._get(v2, 6) == 0 and chunk[p:p + lev] == (uleb(nv << 1) + b"\x01" if optional else b"")
                packed = snappy and bool(PS._get(v2, 7, True))
                page.update(stream_pos=p + lev, stream_bytes=comp - lev, stream_uncompressed=unc - lev, compressed=packed)
                body = inflate(chunk[p + lev:p + comp], unc - lev, packed)
            if page["encoding"] == 0:
                page["values"] = plain_values(body, nv)
            else:
                assert page["encoding"] in (2, 8)
                page["indices"] = py_take(body[1:], body[0], nv, list(range(nv)))
                page["values"] = [dictionary[k] for k in page["indices"]]
            row += nv
        out.append(page)
        p += comp
    return out
