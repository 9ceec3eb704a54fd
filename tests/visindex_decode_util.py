"""What the tests of the index's way back share (tests/test_snappy_decode_cpu.py, tests/test_visindex_pages_cpu.py,
tests/test_gpu_visindex_decode.py): the Snappy streams to decode -- both writers' streams of tests/snappy_util.py's set, hand-built
ones, corrupt ones with the code each must be declined with --, a pure-Python model of the decoder's rules, the index files of
the page tests and a pure-Python walk of a values chunk."""
import functools
import json
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snappy_util as SU  # noqa: E402

E_PREAMBLE, E_TRUNCATED, E_OVERRUN, E_OFFSET, E_TRAILING, E_SHORT = -16, -17, -18, -19, -20, -21


# --------------------------------------------------------------------------------------------------------------- stream builders
def lit(data, extra=None):
    """A literal element; ``extra``: how many length bytes to spend (default: the fewest)."""
    m = len(data) - 1
    if extra is None:
        extra = 0 if m < 60 else (m.bit_length() + 7) // 8
    if extra == 0:
        assert m < 60
        return bytes([m << 2]) + data
    return bytes([(59 + extra) << 2]) + m.to_bytes(extra, "little") + data


def copy1(offset, n):
    assert 4 <= n <= 11 and offset < 2048
    return bytes([1 | (n - 4) << 2 | (offset >> 8) << 5, offset & 255])


def copy2(offset, n):
    assert 1 <= n <= 64 and offset < 65536
    return bytes([2 | (n - 1) << 2]) + offset.to_bytes(2, "little")


def copy4(offset, n):
    assert 1 <= n <= 64
    return bytes([3 | (n - 1) << 2]) + offset.to_bytes(4, "little")


def py_decode(stream, expected):
    """The decoder's rules (csrc/snappy_core.h) restated: the bytes, or the code the stream is declined with."""
    v = shift = p = 0
    while True:
        if p >= len(stream) or p >= 5:
            return E_PREAMBLE
        c = stream[p]
        p += 1
        v |= (c & 127) << shift
        shift += 7
        if c < 128:
            break
    if v != expected:
        return E_PREAMBLE
    out = bytearray()
    while p < len(stream):
        if len(out) == expected:
            return E_TRAILING
        tag = stream[p]
        kind, m = tag & 3, tag >> 2
        extra = (0 if m < 60 else m - 59) if kind == 0 else (1, 2, 4)[kind - 1]
        if p + 1 + extra > len(stream):
            return E_TRUNCATED
        field = int.from_bytes(stream[p + 1:p + 1 + extra], "little")
        if kind == 0:
            n = (field if extra else m) + 1
            if p + 1 + extra + n > len(stream):
                return E_TRUNCATED
            if len(out) + n > expected:
                return E_OVERRUN
            out += stream[p + 1 + extra:p + 1 + extra + n]
            p += 1 + extra + n
            continue
        n, offset = (4 + (m & 7), (tag >> 5) << 8 | field) if kind == 1 else (m + 1, field)
        if offset == 0 or offset > len(out):
            return E_OFFSET
        if len(out) + n > expected:
            return E_OVERRUN
        for _ in range(n):
            out.append(out[-offset])
        p += 1 + extra
    return bytes(out) if len(out) == expected else E_SHORT


FAR_NAME = "hand_copy4_70000_back"          # the one stream whose copy reaches further back than 64 KiB


@functools.lru_cache(maxsize=None)
def valid_streams():
    """[(name, stream, data)]: the whole set of snappy_util.streams() by pyarrow's writer and by the library's own, and the
    hand-built element forms."""
    import pyarrow as pa
    from mspa import _lib
    lib = _lib.load()
    codec = pa.Codec("snappy")
    out = []
    for name, data in SU.streams():
        out.append((f"pa_{name}", codec.compress(data).to_pybytes() if data else b"\x00", data))
        out.append((f"own_{name}", SU.compress_host(lib, data), data))
    rng = np.random.default_rng(77)
    noise = rng.integers(0, 256, size=70000, dtype=np.uint8).tobytes()

    def hand(name, body, data):
        out.append((f"hand_{name}", SU.encode_varint(len(data)) + body, data))

    hand("empty", b"", b"")
    hand("copy4", lit(b"abcdefgh") + copy4(8, 6) + copy4(3, 64), b"abcdefgh" + b"abcdef" + (b"def" * 22)[:64])
    hand("offset1_len64", lit(b"x") + copy2(1, 64), b"x" * 65)
    hand("offset2_len7", lit(b"xy") + copy1(2, 7), b"xy" + b"xyxyxyx")
    hand("offset63_len64", lit(noise[:63]) + copy2(63, 64), noise[:63] + noise[:63] + noise[:1])
    for extra, n in ((1, 100), (2, 1000), (3, 70000), (4, 300), (1, 61), (1, 64), (2, 65), (1, 60), (4, 1)):
        hand(f"lit{extra}_{n}", lit(noise[:n], extra) + copy2(1, 3), noise[:n] + noise[n - 1:n] * 3)
    # elements behind a literal that outruns the input window, and copies around the 32 KiB ring and the 64 KiB mark
    body, data = bytearray(), bytearray()
    for n, back in ((40000, 32768), (300, 32769), (28000, 65535), (900, 32767), (5, 68000)):
        body += lit(noise[:n]) + copy4(back, 37)
        data += noise[:n]
        data += bytes(data[len(data) - back:len(data) - back + 37])
    hand("ring_edges", bytes(body), bytes(data))
    out.append((FAR_NAME, SU.encode_varint(70040) + lit(noise) + copy4(69000, 40), noise + noise[1000:1040]))
    for name, stream, data in out:
        assert py_decode(stream, len(data)) == data, name
    return out


SHORT = SU.encode_varint(40) + lit(b"hello") + copy1(5, 9) + lit(b"0123456789ab", 1) + copy2(12, 10) + copy4(26, 4)


@functools.lru_cache(maxsize=None)
def corrupt_streams():
    """[(name, stream, expected size, code)]."""
    assert py_decode(SHORT, 40) == b"hello" + b"hellohell" + b"0123456789ab" + b"0123456789" + b"hell"
    out = [(f"cut{k}", SHORT[:k], 40, py_decode(SHORT[:k], 40)) for k in range(len(SHORT))]
    assert {c for _, _, _, c in out} == {E_PREAMBLE, E_TRUNCATED, E_SHORT}
    big = SU.encode_varint(300) + lit(bytes(range(200)) + bytes(100), 2)
    out += [
        ("preamble_small", SHORT, 39, E_PREAMBLE),
        ("preamble_large", SHORT, 41, E_PREAMBLE),
        ("preamble_endless", b"\xff\xff\xff\xff\xff\x01" + SHORT[1:], 40, E_PREAMBLE),
        ("offset0_copy1", SU.encode_varint(9) + lit(b"hello") + copy1(0, 4), 9, E_OFFSET),
        ("offset0_copy4", SU.encode_varint(9) + lit(b"hello") + copy4(0, 4), 9, E_OFFSET),
        ("offset_beyond_start", SU.encode_varint(9) + lit(b"hello") + copy2(6, 4), 9, E_OFFSET),
        ("copy_first", SU.encode_varint(4) + copy2(1, 4), 4, E_OFFSET),
        ("offset_huge", SU.encode_varint(9) + lit(b"hello") + copy4(0xFFFFFFFF, 4), 9, E_OFFSET),
        ("overrun_copy", SU.encode_varint(8) + lit(b"hello") + copy2(5, 4), 8, E_OVERRUN),
        ("overrun_literal", SU.encode_varint(4) + lit(b"hello"), 4, E_OVERRUN),
        ("overrun_long_literal", SU.encode_varint(299) + big[2:], 299, E_OVERRUN),
        ("trailing_element", SU.encode_varint(5) + lit(b"hello") + lit(b"x"), 5, E_TRAILING),
        ("trailing_byte", SHORT + b"\x00", 40, E_TRAILING),
        ("trailing_after_empty", b"\x00\x00", 0, E_TRAILING),
        ("literal_4_length_bytes_past_input", SU.encode_varint(5) + bytes([63 << 2, 0xFF, 0xFF, 0xFF, 0xFF]) + b"abc", 5, E_TRUNCATED),
        ("long_literal_cut", big[:-1], 300, E_TRUNCATED),
        ("no_input", b"", 0, E_PREAMBLE),
    ]
    for name, stream, expected, code in out:
        assert code < 0 and py_decode(stream, expected) == code, (name, code, py_decode(stream, expected))
    return out


def decompress_host(lib, stream, expected, guard=64):
    """mspa_snappy_decompress_host between two guard bands: (return value, the bytes of dst)."""
    src = np.frombuffer(stream, dtype=np.uint8) if len(stream) else np.zeros(1, np.uint8)
    dst = np.full(expected + 2 * guard, 0xAB, dtype=np.uint8)
    rc = lib.mspa_snappy_decompress_host(src.ctypes.data if len(stream) else None, len(stream), dst.ctypes.data + guard, expected)
    assert (dst[:guard] == 0xAB).all() and (dst[guard + expected:] == 0xAB).all(), "a write outside dst"
    return int(rc), dst[guard:guard + expected].tobytes()


# ------------------------------------------------------------------------------------------------------------------- index files
def _write(table, path, **options):
    import pyarrow.parquet as pq
    pq.write_table(table, path, **options)
    return path


def two_scene_table():
    import pyarrow as pa
    return pa.concat_tables([SU.index_table("scene0000_00", seed=3), SU.index_table("scene0001_00", n_images=5, n_points=3000, seed=4)])


def index_files(directory):
    """{name: (path, [scene ids], device path expected)} -- the files of the page tests, written once per directory."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mspa import parquet_splice
    d = str(directory)
    one = SU.index_table()
    out = {}
    out["many_pages"] = (_write(one, f"{d}/many_pages.parquet", use_dictionary=False, data_page_size=4096), ["scene0000_00"], True)
    # pyarrow looks at a page's size once per write batch (1 024 values by default: all eight image rows share the first page
    # above); one value per batch gives every image row, 9 KB of text, a page of its own
    out["page_per_row"] = (_write(one, f"{d}/page_per_row.parquet", use_dictionary=False, data_page_size=4096, write_batch_size=1),
                           ["scene0000_00"], True)
    out["uncompressed"] = (_write(one, f"{d}/uncompressed.parquet", use_dictionary=False, compression="none"), ["scene0000_00"], True)
    out["defaults"] = (_write(one, f"{d}/defaults.parquet"), ["scene0000_00"], False)
    out["v2"] = (_write(one, f"{d}/v2.parquet", use_dictionary=False, data_page_version="2.0"), ["scene0000_00"], False)
    out["two_scenes"] = (_write(two_scene_table(), f"{d}/two_scenes.parquet", use_dictionary=False, data_page_size=4096),
                         ["scene0000_00", "scene0001_00"], True)
    out["two_groups"] = (_write(one, f"{d}/two_groups.parquet", use_dictionary=False, data_page_size=4096, row_group_size=2504),
                         ["scene0000_00"], True)
    with pq.ParquetWriter(f"{d}/split_images.parquet", one.schema, use_dictionary=False, data_page_size=4096) as w:
        w.write_table(one.slice(0, 5))                        # the image rows themselves lie in two row groups
        w.write_table(one.slice(5))
    out["split_images"] = (f"{d}/split_images.parquet", ["scene0000_00"], True)
    # K12's layout: the values chunk by the library's host reference, spliced behind pyarrow's key column
    from mspa import _lib
    offs, data = SU.string_buffers(one.column("values"))
    pages = SU.host_pages(_lib.load(), offs, data, 8192)
    buf = parquet_splice.assemble_row_group(one.select(["key"]), "values", pages["chunk"], pages["compressed"], pages["uncompressed"],
                                            pages["num_values"], use_dictionary=False)
    path = f"{d}/assembled.parquet"
    with open(path, "wb") as f:
        f.write(parquet_splice.splice([buf]))
    assert pq.read_table(path).equals(one)
    out["assembled"] = (path, ["scene0000_00"], True)
    return out


def image_ids_of(path, scene_id):
    """The scene's image ids in file order, and {image id: JSON text}."""
    import pyarrow.parquet as pq
    t = pq.read_table(path)
    prefix = f"{scene_id}:image_to_points:"
    texts = {k[len(prefix):]: v for k, v in zip(t.column("key").to_pylist(), t.column("values").to_pylist()) if k.startswith(prefix)}
    return list(texts), texts


def expected_bits(texts, image_ids, n_points):
    from mspa.scene import pack_index_lists
    return pack_index_lists([json.loads(texts[i]) for i in image_ids], n_points)


def python_page_walk(path, group):
    """A pure-Python walk of row group ``group``'s values chunk: [(page type, encoding, [(row in the group, value bytes)],
    (compressed size, uncompressed size))] with the rows of every DATA_PAGE (v1, PLAIN) decoded; other pages come with an empty
    row list.  pyarrow's codec decompresses."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mspa import parquet_splice as PS
    md = pq.ParquetFile(path).metadata
    col = md.row_group(group).column(md.schema.names.index("values") if hasattr(md.schema, "names") else 1)
    start = col.dictionary_page_offset if col.has_dictionary_page else col.data_page_offset
    with open(path, "rb") as f:
        f.seek(start)
        chunk = f.read(col.total_compressed_size)
    optional = md.schema.column(1).max_definition_level > 0
    out, p, row = [], 0, 0
    while p < len(chunk):
        r = PS._Reader(chunk, p)
        h = r.struct()
        p = r.p
        ptype, unc, comp = PS._get(h, 1), PS._get(h, 2), PS._get(h, 3)
        body = chunk[p:p + comp]
        p += comp
        dph = PS._get(h, 5)
        if ptype != 0 or PS._get(dph, 2) != 0:
            nv = PS._get(dph, 1) if dph else (PS._get(PS._get(h, 8), 1) if ptype == 3 else 0)
            out.append((ptype, None if dph is None else PS._get(dph, 2), [], (comp, unc)))
            row += nv if ptype in (0, 3) else 0
            continue
        if col.compression == "SNAPPY":
            body = pa.Codec("snappy").decompress(body, decompressed_size=unc).to_pybytes()
        q = 0
        if optional:
            (L,) = struct.unpack_from("<I", body, 0)
            q = 4 + L
        rows = []
        for _ in range(PS._get(dph, 1)):
            (n,) = struct.unpack_from("<I", body, q)
            rows.append((row, body[q + 4:q + 4 + n]))
            q += 4 + n
            row += 1
        assert q == len(body)
        out.append((ptype, 0, rows, (comp, unc)))
    return out
