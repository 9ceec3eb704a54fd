"""What the Snappy tests share (tests/test_snappy_cpu.py, tests/test_parquet_assemble_cpu.py, tests/test_gpu_parquet_pages.py):
the stream set, a pure-Python reader of Snappy elements, and the library's host reference behind ctypes."""
import json

import numpy as np

BLOCK = 65536
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 65535, 65536, 65537, 131079)
COPY_LENGTHS = (4, 11, 12, 64, 65, 67, 68, 128)
# the pieces a copy of that length must be written in (form 1: 2 bytes, form 2: 3 bytes), at an offset below 2048
COPY_PIECES = {4: [(1, 4)], 11: [(1, 11)], 12: [(2, 12)], 64: [(2, 64)], 65: [(2, 60), (2, 5)], 67: [(2, 60), (2, 7)],
               68: [(2, 64), (2, 4)], 128: [(2, 64), (2, 64)]}


def _digits(period, n):
    unit = ("1234567890"[:period - 2] + ", ").encode()
    return (unit * (n // period + 1))[:n]


def json_lists(seed=5, rows=40):
    """Real ``json.dumps`` text of the index's two kinds of list, PLAIN-encoded as a page would hold them."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    for r in range(rows):
        if r % 2:
            text = json.dumps(sorted(rng.choice(200000, size=int(rng.integers(0, 400)), replace=False).tolist()))
        else:
            text = json.dumps([f"{k:05d}" for k in sorted(rng.choice(320, size=int(rng.integers(0, 40)), replace=False).tolist())])
        out += len(text).to_bytes(4, "little") + text.encode()
    return bytes(out)


def hashes(data, bits=12):
    """H(p) of csrc/snappy_core.h for every p with p + 3 < len(data)."""
    b = np.frombuffer(data, dtype=np.uint8).astype(np.uint64)
    v = b[:-3] | b[1:-2] << np.uint64(8) | b[2:-1] << np.uint64(16) | b[3:] << np.uint64(24)
    return ((v * np.uint64(0x1e35a7bd)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)


def copy_case(length, rng):
    """300 noise bytes, then `length` of them again from position 100 on, then a byte that ends the match, then noise.  The
    noise is drawn again until position 100 is the only one of its hash, so that the candidate of position 300 is position 100
    whatever kHashBits is (12 to 14)."""
    while True:
        head = rng.integers(0, 256, size=300, dtype=np.uint8).tobytes()
        if all(int((hashes(head, bits) == hashes(head, bits)[100]).sum()) == 1 for bits in (12, 13, 14)):
            break
    stop = bytes([head[100 + length] ^ 0xFF])
    return head + head[100:100 + length] + stop + rng.integers(0, 256, size=40, dtype=np.uint8).tobytes()


def far_case(rng):
    """A 40-byte phrase that comes back 3 000 bytes later (drawn again until nothing in between shares its first hash)."""
    while True:
        phrase = rng.integers(0, 256, size=40, dtype=np.uint8).tobytes()
        body = phrase + rng.integers(0, 256, size=2960, dtype=np.uint8).tobytes()
        if all(int((hashes(body + phrase[:3], bits) == hashes(phrase, bits)[0]).sum()) == 1 for bits in (12, 13, 14)):
            return body + phrase + bytes([phrase[0] ^ 0xFF, 1, 2])


def streams():
    """[(name, bytes)]: every length of LENGTHS for zeros, period-7 and period-9 digit text and noise; zeros around the
    60-byte tail rule; the copy lengths; a far match; JSON lists; two identical noise halves around a block boundary."""
    rng = np.random.default_rng(12)
    while True:                                                        # noise whose first block repeats no 4 bytes: one literal
        noise = rng.integers(0, 256, size=max(LENGTHS), dtype=np.uint8).tobytes()
        if len(np.unique(hashes(noise[:BLOCK], 32))) == BLOCK - 3:
            break
    out = []
    for n in LENGTHS:
        out += [(f"zeros{n}", bytes(n)), (f"p7_{n}", _digits(7, n)), (f"p9_{n}", _digits(9, n)), (f"noise{n}", noise[:n])]
    out += [(f"zeros{n}", bytes(n)) for n in range(66, 70)]            # one copy of 65 .. 68 bytes at offset 1
    out += [(f"copy{k}", copy_case(k, rng)) for k in COPY_LENGTHS]
    out.append(("far", far_case(rng)))
    out.append(("json", json_lists()))
    out.append(("halves", noise[:BLOCK] * 2))
    return out


def varint(buf, pos=0):
    out = shift = 0
    while True:
        c = buf[pos]
        pos += 1
        out |= (c & 0x7F) << shift
        if not c & 0x80:
            return out, pos
        shift += 7


def elements(buf):
    """The elements of a run of Snappy elements (no preamble): [("lit", len, data)] / [("copy", form, offset, len)]."""
    out, p = [], 0
    while p < len(buf):
        tag = buf[p]
        kind = tag & 3
        if kind == 0:
            n = tag >> 2
            p += 1
            if n >= 60:
                extra = n - 59
                n = int.from_bytes(buf[p:p + extra], "little")
                p += extra
            n += 1
            assert p + n <= len(buf), "literal runs past the end"
            out.append(("lit", n, bytes(buf[p:p + n])))
            p += n
        elif kind == 1:
            out.append(("copy", 1, (tag >> 5) << 8 | buf[p + 1], 4 + ((tag >> 2) & 7)))
            p += 2
        elif kind == 2:
            out.append(("copy", 2, buf[p + 1] | buf[p + 2] << 8, (tag >> 2) + 1))
            p += 3
        else:
            raise AssertionError("a 5-byte copy: this encoder writes none")
    return out


def decode_elements(els):
    """The bytes a list of elements stands for; a copy that reaches before the first byte is an error."""
    out = bytearray()
    for e in els:
        if e[0] == "lit":
            out += e[2]
        else:
            _, _form, off, n = e
            assert 1 <= off <= len(out), f"copy offset {off} reaches before the start ({len(out)} bytes so far)"
            for _ in range(n):
                out.append(out[-off])
    return bytes(out)


def split_blocks(stream):
    """(n, [elements of block 0, of block 1, ...]) of a stream: no element may straddle a 64 KiB boundary."""
    n, p = varint(stream)
    blocks, cur, done = [], [], 0
    for e in elements(stream[p:]):
        cur.append(e)
        done += e[1] if e[0] == "lit" else e[3]
        assert done <= BLOCK, "an element straddles a block boundary"
        if done == BLOCK:
            blocks.append(cur)
            cur, done = [], 0
    if cur:
        blocks.append(cur)
    return n, blocks


def check_stream(name, data, stream, capacity):
    """Every property a stream of this encoder has, with pyarrow's decoder as the independent oracle."""
    import pyarrow as pa
    n, p = varint(stream)
    assert n == len(data) and stream[:p] == encode_varint(n), name
    assert len(stream) <= capacity, name
    if len(data):
        assert pa.Codec("snappy").decompress(stream, decompressed_size=len(data)).to_pybytes() == data, name
    else:
        assert stream == b"\x00", name
    _, blocks = split_blocks(stream)
    assert len(blocks) == (len(data) + BLOCK - 1) // BLOCK, name
    for k, els in enumerate(blocks):                                       # each block's elements decode alone
        assert decode_elements(els) == data[k * BLOCK:(k + 1) * BLOCK], (name, k)
        for e in els:
            assert e[1] <= BLOCK if e[0] == "lit" else (4 <= e[3] <= 64 and (e[1] == 2 or (e[3] <= 11 and e[2] < 2048))), (name, e[:2])
    return blocks


def encode_varint(v):
    out = bytearray()
    while True:
        c = v & 0x7F
        v >>= 7
        out.append(c | 0x80 if v else c)
        if not v:
            return bytes(out)


def compress_host(lib, data):
    """mspa_snappy_compress_host on ``data``."""
    cap = lib.mspa_snappy_capacity(len(data))
    src = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    dst = np.empty(cap, dtype=np.uint8)
    m = lib.mspa_snappy_compress_host(src.ctypes.data if len(data) else None, len(data), dst.ctypes.data, cap)
    assert m > 0, m
    return dst[:m].tobytes()


def page_cuts_host(lib, offsets, page_bytes):
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    rows = len(offsets) - 1
    cuts = np.empty(rows + 1, dtype=np.int64)
    pages = lib.mspa_parquet_page_cuts_host(offsets.ctypes.data, rows, page_bytes, cuts.ctypes.data, rows + 1)
    assert pages >= 0, pages
    return cuts[:pages + 1].copy() if pages else np.zeros(1, np.int64)


def page_payload_host(lib, offsets, data, v0, v1):
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = lib.mspa_parquet_page_payload_bytes_host(offsets.ctypes.data, int(v0), int(v1))
    assert n > 0
    dst = np.empty(n, dtype=np.uint8)
    rc = lib.mspa_parquet_page_payload_host(offsets.ctypes.data, data.ctypes.data if data.size else None, int(v0), int(v1),
                                            dst.ctypes.data, n)
    assert rc == 0, rc
    return dst.tobytes()



def host_pages(lib, offsets, data, page_bytes):
    """The values chunk by the host reference: {"payload", "chunk" (bytes), "compressed", "uncompressed", "num_values" (lists)}."""
    cuts = page_cuts_host(lib, offsets, page_bytes)
    payloads = [page_payload_host(lib, offsets, data, cuts[k], cuts[k + 1]) for k in range(len(cuts) - 1)]
    streams_ = [compress_host(lib, p) for p in payloads]
    return {"payload": b"".join(payloads), "chunk": b"".join(streams_), "compressed": [len(s) for s in streams_],
            "uncompressed": [len(p) for p in payloads], "num_values": np.diff(cuts).tolist()}


def index_table(scene_id="scene0000_00", n_images=8, n_points=5000, seed=3):
    """A (key, values) table shaped like one scene's visibility index: image rows first, JSON text as values."""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    ids = [f"{k * 10:05d}" for k in range(n_images)]
    seen = rng.random((n_images, n_points)) < 0.3
    keys = [f"{scene_id}:image_to_points:{i}" for i in ids] + [f"{scene_id}:point_to_images:{v}" for v in range(n_points)]
    values = [json.dumps(np.nonzero(seen[k])[0].tolist()) for k in range(n_images)]
    values += [json.dumps([ids[k] for k in np.nonzero(seen[:, v])[0]]) for v in range(n_points)]
    return pa.table({"key": pa.array(keys, type=pa.string()), "values": pa.array(values, type=pa.string())})


def string_buffers(column):
    """(int32 offsets [rows + 1] starting at 0, uint8 data) of a pyarrow string column."""
    arr = column.combine_chunks() if hasattr(column, "combine_chunks") else column
    bufs = arr.buffers()
    offs = np.frombuffer(bufs[1], dtype=np.int32)[arr.offset:arr.offset + len(arr) + 1]
    data = np.frombuffer(bufs[2], dtype=np.uint8)[offs[0]:offs[-1]] if bufs[2] is not None else np.zeros(0, np.uint8)
    return (offs - offs[0]).astype(np.int32), data.copy()
