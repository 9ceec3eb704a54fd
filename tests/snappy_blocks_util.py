"""What the tests of the Snappy decoder's block route share (tests/test_snappy_blocks_cpu.py, tests/test_gpu_snappy_blocks.py):
a pure-Python walk that says where a stream's 64 KiB blocks begin in its compressed bytes (or why it has none), both writers'
streams, hand-built streams that are and are not blockwise, the shapes at which a scan by segments of SEG compressed bytes can go
wrong, and the corrupt set."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snappy_util as SU  # noqa: E402
import visindex_decode_util as VU  # noqa: E402
from visindex_decode_util import copy1, copy2, copy4, lit  # noqa: E402

BLOCK = SU.BLOCK
SEG = 2048                       # csrc/snappy_decode.hip: kSeg
NOT_BLOCKWISE = -22


def block_count(n):
    return (n + BLOCK - 1) // BLOCK


def py_block_starts(stream, expected):
    """csrc/snappy_core.h's block_starts restated: (block count, [starts ..., len(stream)]), or (code, None) -- the decoder's code
    (VU.py_decode's) for a stream it declines, NOT_BLOCKWISE for a valid one with an element that straddles a multiple of 64 KiB
    or a copy that reaches in front of its block."""
    code = VU.py_decode(stream, expected)
    if isinstance(code, int):
        return code, None
    _, p = SU.varint(stream)
    o, starts, blockwise = 0, [], True
    while p < len(stream):
        tag = stream[p]
        kind, m = tag & 3, tag >> 2
        extra = (0 if m < 60 else m - 59) if kind == 0 else (1, 2, 4)[kind - 1]
        field = int.from_bytes(stream[p + 1:p + 1 + extra], "little")
        if o % BLOCK == 0:
            starts.append(p)
        if kind == 0:
            n = (field if extra else m) + 1
            adv = 1 + extra + n
        else:
            n, offset = (4 + (m & 7), (tag >> 5) << 8 | field) if kind == 1 else (m + 1, field)
            adv = 1 + extra
            if offset > o % BLOCK:
                blockwise = False
        if o % BLOCK + n > BLOCK:
            blockwise = False
        p += adv
        o += n
    if not blockwise:
        return NOT_BLOCKWISE, None
    assert len(starts) == block_count(expected)
    return len(starts), starts + [len(stream)]


def _noise(n, seed=77):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _stream(elements, data):
    return SU.encode_varint(len(data)) + b"".join(elements), data


def _finish_block(els, data, noise, tail=b"tail!"):
    """Fill the running block with one noise literal (a literal far longer than 3 SEG: whole segments are jumped) and put a
    short second block behind it."""
    rest = BLOCK - len(data) % BLOCK
    els.append(lit(noise[:rest]))
    data += noise[:rest]
    els.append(lit(tail))
    data += tail
    return els, data


@functools.lru_cache(maxsize=None)
def list_text():
    """PLAIN-encoded JSON list text of a little more than five blocks."""
    text = SU.json_lists(seed=9, rows=520)
    assert len(text) >= 5 * BLOCK + 1234
    return text[:5 * BLOCK + 1234]


@functools.lru_cache(maxsize=None)
def writer_streams():
    """[(name, stream, data)]: the shared set and the list text by pyarrow's writer and by the library's own.  All blockwise."""
    import pyarrow as pa
    from mspa import _lib
    lib = _lib.load()
    codec = pa.Codec("snappy")
    out = [(n, s, d) for n, s, d in VU.valid_streams() if not n.startswith("hand_") and n != VU.FAR_NAME]
    mix = _noise(3 * BLOCK, 5)[:BLOCK + 100] + bytes(BLOCK) + list_text()[:BLOCK - 100]          # 3 x 65 536: noise, zeros, text
    for name, data in (("lists5", list_text()), ("mix3", mix)):
        assert name != "mix3" or len(data) == 3 * BLOCK
        out.append((f"pa_{name}", codec.compress(data).to_pybytes(), data))
        out.append((f"own_{name}", SU.compress_host(lib, data), data))
    return out


@functools.lru_cache(maxsize=None)
def hand_streams():
    """[(name, stream, data, blockwise)]: hand-built valid streams."""
    noise = _noise(2 * BLOCK)
    out = []

    def add(name, els, data, blockwise):
        s, d = _stream(els, bytes(data))
        out.append((name, s, d, blockwise))

    # not blockwise: the decoder takes them, the block route must not
    add("nb_literal_70000", [lit(noise[:70000])], noise[:70000], False)
    d = bytearray(noise[:BLOCK] + b"abcd")
    d += bytes(d[len(d) - 10:len(d) - 2])
    add("nb_copy_into_block0", [lit(noise[:BLOCK]), lit(b"abcd"), copy2(10, 8)], d, False)
    d = bytearray(noise[:BLOCK - 6])
    d += bytes(d[len(d) - 100:len(d) - 80])
    add("nb_copy2_crosses", [lit(noise[:BLOCK - 6]), copy2(100, 20)], d, False)
    # blockwise: copy-4 elements inside a block, literals with 1 to 4 length bytes
    els, d = [], bytearray()
    for extra, a, b in ((1, 0, 100), (2, 100, 1100), (4, 1100, 1400), (3, 1400, 65000)):
        els.append(lit(noise[a:b], extra))
        d += noise[a:b]
    for n in [64] * 8 + [24]:
        els.append(copy4(60000, n))
        d += bytes(d[len(d) - 60000:len(d) - 60000 + n])
    assert len(d) == BLOCK
    els += [lit(b"xyz", 4), copy4(3, 50), lit(noise[:300], 2), copy4(353, 64), copy1(7, 11)]
    d += b"xyz"
    for off, n in ((3, 50),):
        for _ in range(n):
            d.append(d[-off])
    d += noise[:300]
    d += bytes(d[len(d) - 353:len(d) - 353 + 64])
    for _ in range(11):
        d.append(d[-7])
    add("bw_copy4_literal_heads", els, d, True)
    for name, s, d, _ in out:
        assert VU.py_decode(s, len(d)) == d, name
    return out


@functools.lru_cache(maxsize=None)
def segment_streams():
    """[(name, stream, data)]: valid blockwise streams whose elements sit exactly where a scan by segments of SEG compressed
    bytes can go wrong.  (The expected sizes 0, 1, 65 535, 65 536, 65 537 are in the writers' set, 3 x 65 536 is its mix3.)"""
    noise = _noise(2 * BLOCK, 31)
    out = []
    # a compressed length below SEG, exactly SEG and SEG + 1: varint (2 bytes), a literal's 3 head bytes, its bytes
    for name, total in (("below", SEG - 48), ("exact", SEG), ("plus1", SEG + 1)):
        s, d = _stream([lit(noise[:total - 5])], noise[:total - 5])
        assert len(s) == total
        out.append((f"seg_len_{name}", s, d))
    # the element behind the first literal starts at SEG - back, so that the boundary falls inside its head of 2, 3 or 5 bytes
    # (back = 0: it starts exactly on the boundary; the literal in front of it has the boundary inside its bytes -- or, for
    # back = 0, ends on it).  Preamble 3 bytes (two blocks), literal head 3 bytes.
    for name, back, el, n in (("head2", 1, copy1(700, 9), 9), ("head3", 1, copy2(700, 30), 30), ("head3_late", 2, copy2(700, 30), 30),
                              ("head5", 3, copy4(700, 30), 30), ("head5_first", 1, copy4(700, 30), 30), ("on_boundary", 0, copy2(700, 30), 30),
                              ("lit2_head", 1, lit(noise[5000:5100], 1), 0), ("lit5_head", 2, lit(noise[5000:5100], 4), 0)):
        L = SEG - back - 6
        els, d = [lit(noise[:L])], bytearray(noise[:L])
        els.append(el)
        d += bytes(d[len(d) - 700:len(d) - 700 + n]) if n else noise[5000:5100]
        els, d = _finish_block(els, d, noise)
        s, d = _stream(els, bytes(d))
        assert s[SEG - back] == el[0] and len(d) == BLOCK + 5, name
        out.append((f"seg_{name}", s, d))
    # block 1's first element exactly on a segment boundary: 3 + 3 + 65 527 + 3 = 32 SEG compressed bytes make block 0
    d = bytearray(noise[:BLOCK - 9])
    d += bytes(d[len(d) - 100:len(d) - 91])
    els = [lit(noise[:BLOCK - 9]), copy2(100, 9), lit(noise[:3000]), copy2(3000, 64)]
    d += noise[:3000] + noise[:64]
    s, d = _stream(els, bytes(d))
    assert py_block_starts(s, len(d))[1][1] == 32 * SEG
    out.append(("seg_block_start_on_boundary", s, d))
    for name, s, d in out:
        assert VU.py_decode(s, len(d)) == d, name
        assert py_block_starts(s, len(d))[0] == block_count(len(d)), name
    return out


@functools.lru_cache(maxsize=None)
def corrupt_streams():
    """[(name, stream, expected size)]: the existing corrupt set, and a three-block stream cut at every byte of the 16 around its
    second block's start (the expected code is whatever the decoder says: tests compare against it)."""
    out = [(n, s, e) for n, s, e, _ in VU.corrupt_streams()]
    name, s, d = next(w for w in writer_streams() if w[0] == "pa_mix3")
    at = py_block_starts(s, len(d))[1][1]
    out += [(f"cut_block1_{k - at:+d}", s[:k], len(d)) for k in range(at - 8, at + 8)]
    return out


def block_starts_host(lib, stream, expected):
    """mspa_snappy_block_starts_host on an exactly sized table: (return value, starts list)."""
    src = np.frombuffer(stream, dtype=np.uint8) if len(stream) else np.zeros(1, np.uint8)
    cap = block_count(expected) + 1
    starts = np.full(cap, -7, dtype=np.int64)
    rc = int(lib.mspa_snappy_block_starts_host(src.ctypes.data if len(stream) else None, len(stream), expected, starts.ctypes.data, cap))
    return rc, starts.tolist()
