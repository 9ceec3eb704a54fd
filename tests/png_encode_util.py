"""Shared pieces of the 16-bit PNG encoder tests: the content grid, a g++ build of csrc/png_encode_core.h, and a strict
reader of PNG files that checks every structural rule of the container and the zlib stream."""
import os
import struct
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-spatialmllm_amd", "csrc")

# Reads any number of (h, w) int32 pairs, each followed by h * w uint16 samples, from stdin; for each writes int64 file length,
# the file, then the h * (1 + 2 w) filtered bytes.
DRIVER = r"""
#include "png_encode_core.h"
#include <cstdio>
#include <vector>
using namespace mspa::pnge;
int main() {
    int32_t a[2];
    while (fread(a, 4, 2, stdin) == 2) {
        if (!valid_size(a[0], a[1])) return 3;
        const Geom g = geom(a[0], a[1]);
        std::vector<int16_t> img((size_t)a[0] * a[1]);
        if (fread(img.data(), 2, img.size(), stdin) != img.size()) return 4;
        std::vector<uint8_t> out((size_t)g.cap), filt((size_t)g.n);
        const int64_t n = encode_file_host(img.data(), a[0], a[1], out.data(), filt.data());
        if (n > g.cap) return 5;
        fwrite(&n, 8, 1, stdout);
        fwrite(out.data(), 1, (size_t)n, stdout);
        fwrite(filt.data(), 1, filt.size(), stdout);
    }
    return 0;
}
"""

SIZES = [(1, 1), (1, 37), (29, 1), (7, 13), (480, 640), (968, 1296), (1, 8192), (6, 8192), (3000, 5)]
KINDS = ["zeros", "constant", "ramp", "smooth", "planar", "noise", "runs", "repeat32k", "alternate"]


def content(kind: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    """[h, w] uint16 depth-like content of one kind of the test grid."""
    rng = np.random.default_rng(seed + 7919 * KINDS.index(kind))
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "zeros":
        d = np.zeros((h, w))
    elif kind == "constant":
        d = np.full((h, w), 1234.0)
    elif kind == "ramp":
        d = 500 + 3 * x + 2 * y
    elif kind == "smooth":      # a smooth surface with a few mm of sensor noise
        d = 1500 + 600 * np.sin(x / 90 + 0.3) * np.cos(y / 70) + 0.4 * x + rng.normal(0, 1.5, (h, w))
    elif kind == "planar":      # piecewise planes with 30 % holes in blobs
        d = np.where(x + 0.7 * y < 0.6 * (w + h), 900 + 2.5 * x + 1.5 * y, 3000 - 1.2 * x + 0.8 * y)
        holes = rng.random((max(1, h // 8 + 1), max(1, w // 8 + 1))) < 0.3
        d = np.where(np.kron(holes, np.ones((8, 8)))[:h, :w] > 0, 0, d)
    elif kind == "noise":
        d = rng.integers(0, 65536, (h, w))
    elif kind == "runs":        # constant runs of 200..2000 samples (> 258 bytes)
        flat = np.empty(h * w)
        i = 0
        while i < flat.size:
            r = int(rng.integers(200, 2000))
            flat[i:i + r] = rng.integers(0, 65536)
            i += r
        d = flat.reshape(h, w)
    elif kind == "repeat32k":   # a random block every 32 KiB of sample bytes: in the filtered stream just past the window
        flat = np.resize(rng.integers(0, 65536, 16384), h * w)
        d = flat.reshape(h, w)
    elif kind == "alternate":   # rows alternate between two random walks: repeats two rows back (beyond the window at w = 8192)
        walks = np.cumsum(rng.integers(-3, 4, (2, w)), axis=1) + 30000
        d = walks[np.arange(h) % 2]
    else:
        raise ValueError(kind)
    return np.clip(np.rint(d), 0, 65535).astype(np.uint16)


def build_driver(tmpdir: str) -> str:
    src = os.path.join(tmpdir, "png_driver.cpp")
    exe = os.path.join(tmpdir, "png_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, src, "-o", exe])
    return exe


def encode_core(exe: str, images):
    """[(file bytes, filtered stream bytes)] of the host reference for a list of [h, w] uint16 arrays."""
    inp = b"".join(struct.pack("<ii", *im.shape) + np.ascontiguousarray(im, dtype="<u2").tobytes() for im in images)
    out = subprocess.run([exe], input=inp, stdout=subprocess.PIPE, check=True).stdout
    res, pos = [], 0
    for im in images:
        n = struct.unpack_from("<q", out, pos)[0]
        pos += 8
        f = out[pos:pos + n]
        pos += n
        m = im.shape[0] * (1 + 2 * im.shape[1])
        res.append((f, out[pos:pos + m]))
        pos += m
    return res


def chunks(data: bytes):
    """[(type, payload)] of a PNG file, checking the signature, every CRC and that nothing follows IEND."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while True:
        n, = struct.unpack_from(">I", data, pos)
        typ = data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack_from(">I", data, pos + 8 + n)
        assert crc == zlib.crc32(typ + body), f"bad CRC in {typ!r}"
        out.append((typ, body))
        pos += 12 + n
        if typ == b"IEND":
            assert pos == len(data), "bytes after IEND"
            return out


def strict_idat(data: bytes, h: int, w: int) -> bytes:
    """The inflated IDAT of a strictly valid 16-bit greyscale file of h x w (IHDR, zlib header, window, Adler-32)."""
    cs = chunks(data)
    assert [t for t, _ in cs][0] == b"IHDR" and [t for t, _ in cs][-1] == b"IEND"
    assert set(t for t, _ in cs[1:-1]) == {b"IDAT"}, "only IDAT chunks between IHDR and IEND"
    assert cs[0][1] == struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0)
    z = b"".join(b for t, b in cs if t == b"IDAT")
    assert z[0] == 0x78 and (z[0] << 8 | z[1]) % 31 == 0 and not (z[1] & 0x20), "zlib header"
    d = zlib.decompressobj(15)            # a 32 KiB window: a longer back-reference fails here
    raw = d.decompress(z) + d.flush()
    assert d.eof and d.unused_data == b"", "zlib stream must end exactly at the end of the IDAT data"
    assert struct.unpack(">I", z[-4:])[0] == zlib.adler32(raw)
    return raw


def pillow_png(img: np.ndarray) -> bytes:
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")
    return buf.getvalue()
