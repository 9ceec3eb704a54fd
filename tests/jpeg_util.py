"""Seeded procedural colour frames and Pillow JPEG helpers shared by the JPEG decode tests."""
import io

import numpy as np


def content(h, w, seed, kind="mixed"):
    """[h, w, 3] uint8: gradients, edges, texture, noise and a flat patch (long EOB runs); ``kind="saturated"``: a one-pixel
    checkerboard of full-scale primaries that drives the IDCT past the range limits."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "saturated":
        img = np.where(((x + y) % 2)[..., None] == 0, 255, 0) * np.array([1, 0, 1])[None, None]
        img = img.astype(np.uint8)
        img[::3, :, 1] = 255
        return img
    img = np.zeros((h, w, 3), np.float64)
    img[..., 0] = 255.0 * x / max(w - 1, 1)
    img[..., 1] = 255.0 * y / max(h - 1, 1)
    img[..., 2] = np.where((x // 7 + y // 5) % 2, 220, 30)
    img += (40.0 * np.sin(x * 0.37 + seed) * np.cos(y * 0.21))[..., None]
    img += rng.normal(0, 18, img.shape)
    img[h // 3: h // 2, w // 3: w // 2] = 128.0
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(img, **kw) -> bytes:
    from PIL import Image, ImageFile
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 1 << 24)      # optimize=True needs the whole stream in one buffer
    bio = io.BytesIO()
    Image.fromarray(img).save(bio, "JPEG", **kw)
    return bio.getvalue()


def pillow_rgb(data: bytes) -> np.ndarray:
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def sos_end(data: bytes) -> int:
    """Offset of the first entropy-coded byte (one past the SOS segment)."""
    i = 2
    while True:
        assert data[i] == 0xFF
        m = data[i + 1]
        n = (data[i + 2] << 8) | data[i + 3]
        if m == 0xDA:
            return i + 2 + n
        i += 2 + n


def marker_offset(data: bytes, code: int) -> int:
    """Offset of the first header marker 0xFF ``code`` before the scan."""
    i = 2
    while True:
        m = data[i + 1]
        if m == code:
            return i
        assert m != 0xDA, f"marker {code:#x} not in the header"
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
