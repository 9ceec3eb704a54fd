"""The shape / content grid shared by the resize tests (CPU build of csrc/resize_core.h and the device kernels), and the
Pillow reference they compare with."""
import numpy as np

FILTERS = {"bilinear": 2, "bicubic": 3}          # Pillow's Image.Resampling numbers

# (h, w) -> (H, W): the pairs of the feature's description that lie inside the device range (factors within 1/8 .. 8)
NAMED_PAIRS = [((512, 512), (968, 1296)), ((360, 640), (968, 1296)), ((968, 1296), (484, 648)), ((800, 600), (100, 75)),
               ((64, 64), (8, 8)), ((64, 64), (512, 512)), ((17, 23), (136, 184)), ((17, 23), (3, 3)), ((2, 2), (9, 9)),
               ((37, 53), (101, 7)), ((1, 1), (5, 5)), ((480, 640), (480, 1296)), ((100, 100), (13, 100))]
# sizes 1 and 2 on either axis, as source and as target
TINY_PAIRS = [((1, 7), (4, 20)), ((7, 1), (20, 4)), ((2, 9), (9, 2)), ((9, 2), (2, 9)), ((8, 8), (1, 1)), ((5, 9), (2, 2)),
              ((16, 3), (2, 24)), ((3, 16), (24, 2)), ((1, 1), (1, 8)), ((1, 1), (8, 1)), ((2, 1), (1, 2)), ((1, 2), (2, 1)),
              ((2, 2), (1, 16)), ((16, 16), (2, 128)), ((1, 64), (1, 8)), ((64, 1), (8, 1)), ((2, 30), (2, 31)), ((30, 2), (31, 2))]
OUTSIDE = ((2000, 3), (5, 900))                  # a 400-fold reduction with a 300-fold enlargement: declined by the kernels


def factor_range(n):
    """Every size from 1/8 to 8 x of n."""
    return range(-(-n // 8), 8 * n + 1)


def grid_pairs():
    """[((h, w), (H, W))]: the named and tiny pairs, then every output size from 1/8 to 8 x of a 17 x 23 and of a 64 x 40 image
    (width x height) per axis, and mixed -- while one axis walks its range the other takes a size from the opposite side of 1
    (a reduction on one axis with an enlargement on the other) that changes from step to step."""
    pairs = list(NAMED_PAIRS) + list(TINY_PAIRS)
    for h, w in ((23, 17), (40, 64)):
        hs, ws = list(factor_range(h)), list(factor_range(w))
        for k, H in enumerate(hs):
            pairs.append(((h, w), (H, w)))
            up = [x for x in ws if x > w]
            down = [x for x in ws if x < w]
            other = down if H > h else up                 # H == h: an enlargement beside an unchanged axis
            pairs.append(((h, w), (H, other[(k * 7) % len(other)])))
        for k, W in enumerate(ws):
            pairs.append(((h, w), (h, W)))
            up = [y for y in hs if y > h]
            down = [y for y in hs if y < h]
            other = down if W > w else up
            pairs.append(((h, w), (other[(k * 5) % len(other)], W)))
    return pairs


def patterns(h, w, seed):
    """[4, h, w, 3] uint8: noise, flat 0, flat 255 and a one-pixel checkerboard (bicubic over- and undershoot must clamp)."""
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    checker = np.where(((x + y) % 2)[..., None] == 0, 255, 0).repeat(3, axis=2).astype(np.uint8)
    return np.stack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.zeros((h, w, 3), np.uint8),
                     np.full((h, w, 3), 255, np.uint8), checker])


def pillow_resize(img, hw, filt):
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((int(hw[1]), int(hw[0])), int(filt)))
