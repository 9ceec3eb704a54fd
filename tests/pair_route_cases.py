"""What tests/test_pair_route_cpu.py (no GPU) and tests/test_gpu_route_walk.py share: K3's output-set bits, flags and kernel
families as include/mspa.h and csrc/pair_route.h spell them, an independent restatement of the launch rules, and the walk --
one launch per compiled instantiation, on the smallest shape at which it exists.

``parent_route`` restates the rules from the launch code as it stood before csrc/pair_route.h existed (the `if` ladder of
pair_reproject_impl and mspa_pair_correspondences_workspace_bytes), branch by branch in that code's order, not from the header.
"""
from collections import namedtuple

O_VIS_BITS, O_VIS_U8, O_VALID_U8, O_PIX, O_XYZ32, O_RGBA, O_XYZ64, O_UV64, O_DEPTH64, O_COUNTS, O_CPIX = (1 << i for i in range(11))
OUTPUT_BITS = {"vis_bits": O_VIS_BITS, "vis_u8": O_VIS_U8, "valid_u8": O_VALID_U8, "pix_i16": O_PIX, "xyz_f32": O_XYZ32,
               "rgba": O_RGBA, "xyz_f64": O_XYZ64, "uv_f64": O_UV64, "depth_f64": O_DEPTH64, "counts": O_COUNTS, "cpix": O_CPIX}
CORR = O_VIS_BITS | O_PIX | O_COUNTS
DENSE = O_VIS_U8 | O_PIX | O_XYZ32 | O_RGBA | O_COUNTS
DENSE_XYZ = O_VIS_U8 | O_PIX | O_XYZ32 | O_COUNTS
MINIMAL = O_VIS_BITS | O_COUNTS
COMPACT = O_VIS_BITS | O_CPIX | O_COUNTS
NAMED = {"corr": CORR, "dense": DENSE, "dense_xyz": DENSE_XYZ, "minimal": MINIMAL, "compact": COMPACT}
FAST, STREAM, WORD_STRIPES = 1, 2, 0x200
EXACT_FAMILY, FAST_FAMILY, LINEAR_FAMILY, TIGHT_FAMILY, RECT_FAMILY = 1, 2, 3, 4, 6      # MSPA_KERNEL_PAIR_*; 5 is retired
K_EXACT, K_FAST, K_TIGHT = 0, 1, 2                                                        # which kernel template a key instantiates
ERR_SIZE, ERR_TOO_LARGE, ERR_FLAG, ERR_NEEDS_TIGHT = 1, 2, 3, 4

Key = namedtuple("Key", "kernel set ident whole_tiles linear scaled stream")
Route = namedtuple("Route", "err family key rows waves threads n_stripes n_tiles groups")


def bits(names):
    m = 0
    for n in names:
        m |= OUTPUT_BITS[n]
    return m


def _tight_shape(dh, dw, H, W, rows=48):
    return dh == H and dw == W and W % 64 == 0 and H % rows == 0 and H * W * 4 < 2 ** 31


def _rect_shape(dh, dw, H, W):
    return (not _tight_shape(dh, dw, H, W) and dw <= W and dh <= H and W % 16 == 0 and H % 4 == 0 and dw % 4 == 0 and dh % 2 == 0
            and H * W * 4 < 2 ** 31 and dh * dw * 2 < 2 ** 31)


def _ceil(a, b):
    return -(-a // b)


def parent_route(dh, dw, H, W, outputs, aligned, flags):
    """The route of one mspa_pair_reproject / fused mspa_pair_correspondences call, restated from the earlier launch code."""
    def error(e):
        return Route(e, 0, None, 0, 0, 0, 0, 0, 0)
    if min(dh, dw, H, W) < 2 or max(dh, dw, H, W) > 32767:
        return error(ERR_SIZE)
    P = H * W
    if P * W >= 2 ** 32:
        return error(ERR_TOO_LARGE)
    if flags & ~(FAST | STREAM | WORD_STRIPES):
        return error(ERR_FLAG)
    ident = dh == H and dw == W
    fast = bool(flags & FAST) and not outputs & (O_XYZ64 | O_UV64 | O_DEPTH64) and dw <= W and dh <= H
    linear = fast and bool(outputs & O_VIS_BITS) and W % 64 != 0
    s = outputs & ~(O_XYZ64 | O_UV64 | O_DEPTH64)
    dense_like = bool(s & (O_XYZ32 | O_RGBA | O_VIS_U8))
    tight24 = fast and aligned and _tight_shape(dh, dw, H, W, 32 if dense_like else 48) and s in NAMED.values()
    rect = fast and not tight24 and aligned and _rect_shape(dh, dw, H, W) and s in (COMPACT, CORR, MINIMAL)
    if outputs & O_CPIX and not (tight24 or rect):
        return error(ERR_NEEDS_TIGHT)
    stream = bool(flags & STREAM)
    if not fast:
        return Route(0, EXACT_FAMILY, Key(K_EXACT, 0, ident, False, False, False, False), 0, 4, 256, 0, 0, _ceil(P, 4096))
    n_stripes = _ceil(W, 64)
    if rect:                              # MSPA_LAUNCH_RECT
        rows = 48 if s in (CORR, COMPACT) else 64
        tiles = n_stripes * _ceil(H, rows)
        return Route(0, RECT_FAMILY, Key(K_TIGHT, s, False, False, False, True, stream), rows, 4, 256, n_stripes, tiles, _ceil(tiles, 4))
    if tight24:                           # MSPA_LAUNCH_TIGHT
        rows = 32 if dense_like else 48
        waves = {CORR: 4, DENSE: 4, DENSE_XYZ: 8, MINIMAL: 2, COMPACT: 2}[s]
        tiles = n_stripes * (H // rows)
        return Route(0, TIGHT_FAMILY, Key(K_TIGHT, s, False, False, False, False, stream), rows, waves, 64 * waves, n_stripes, tiles,
                     _ceil(tiles, waves))
    tiles = _ceil(P, 16 * 64) if linear else n_stripes * _ceil(H, 16)
    if ident and W % 64 == 0 and H % 16 == 0:          # MSPA_LAUNCH_FAST(true, true, ..)
        key = Key(K_FAST, s if s in (CORR, DENSE, MINIMAL) else 0, True, True, False, False, False)
    elif linear:                                       # MSPA_LAUNCH_LINEAR
        key = Key(K_FAST, s if s in (CORR, MINIMAL) else 0, ident, False, True, False, False)
    else:
        key = Key(K_FAST, 0, ident, False, False, False, False)
    return Route(0, LINEAR_FAMILY if linear else FAST_FAMILY, key, 16, 4, 256, n_stripes, tiles, _ceil(tiles, 4))


def parent_workspace_bytes(n_pairs, dh, dw, H, W, flags):
    if n_pairs < 0 or min(H, W) < 2 or max(H, W) > 32767:
        return -1
    if flags & FAST and (_tight_shape(dh, dw, H, W) or _rect_shape(dh, dw, H, W)):
        return 0
    return n_pairs * H * W * 4


# The walk: one launch per instantiation.  hw / dhw: colour and depth grid; outputs: names of mspa_pair_reproject's outputs, or
# "compact" for mspa_pair_correspondences; misaligned: the depth table is a view one int16 element into a larger buffer (the
# tight kernel's LDS-DMA cannot take it); key: the instantiation route() must name for it.
Walk = namedtuple("Walk", "name hw dhw outputs flags misaligned key")
SETS = {
    "corr": ("vis_bits", "pix_i16", "counts"),
    "dense": ("vis_u8", "pix_i16", "xyz_f32", "rgba", "counts"),
    "dense_xyz": ("vis_u8", "pix_i16", "xyz_f32", "counts"),
    "minimal": ("vis_bits", "counts"),
    "compact": "compact",
    "bytes": ("vis_u8", "pix_i16", "counts"),            # unnamed sets: the GENERIC instantiations
    "bits_bytes": ("vis_bits", "vis_u8", "counts"),
}


def _walk():
    w = []
    tight, rect_a, rect_b, whole, ragged, half = (96, 128), (100, 144), (64, 128), (48, 128), (100, 150), (50, 75)
    for name, mask in NAMED.items():
        for st in (0, STREAM):
            w.append(Walk(f"tight_{name}{'_stream' if st else ''}", tight, tight, SETS[name], FAST | st, False,
                          Key(K_TIGHT, mask, False, False, False, False, bool(st))))
    for name in ("corr", "minimal", "compact"):
        w.append(Walk(f"rect_{name}", rect_a, (48, 72), SETS[name], FAST, False, Key(K_TIGHT, NAMED[name], False, False, False, True, False)))
        w.append(Walk(f"rect_{name}_stream", rect_b, rect_b, SETS[name], FAST | STREAM, False,
                      Key(K_TIGHT, NAMED[name], False, False, False, True, True)))
    w.append(Walk("whole_corr_misaligned", whole, whole, SETS["corr"], FAST, True, Key(K_FAST, CORR, True, True, False, False, False)))
    w.append(Walk("whole_minimal_misaligned", whole, whole, SETS["minimal"], FAST, True, Key(K_FAST, MINIMAL, True, True, False, False, False)))
    w.append(Walk("whole_dense", whole, whole, SETS["dense"], FAST, False, Key(K_FAST, DENSE, True, True, False, False, False)))
    w.append(Walk("whole_generic", whole, whole, SETS["bytes"], FAST, False, Key(K_FAST, 0, True, True, False, False, False)))
    for tag, dhw, ident in (("ident", ragged, True), ("scaled", half, False)):
        w.append(Walk(f"linear_corr_{tag}", ragged, dhw, SETS["corr"], FAST, False, Key(K_FAST, CORR, ident, False, True, False, False)))
        w.append(Walk(f"linear_minimal_{tag}", ragged, dhw, SETS["minimal"], FAST, False, Key(K_FAST, MINIMAL, ident, False, True, False, False)))
        w.append(Walk(f"linear_generic_{tag}", ragged, dhw, SETS["bits_bytes"], FAST, False, Key(K_FAST, 0, ident, False, True, False, False)))
        w.append(Walk(f"fast_generic_{tag}", ragged, dhw, SETS["bytes"], FAST, False, Key(K_FAST, 0, ident, False, False, False, False)))
        w.append(Walk(f"exact_{tag}", ragged, dhw, SETS["corr"], 0, False, Key(K_EXACT, 0, ident, False, False, False, False)))
    return w


WALK = _walk()
# mspa_pair_correspondences on a shape the fused kernel does not take: the dense table (this instantiation) + compact_corr_kernel
DENSE_ROUTE = Walk("compact_through_dense_table", (100, 150), (100, 150), "compact", FAST, False,
                   Key(K_FAST, CORR, True, False, True, False, False))


def walk_route_inputs(c):
    """(dh, dw, H, W, outputs, aligned, flags) as pair_reproject_impl hands them to route() for a walk case."""
    if c.outputs == "compact" and c is not DENSE_ROUTE:
        mask = COMPACT
    else:
        mask = bits(SETS["corr"] if c.outputs == "compact" else c.outputs)
    return (*c.dhw, *c.hw, mask, not c.misaligned, c.flags)
