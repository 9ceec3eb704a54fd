"""A NumPy restatement of K5d (csrc/track_mining_core.h), shaped like the four ``mspa.engine`` calls that
``heads._mine_pairs_device`` makes -- ``heads.TRACK_MINING_BACKEND = track_mining_util`` runs the device line of
``object_movement_mine_pairs`` without a GPU -- and the reference the GPU tests compare the kernels with.  Arrays are NumPy's
throughout; ``world`` is the [T, P, 3] float64 block itself."""
import numpy as np

TRACK_MINING_BUDGET_BYTES = 1 << 30
TRACK_MINING_PAIR_BYTES = 24
BINS, CLASS_STATIC = 10, 10


class Refused(ValueError):
    """What the library answers with MSPA_EINVAL."""


def point_pairs(world, visibility, p, threshold=0.01, window=1e8):
    """One point's pairs in row-major order: (frames, i, j, d, static mask, moving mask)."""
    frames = np.nonzero(np.asarray(visibility)[:, p])[0]
    ii, jj = np.triu_indices(len(frames), 1)
    delta = world[frames[jj], p] - world[frames[ii], p]
    dx, dy, dz = delta[:, 0], delta[:, 1], delta[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)                  # K5c's expression
        keep = ~(frames[ii].astype(np.float64) > d + window)         # OM_C:505-507 as written
        static = keep & (d < threshold)
    return frames, ii, jj, d, static, keep & ~static


def track_pair_stats(world, visibility, points, object_not_moving_threshold=0.01, future_frame_windows=1e8):
    T = world.shape[0]
    n = len(points)
    stats = np.zeros((n, 6), dtype=np.int64)
    frames_out = np.zeros((n, T), dtype=np.int32)
    for r, p in enumerate(points):
        frames, _ii, _jj, d, static, moving = point_pairs(world, visibility, int(p), object_not_moving_threshold, future_frame_windows)
        bits = d[moving].view(np.uint64)
        frames_out[r, :len(frames)] = frames
        stats[r, :3] = len(frames), static.sum(), moving.sum()
        stats[r, 3] = np.uint64(bits.min() if bits.size else 0xffffffffffffffff).astype(np.int64)
        stats[r, 4] = np.uint64(bits.max() if bits.size else 0).astype(np.int64)
        stats[r, 5] = int(not np.isfinite(d[moving]).all())
    return {"stats": stats, "frames": frames_out, "world": world, "visibility": np.asarray(visibility), "points": np.asarray(points)}


def _pairs_of_row(state, row, threshold, window):
    return point_pairs(state["world"], state["visibility"], int(state["points"][row]), threshold, window)


def track_pair_bin_counts(state, edges, object_not_moving_threshold=0.01, future_frame_windows=1e8):
    out = np.zeros((len(state["points"]), BINS), dtype=np.int32)
    for r in range(len(state["points"])):
        _f, _ii, _jj, d, _s, moving = _pairs_of_row(state, r, object_not_moving_threshold, future_frame_windows)
        if moving.any():
            out[r] = np.bincount(np.minimum(np.digitize(d[moving], edges[r]) - 1, 9), minlength=BINS)
    return out


def sorted_segment(key_bits, payload):
    """The order the sort must give: by (key, payload), both unsigned."""
    return np.lexsort((np.asarray(payload).view(np.uint32), np.asarray(key_bits).view(np.uint64)))


def track_pair_order(state, rows, seg_offsets, n_total, object_not_moving_threshold=0.01, future_frame_windows=1e8):
    keys = np.zeros((2, n_total), dtype=np.int64)
    payload = np.zeros((2, n_total), dtype=np.int32)
    for s, row in enumerate(rows):
        _f, ii, jj, d, _s, moving = _pairs_of_row(state, int(row), object_not_moving_threshold, future_frame_windows)
        k = d[moving].view(np.int64)
        pl = ((ii[moving] << 16) | jj[moving]).astype(np.uint32).view(np.int32)
        assert len(k) == seg_offsets[s + 1] - seg_offsets[s]
        order = sorted_segment(k, pl)
        keys[0, seg_offsets[s]:seg_offsets[s + 1]] = k[order]
        payload[0, seg_offsets[s]:seg_offsets[s + 1]] = pl[order]
    return keys, payload


def track_pair_resolve(state, bin_counts, rows, seg_offsets, payload, picks, class_counts, object_not_moving_threshold=0.01,
                       future_frame_windows=1e8):
    out = np.zeros((len(picks), 2), dtype=np.int32)
    for k, (sel, cls, rank) in enumerate(np.asarray(picks).reshape(-1, 3).tolist()):
        if not (0 <= sel < len(rows) and 0 <= cls <= CLASS_STATIC and 0 <= rank < class_counts[sel][cls]):
            raise Refused(f"pick {k}: rank {rank} of class {cls}")
    for k, (sel, cls, rank) in enumerate(np.asarray(picks).reshape(-1, 3).tolist()):
        frames, ii, jj, _d, static, _m = _pairs_of_row(state, int(rows[sel]), object_not_moving_threshold, future_frame_windows)
        if cls == CLASS_STATIC:
            m = np.nonzero(static)[0][rank]
            i, j = ii[m], jj[m]
        else:
            pl = int(np.asarray(payload)[0].view(np.uint32)[seg_offsets[sel] + int(bin_counts[int(rows[sel]), :cls].sum()) + rank])
            i, j = pl >> 16, pl & 0xffff
        out[k] = frames[i], frames[j]
    return out


def point_edges(stats_row):
    """The 11 edges the host derives from a statistics record (zeros where the point has no moving pair)."""
    if stats_row[2] == 0:
        return np.zeros(BINS + 1)
    lo, hi = np.asarray(stats_row[3:5], dtype=np.int64).view(np.float64)
    return np.histogram_bin_edges(np.array([lo, hi]), bins=BINS)


def make_block(seed, T, P=24, n_groups=3):
    """A track block with the mining's hard cases: ``(world [T,P,3], visibility [T,P] bool, groups)``.  Coordinates are rounded to
    0.01 m (ties among moving pairs); point 0 is nearly static, point 1 visible in no frame, point 2 in one, point 3 jumps between
    two places (its moving distances are all equal), point 4 is static to the last bit."""
    rng = np.random.default_rng(seed)
    world = np.round(np.cumsum(rng.normal(0, 0.02, (T, P, 3)), axis=0) + rng.normal(0, 1, (1, P, 3)), 2)
    world[:, 0] = world[0, 0] + np.round(rng.normal(0, 0.004, (T, 3)), 3)
    a, b = rng.normal(0, 1, 3), rng.normal(0, 1, 3)
    world[:, 3] = np.where((np.arange(T) % 2 == 0)[:, None], a, b)
    world[:, 4] = world[0, 4]
    visibility = rng.random((T, P)) > 0.25
    visibility[:, 1] = False
    visibility[:, 2] = False
    visibility[T // 2, 2] = True
    visibility[:, 3] = True
    order = rng.permutation(P)
    groups = [sorted(int(p) for p in order[g::n_groups]) for g in range(n_groups)]
    return world, visibility, groups
