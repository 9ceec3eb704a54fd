"""Shared by the pair-table tests (CPU and GPU): overlap values that sit on and beside the bin edges, small tables in the pair
table's schema, the writers whose layouts the device path takes, and the host line's results to compare with."""
import contextlib
import io

import numpy as np

COLUMNS = ["scene_id", "image_id1", "image_id2", "overlap", "distance", "yaw", "pitch"]
EDGE_SETS = ((6, 35, 1), (0, 100, 5), (6, 35, 0.5))
# (all_overlap_samples, non_overlap_samples, overlap_min, overlap_max, interval): a plain draw; a quota larger than the table
# (every bin whole, the leftover warning); a zero part that is drawn from; half-wide bins; a zero part kept whole
PARAMETER_SETS = ((300, 0, 6, 35, 1), (10 ** 6, 0, 6, 35, 1), (200, 50, 0, 100, 5), (240, 0, 6, 35, 0.5), (100, 10 ** 6, 0, 100, 5))


def edges_of(lo, hi, step):
    return np.arange(lo, hi + step, step)


def edge_values(edge_sets=EDGE_SETS) -> np.ndarray:
    """Every edge of every set, one ulp on either side of each, +-0, NaN, +-inf, values below and above every range."""
    e = np.unique(np.concatenate([edges_of(*s).astype(np.float64) for s in edge_sets]))
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -3.5, -1e-300, 5e-324, 1e-300, 5.999, 100.0001, 250.0, 1e300])
    return np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), special])


def cut_reference(x: np.ndarray, edges) -> np.ndarray:
    """The class bytes by the host line's own means: the ``== 0`` split, then ``pd.cut(..., include_lowest=True)`` and ``dropna``."""
    import pandas as pd
    from mspa import _lib
    x = np.asarray(x, dtype=np.float64)
    out = np.full(len(x), _lib.PAIR_CLASS_DROPPED, dtype=np.uint8)
    zero = x == 0
    cat = pd.cut(pd.Series(x[~zero]), bins=edges, include_lowest=True).cat.codes.to_numpy()
    out[~zero] = np.where(cat >= 0, cat, _lib.PAIR_CLASS_DROPPED).astype(np.uint8)
    out[zero] = _lib.PAIR_CLASS_ZERO
    return out


def classify_numpy(overlap: np.ndarray, edges: np.ndarray) -> np.ndarray:
    """The bin rule of csrc/pair_bins_core.h restated in NumPy (and the stub that stands in for the device): uint8 codes."""
    from mspa import _lib
    x = np.asarray(overlap, dtype=np.float64)
    code = np.searchsorted(edges, x, side="left")
    code[x == edges[0]] = 1
    out = np.where((code >= 1) & (code <= len(edges) - 1) & ~np.isnan(x), code - 1, _lib.PAIR_CLASS_DROPPED)
    out[x == 0] = _lib.PAIR_CLASS_ZERO
    return out.astype(np.uint8)


def overlap_column(n: int, seed: int, zero_fraction: float = 0.6) -> np.ndarray:
    """``n`` overlap values: the edge values first (as many as fit), then about ``zero_fraction`` zeros among values spread over
    [0, 110) with a few NaNs."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 110.0, size=n)
    x[rng.random(n) < 0.01] = np.nan
    x[rng.random(n) < zero_fraction] = 0.0
    ev = edge_values()
    rng.shuffle(ev)
    x[:min(n, len(ev))] = ev[:n]
    return x


def frame(n: int, seed: int, zero_fraction: float = 0.6, scene: str = "scene0000_00", overlap=None):
    import pandas as pd
    rng = np.random.default_rng(seed + 1)
    ids = np.array([f"{k:05d}" for k in range(0, 4000, 10)], dtype=object)
    x = overlap_column(n, seed, zero_fraction) if overlap is None else np.asarray(overlap, dtype=np.float64)
    yaw = rng.normal(size=n)
    yaw[rng.random(n) < 0.02] = np.nan
    return pd.DataFrame({"scene_id": np.full(n, scene, dtype=object), "image_id1": ids[rng.integers(0, len(ids), n)],
                         "image_id2": ids[rng.integers(0, len(ids), n)], "overlap": x, "distance": rng.uniform(0, 9, n),
                         "yaw": yaw, "pitch": np.round(rng.normal(size=n), 1)}, columns=COLUMNS)


def write_project(path: str, frames) -> None:
    """(a) this project's layout: a row group per scene through ``parquet_splice.encode_row_group`` (ids dictionary-coded, doubles
    PLAIN -- a NaN stays a NaN value), spliced into one file."""
    import pyarrow as pa
    from mspa import parquet_splice
    def table(f):                                              # arrays from NumPy, as the sweep builds them: NaN is a value, not a null
        return pa.table({c: pa.array(f[c].tolist(), type=pa.string()) if c in COLUMNS[:3] else pa.array(f[c].to_numpy()) for c in COLUMNS})

    parquet_splice.splice([parquet_splice.encode_row_group(table(f), use_dictionary=COLUMNS[:3]) for f in frames], path)


def write_pandas(path: str, frames, **options) -> None:
    """(b) ``DataFrame.to_parquet(index=False)``: a NaN becomes a null; ``options`` go to pyarrow's writer."""
    import pandas as pd
    pd.concat(frames, ignore_index=True).to_parquet(path, index=False, **options)


def host_line(path: str, args):
    """(frame, printed text, generator state) of ``sample_dataframe(pd.read_parquet(path), *args)`` under the seed set by the caller."""
    import pandas as pd
    from mspa.sampling import sample_dataframe
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        got = sample_dataframe(pd.read_parquet(path), *args)
    return got, out.getvalue(), np.random.get_state()


def same_state(a, b) -> bool:
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def assert_same_sample(path: str, args, sample, seed: int = 7):
    """``sample(*args)`` against the host line under the same seed: frame (exact, and the floats' bits), printed text, state."""
    import pandas as pd
    np.random.seed(seed)
    want, want_text, want_state = host_line(path, args)
    np.random.seed(seed)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        got = sample(*args)
    state = np.random.get_state()
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    assert list(got.columns) == COLUMNS and [str(t) for t in got.dtypes] == [str(t) for t in want.dtypes]
    for name in COLUMNS[3:]:
        assert np.array_equal(got[name].to_numpy().view(np.int64), want[name].to_numpy().view(np.int64)), name
    assert out.getvalue() == want_text
    assert same_state(state, want_state)
    return got
