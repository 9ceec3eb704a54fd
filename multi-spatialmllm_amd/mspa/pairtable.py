"""The pair table (`*_camera_info_D5.parquet`: scene_id, image_id1, image_id2, overlap, distance, yaw, pitch) sampled on the GPU.

The builders that draw their rows from the table (camera movement, the two visual-correspondence heads) used to load it whole
with ``pd.read_parquet`` and push it through ``sampling.sample_dataframe`` -- two masked copies of the frame, ``pd.cut``, a
``groupby`` and a ``DataFrame.sample`` per bin -- once per question type.  ``MSPA_PAIRTABLE=device`` sends them here instead
(``sampled_rows``); unset, nothing changes.  The result is the host line's: the same frame (rows, order, columns, dtypes, floats
bit for bit), the same printed lines, the same state of the global NumPy generator afterwards.

  * ``PairTable`` walks the DOUBLE chunks' page headers (``visindex.column_chunk_pages``), uploads the pages as they lie in the
    file, decompresses them with the Snappy-by-blocks route and assembles the four float64 columns
    (``engine.parquet_double_columns_device``: PLAIN and dictionary-coded pages, v1 and v2, nulls as NaN) -- once per file;
  * per (bins, min, max, interval) the ``overlap`` column becomes one class byte per row and, per class, the ascending file
    rows (``engine.pair_bin_codes`` / ``pair_partition``; the rule is csrc/pair_bins_core.h's) -- once per parameter set;
  * a sample then needs the class counts, the host's draws (``plan_draws``: upstream's calls in upstream's order), a lookup of
    the drawn positions in the row lists and a gather of the four columns on the device, and the three id columns of the
    sampled rows from arrow (dictionary-read row groups, ``take``: no Python string for an unsampled row).

Whatever the device path does not take -- another schema, codec or encoding, a damaged page, arguments the host function
rejects -- goes through the host line with the reason recorded (``last_decline``, ``stats``).
"""
from __future__ import annotations

import collections
import os
from typing import Dict, List, Optional

import numpy as np

from . import _lib
from .sampling import sample_dataframe

ID_COLUMNS = ("scene_id", "image_id1", "image_id2")
DOUBLE_COLUMNS = ("overlap", "distance", "yaw", "pitch")
COLUMNS = ID_COLUMNS + DOUBLE_COLUMNS

# parquet.thrift numbers
_DATA_PAGE, _INDEX_PAGE, _DICTIONARY_PAGE, _DATA_PAGE_V2 = 0, 1, 2, 3
_PLAIN, _PLAIN_DICTIONARY, _RLE, _RLE_DICTIONARY = 0, 2, 3, 8
_CODECS = {"UNCOMPRESSED": False, "SNAPPY": True}


def mode() -> str:
    """Who samples the pair table: "host" (the default: ``pd.read_parquet`` and ``sampling.sample_dataframe``) or "device"
    (``MSPA_PAIRTABLE=device``: ``PairTable``).  Read at every call."""
    value = os.environ.get("MSPA_PAIRTABLE", "host").strip().lower() or "host"
    if value not in ("host", "device"):
        raise ValueError(f"MSPA_PAIRTABLE={value!r}: expected 'host' or 'device'")
    return value


def bin_edges(overlap_min, overlap_max, interval) -> np.ndarray:
    """``sample_dataframe``'s edges as float64 (what ``pd.cut`` compares the float64 column with)."""
    return np.arange(overlap_min, overlap_max + interval, interval).astype(np.float64)


def arguments_reason(all_overlap_samples, non_overlap_samples, overlap_min, overlap_max, interval) -> Optional[str]:
    """None when the device path takes these arguments, otherwise why not: whatever the host function raises for, fewer than
    one bin, or more bins than a class byte holds goes to the host function."""
    for name, v in (("all_overlap_samples", all_overlap_samples), ("non_overlap_samples", non_overlap_samples)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            return f"{name} is not a non-negative int"
    for name, v in (("overlap_min", overlap_min), ("overlap_max", overlap_max), ("interval", interval)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            return f"{name} is not a finite number"
    if not interval > 0:
        return "interval is not positive"
    if (overlap_max - overlap_min) / interval > _lib.PAIR_MAX_BINS + 1:
        return f"more than {_lib.PAIR_MAX_BINS} bins"
    edges = bin_edges(overlap_min, overlap_max, interval)
    if len(edges) < 2:
        return "fewer than one bin"
    if len(edges) - 1 > _lib.PAIR_MAX_BINS:
        return f"more than {_lib.PAIR_MAX_BINS} bins"
    if not bool((np.diff(edges) > 0).all()):
        return "edges that do not ascend"
    return None


def draw_positions(length: int, want: int) -> np.ndarray:
    """The positions ``DataFrame.sample(n=want)`` picks in a frame of ``length`` rows, drawn from the global NumPy generator by
    the installed pandas itself (today ``np.random.choice(length, size=want, replace=False)``, which permutes the whole
    population even for ``want == 0``).  Going through pandas costs one throw-away index and keeps the draws those of the host
    line should pandas ever change how it draws; calling NumPy directly would pin today's behaviour instead."""
    import pandas as pd
    return pd.DataFrame(index=pd.RangeIndex(int(length))).sample(n=int(want)).index.to_numpy()


def plan_draws(counts, n_bins: int, all_overlap_samples: int, non_overlap_samples: int, draw=draw_positions, out=print) -> List[tuple]:
    """The host half of the sampler: ``counts[c]`` rows per class (bins 0 .. n_bins - 1, ``_lib.PAIR_CLASS_ZERO``) -> the picks in
    FRAME order, [(class, positions)] with positions None for "the whole group in file order" or the drawn positions (an
    int array, in drawn order) inside the group.  Draws and printed lines are ``sample_dataframe``'s, in its order: the zero
    part first (drawn iff it is longer than ``non_overlap_samples``, ``n = 0`` included), then the bins from the smallest to the
    largest (ties keep bin order), a bin that cannot fill its quota passing the shortfall on.  The zero part stands last in
    the frame."""
    n_zero = int(counts[_lib.PAIR_CLASS_ZERO])
    zero_pick = (_lib.PAIR_CLASS_ZERO, None if n_zero <= non_overlap_samples else draw(n_zero, non_overlap_samples))
    sizes = [int(counts[k]) for k in range(n_bins)]
    base, extra = divmod(all_overlap_samples, n_bins)
    quota = [base + (1 if k < extra else 0) for k in range(n_bins)]
    picks, carry = [], 0
    for k in sorted(range(n_bins), key=lambda k: sizes[k]):
        want = quota[k] + carry
        out(f"[sample_dataframe] current_quota v.s. group_df: {want} v.s. {sizes[k]}")
        if sizes[k] <= want:
            picks.append((k, None))
            carry = want - sizes[k]
        else:
            picks.append((k, draw(sizes[k], want)))
            carry = 0
    if carry > 0:
        out(f"[sample_dataframe] Warning: bins not enough to reach {all_overlap_samples}; leftover {carry}")
    return picks + [zero_pick]


def pick_positions(picks: List[tuple], begin: np.ndarray) -> np.ndarray:
    """``plan_draws``' picks -> positions in the partition's row list (int64): class c's rows are ``order[begin[c] : begin[c + 1]]``."""
    parts = [np.arange(begin[c], begin[c + 1], dtype=np.int64) if pos is None else begin[c] + np.asarray(pos, dtype=np.int64) for c, pos in picks]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


class PairTable:
    """One pair-table file, decoded on the device at first use and kept: ``len()`` rows, ``sample(...)`` -> DataFrame.

    Taken: exactly the seven columns ``COLUMNS`` in that order, the ids flat UTF8 BYTE_ARRAY, the others flat DOUBLE, no index
    column; the DOUBLE chunks Snappy-compressed or not, their data pages v1 (RLE levels) or v2, PLAIN or dictionary-coded behind a
    PLAIN dictionary page; fewer than 2^31 rows.  Anything else declines the whole file: ``sample`` then returns the host line's
    frame, ``last_decline`` says why and ``stats["samples_declined"]`` counts it.  ``stats``: samples, samples_declined,
    decodes (of the file), partitions (per parameter set), rows, pages, h2d_bytes, blocks (64 KiB Snappy blocks decoded in
    parallel), serial_streams (pages the one-wave kernel took), dict_pages, v2_pages, null_pages."""

    MAX_PARTITIONS = 2

    def __init__(self, path, device="cuda"):
        import pyarrow.parquet as pq
        self.path, self.device = os.fspath(path), device
        self.file = pq.ParquetFile(self.path)
        self.num_rows = int(self.file.metadata.num_rows)
        self.stats = {"samples": 0, "samples_declined": 0, "decodes": 0, "partitions": 0, "rows": self.num_rows, "pages": 0, "h2d_bytes": 0,
                      "blocks": 0, "serial_streams": 0, "dict_pages": 0, "v2_pages": 0, "null_pages": 0}
        self.last_decline: Optional[str] = None
        self.stage_times: Optional[dict] = None
        self._stage_start = 0.0
        self._reason = self.schema_reason()
        self._columns = None                                   # float64 [4, rows] on the device
        self._partitions: "collections.OrderedDict[tuple, tuple]" = collections.OrderedDict()
        self._ids = None                                       # a second handle that reads the id columns as dictionaries
        md = self.file.metadata
        self._group_first = np.concatenate([[0], np.cumsum([md.row_group(g).num_rows for g in range(md.num_row_groups)])]).astype(np.int64)

    def __len__(self) -> int:
        return self.num_rows

    # ------------------------------------------------------------------------------------------------ what the device path takes
    def schema_reason(self) -> Optional[str]:
        """None when the file has the schema the device path takes, otherwise what is in the way."""
        import pandas as pd
        md, schema = self.file.metadata, self.file.schema
        names = [schema.column(k).path for k in range(md.num_columns)]
        if any(n.startswith("__index_level_") for n in names):
            return "a pandas index column"
        extra, missing = [n for n in names if n not in COLUMNS], [n for n in COLUMNS if n not in names]
        if missing:
            return f"a missing column: {missing[0]}"
        if extra:
            return f"an extra column: {extra[0]}"
        if tuple(names) != COLUMNS or len(self.file.schema_arrow.names) != len(COLUMNS):
            return "columns that are not the seven of the pair table, in its order"
        for k, name in enumerate(names):
            leaf = schema.column(k)
            if leaf.max_repetition_level != 0 or leaf.max_definition_level > 1:
                return f"column {name} is not flat"
            if name in ID_COLUMNS and (leaf.physical_type != "BYTE_ARRAY" or str(leaf.logical_type) != "String"):
                return f"column {name} is {leaf.physical_type} / {leaf.logical_type}, not a UTF8 BYTE_ARRAY"
            if name in DOUBLE_COLUMNS and leaf.physical_type != "DOUBLE":
                return f"column {name} is {leaf.physical_type}, not DOUBLE"
        if self.num_rows > 0x7fffffff:
            return "2^31 rows or more"
        try:
            if pd.get_option("future.infer_string"):
                return "pandas reads strings as a string dtype"
        except (KeyError, pd.errors.OptionError):
            pass
        return None

    def plan(self):
        """The host's step alone: the page headers of the four DOUBLE columns' chunks, every row group -> (plan, None) or
        (None, why the device path does not take the file).  The plan: ``pieces`` -- the byte ranges to upload, each (bytes,
        uncompressed size, Snappy or not), dictionary pages and the level bytes of v2 pages among them -- and ``pages``, the
        data pages in (column, row group, page) order: (piece of the payload, piece of a v2 page's levels or -1, piece of the
        dictionary or -1, rows, first row in the [4, rows] output, flags of ``engine.parquet_double_columns_device``)."""
        from .visindex import column_chunk_pages
        if self._reason is not None:
            return None, self._reason
        md, schema = self.file.metadata, self.file.schema
        col_of = {schema.column(k).path: k for k in range(md.num_columns)}
        pieces, per_chunk = [], {}
        with open(self.path, "rb") as f:
            for g in range(md.num_row_groups):
                for c, name in enumerate(DOUBLE_COLUMNS):
                    k = col_of[name]
                    try:
                        table, chunk = column_chunk_pages(self.path, md.row_group(g).column(k), "pairtable", f"{name} chunk of row group {g}",
                                                          file=f)
                    except (ValueError, IndexError, TypeError) as e:
                        return None, f"row group {g}, {name}: damaged page headers ({e})"
                    got = self._plan_chunk(table, chunk, schema.column(k).max_definition_level == 1, md.row_group(g).num_rows, pieces)
                    if isinstance(got, str):
                        return None, f"row group {g}, {name}: {got}"
                    per_chunk[c, g] = got
        pages = []
        for c in range(len(DOUBLE_COLUMNS)):
            for g in range(md.num_row_groups):
                first = c * self.num_rows + int(self._group_first[g])
                pages += [(payload, levels, dictionary, rows, first + row0, flags) for payload, levels, dictionary, rows, row0, flags in per_chunk[c, g]]
        return {"pieces": pieces, "pages": pages}, None

    @staticmethod
    def _plan_chunk(table: dict, chunk: bytes, has_levels: bool, group_rows: int, pieces: list):
        """One chunk's pages -> its data pages as ``plan`` lists them (pieces appended to ``pieces``), or why not."""
        if table["codec"] not in _CODECS:
            return f"codec {table['codec']}"
        snappy = _CODECS[table["codec"]]
        view = memoryview(chunk)
        kind, enc = table["type"], table["encoding"]
        if bool(((kind != _DATA_PAGE) & (kind != _DICTIONARY_PAGE) & (kind != _DATA_PAGE_V2)).any()):
            return "a page that is neither a data nor a dictionary page"
        if int(table["uncompressed"].max(initial=0)) > 0x7fffffff or int(table["compressed"].max(initial=0)) > 0x7fffffff:
            return "a page of 2 GiB"
        if bool((table["compressed"] < 0).any()) or bool((table["uncompressed"] < 0).any()) or bool((table["num_values"] < 0).any()):
            return "a page header with a negative size"
        data = np.nonzero(kind != _DICTIONARY_PAGE)[0]
        if int(table["num_values"][data].sum()) != group_rows:
            return "pages that do not add up to the row group's rows"

        def piece(lo, hi, unc, compressed):
            if not compressed and hi - lo != unc:
                return None
            pieces.append((view[lo:hi], int(unc), bool(compressed)))
            return len(pieces) - 1

        dictionary, dict_count, out = -1, 0, []
        for p in range(len(kind)):
            pos, comp, unc = int(table["pos"][p]), int(table["compressed"][p]), int(table["uncompressed"][p])
            if kind[p] == _DICTIONARY_PAGE:
                dict_count = int(table["dict_values"][p])
                if dictionary >= 0 or int(enc[p]) not in (_PLAIN, _PLAIN_DICTIONARY) or unc != 8 * dict_count:
                    return "a dictionary page that is not one PLAIN page of doubles"
                dictionary = piece(pos, pos + comp, unc, snappy)
                if dictionary is None:
                    return "an uncompressed page whose sizes differ"
                continue
            coded = int(enc[p]) in (_PLAIN_DICTIONARY, _RLE_DICTIONARY)
            if not coded and int(enc[p]) != _PLAIN:
                return f"a data page with encoding {int(enc[p])}"
            if coded and dictionary < 0:
                return "dictionary-coded pages without a PLAIN dictionary page in front"
            flags, levels = _lib.PAGE_DICT_CODED if coded else 0, -1
            if kind[p] == _DATA_PAGE:
                if has_levels and int(table["levels"][p]) != _RLE:
                    return "definition levels that are not RLE"
                flags |= _lib.PAGE_LEVELS_INLINE if has_levels else 0
                payload = piece(pos, pos + comp, unc, snappy)
            else:
                lev, rep = int(table["def_bytes"][p]), int(table["rep_bytes"][p])
                if rep != 0 or lev < 0 or lev > comp or lev > unc or (lev and not has_levels):
                    return "a v2 page with repetition levels, or level bytes that pass the page"
                if has_levels and not lev and int(table["num_nulls"][p]):
                    return "a v2 page with nulls and no definition levels"
                if lev:
                    flags |= _lib.PAGE_LEVELS_GIVEN
                    levels = piece(pos, pos + lev, lev, False)
                payload = piece(pos + lev, pos + comp, unc - lev, snappy and bool(table["is_compressed"][p]))
            if payload is None:
                return "an uncompressed page whose sizes differ"
            out.append((payload, levels, dictionary if coded else -1, int(table["num_values"][p]), int(table["first_row"][p]), flags))
        return out

    # ------------------------------------------------------------------------------------------------ the device's steps
    def _mark(self, stage: str):
        """The stage clock of tools/pairtable_bench.py: off unless ``stage_times`` is a dict, then every stage ends with a device
        synchronise and its wall time is added under its name."""
        if self.stage_times is None:
            return
        import time
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        now = time.perf_counter()
        self.stage_times[stage] = self.stage_times.get(stage, 0.0) + now - self._stage_start
        self._stage_start = now

    def _start_clock(self):
        if self.stage_times is not None:
            import time
            self._stage_start = time.perf_counter()

    def columns(self):
        """The four DOUBLE columns as float64 [4, rows] on the device (decoded at the first call), or a str: why not."""
        import torch
        from . import engine
        if self._columns is not None:
            return self._columns
        plan, why = self.plan()
        self._mark("file_read")
        if plan is None:
            return why
        pieces, pages = plan["pieces"], plan["pages"]
        dev = torch.device(self.device)
        if not pages:                                            # a file without rows
            self._columns = torch.empty((len(DOUBLE_COLUMNS), 0), dtype=torch.float64, device=dev)
            return self._columns
        sizes = np.array([len(b) for b, _u, _s in pieces], dtype=np.int64)
        unc = np.array([u for _b, u, _s in pieces], dtype=np.int64)
        snappy = np.array([s for _b, _u, s in pieces], dtype=bool)
        src_at = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        upload = int(src_at[-1])
        staged = torch.empty((max(upload, 1),), dtype=torch.uint8, pin_memory=True)
        flat = staged.numpy()
        for k, (b, _u, _s) in enumerate(pieces):
            flat[src_at[k]:src_at[k + 1]] = np.frombuffer(b, dtype=np.uint8)
        src = staged.to(dev, non_blocking=True)[:upload]
        self.stats["h2d_bytes"] += upload
        self._mark("h2d")
        # where every piece's uncompressed bytes lie in the buffer the column kernels read: the Snappy pieces decoded back to
        # back, behind the upload itself when some piece is not compressed (its bytes are read where they were uploaded)
        at = src_at[:-1].copy()
        which = np.nonzero(snappy)[0]
        stream_status = route = None
        payloads = src
        if len(which):
            table = torch.from_numpy(np.stack([src_at[which], sizes[which], unc[which]])).to(dev)
            part, _part_at, stream_status, route = engine.snappy_decompress_blocks_device(src, table[0].contiguous(), table[1].contiguous(),
                                                                                          table[2].contiguous())
            base = 0 if len(which) == len(pieces) else upload
            at[which] = base + np.concatenate([[0], np.cumsum(unc[which])])[:-1]
            payloads = part if base == 0 else torch.cat([src, part])
        self._mark("decompress")
        pg = np.array(pages, dtype=np.int64).reshape(-1, 6)
        payload, levels, dictionary = pg[:, 0], pg[:, 1], pg[:, 2]
        host = np.stack([at[payload], unc[payload], pg[:, 3], pg[:, 4], np.where(levels >= 0, at[levels], 0), np.where(levels >= 0, unc[levels], 0),
                         np.where(dictionary >= 0, at[dictionary], 0), np.where(dictionary >= 0, unc[dictionary] // 8, 0)])
        t = torch.from_numpy(host).to(dev)
        flags = torch.from_numpy(pg[:, 5].astype(np.int32)).to(dev)
        out, status = engine.parquet_double_columns_device(payloads, t[0].contiguous(), t[1].contiguous(), t[2].contiguous(), flags, t[3].contiguous(),
                                                           len(DOUBLE_COLUMNS) * self.num_rows, t[4].contiguous(), t[5].contiguous(),
                                                           t[6].contiguous(), t[7].contiguous())
        bad = torch.stack([status[k].ne(0).any() for k in ("layout", "levels", "indices", "values")] +
                          [stream_status.ne(0).any() if stream_status is not None else torch.zeros((), dtype=torch.bool, device=dev)])
        bad = bad.cpu().numpy()                                  # THE read-back: nothing leaves unchecked
        self._mark("columns")
        if bad.any():
            what = ("a page's layout", "definition levels", "dictionary indices", "a page's values", "a Snappy stream")
            return "the device declined " + ", ".join(w for w, b in zip(what, bad) if b)
        if route is not None:
            routes = route.cpu().numpy()
            self.stats["blocks"] += int(routes.sum())
            self.stats["serial_streams"] += int((routes == 0).sum())
        self.stats["decodes"] += 1
        self.stats["pages"] += len(pages)
        self.stats["dict_pages"] += int((pg[:, 5] & _lib.PAGE_DICT_CODED != 0).sum())
        self.stats["v2_pages"] += int((pg[:, 5] & _lib.PAGE_LEVELS_GIVEN != 0).sum())
        self.stats["null_pages"] += int(status["null_pages"])
        self._columns = out.view(len(DOUBLE_COLUMNS), self.num_rows)
        return self._columns

    def partition(self, overlap_min, overlap_max, interval):
        """(counts int64 [256] on the host, order int32 [rows] and begin int64 [257] on the device) of the parameter set: class
        c's file rows, ascending, are ``order[begin[c] : begin[c + 1]]``.  Cached per (bins, min, max, interval)."""
        import torch
        from . import engine
        edges = bin_edges(overlap_min, overlap_max, interval)
        key = (len(edges) - 1, float(overlap_min), float(overlap_max), float(interval))
        if key in self._partitions:
            self._partitions.move_to_end(key)
            return self._partitions[key]
        overlap = self._columns[0]
        codes, tile_counts = engine.pair_bin_codes(overlap, torch.from_numpy(edges).to(overlap.device))
        self._mark("codes")
        order, begin = engine.pair_partition(codes, tile_counts)
        counts = np.diff(begin.cpu().numpy())
        self._mark("partition")
        self.stats["partitions"] += 1
        self._partitions[key] = (counts, order, begin)
        while len(self._partitions) > self.MAX_PARTITIONS:
            self._partitions.popitem(last=False)
        return self._partitions[key]

    def rows_of(self, positions: np.ndarray, order):
        """Positions in the partition's row list -> file rows, int64 on the device (torch indexing: plumbing)."""
        import torch
        return order[torch.from_numpy(np.ascontiguousarray(positions, dtype=np.int64)).to(order.device)].to(torch.int64)

    def id_columns(self, rows: np.ndarray) -> Dict[str, np.ndarray]:
        """The three id columns of file rows ``rows`` (any order, repeats allowed) as object arrays of str: every touched row
        group's id columns are read as dictionaries and taken from, so no Python string exists for a row that was not asked for."""
        import pyarrow as pa
        import pyarrow.parquet as pq
        ids = list(ID_COLUMNS)
        if len(rows) == 0:
            return {name: np.empty(0, dtype=object) for name in ids}
        if self._ids is None:
            self._ids = pq.ParquetFile(self.path, read_dictionary=ids)
        types = {name: self.file.schema_arrow.field(name).type for name in ids}
        group = np.searchsorted(self._group_first[1:], rows, side="right")
        perm = np.argsort(group, kind="stable")
        by_group, groups = rows[perm], group[perm]
        cuts = np.concatenate([[0], np.flatnonzero(np.diff(groups)) + 1, [len(rows)]])
        taken = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            g = int(groups[lo])
            t = self._ids.read_row_group(g, columns=ids).take(pa.array(by_group[lo:hi] - self._group_first[g]))
            taken.append(pa.table({name: t.column(name).cast(types[name]) for name in ids}))
        inverse = np.empty(len(rows), dtype=np.int64)
        inverse[perm] = np.arange(len(rows))
        whole = pa.concat_tables(taken).take(pa.array(inverse))
        return {name: whole.column(name).to_pandas().to_numpy(dtype=object) for name in ids}

    def _decline(self, why: str, args):
        import pandas as pd
        self.stats["samples_declined"] += 1
        self.last_decline = why
        return sample_dataframe(pd.read_parquet(self.path), *args)

    def sample(self, all_overlap_samples: int, non_overlap_samples: int, overlap_min=0, overlap_max=100, interval=1):
        """``sample_dataframe(pd.read_parquet(path), ...)``: the same frame, printed lines and generator state, the rows chosen
        and gathered on the device.  What the device path does not take goes through that very line (``last_decline``)."""
        import pandas as pd
        args = (all_overlap_samples, non_overlap_samples, overlap_min, overlap_max, interval)
        self.stats["samples"] += 1
        self._start_clock()
        why = self._reason or arguments_reason(*args)
        if why is None:
            cols = self.columns()
            why = cols if isinstance(cols, str) else None
        if why is not None:
            return self._decline(why, args)
        counts, order, begin = self.partition(overlap_min, overlap_max, interval)
        self._start_clock()
        picks = plan_draws(counts, len(bin_edges(overlap_min, overlap_max, interval)) - 1, int(all_overlap_samples), int(non_overlap_samples))
        self._mark("draws")
        rows = self.rows_of(pick_positions(picks, np.concatenate([[0], np.cumsum(counts)])), order)
        doubles = cols[:, rows].cpu().numpy()
        rows = rows.cpu().numpy()
        self._mark("row_gather")
        ids = self.id_columns(rows)
        self._mark("id_columns")
        frame = pd.DataFrame({**ids, **{name: doubles[k] for k, name in enumerate(DOUBLE_COLUMNS)}}, columns=list(COLUMNS))
        self._mark("frame")
        return frame


_TABLES: "collections.OrderedDict[tuple, PairTable]" = collections.OrderedDict()
MAX_TABLES = 2


def open_table(path, device="cuda") -> PairTable:
    """The ``PairTable`` of ``path``, from a small cache of the last ``MAX_TABLES`` files keyed by (real path, size, mtime_ns,
    device): the passes of one builder run (a question type each, train and val) decode each table once."""
    st = os.stat(path)
    key = (os.path.realpath(path), st.st_size, st.st_mtime_ns, str(device))
    if key in _TABLES:
        _TABLES.move_to_end(key)
        return _TABLES[key]
    table = _TABLES[key] = PairTable(path, device)
    while len(_TABLES) > MAX_TABLES:
        _TABLES.popitem(last=False)
    return table


def sampled_rows(parquet_path, all_overlap_samples: int, non_overlap_samples: int, overlap_min=0, overlap_max=100, interval=1,
                 on_loaded=None, device="cuda"):
    """THE entry of the builders that sample the pair table: the frame ``sample_dataframe(pd.read_parquet(parquet_path), ...)``
    returns, by that line itself (``MSPA_PAIRTABLE`` unset) or by ``PairTable.sample`` (``MSPA_PAIRTABLE=device``).
    ``on_loaded(rows)`` is called once the table's row count is known and before anything is sampled (the builders print
    their "Loaded ..." line there).  Every rank of a sharded job samples for itself, as before: no collective."""
    if mode() == "host":
        import pandas as pd
        df = pd.read_parquet(parquet_path)
        if on_loaded is not None:
            on_loaded(len(df))
        return sample_dataframe(df, all_overlap_samples=all_overlap_samples, non_overlap_samples=non_overlap_samples, overlap_min=overlap_min,
                                overlap_max=overlap_max, interval=interval)
    table = open_table(parquet_path, device)
    if on_loaded is not None:
        on_loaded(len(table))
    return table.sample(all_overlap_samples, non_overlap_samples, overlap_min, overlap_max, interval)
