"""The visibility index of a scene (MVI.process_scene, make_visibility_info.py:75-125) as columns.

``image_to_points`` (per image: ascending indices of the vertices it sees) and ``point_to_images`` (per vertex: the
images that see it, in image order) are two compactions of K1's bit matrix -- the second one of its transpose -- done
on the device (K9: mspa_bits_popcount / mspa_bits_expand / mspa_bits_transpose).  What comes back to the host is a
pair of CSR tables; from there

  * ``to_arrow``  builds the (key, values) table every reader of the index expects -- keys
    ``scene:image_to_points:img`` / ``scene:point_to_images:idx``, values the JSON text of the list, byte for byte what
    ``json.dumps`` gives (make_visibility_info.py:38-73) -- with arrow compute kernels, no Python object per row;
  * ``to_dict``   builds the reference's nested dict (for the .pkl output and for callers that want the original type).
"""
from __future__ import annotations

import dataclasses
import json
import os
from typing import Dict, List, NamedTuple, Optional

import numpy as np


def encode_mode() -> str:
    """Who encodes the index's ``values`` column chunk: "host" (the default: pyarrow, on the encoder thread) or "device"
    (``MSPA_VISINDEX_ENCODE=device``: K12 writes the Snappy-compressed data pages on the GPU and only they cross PCIe).  Read at
    every call."""
    value = os.environ.get("MSPA_VISINDEX_ENCODE", "host").strip().lower() or "host"
    if value not in ("host", "device"):
        raise ValueError(f"MSPA_VISINDEX_ENCODE={value!r}: expected 'host' or 'device'")
    return value


def decode_mode() -> str:
    """Who turns the index's ``image_to_points`` rows back into bitsets: "host" (the default: pyarrow reads the row group,
    ``json.loads`` and ``scene.pack_index_lists`` on the CPU) or "device" (``MSPA_VISINDEX_DECODE=device``:
    ``SceneRowGroups.scene_bits`` uploads the needed pages as they lie in the file and decompresses, parses and packs them on
    the GPU; the depth builders, which use the rows as lists, take ``scene_lists`` then: ``index_reader_route``).  Read at every
    call."""
    value = os.environ.get("MSPA_VISINDEX_DECODE", "host").strip().lower() or "host"
    if value not in ("host", "device"):
        raise ValueError(f"MSPA_VISINDEX_DECODE={value!r}: expected 'host' or 'device'")
    return value


@dataclasses.dataclass
class VisibilityCSR:
    image_ids: List[str]
    n_points: int
    i2p_offsets: np.ndarray      # [F + 1] int64
    i2p_indices: np.ndarray      # [nnz] int32 vertex indices, ascending within an image
    p2i_offsets: np.ndarray      # [N + 1] int64
    p2i_indices: np.ndarray      # [nnz] int32 image indices (positions in image_ids), ascending within a vertex
    # the lists' JSON text already written on the device (K10, engine.format_lists_device), as arrow string buffers
    # (int32 offsets [rows + 1], uint8 data): what ``to_arrow`` uses instead of the host formatters when present
    i2p_text: Optional[tuple] = None
    p2i_text: Optional[tuple] = None
    # the ``values`` column chunk already encoded on the device (K12, engine.parquet_string_pages_device): its data pages'
    # compressed bytes (uint8) and, per page, compressed size, uncompressed size and value count -- what ``to_row_group`` uses
    values_pages: Optional[dict] = None

    def empty_images(self) -> List[str]:
        n = np.diff(self.i2p_offsets)
        return [self.image_ids[k] for k in np.nonzero(n == 0)[0]]

    def _p2i_sorted_ids(self):
        """Image ids per entry of p2i, each vertex's list in sorted() order (MVI:117).  Image order == sorted order whenever
        the ids are sorted (zero-padded frame numbers: always, in ScanNet exports); otherwise re-rank per vertex."""
        ids = self.image_ids
        if ids == sorted(ids):
            return self.p2i_indices
        rank = np.argsort(np.argsort(np.array(ids, dtype=object), kind="stable"), kind="stable")   # image -> rank in sorted()
        r = rank[self.p2i_indices]
        row = np.repeat(np.arange(self.n_points), np.diff(self.p2i_offsets))
        order = np.lexsort((r, row))
        return self.p2i_indices[order]

    def to_dict(self) -> Dict[str, dict]:
        """The reference's nested dict.  131 k small lists and 0.6 M references per scene are created here; the cyclic
        collector is paused meanwhile (none of these objects can form a cycle, and its generation-0 passes otherwise take
        more than half of the time)."""
        import gc
        was_enabled = gc.isenabled()
        gc.disable()
        try:
            return self._to_dict()
        finally:
            if was_enabled:
                gc.enable()

    def _to_dict(self) -> Dict[str, dict]:
        off = self.i2p_offsets.tolist()
        flat = self.i2p_indices.tolist()
        image_to_points = {img: flat[off[k]:off[k + 1]] for k, img in enumerate(self.image_ids)}
        ids_obj = np.array(self.image_ids, dtype=object)
        pflat = ids_obj[self._p2i_sorted_ids()].tolist() if len(self.p2i_indices) else []
        poff = self.p2i_offsets.tolist()
        point_to_images = {v: pflat[poff[v]:poff[v + 1]] for v in range(self.n_points)}
        return {"image_to_points": image_to_points, "point_to_images": point_to_images}

    def to_arrow(self, scene_id: str):
        """pyarrow table (key: string, values: string), image_to_points rows first -- the order and the text of
        ``visibility_dict_to_frame``.  The JSON text is written by libmspa's host-side formatters straight into arrow's
        (offsets, data) buffers: no Python object per row, no intermediate string arrays."""
        import pyarrow as pa
        from . import _lib
        lib = _lib.load()

        def string_array(n, text, offsets, nbytes):
            if nbytes < 0:
                _lib.check(int(nbytes))
            return pa.StringArray.from_buffers(n, pa.py_buffer(offsets), pa.py_buffer(text[:nbytes]))

        def ptr(a):
            return a.ctypes.data if a.size else None

        F, N = len(self.image_ids), self.n_points

        def preformatted(n, pair):
            offs, data = pair
            return pa.StringArray.from_buffers(n, pa.py_buffer(offs), pa.py_buffer(data)) if n else pa.array([], type=pa.string())

        if self.i2p_text is not None and self.p2i_text is not None:
            i2p_vals, p2i_vals = preformatted(F, self.i2p_text), preformatted(N, self.p2i_text)
        else:
            i2p_vals, p2i_vals = self._format_on_host(lib, string_array, ptr, pa)
        return pa.table({"key": self._key_column(scene_id), "values": pa.concat_arrays([i2p_vals, p2i_vals])})

    def _key_column(self, scene_id: str):
        """The ``key`` column: image_to_points rows first."""
        import pyarrow as pa
        from . import _lib
        lib = _lib.load()
        N = self.n_points
        i2p_keys = pa.array([f"{scene_id}:image_to_points:{i}" for i in self.image_ids], type=pa.string())
        prefix = f"{scene_id}:point_to_images:".encode()
        cap = (len(prefix) + 21) * N + 16
        text, offs = np.empty(cap, dtype=np.uint8), np.empty(N + 1, dtype=np.int32)
        nb = lib.mspa_format_int_keys_host(prefix, 0, N, text.ctypes.data, cap, offs.ctypes.data) if N else 0
        if nb < 0:
            _lib.check(int(nb))
        p2i_keys = (pa.StringArray.from_buffers(N, pa.py_buffer(offs), pa.py_buffer(text[:nb])) if N
                    else pa.array([], type=pa.string()))
        return pa.concat_arrays([i2p_keys, p2i_keys])

    def to_row_group(self, scene_id: str) -> bytes:
        """This scene's row group as a self-contained one-row-group parquet file (what ``SplicedParquetWriter.append`` takes).
        With ``values_pages`` (the device encoded the values chunk: ``from_bits(..., pages=True)``) only the ``key`` column goes
        through pyarrow and the file is put together by ``parquet_splice.assemble_row_group``; otherwise it is pyarrow's encode
        of ``to_arrow`` -- the same schema, so one file may hold row groups of both kinds."""
        import pyarrow as pa
        from . import parquet_splice
        if self.values_pages is None:
            return parquet_splice.encode_row_group(self.to_arrow(scene_id), use_dictionary=False)
        pg = self.values_pages
        return parquet_splice.assemble_row_group(pa.table({"key": self._key_column(scene_id)}), "values", pg["chunk"], pg["compressed"],
                                                 pg["uncompressed"], pg["num_values"], use_dictionary=False)

    def quoted_image_ids(self) -> List[bytes]:
        return [json.dumps(i).encode() for i in self.image_ids]

    def _format_on_host(self, lib, string_array, ptr, pa):
        """Both value columns by libmspa's host formatters (sequential loops: ~40 ms of one core per 320-frame scene)."""
        F, N = len(self.image_ids), self.n_points
        i2p_off = np.ascontiguousarray(self.i2p_offsets, dtype=np.int64)
        i2p_idx = np.ascontiguousarray(self.i2p_indices, dtype=np.int32)
        p2i_off = np.ascontiguousarray(self.p2i_offsets, dtype=np.int64)
        p2i_idx = np.ascontiguousarray(self._p2i_sorted_ids(), dtype=np.int32)
        # values of image_to_points: integer lists
        cap = 2 * F + 13 * len(i2p_idx) + 16
        text, offs = np.empty(cap, dtype=np.uint8), np.empty(F + 1, dtype=np.int32)
        nb = lib.mspa_format_int_lists_host(ptr(i2p_off), ptr(i2p_idx), F, text.ctypes.data, cap, offs.ctypes.data) if F else 0
        i2p_vals = string_array(F, text, offs, nb) if F else pa.array([], type=pa.string())
        # values of point_to_images: lists of quoted image ids
        quoted = self.quoted_image_ids()
        tok_off = np.concatenate([[0], np.cumsum([len(q) for q in quoted])]).astype(np.int32)
        tokens = np.frombuffer(b"".join(quoted) or b"\0", dtype=np.uint8)
        longest = max([len(q) for q in quoted], default=0)
        cap = 2 * N + (longest + 2) * len(p2i_idx) + 16
        text, offs = np.empty(cap, dtype=np.uint8), np.empty(N + 1, dtype=np.int32)
        nb = lib.mspa_format_token_lists_host(ptr(p2i_off), ptr(p2i_idx), N, tokens.ctypes.data, tok_off.ctypes.data, F,
                                              text.ctypes.data, cap, offs.ctypes.data) if N else 0
        p2i_vals = string_array(N, text, offs, nb) if N else pa.array([], type=pa.string())
        return i2p_vals, p2i_vals


def from_bits(bits, image_ids: List[str], n_points: int, text: bool = False, indices: bool = True, pages: bool = False,
              page_bytes: int = 1 << 20) -> VisibilityCSR:
    """K1's bitsets [F, ceil(N/64)] (device int64 tensor) -> both CSR tables, compacted on the device.
    ``text``: also write both lists' JSON text on the device (K10) and bring it along as arrow string buffers -- what
    ``to_arrow`` then uses (only when the image ids are in sorted() order, MVI:117: always, for ScanNet's zero-padded frame
    numbers).  ``indices=False``: the index arrays themselves stay on the device (a parquet sweep that keeps nothing needs only
    the text: 83 MB instead of 83 + 39).  ``pages`` (with ``text``): the text stays on the device too -- K12 turns it into the
    ``values`` column chunk's Snappy-compressed data pages (of ``page_bytes`` PLAIN bytes) and only those come along, as
    ``values_pages``; image ids that are not sorted, or 2 GiB of text, fall back to ``text``."""
    from . import engine
    F = len(image_ids)
    if F == 0 or n_points == 0:
        return VisibilityCSR(list(image_ids), n_points, np.zeros(F + 1, np.int64), np.zeros(0, np.int32),
                             np.zeros(n_points + 1, np.int64), np.zeros(0, np.int32))
    import torch
    o1, i1 = engine.bitset_csr(bits)
    t = engine.bits_transpose(bits)                      # [n_words * 64, ceil(F / 64)]; rows >= N are padding (all zero)
    o2, i2 = engine.bitset_csr(t[:n_points].contiguous() if t.shape[0] != n_points else t)
    ids = list(image_ids)
    text = text and ids == sorted(ids)
    want = [o1, i1 if indices or not text else None, o2, i2 if indices or not text else None]
    encoded = None
    if text:
        csr0 = VisibilityCSR(ids, n_points, None, None, None, None)
        t1, t2 = engine.format_lists_device(o1, i1), engine.format_lists_device(o2, i2, csr0.quoted_image_ids())
        if pages and t1[0].numel() + t2[0].numel() <= 0x7fffffff:
            # one string column, image_to_points rows first (as to_arrow concatenates them) -> its data pages, on the device
            offsets = torch.cat([t1[1][:-1], t2[1] + t1[0].numel()])
            encoded = engine.parquet_string_pages_device(offsets, torch.cat([t1[0], t2[0]]), page_bytes)
            want.append(encoded.pop("chunk"))
        else:
            want += list(t1[::-1]) + list(t2[::-1])
    # ~100 MB per 320-frame scene: into pinned blocks (torch's caching host allocator), all copies behind ONE wait on the
    # CURRENT stream -- the sweeps call this on an encoder thread with a stream of its own, next to the sweep thread's kernels
    host = []
    for a in want:
        if a is None:
            host.append(None)
            continue
        h = torch.empty(a.shape, dtype=a.dtype, pin_memory=True)
        h.copy_(a, non_blocking=True)
        host.append(h)
    torch.cuda.current_stream(bits.device).synchronize()
    host = [None if h is None else h.numpy() for h in host]
    csr = VisibilityCSR(ids, n_points, *host[:4])
    if encoded is not None:
        csr.values_pages = dict(encoded, chunk=host[4])
    elif text:
        csr.i2p_text, csr.p2i_text = (host[4], host[5]), (host[6], host[7])
    return csr


def _uleb128(v: int) -> bytes:
    out = bytearray()
    while True:
        out.append((v & 0x7F) | (0x80 if v > 0x7F else 0))
        v >>= 7
        if not v:
            return bytes(out)


class _Page(NamedTuple):
    """One page ``SceneRowGroups.scene_bits`` uploads: page ``index`` of row group ``group``'s ``values_pages`` table."""
    group: int
    index: int
    data: np.ndarray          # its bytes as they lie in the file (uint8, ``compressed`` of them)
    src: int                  # where they start in the upload: the pages' bytes back to back
    compressed: int
    uncompressed: int
    num_values: int
    snappy: bool              # False: the chunk is not compressed
    rows: np.ndarray          # the wanted rows as value numbers inside the page (its first row is 0), ascending
    # page_kinds "any" only (a "plain" plan leaves the defaults).  ``kind``: _PLAIN_PAGE, _DICT_CODED (a data page of dictionary
    # indices) or _DICTIONARY (the chunk's dictionary page: no rows; ``num_values`` = its entries); ``dictionary``: where a
    # _DICT_CODED page's dictionary page stands in the plan; ``v2``: a DATA_PAGE_V2 -- ``data`` / ``src`` / the sizes are then
    # those of the values part alone, behind the level bytes the host has checked
    kind: int = 0
    dictionary: int = -1
    v2: bool = False


_PLAIN_PAGE, _DICT_CODED, _DICTIONARY = range(3)


# the rows of the page table ``scene_bits`` sends to the device (one column per page, one more for the running sums' ends)
_SRC, _COMPRESSED, _UNCOMPRESSED, _PAYLOAD, _VALUES, _ROW_BEGIN = range(6)


class _DeviceRows(NamedTuple):
    """What ``SceneRowGroups._rows_on_device`` hands ``scene_bits`` and ``scene_lists``."""
    present: list             # the requested ids the file has, in request order
    order: list               # per present id: its row in ``got``'s tables (the distinct rows in (row group, row) order)
    payloads: object          # the decompressed pages, on the device (the declined rows' texts are read back from them)
    got: Optional[dict]       # ``engine.index_spans_to_bits``' or ``index_spans_to_lists``' dict


def column_chunk_pages(path: str, col, who: str = "parquet", chunk_name: str = "column chunk", mark=None, file=None) -> tuple:
    """THE walk of one column chunk's thrift page headers (``parquet_splice._Reader``), for any column: ``col`` is pyarrow's
    ``ColumnChunkMetaData`` of a chunk of the parquet file at ``path`` (``file``: that file, already open for reading).  Returns
    (table, the chunk's bytes as they lie in the file).  The table: ``start`` (the chunk's position in the file), ``bytes`` (its
    compressed size), ``codec`` (the chunk's, as pyarrow names it) and, per page in file order, int64 arrays ``pos`` (the
    payload's position inside the chunk), ``compressed``, ``uncompressed``, ``num_values``, ``type``, ``encoding`` (-1 where
    the page has none), ``levels`` (a v1 data page's definition-level encoding, else -1) and ``first_row`` (rows of the group
    in front of it; ``n_pages + 1`` entries); ``dict_values`` (a dictionary page's entry count, else 0 -- ``num_values`` stays
    0 there: a dictionary page holds no row) and, for v2 data pages, ``def_bytes`` / ``rep_bytes`` (the level bytes that lie
    uncompressed in front of the values), ``num_nulls`` and ``is_compressed`` (0 / 0 / 0 / 1 for every other page); ``chunk``
    None (the bytes are the caller's to keep or drop).  ``mark(stage)``: a stage clock, called after the read ("file_read") and
    after the walk ("header_walk").  A chunk that ends beyond the file, or headers that do not add up to it, raise ValueError
    (``who`` and ``chunk_name`` word the message)."""
    from . import parquet_splice as PS
    start = col.data_page_offset
    if col.has_dictionary_page and col.dictionary_page_offset:
        start = min(start, col.dictionary_page_offset)
    size = col.total_compressed_size
    if file is None:
        with open(path, "rb") as f:
            f.seek(start)
            chunk = f.read(size)
    else:
        file.seek(start)
        chunk = file.read(size)
    if len(chunk) != size:
        raise ValueError(f"{who}: the {chunk_name} ends beyond the file")
    if mark is not None:
        mark("file_read")
    rows, more, p = [], [], 0
    while p < size:
        r = PS._Reader(chunk, p)
        h = r.struct()
        v1, v2, dic = PS._get(h, 5), PS._get(h, 8), PS._get(h, 7)
        body = v1 or v2 or dic or []
        comp = PS._get(h, 3)
        rows.append((r.p, comp, PS._get(h, 2), PS._get(body, 1, 0) if (v1 or v2) else 0, PS._get(h, 1),
                     PS._get(body, 4 if v2 else 2, -1) if body else -1, PS._get(v1, 3, -1) if v1 else -1))
        more.append((PS._get(dic, 1, 0) if dic else 0, PS._get(v2, 5, 0) if v2 else 0, PS._get(v2, 6, 0) if v2 else 0,
                     PS._get(v2, 2, 0) if v2 else 0, int(bool(PS._get(v2, 7, True))) if v2 else 1))
        p = r.p + comp
    if p != size:
        raise ValueError(f"{who}: the page headers do not add up to the {chunk_name}")
    t = np.array(rows, dtype=np.int64).reshape(-1, 7)
    m = np.array(more, dtype=np.int64).reshape(-1, 5)
    table = {"start": int(start), "bytes": int(size), "codec": str(col.compression), "pos": t[:, 0], "compressed": t[:, 1],
             "uncompressed": t[:, 2], "num_values": t[:, 3], "type": t[:, 4], "encoding": t[:, 5], "levels": t[:, 6],
             "first_row": np.concatenate([[0], np.cumsum(t[:, 3])]), "dict_values": m[:, 0], "def_bytes": m[:, 1], "rep_bytes": m[:, 2],
             "num_nulls": m[:, 3], "is_compressed": m[:, 4], "chunk": None}
    if mark is not None:
        mark("header_walk")
    return table, chunk


def index_reader_route(visibility_info_path: str) -> str:
    """Which reader a builder that uses the index's rows as lists (the depth builders) takes: "lists"
    (``SceneRowGroups.scene_lists``: ``MSPA_VISINDEX_DECODE=device`` and a parquet index) or "handler"
    (``VisibilityInfoHandler``: the switch unset, or a .pkl index).  A wrong value of the switch raises ``decode_mode``'s
    ValueError whatever the file is."""
    return "lists" if decode_mode() == "device" and str(visibility_info_path).endswith(".parquet") else "handler"


class IndexLists:
    """A scene's ``image_to_points`` rows as the LISTS the text holds -- ``len(row)`` and ``row[j]``, duplicates counted, in the
    text's order -- behind one interface in two forms: the device form (``values`` / ``offsets`` of
    ``engine.index_spans_to_lists`` stay on the GPU, ``pick`` is ``engine.index_lists_pick``; the rows the device declined
    are served from their text) and the host form (every row from its text: ``json.loads`` at first use, as
    ``VisibilityInfoHandler`` does per call).  ``present``: the requested ids the file has, in request order."""

    def __init__(self, scene_id: str, present: list, device, texts: Dict[str, str], values=None, offsets=None, row_of: Optional[Dict[str, int]] = None,
                 row_counts: Optional[np.ndarray] = None):
        self.scene_id, self.present, self.device = scene_id, list(present), device
        self.values, self.offsets = values, offsets
        self._texts = texts                       # image id -> JSON text of the rows served on the host
        self._row_of = row_of or {}               # image id -> row of values / offsets, for the others
        self._row_counts = row_counts
        self._parsed: Dict[str, object] = {}
        self._counts: Optional[np.ndarray] = None

    def _key_error(self, image_id):
        return ValueError(f"Key {self.scene_id}:image_to_points:{image_id} not found in visibility info.")

    def _host_list(self, image_id):
        if image_id not in self._parsed:
            self._parsed[image_id] = json.loads(self._texts[image_id])
        return self._parsed[image_id]

    def count(self, image_id) -> int:
        """``len`` of the image's list; an id the index lacks raises ``VisibilityInfoHandler``'s ValueError."""
        if image_id in self._texts:
            return len(self._host_list(image_id))
        if image_id not in self._row_of:
            raise self._key_error(image_id)
        return int(self._row_counts[self._row_of[image_id]])

    @property
    def counts(self) -> np.ndarray:
        """int64, one entry per present id."""
        if self._counts is None:
            self._counts = np.array([self.count(i) for i in self.present], dtype=np.int64)
        return self._counts

    def _range_error(self, image_id, vertex, n_points):
        return ValueError(f"visindex: scene {self.scene_id}, image {image_id}: vertex {vertex} of the visibility index lies outside "
                          f"[0, {n_points})")

    def pick(self, samples, n_points: int):
        """``[int(row(image_id)[position]) for image_id, position in samples]`` as an int32 tensor on ``device``, every vertex
        inside [0, n_points) -- it may index the scene's vertex table unchecked.  The first sample that is not: an id the
        index lacks raises ``count``'s ValueError, a position outside the list IndexError (``list[j]``), a vertex outside
        [0, n_points) ValueError.  Device form: one launch, one read-back of the status."""
        import torch
        samples = list(samples)
        n_points = int(n_points)
        errors: Dict[int, Exception] = {}
        on_host, on_device = {}, []
        for s, (image_id, position) in enumerate(samples):
            if image_id in self._texts:
                seen = self._host_list(image_id)
                if int(position) < 0:
                    errors[s] = IndexError("list index out of range")
                    continue
                try:
                    vertex = int(seen[position])
                except IndexError as e:
                    errors[s] = e
                    continue
                if 0 <= vertex < n_points:
                    on_host[s] = vertex
                else:
                    errors[s] = self._range_error(image_id, vertex, n_points)
            elif image_id in self._row_of:
                on_device.append(s)
            else:
                errors[s] = self._key_error(image_id)
        if errors and not on_device:
            raise errors[min(errors)]
        if not on_device:
            return torch.tensor([on_host[s] for s in range(len(samples))], dtype=torch.int32).to(self.device)
        from . import _lib, engine
        table = torch.tensor([[self._row_of[samples[s][0]], int(samples[s][1])] for s in on_device], dtype=torch.int64).to(self.device)
        vertex, status = engine.index_lists_pick(self.values, self.offsets, table, n_points)
        status = status.cpu().numpy()                                          # THE read-back: nothing leaves unchecked
        for k in np.nonzero(status)[0][:1]:                                    # the first one in sample order
            s = on_device[int(k)]
            image_id, position = samples[s]
            code = int(status[k])
            if code == _lib.PICK_EPOSITION:
                errors[s] = IndexError("list index out of range")
            elif code == _lib.PICK_ERANGE:
                at = int(self.offsets[self._row_of[image_id]].item()) + int(position)
                errors[s] = self._range_error(image_id, int(self.values[at].item()), n_points)
            else:
                errors[s] = RuntimeError(f"visindex: scene {self.scene_id}, image {image_id}: pick status {code} (the list tables are damaged)")
        if errors:
            raise errors[min(errors)]
        if not on_host:
            return vertex
        out = torch.empty((len(samples),), dtype=torch.int32, device=vertex.device)
        out[torch.tensor(on_device, dtype=torch.int64, device=vertex.device)] = vertex
        out[torch.tensor(list(on_host), dtype=torch.int64, device=vertex.device)] = torch.tensor(list(on_host.values()), dtype=torch.int32,
                                                                                               device=vertex.device)
        return out


class SceneRowGroups:
    """Scene-addressable reader of the visibility-index parquet (columns ``key`` = "scene:kind:item", ``values`` = JSON text;
    MVI:38-73): which row groups hold which scene is read off the ``key`` column's min / max statistics in the footer, so a rank
    of a sharded job loads the rows of ITS scenes only -- the reference loads the whole table (13 GB for the train split) into a
    dict in every process (COVIS:60-70, IH:486-500).  A row group whose keys span several scenes (files written with pandas'
    default 1 M-row groups) is read once and kept.  ``scene_dict(scene_id)`` -> {key: JSON text} of that scene."""

    def __init__(self, parquet_file: str):
        import pyarrow.parquet as pq
        self.file = pq.ParquetFile(parquet_file)
        md = self.file.metadata
        key_col = self.file.schema_arrow.get_field_index("key")
        self._by_scene: Dict[str, List[int]] = {}
        self._mixed: List[tuple] = []                       # (row group, first scene, last scene)
        self._cache: Dict[int, Dict[str, Dict[str, str]]] = {}
        # what ``scene_bits`` needs besides: the file itself (raw page bytes), where ``values`` sits and how it is nested
        self._path = os.fspath(parquet_file) if isinstance(parquet_file, (str, os.PathLike)) else None
        self._values_col = self.file.schema_arrow.get_field_index("values")
        self._page_tables: Dict[int, dict] = {}
        self._keys: Dict[int, object] = {}
        self.decode_stats = {"scenes": 0, "scenes_declined": 0, "rows": 0, "rows_declined": 0, "h2d_bytes": 0, "blocks": 0,
                             "serial_streams": 0, "dict_pages": 0, "v2_pages": 0}
        self.decode_by_blocks = True      # False: every page by the one-wave kernel (tools/visindex_decode_bench.py times both)
        self.last_decline: Optional[str] = None
        self.stage_times: Optional[dict] = None
        self._stage_start = 0.0
        self._has_levels, self._device_schema = False, False
        if self._values_col >= 0 and self.file.metadata.num_columns == len(self.file.schema_arrow.names):
            leaf = self.file.schema.column(self._values_col)
            self._has_levels = leaf.max_definition_level == 1
            self._device_schema = (leaf.physical_type == "BYTE_ARRAY" and leaf.max_repetition_level == 0 and leaf.max_definition_level <= 1)
        for g in range(md.num_row_groups):
            st = md.row_group(g).column(key_col).statistics
            if st is None or not st.has_min_max:
                self._mixed.append((g, "", "\U0010ffff"))
                continue
            lo, hi = str(st.min).split(":", 1)[0], str(st.max).split(":", 1)[0]
            if lo == hi:
                self._by_scene.setdefault(lo, []).append(g)
            else:
                self._mixed.append((g, lo, hi))

    # ------------------------------------------------------------------------------------------------ pages -> bitsets, on the device
    # parquet.thrift numbers
    _DATA_PAGE, _PLAIN, _RLE = 0, 0, 3
    _DICTIONARY_PAGE, _DATA_PAGE_V2, _PLAIN_DICTIONARY, _RLE_DICTIONARY = 2, 3, 2, 8
    _CODECS = {"UNCOMPRESSED": 0, "SNAPPY": 1}
    # which of a scene's needed pages ``scene_bits`` takes.  "plain": v1 DATA_PAGEs with PLAIN values only -- any other needed
    # page sends the whole scene to the host path.  "any" (what the readers set with MSPA_VISINDEX_DECODE=device): dictionary-coded
    # data pages (RLE_DICTIONARY, PLAIN_DICTIONARY) behind their chunk's dictionary page and DATA_PAGE_V2 as well -- the
    # layouts of pyarrow's defaults, of version="1.0" and of data_page_version="2.0"
    page_kinds = "plain"

    def values_pages(self, g: int) -> dict:
        """The page table of row group ``g``'s ``values`` column chunk: ``column_chunk_pages``' table (which see), with the
        chunk's bytes under ``chunk`` at the call that walks the headers.  Cached: a few numbers per page, not the bytes."""
        if g in self._page_tables:
            return self._page_tables[g]
        if self._path is None:
            raise ValueError("visindex: the page table needs the index as a file on disk")
        table, chunk = column_chunk_pages(self._path, self.file.metadata.row_group(g).column(self._values_col), "visindex", "values chunk",
                                          self._mark)
        self._page_tables[g] = table
        table = dict(table, chunk=chunk)                      # the bytes go to this caller only: the cache keeps numbers
        return table

    def _group_keys(self, g: int, keep: bool):
        """Row group ``g``'s ``key`` column as one arrow array (kept for groups that several scenes share)."""
        if g in self._keys:
            return self._keys[g]
        keys = self.file.read_row_group(g, columns=["key"]).column("key").combine_chunks()
        if keep:
            self._keys[g] = keys
        return keys

    def image_rows(self, scene_id: str, image_ids) -> Dict[int, tuple]:
        """{position in ``image_ids``: (row group, row in the group)} of the ``scene:image_to_points:image`` rows the index has --
        the ``key`` column is matched with arrow compute, no Python string per row.  A key that several row groups hold
        resolves to the group ``scene_dict`` lets win (the last one read)."""
        import pyarrow as pa
        import pyarrow.compute as pc
        wanted = pa.array([f"{scene_id}:image_to_points:{i}" for i in image_ids], type=pa.string())
        groups = [(g, False) for g in self._by_scene.get(scene_id, [])] + [(g, True) for g, lo, hi in self._mixed if lo <= scene_id <= hi]
        found: Dict[int, tuple] = {}
        for g, keep in groups:
            keys = self._group_keys(g, keep)
            if keys.type != wanted.type:
                keys = keys.cast(wanted.type)
            at = pc.index_in(wanted, value_set=keys).fill_null(-1).to_numpy(zero_copy_only=False)
            for k in np.nonzero(at >= 0)[0]:
                found[int(k)] = (g, int(at[k]))
        return found

    def needed_pages(self, g: int, rows) -> tuple:
        """(page table of group ``g`` with its chunk's bytes, page index of every row of ``rows``, reason) -- ``reason`` is None
        when the device path takes every page these rows lie in: v1 DATA_PAGE, PLAIN, codec SNAPPY or none, RLE definition
        levels; otherwise it says what is in the way (a dictionary page in front does not matter by itself, dictionary-encoded
        data pages do).  With ``page_kinds = "any"`` dictionary-coded and v2 pages are taken too (``_any_reason``)."""
        table = self.values_pages(g)
        if table["chunk"] is None:
            with open(self._path, "rb") as f:
                f.seek(table["start"])
                table = dict(table, chunk=f.read(table["bytes"]))
            self._mark("file_read")
        rows = np.asarray(rows, dtype=np.int64)
        data = np.nonzero((table["type"] == 0) | (table["type"] == 3))[0]               # the pages that hold rows
        page = data[np.searchsorted(table["first_row"][data + 1], rows, side="right").clip(max=max(len(data) - 1, 0))] if len(data) else None
        reason = None
        if page is None or bool((rows >= table["first_row"][-1]).any()):
            return table, page, "rows beyond the chunk's pages"
        used = np.unique(page)
        if self.page_kinds != "plain":
            if self.page_kinds != "any":
                raise ValueError(f"visindex: page_kinds {self.page_kinds!r}: expected 'plain' or 'any'")
            return table, page, self._any_reason(table, used)
        if table["codec"] not in self._CODECS:
            reason = f"codec {table['codec']}"
        elif bool((table["type"][used] != self._DATA_PAGE).any()):
            reason = "a data page that is not v1"
        elif bool((table["encoding"][used] != self._PLAIN).any()):
            reason = "a data page that is not PLAIN"
        elif self._has_levels and bool((table["levels"][used] != self._RLE).any()):
            reason = "definition levels that are not RLE"
        elif int(table["uncompressed"][used].max()) > 0x7fffffff or int(table["compressed"][used].max()) > 0x7fffffff:
            reason = "a page of 2 GiB"
        return table, page, reason

    def _dictionary_page(self, table: dict) -> int:
        """The chunk's dictionary page (a chunk has at most one, in front of its data pages), or -1."""
        at = np.nonzero(table["type"] == self._DICTIONARY_PAGE)[0]
        return int(at[0]) if len(at) else -1

    def _any_reason(self, table: dict, used) -> Optional[str]:
        """``needed_pages``' verdict with ``page_kinds = "any"``: None when the data pages ``used`` are PLAIN or dictionary-coded
        (then behind a PLAIN dictionary page), v1 or v2, Snappy or uncompressed, without nulls and repetition levels."""
        kind, enc = table["type"][used], table["encoding"][used]
        if table["codec"] not in self._CODECS:
            return f"codec {table['codec']}"
        coded = (enc == self._RLE_DICTIONARY) | (enc == self._PLAIN_DICTIONARY)
        if bool(((enc != self._PLAIN) & ~coded).any()):
            return f"a data page with encoding {int(enc[(enc != self._PLAIN) & ~coded][0])}"
        sizes = used
        if bool(coded.any()):
            d = self._dictionary_page(table)
            if d < 0 or d > int(used[coded].min()) or int(table["encoding"][d]) not in (self._PLAIN, self._PLAIN_DICTIONARY):
                return "dictionary-coded pages without a PLAIN dictionary page in front"
            sizes = np.append(used, d)
        v1, v2 = used[kind == self._DATA_PAGE], used[kind == self._DATA_PAGE_V2]
        if self._has_levels and bool((table["levels"][v1] != self._RLE).any()):
            return "definition levels that are not RLE"
        if bool((table["num_nulls"][v2] != 0).any()):
            return "a v2 page with nulls"
        if bool((table["rep_bytes"][v2] != 0).any()):
            return "a v2 page with repetition levels"
        for k in v2:                       # the level bytes lie uncompressed in front of the values: one run of ones, no length prefix
            pos, n, nv = int(table["pos"][k]), int(table["def_bytes"][k]), int(table["num_values"][k])
            want = _uleb128(nv << 1) + b"\x01" if self._has_levels else b""
            if n > int(table["compressed"][k]) or bytes(table["chunk"][pos:pos + n]) != want:
                return "a v2 page whose definition levels are not one run of ones"
        if int(table["uncompressed"][sizes].max()) > 0x7fffffff or int(table["compressed"][sizes].max()) > 0x7fffffff:
            return "a page of 2 GiB"
        return None

    def _mark(self, stage: str):
        """The stage clock of tools/visindex_decode_bench.py: off unless ``stage_times`` is a dict, then every stage ends with a
        device synchronise and its wall time is added under its name."""
        if self.stage_times is None:
            return
        import time
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        now = time.perf_counter()
        self.stage_times[stage] = self.stage_times.get(stage, 0.0) + now - self._stage_start
        self._stage_start = now

    def _decline(self, why: str):
        self.decode_stats["scenes_declined"] += 1
        self.last_decline = why

    def _scene_bits_host(self, scene_id: str, image_ids, n_points, device):
        """Today's path: ``scene_dict`` -> ``json.loads`` -> ``scene.pack_index_lists`` -> upload."""
        import torch
        from .scene import pack_index_lists
        texts = self.scene_dict(scene_id)
        present = [i for i in image_ids if f"{scene_id}:image_to_points:{i}" in texts]
        lists = [json.loads(texts[f"{scene_id}:image_to_points:{i}"]) for i in present]
        if n_points is None:
            n_points = max((max(seen) for seen in lists if len(seen)), default=0) + 1
        return present, torch.from_numpy(pack_index_lists(lists, int(n_points))).to(device)

    def _plan_pages(self, distinct: List[tuple]):
        """``scene_bits`` step 1, on the host alone: the wanted (row group, row), ascending -> (the ``_Page``s that hold them, in
        that order, None), or (None, why the device path does not take them).  With ``page_kinds = "any"`` the dictionary
        pages of the dictionary-coded pages follow, once each, behind every data page."""
        pages, upload, dictionaries = [], 0, {}
        for g in sorted({g for g, _ in distinct}):
            rows = np.array([r for gg, r in distinct if gg == g], dtype=np.int64)
            table, page, reason = self.needed_pages(g, rows)
            if reason is not None:
                return None, f"row group {g}: {reason}"
            chunk = memoryview(table["chunk"])
            snappy = self._CODECS[table["codec"]] == 1
            for pg in np.unique(page):
                pos, comp = int(table["pos"][pg]), int(table["compressed"][pg])
                kind = _PLAIN_PAGE if int(table["encoding"][pg]) == self._PLAIN else _DICT_CODED
                lev = int(table["def_bytes"][pg]) + int(table["rep_bytes"][pg])          # 0 but for v2 pages
                if kind == _DICT_CODED and g not in dictionaries:
                    d = self._dictionary_page(table)
                    at, n = int(table["pos"][d]), int(table["compressed"][d])
                    dictionaries[g] = _Page(g, d, np.frombuffer(chunk[at:at + n], dtype=np.uint8), 0, n, int(table["uncompressed"][d]),
                                            int(table["dict_values"][d]), snappy, np.zeros(0, np.int64), _DICTIONARY)
                pages.append(_Page(g, int(pg), np.frombuffer(chunk[pos + lev:pos + comp], dtype=np.uint8), upload, comp - lev,
                                   int(table["uncompressed"][pg]) - lev, int(table["num_values"][pg]),
                                   snappy and bool(table["is_compressed"][pg]), rows[page == pg] - int(table["first_row"][pg]), kind,
                                   g if kind == _DICT_CODED else -1, int(table["type"][pg]) == self._DATA_PAGE_V2))
                upload += comp - lev
        # the dictionary pages stand behind every data page, so that the data pages keep their places in the tables
        n_data = len(pages)
        for g, d in dictionaries.items():
            pages[:n_data] = [p._replace(dictionary=len(pages)) if p.kind == _DICT_CODED and p.group == g else p for p in pages[:n_data]]
            pages.append(d._replace(src=upload))
            upload += d.compressed
        if self._has_levels and len({p.v2 for p in pages[:n_data]}) == 2:
            return None, "v1 pages with levels and v2 pages in one scene"
        if sum(p.uncompressed for p in pages) > 0x7fffffff:
            return None, "2 GiB of pages or more"
        return pages, None

    def _decompress_pages(self, src, pages: List[_Page], tab_dev):
        """``scene_bits`` step 3: the uploaded pages -> (their payloads back to back, the Snappy streams' status or None for none,
        their routes or None for the one-wave kernel's).  An uncompressed page has ``compressed == uncompressed``."""
        import torch
        from . import engine
        n_pages = len(pages)

        def decompress(sel):                                           # the pages ``sel`` of the table; None: all of them
            offs, sizes, unc = (tab_dev[r, :n_pages].contiguous() if sel is None else tab_dev[r].index_select(0, sel)
                                for r in (_SRC, _COMPRESSED, _UNCOMPRESSED))
            if not self.decode_by_blocks:
                return (*engine.snappy_decompress_device(src, offs, sizes, unc), None)
            return engine.snappy_decompress_blocks_device(src, offs, sizes, unc)

        snappy = np.array([k for k, p in enumerate(pages) if p.snappy], dtype=np.int64)
        if len(snappy) == n_pages:
            payloads, _, status, route = decompress(None)
            return payloads, status, route
        # uncompressed chunks (and files that mix both): plain copies
        unc_total = sum(p.uncompressed for p in pages)
        payloads = torch.empty((max(unc_total, 1),), dtype=torch.uint8, device=src.device)[:unc_total]
        status = route = None
        if len(snappy):
            part, part_off, status, route = decompress(torch.from_numpy(snappy).to(src.device))
            part_off = part_off.cpu().numpy()
        at = 0
        for k, p in enumerate(pages):
            if p.snappy:
                j = int(np.searchsorted(snappy, k))
                payloads[at:at + p.uncompressed] = part[int(part_off[j]):int(part_off[j]) + p.uncompressed]
            else:
                payloads[at:at + p.uncompressed] = src[p.src:p.src + p.compressed]
            at += p.uncompressed
        return payloads, status, route

    def _mixed_row_spans(self, payloads, pages: List[_Page], tab, has_levels: bool, device):
        """``scene_bits`` step 4 for a plan with dictionary-coded pages: the dictionary pages' entries -> a span table
        (``engine.parquet_plain_spans_device`` without levels, every entry a row); the dictionary-coded pages' rows -> spans
        through it (``engine.parquet_dict_spans_device``); the PLAIN pages' rows -> spans as ever; both merged into the one
        row-ordered span table ``engine.index_spans_to_bits`` / ``index_spans_to_lists`` take.  Returns (start, length, page
        status of every call's pages), on the device."""
        import torch
        from . import engine

        def tables(kind, rows_of):
            """(which pages, device tensors: payload offsets, sizes, values, row_begin, row_index) of the pages of ``kind``."""
            which = [k for k, p in enumerate(pages) if p.kind == kind]
            rows = [rows_of(pages[k]) for k in which]
            row_begin = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
            row_index = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
            host = [tab[_PAYLOAD, which], tab[_UNCOMPRESSED, which], tab[_VALUES, which], row_begin, row_index]
            return which, [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device) for a in host]

        def slots(which):                                              # the rows of these pages in the scene's row table
            return torch.from_numpy(np.concatenate([np.arange(tab[_ROW_BEGIN, k], tab[_ROW_BEGIN, k + 1]) for k in which]).astype(np.int64)).to(device)

        n_rows = int(tab[_ROW_BEGIN, -1])
        start, length = (torch.zeros((n_rows,), dtype=torch.int64, device=device) for _ in range(2))
        status = []
        dictionaries, t = tables(_DICTIONARY, lambda p: np.arange(p.num_values))
        dict_start, dict_length, st = engine.parquet_plain_spans_device(payloads, *t, has_levels=False)
        status.append(st)
        dict_begin = dict(zip(dictionaries, np.concatenate([[0], np.cumsum(tab[_VALUES, dictionaries])])[:-1]))
        coded, t = tables(_DICT_CODED, lambda p: p.rows)
        begin = torch.tensor([int(dict_begin[pages[k].dictionary]) for k in coded], dtype=torch.int64, device=device)
        count = torch.tensor([pages[pages[k].dictionary].num_values for k in coded], dtype=torch.int64, device=device)
        _, a, n, st, _code = engine.parquet_dict_spans_device(payloads, *t, begin, count, dict_start, dict_length, has_levels=has_levels)
        at = slots(coded)
        start[at], length[at] = a, n
        status.append(st)
        plain, t = tables(_PLAIN_PAGE, lambda p: p.rows)
        if plain:
            a, n, st = engine.parquet_plain_spans_device(payloads, *t, has_levels=has_levels)
            at = slots(plain)
            start[at], length[at] = a, n
            status.append(st)
        return start, length, torch.cat(status)

    def _repair_rows(self, got: dict, payloads, n_points):
        """``scene_bits`` step 5: the rows the device declined get their text back from the device's pages and take the host path --
        ``json.loads``, ``pack_index_lists`` -- into ``got["bits"]`` (widened where ``n_points`` is None and they say so)."""
        import torch
        from .scene import pack_index_lists
        bits, width = got["bits"], got["n_points"]
        declined = np.nonzero(got["row_status"])[0]
        if not len(declined):
            return bits
        self.decode_stats["rows_declined"] += len(declined)
        which = torch.from_numpy(declined).to(bits.device)
        spans = torch.stack([got["start"], got["length"]])[:, which].cpu().numpy()
        lists = [json.loads(bytes(payloads[int(a):int(a) + int(n)].cpu().numpy()).decode()) for a, n in zip(spans[0], spans[1])]
        if n_points is None:
            # the width comes from every list.  The device's figure covers every value it parsed (a row it declined for its
            # order included; a row its parser declined counts as 0 there), these lists are the rest
            width = max(width, max((max(seen) for seen in lists if len(seen)), default=0) + 1)
        n_words = (width + 63) // 64
        if n_words != bits.shape[1]:
            wider = torch.zeros((bits.shape[0], n_words), dtype=torch.int64, device=bits.device)
            wider[:, :min(n_words, bits.shape[1])] = bits[:, :n_words]
            bits = wider
        bits[which] = torch.from_numpy(pack_index_lists(lists, width)).to(bits.device)
        return bits

    def scene_bits(self, scene_id: str, image_ids, n_points: Optional[int] = None, device="cuda"):
        """(present ids, bits): the requested image ids the index has, in request order, and their visible-vertex bitsets as an
        int64 device tensor [len(present), ceil(n_points / 64)] -- ``scene.pack_index_lists``' layout; ``n_points`` None: 1 + the
        largest index in these lists.

        The rows go from the file to the device as their pages lie there: the ``values`` chunk's page headers are walked on
        the host, the ``key`` column says which rows are wanted, only the pages that hold them are uploaded (compressed), and
        the device decompresses (``engine.snappy_decompress_blocks_device``: one wave per 64 KiB block of a page, the one-wave
        kernel for a page that is not cut that way), finds the rows, parses the lists and sets the bits
        (``engine.index_rows_to_bits``).  Whatever the device path does not take -- a page that is not v1 / PLAIN / Snappy or
        uncompressed, a stream or a page it declines, a row that is not an ascending list inside ``n_points`` -- goes through
        ``json.loads`` and ``pack_index_lists``, so the result is the host path's for every input.  With ``page_kinds = "any"``
        dictionary-coded data pages (their dictionary page uploaded and decompressed with them, the rows' indices walked by
        ``engine.parquet_dict_spans_device``) and v2 data pages (level bytes checked here, the values part uploaded) are
        taken as well; ``decode_stats["dict_pages"]`` / ``["v2_pages"]`` count them.  ``decode_stats`` counts scenes,
        declined scenes, rows, declined rows, uploaded bytes, ``blocks`` (64 KiB blocks decoded in parallel) and ``serial_streams``
        (Snappy pages the one-wave kernel took); ``last_decline`` says why the last scene was declined."""
        import torch
        from . import engine
        image_ids = list(image_ids)
        self.decode_stats["scenes"] += 1
        rows = self._rows_on_device(scene_id, image_ids, device, "rows_to_bits",
                                    lambda payloads, start, length, status: engine.index_spans_to_bits(payloads, start, length, n_points, status))
        if isinstance(rows, str):
            self._decline(rows)
            return self._scene_bits_host(scene_id, image_ids, n_points, device)
        if not rows.present:
            n = 1 if n_points is None else int(n_points)
            return rows.present, torch.zeros((0, (n + 63) // 64), dtype=torch.int64, device=device)
        bits = self._repair_rows(rows.got, rows.payloads, n_points)
        order = torch.tensor(rows.order, dtype=torch.int64, device=bits.device)
        if len(order) != bits.shape[0] or not bool((order == torch.arange(len(order), device=bits.device)).all().item()):
            bits = bits.index_select(0, order)
        return rows.present, bits

    def _rows_on_device(self, scene_id: str, image_ids: list, device, stage: str, spans_to):
        """``scene_bits``' and ``scene_lists``' steps 1 - 4: the wanted rows (``image_rows``), the pages that hold them
        (``_plan_pages``), their upload, ``_decompress_pages`` and the rows' spans (PLAIN, or dictionary-coded and PLAIN merged),
        handed to ``spans_to(payloads, start, length, page_status)`` -- ``engine.index_spans_to_bits`` or ``index_spans_to_lists``
        -- whose dict comes back as ``got`` of a ``_DeviceRows``; ``stage`` names that call on the stage clock.  A str instead:
        why the device path does not take this scene (the caller declines it and takes the host path).  No present id: a
        ``_DeviceRows`` with nothing but the empty ``present``.  Counts everything in ``decode_stats`` but scenes and declines."""
        import torch
        from . import engine
        if self._path is None or not self._device_schema:
            return "not a file on disk" if self._path is None else "values is not a flat BYTE_ARRAY column"
        if self.stage_times is not None:
            import time
            self._stage_start = time.perf_counter()
        found = self.image_rows(scene_id, image_ids)
        self._mark("key_read")
        present_pos = sorted(found)
        present = [image_ids[k] for k in present_pos]
        if not present:
            return _DeviceRows(present, [], None, None)
        # the distinct rows, in (row group, row) order: what the device walks; the request refers to them by position
        distinct = sorted(set(found.values()))
        pages, why = self._plan_pages(distinct)
        if pages is None:
            return why
        n_pages, upload = len(pages), sum(p.compressed for p in pages)
        staged = torch.empty((max(upload, 1),), dtype=torch.uint8, pin_memory=True)
        if upload:
            np.concatenate([p.data for p in pages], out=staged.numpy()[:upload])
        src = staged.to(device, non_blocking=True)[:upload]
        self.decode_stats["h2d_bytes"] += upload
        self._mark("h2d")
        tab = np.zeros((6, n_pages + 1), dtype=np.int64)
        tab[_SRC, :n_pages] = [p.src for p in pages]
        tab[_COMPRESSED, :n_pages] = [p.compressed for p in pages]
        tab[_UNCOMPRESSED, :n_pages] = [p.uncompressed for p in pages]
        np.cumsum(tab[_UNCOMPRESSED, :n_pages], out=tab[_PAYLOAD, 1:])
        tab[_VALUES, :n_pages] = [p.num_values for p in pages]
        np.cumsum([len(p.rows) for p in pages], out=tab[_ROW_BEGIN, 1:])
        row_index = np.concatenate([p.rows for p in pages]).astype(np.int64)
        tab_dev = torch.from_numpy(tab).to(device)
        if any(not p.snappy and p.compressed != p.uncompressed for p in pages):
            return "an uncompressed page whose sizes differ"
        payloads, stream_status, route = self._decompress_pages(src, pages, tab_dev)
        self._mark("decompress")
        # the data pages open the tables (``_plan_pages``); dictionary pages, if any, stand behind them and hold no row
        n_data = sum(1 for p in pages if p.kind != _DICTIONARY)
        has_levels = self._has_levels and not any(p.v2 for p in pages)      # a v2 page's levels stayed on the host, checked
        if all(p.kind == _PLAIN_PAGE for p in pages):
            spans = engine.parquet_plain_spans_device(payloads, tab_dev[_PAYLOAD, :n_data].contiguous(), tab_dev[_UNCOMPRESSED, :n_data].contiguous(),
                                                      tab_dev[_VALUES, :n_data].contiguous(), tab_dev[_ROW_BEGIN, :n_data + 1].contiguous(),
                                                      torch.from_numpy(row_index).to(device), has_levels=has_levels)
        else:
            spans = self._mixed_row_spans(payloads, pages, tab, has_levels, device)
        got = spans_to(payloads, *spans)
        if (stream_status is not None and bool((stream_status != 0).any().item())) or bool(got["page_status"].any()):
            return "the device declined a page"
        self._mark(stage)
        if stream_status is not None:
            routes = route.cpu().numpy() if route is not None else np.zeros(len(stream_status), dtype=np.int32)
            self.decode_stats["blocks"] += int(routes.sum())
            self.decode_stats["serial_streams"] += int((routes == 0).sum())
        self.decode_stats["rows"] += len(distinct)
        self.decode_stats["dict_pages"] += sum(1 for p in pages if p.kind == _DICT_CODED)
        self.decode_stats["v2_pages"] += sum(1 for p in pages if p.v2)
        slot = {gr: k for k, gr in enumerate(distinct)}
        return _DeviceRows(present, [slot[found[k]] for k in present_pos], payloads, got)

    def _scene_lists_host(self, scene_id: str, image_ids: list, device) -> IndexLists:
        """The host form: the present rows' texts from ``scene_dict``."""
        texts = self.scene_dict(scene_id)
        present = [i for i in image_ids if f"{scene_id}:image_to_points:{i}" in texts]
        return IndexLists(scene_id, present, device, {i: texts[f"{scene_id}:image_to_points:{i}"] for i in present})

    def scene_lists(self, scene_id: str, image_ids, device="cuda") -> IndexLists:
        """The requested images' ``image_to_points`` rows as lists (``IndexLists``: ``count(image)``, ``pick([(image, position)],
        n_points)``) for the readers that take ``len(row)`` and ``row[j]`` -- a bitset answers neither for a row with a
        duplicate or out of order.  ``scene_bits``' way to the device up to the parsed lists (``_rows_on_device`` with
        ``engine.index_spans_to_lists``); ``values`` / ``offsets`` stay there.  A row the device declines (a '-', a non-digit,
        more than 10 digits, a leading zero, no [...]) gets its text back from the device's pages and is served through
        ``json.loads`` (``decode_stats["rows_declined"]``); a scene it does not take (a codec, a declined page, not a file on
        disk: ``scenes_declined``, ``last_decline``) comes in the host form, as does every scene with ``device="cpu"``."""
        image_ids = list(image_ids)
        self.decode_stats["scenes"] += 1
        if str(device) == "cpu":
            return self._scene_lists_host(scene_id, image_ids, "cpu")
        import torch
        from . import engine
        rows = self._rows_on_device(scene_id, image_ids, device, "rows_to_lists", engine.index_spans_to_lists)
        if isinstance(rows, str):
            self._decline(rows)
            return self._scene_lists_host(scene_id, image_ids, device)
        if not rows.present:
            return IndexLists(scene_id, [], device, {})
        got = rows.got
        row_of = dict(zip(rows.present, rows.order))
        texts: Dict[str, str] = {}
        declined = np.nonzero(got["row_status"])[0]
        if len(declined):                                          # their text back from the device's pages, as ``_repair_rows``
            self.decode_stats["rows_declined"] += len(declined)
            which = torch.from_numpy(declined).to(got["start"].device)
            spans = torch.stack([got["start"], got["length"]])[:, which].cpu().numpy()
            text_of = {int(r): bytes(rows.payloads[int(a):int(a) + int(n)].cpu().numpy()).decode() for r, a, n in zip(declined, spans[0], spans[1])}
            texts = {i: text_of[r] for i, r in row_of.items() if r in text_of}
            row_of = {i: r for i, r in row_of.items() if r not in text_of}
        return IndexLists(scene_id, rows.present, got["values"].device, texts, got["values"], got["offsets"], row_of, got["counts"])

    def _split_group(self, g: int) -> Dict[str, Dict[str, str]]:
        if g not in self._cache:
            t = self.file.read_row_group(g, columns=["key", "values"])
            per: Dict[str, Dict[str, str]] = {}
            for k, v in zip(t.column("key").to_pylist(), t.column("values").to_pylist()):
                per.setdefault(k.split(":", 1)[0], {})[k] = v
            self._cache[g] = per
        return self._cache[g]

    def scene_dict(self, scene_id: str) -> Dict[str, str]:
        out: Dict[str, str] = {}
        for g in self._by_scene.get(scene_id, []):
            t = self.file.read_row_group(g, columns=["key", "values"])
            out.update(zip(t.column("key").to_pylist(), t.column("values").to_pylist()))
        for g, lo, hi in self._mixed:
            if lo <= scene_id <= hi:
                out.update(self._split_group(g).get(scene_id, {}))
        return out
