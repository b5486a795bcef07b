"""What the search path keeps resident between calls, shared by io.index and io.coder.

* mmap'd Arrow tables, one per file version (io.arrow.load, arrow.py:6-8, is
  re-run by the reference on every search; here it is re-run only when the
  file's version (size, mtime, inode, rewrite count) changes — do_put rewrites invalidate it);
* single-chunk copies of small result columns for ``take`` (index.py:166);
* the HBM shards of embedding columns (engine.CACHE) and of index code
  columns (``__CODED_ID__``, int64 per row) used to build probe masks on the
  device;
* the scalar columns a row filter reads (``pred_column``), staged whole per
  device for fx_pred_eval and accounted in ``engine.RESIDENT``.
"""

from __future__ import annotations

import os
import threading
from typing import Dict, List, Sequence, Tuple

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import torch

from .. import engine as _engine
from . import arrow, predicate, table

_lock = threading.Lock()
_TABLES: Dict[str, Tuple[tuple, pa.Table]] = {}  # path -> (stat key, mmap'd table)
# (version, column) -> single-chunk column; (version, column, "null") -> null slots
_COMBINED: Dict[tuple, object] = {}
_CODES: Dict[tuple, torch.Tensor] = {}  # (stat key, column, device) -> int64 [rows]
_PRED: Dict[tuple, _engine.PredColumn] = {}  # (stat key, column, device) -> staged column


def stat_key(path: str) -> tuple:
    return (os.path.abspath(path),) + arrow.file_version(path)


def load_table(path: str) -> Tuple[tuple, pa.Table]:
    """io.arrow.load once per file version."""
    key = stat_key(path)
    with _lock:
        hit = _TABLES.get(key[0])
        if hit is not None and hit[0] == key:
            return hit
    t = arrow.load(path)
    with _lock:
        _TABLES[key[0]] = (key, t)
        for k in [k for k in _COMBINED if key[0] in (s[0] for s in k[0]) and key not in k[0]]:
            del _COMBINED[k]
        for k in [k for k in _CODES if k[0][0] == key[0] and k[0] != key]:
            del _CODES[k]
        for k in [k for k in _PRED if k[0][0] == key[0] and k[0] != key]:
            del _PRED[k]
            _engine.RESIDENT.remove(("pred",) + k)
    return key, t


def sources(root: str, source) -> Tuple[pa.Table, List[Tuple[str, pa.Table]], tuple]:
    """-> (row-wise joined table, [(path, table)] per source, version key)."""
    names = [source] if isinstance(source, str) else list(source)
    loaded = [(table.path(root, n),) + load_table(table.path(root, n)) for n in names]
    parts = [(p, t) for p, _, t in loaded]
    return table.join(*[t for _, t in parts]), parts, tuple(k for _, k, _ in loaded)


def combined(version: tuple, name: str, col: pa.ChunkedArray) -> pa.Array:
    key = (version, name)
    with _lock:
        comb = _COMBINED.get(key)
    if comb is None:
        comb = col.combine_chunks()
        with _lock:
            _COMBINED[key] = comb
    return comb


def null_count(version: tuple, name: str, col: pa.ChunkedArray) -> int:
    """A column's null count, cached per file version (ChunkedArray.null_count
    walks every chunk: ~0.1 ms per search over 10 000 1 000-row batches)."""
    key = (version, name, "null_count")
    with _lock:
        hit = _COMBINED.get(key)
    if hit is None:
        hit = int(col.null_count)
        with _lock:
            _COMBINED[key] = hit
    return hit


def null_mask(version: tuple, name: str, col: pa.ChunkedArray) -> np.ndarray:
    """bool[rows]: the null slots of a column (cached per file version)."""
    key = (version, name, "null")
    with _lock:
        hit = _COMBINED.get(key)
    if hit is None:
        hit = pc.is_null(col).to_numpy(zero_copy_only=False).astype(bool)
        with _lock:
            _COMBINED[key] = hit
    return hit


def shards(parts, column: str, devs) -> List[Tuple[_engine.Shard, int, int]]:
    """HBM shards of every source's ``column``, row-range split over ``devs``.
    Returns (shard, source index, first source row); global rows continue
    across sources in order (table.py:19-21)."""
    out, base = [], 0
    for i, (path, t) in enumerate(parts):
        if path is not None:
            pieces = _engine.CACHE.get(path, t, column, devs).pieces
        else:
            pieces = _engine.stage_sharded(t.column(column), devs)
        scale, zp = _engine.qparams(t.schema.field(column).type)
        out.extend((_engine.Shard(p.data, base + p.start, scale, zp), i, p.start)
                   for p in pieces if p.data.shape[0])
        base += t.num_rows
    return out


def gather_rows(shard_list: Sequence[_engine.Shard], rows: np.ndarray,
                device: torch.device, dequantize: bool = False) -> torch.Tensor:
    """Rows (global, ascending) of the resident shards, in order, on ``device``.
    ``dequantize``: quint8 codes come back as their f32 values, each shard
    under its own map (scale * (code - zero_point), QUInt8NDArray.dequantize)."""
    rows = np.asarray(rows, dtype=np.int64)
    out = []
    for s in shard_list:
        lo, hi = np.searchsorted(rows, [s.row_base, s.row_base + s.n])
        if hi > lo:
            idx = torch.from_numpy(rows[lo:hi] - s.row_base).to(s.data.device)
            g = s.data.index_select(0, idx)
            if dequantize and g.dtype == torch.uint8:
                g = (g.to(torch.float32) - s.zero_point) * s.scale
            out.append(g.to(device))
    if not out:
        raise ValueError("no rows selected")
    return torch.cat(out) if len(out) > 1 else out[0]


def code_column(key: tuple, t: pa.Table, column: str, device: torch.device) -> torch.Tensor:
    """int64 code column of an index file, resident on ``device`` (cached per file version)."""
    ck = (key, column, str(device))
    with _lock:
        hit = _CODES.get(ck)
    if hit is not None:
        return hit
    col = t.column(column).cast(pa.int64()).fill_null(-1)  # a null code matches no probe
    host = col.to_numpy() if len(col) else np.zeros(0, np.int64)
    dev = torch.from_numpy(np.array(host, dtype=np.int64)).to(device)  # writable copy
    with _lock:
        _CODES[ck] = dev
    return dev


def _pred_evicted(ck: tuple) -> None:
    with _lock:
        _PRED.pop(ck, None)


def pred_column(key: tuple, t: pa.Table, column: str,
                device: torch.device) -> _engine.PredColumn:
    """A scalar column of a source as fx_pred_eval reads it, whole, resident on
    ``device`` (cached per file version; a shard addresses it with row0 = its
    first source row): the values in the column's own width, the validity
    words repacked to start at bit 0 (only when the column has nulls) and, for
    string columns, int32 codes into the distinct strings kept on the host."""
    ck = (key, column, str(device))
    rkey = ("pred",) + ck
    with _lock:
        hit = _PRED.get(ck)
    if hit is not None:
        _engine.RESIDENT.touch(rkey)
        return hit
    values, valid, dictionary = predicate.host_column(t.column(column))
    words = predicate.pack_validity(valid) if valid is not None else None
    need = {device.index: values.nbytes + (words.nbytes if words is not None else 0)}
    # as CorpusCache.get: reserve evicts what it may; a column that still does
    # not fit the budget is staged all the same (the search needs it now) and
    # is the first to go at the next reservation
    _engine.RESIDENT.reserve(need)
    dtype = predicate._column_kind(t.schema.field(column).type)[1]
    signed = {"u": "i"}.get(values.dtype.kind, values.dtype.kind) + str(values.dtype.itemsize)
    with torch.cuda.device(device):
        staged = _engine.PredColumn(
            torch.from_numpy(values.view(signed)).to(device),  # the bits; dtype names the type
            torch.from_numpy(words.view(np.int32)).to(device) if words is not None else None,
            dictionary, dtype)
    with _lock:
        _PRED[ck] = staged
    _engine.RESIDENT.add(rkey, _engine.Residency.PRED, need, lambda: _pred_evicted(ck))
    return staged
