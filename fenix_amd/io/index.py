"""``call`` — the search entry point — and the coded index, on the GPU.

Drop-in for src/fenix/io/index/index.py of the reference.

``call(root, coding, source, column, target, metric, select, filter, maxval,
probes)`` (index.py:81-170, the function ``Server.do_exchange`` invokes,
flight.py:74).  Same signature, argument meaning, output schema and error
behaviour:

* source: name or list of names under ``<root>/sources`` (index.py:93-97); a
  ``pa.Table`` is also accepted (the reference leaves ``data`` unbound there,
  index.py:93-99, an UnboundLocalError);
* target: Array / ChunkedArray / FixedSizeListScalar / ndarray / Tensor,
  normalised and cast to the column's value type exactly as index.py:101-111
  (``pa.scalar(target, type=column type)``: a wrong length raises
  ``ArrowInvalid``);
* ``coding`` given: the table is joined with its ``__CODED_ID__`` column
  (``load``, index.py:19-34); with ``probes`` the metric defaults to the
  coding's and only rows whose code is among the ``probes`` composites
  nearest the target are searched (index.py:113-126) — the probe set is
  computed on the GPU (fx_code_probe) and turned into a row bitmap there
  (fx_code_mask, AND the filter), which the masked scan consumes without
  loading the excluded rows;
* ``select`` default = every column, then ``__DISTANCE__`` appended
  (index.py:128-129); ``assert metric is not None`` (index.py:131); an unknown
  metric raises ``ValueError()`` (coder.py:50);
* ``filter`` (pc.Expression) restricts the rows before the scan (index.py:161):
  an expression ``io.predicate`` compiles is evaluated on the device over the
  source's resident scalar columns (fx_pred_eval), every other one by pyarrow
  on the host; the rows kept are the same (``filter_stats``);
* if ``maxval is not None and rows > maxval``: the ``maxval`` nearest rows,
  ascending by distance (index.py:165-168, select_k_unstable), here with the
  deterministic (distance, row) tie-break; otherwise every row in table order
  with its distance (index.py:165 not taken);
* the result is one chunk (``combine_chunks``, index.py:170); ``__DISTANCE__``
  has the column's value type (the UDF's output type, index.py:153-159).

``call_many(root, coding, source, column, targets, ...)`` (an extension, no
counterpart in the reference): ``call`` for nq targets in one request, the
result carrying ``__TARGET__``.  One filter evaluation, one batched search;
with ``probes`` the per-target row masks come from one pass over the code
column (fx_code_qmask) and feed one per-query-mask search.

``make`` / ``load`` / ``list`` / ``drop`` (index.py:19-78): index files
``<root>/indexes/<source>/<column>/<name>.arrow`` holding one int64
``__CODED_ID__`` per row, written in the source's batch layout; ``make``
encodes the HBM-resident column with fx_code_assign (MFMA nearest codeword per
codebook; fx_code_assign_ex over the 1-byte codes of a quint8 column, each
shard under its own map) instead of the per-batch pyarrow UDF (index.py:46-49).

What changes underneath: the corpus column is resident in HBM (engine.CACHE)
instead of re-read and scanned per chunk by a Python UDF, top-k is fused into
the gfx950 scan, and only the k winning rows are gathered (chunk-aware, no
``Table.take`` over the whole chunked vector column, index.py:166).
"""

from __future__ import annotations

import os
import threading
from typing import Iterator, List, Sequence

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import torch
from torch import Tensor

from .. import engine as _engine
from .. import _lib
from . import _resident, arrow, coder, predicate, table

CODE_COL: str = "__CODED_ID__"
DIST_COL: str = "__DISTANCE__"
LOCATION: str = "indexes"


def _quint8_target(target, type: pa.DataType) -> np.ndarray:
    """A quint8 tensor column (ex/arrow/quint8) is searched with a float target
    of prod(shape) values (only the corpus is coded); a wrong length raises
    ArrowInvalid like index.py:111's pa.scalar."""
    if isinstance(target, pa.ChunkedArray):
        target = target.combine_chunks()
    if isinstance(target, pa.ExtensionScalar):
        target = target.to_numpy().dequantize()
    elif isinstance(target, pa.Scalar):
        target = target.values.to_numpy(zero_copy_only=False)
    elif isinstance(target, pa.Array):
        target = target.to_numpy(zero_copy_only=False)
    elif isinstance(target, Tensor):
        target = target.numpy()
    values = np.array(target, dtype=np.float32).ravel()
    d = _engine.list_size(type)
    if values.size != d:
        raise pa.ArrowInvalid(f"target has {values.size} values, the column {d}")
    return values.reshape(1, -1)


def _dist_type(type: pa.DataType) -> pa.DataType:
    """__DISTANCE__ has the column's value type (index.py:153-159); float32 for quint8."""
    return pa.float32() if isinstance(type, pa.ExtensionType) else type.value_type


def _target_values(target, type: pa.DataType) -> np.ndarray:
    """index.py:101-111: normalise the target and cast it to the column type."""
    if isinstance(type, pa.ExtensionType):
        return _quint8_target(target, type)
    if isinstance(target, pa.ChunkedArray):
        target = target.combine_chunks()
    if isinstance(target, pa.Array):
        target = target.to_numpy(zero_copy_only=False)
    if isinstance(target, Tensor):
        target = target.numpy()
    if isinstance(target, np.ndarray):
        if pa.types.is_float16(type.value_type):
            target = np.asarray(target).astype(np.float16)
        target = pa.scalar(target, type=type)
    if not isinstance(target, pa.FixedSizeListScalar):
        raise TypeError(f"unsupported target type {type(target)}")
    if target.type != type:
        target = target.cast(type)
    values = target.values.to_numpy(zero_copy_only=False)
    return np.array(values, dtype=np.float32).reshape(1, -1)  # writable copy


def _filter_mask(data: pa.Table, filter: pc.Expression) -> np.ndarray:
    """Evaluate the row predicate of index.py:161 into a bool mask (nulls drop)."""
    import pyarrow.dataset as ds

    m = ds.dataset(data).to_table(columns={"__m__": filter}).column("__m__")
    return m.fill_null(False).to_numpy(zero_copy_only=False).astype(bool)


_stats_lock = threading.Lock()
_FILTER_STATS = {"device": 0, "host": 0, "reasons": {}}


def filter_stats() -> dict:
    """How many filters were evaluated on the device (fx_pred_eval) and how
    many by pyarrow on the host, and why the latter: {"device": n, "host": n,
    "reasons": {reason: n}}."""
    with _stats_lock:
        return {"device": _FILTER_STATS["device"], "host": _FILTER_STATS["host"],
                "reasons": dict(_FILTER_STATS["reasons"])}


def _count_filter(reason: str | None) -> None:
    with _stats_lock:
        if reason is None:
            _FILTER_STATS["device"] += 1
        else:
            _FILTER_STATS["host"] += 1
            _FILTER_STATS["reasons"][reason] = _FILTER_STATS["reasons"].get(reason, 0) + 1


def _device_filter(data: pa.Table, parts, filter: pc.Expression):
    """The program of a filter the device evaluates, or None (and the reason
    counted): ``FENIX_AMD_DEVICE_FILTER=0`` switches the device path off,
    ``pa.Table`` sources, tables below the library option
    "device_filter_min_rows" and every expression ``predicate.compile``
    refuses keep pyarrow's evaluation."""
    reason, program = None, None
    if os.environ.get("FENIX_AMD_DEVICE_FILTER", "1").strip() == "0":
        reason = "switched off"
    elif any(path is None for path, _ in parts):
        reason = "table source"
    elif data.num_rows < max(1, _lib.get_option("device_filter_min_rows")):
        reason = "below device_filter_min_rows"
    else:
        program, why = predicate.explain(filter, data.schema)
        if program is None:
            reason = "expression: " + why
        elif any(t.schema.get_field_index(c.name) < 0
                 or t.schema.field(c.name).type != data.schema.field(c.name).type
                 for _, t in parts for c in program.columns):
            reason, program = "column outside the source files", None
    _count_filter(reason)
    return program


def _device_masks(program, shard_info, parts, version, want_counts: bool = True):
    """fx_pred_eval per shard over the source's resident predicate columns.
    -> (per-shard bitmaps, per-shard kept rows: one D2H per device; None when
    not wanted: a probe search counts behind its own mask)."""
    masks, cnts = [], []
    for s, src, start in shard_info:
        dev = s.data.device
        with torch.cuda.device(dev):
            cols = [_resident.pred_column(version[src], parts[src][1], c.name, dev)
                    for c in program.columns]
            mk, cnt = _engine.Engine.get(dev).pred_eval(program, cols, s.n, start)
        masks.append(mk)
        cnts.append(cnt)
    if not want_counts:
        return masks, None
    counts = [0] * len(cnts)
    by_dev = {}
    for i, c in enumerate(cnts):
        by_dev.setdefault(c.device, []).append(i)
    for dev, idx in by_dev.items():
        with torch.cuda.device(dev):
            got = torch.cat([cnts[i] for i in idx]).cpu().numpy()
        for i, v in zip(idx, got):
            counts[i] = int(v)
    return masks, counts


def _take_chunked(col: pa.ChunkedArray, rows: np.ndarray) -> pa.Array:
    """Gather ``rows`` of a chunked column without concatenating it first."""
    lens = np.fromiter((len(c) for c in col.chunks), dtype=np.int64, count=col.num_chunks)
    starts = np.concatenate([[0], np.cumsum(lens)])
    ci = np.searchsorted(starts, rows, side="right") - 1
    order = np.argsort(ci, kind="stable")
    pieces = []
    for c in np.unique(ci):
        sel = order[ci[order] == c]
        pieces.append(col.chunk(int(c)).take(pa.array(rows[sel] - starts[c])))
    if not pieces:
        return pa.array([], type=col.type)
    cat = pa.concat_arrays(pieces)
    return cat.take(pa.array(np.argsort(order, kind="stable")))


def take_rows(data: pa.Table, rows: np.ndarray) -> pa.Table:
    rows = np.asarray(rows, dtype=np.int64)
    cols = [_take_chunked(data.column(i), rows) for i in range(data.num_columns)]
    return pa.Table.from_arrays(cols, schema=data.schema)


def _gather_vectors(shards, rows: np.ndarray, type: pa.DataType,
                    null: np.ndarray | None = None,
                    values: np.ndarray | None = None) -> pa.Array:
    """The k winning embeddings, read back from their HBM shards (they are the
    stored Arrow values, staged verbatim) instead of gathered from Arrow
    chunks (index.py:166's take): one H2D of (result position, local row)
    pairs per device, an ``index_select`` per shard placed by ``index_copy_``
    into one result buffer on the first shard's device (other devices' rows
    travel there peer to peer), and ONE D2H into pinned memory with one
    synchronisation — not a round trip per shard (configs[4]'s 8 shards:
    0.63 -> 0.41 ms, profiles/r05_profile_call_cfg4_{before,after}.json,
    DESIGN §6.2).  ``null``: which
    result rows are null slots of the column; their stored values are
    gathered like any other (they were scanned) and the slot stays null, as
    index.py:166's ``take`` keeps validity (tests/golden g7_nulls).
    ``values``: the rows' stored values, already gathered on the device
    behind the search (engine.search_host, one D2H with the distances); only
    the Arrow array is built then."""
    d = _engine.list_size(type)
    _, tdt, ndt = _engine.value_dtype(type)
    m = rows.size
    if values is not None:
        out = np.ascontiguousarray(values).view(ndt).reshape(m, d)
    elif m == 0 or not shards:
        out = np.empty((m, d), dtype=ndt)
    else:
        bases = np.array([s.row_base for s in shards], dtype=np.int64)
        sizes_n = np.array([s.n for s in shards], dtype=np.int64)
        if np.any(np.diff(bases) < 0):
            raise ValueError("_gather_vectors: shards must be in row order")
        which = np.searchsorted(bases, rows, side="right") - 1
        if np.any(which < 0) or np.any(rows - bases[np.maximum(which, 0)] >= sizes_n[which]):
            raise ValueError("_gather_vectors: a result row lies outside every shard")
        dev0 = shards[0].data.device
        with torch.cuda.device(dev0):
            acc = torch.empty((m, d), dtype=shards[0].data.dtype, device=dev0)
            by_dev = {}
            for i, s in enumerate(shards):
                by_dev.setdefault(s.data.device, []).append(i)
            for dev, idx in by_dev.items():
                # (position in the result, local row) of every row this device holds
                pos = [np.nonzero(which == i)[0] for i in idx]
                sizes = [p.size for p in pos]
                if not sum(sizes):
                    continue
                pairs = np.empty((2, sum(sizes)), dtype=np.int64)
                pairs[0] = np.concatenate(pos)
                pairs[1] = rows[pairs[0]] - np.repeat(bases[idx], sizes)
                with torch.cuda.device(dev):
                    pd = torch.from_numpy(pairs).to(dev)
                    off = 0
                    for i, c in zip(idx, sizes):
                        if c:
                            g = shards[i].data.index_select(0, pd[1, off : off + c])
                            p = pd[0, off : off + c]
                            if dev != dev0:
                                g, p = g.to(dev0), p.to(dev0)
                            acc.index_copy_(0, p, g)
                        off += c
                    if dev != dev0:  # the peer copies above read on this device's stream
                        torch.cuda.current_stream(dev0).wait_stream(torch.cuda.current_stream(dev))
            host = torch.empty((m, d), dtype=acc.dtype, pin_memory=True)
            host.copy_(acc, non_blocking=True)
            torch.cuda.current_stream(dev0).synchronize()
        out = host.numpy().view(ndt)
    mask = pa.array(null) if null is not None and null.any() else None
    lists = pa.FixedSizeListArray.from_arrays(pa.array(out.ravel()), list_size=d, mask=mask)
    if isinstance(type, pa.ExtensionType):  # quint8 codes: same type, same parameters
        return pa.ExtensionArray.from_storage(type, lists.cast(type.storage_type))
    return lists.cast(type)


def _null_mask(col: pa.ChunkedArray) -> np.ndarray:
    """bool[rows]: which slots of ``col`` are null."""
    return pc.is_null(col).to_numpy(zero_copy_only=False).astype(bool)


def _take_columns(data: pa.Table, cols: List[str], rows: np.ndarray, column: str, shards,
                  version, values: np.ndarray | None = None) -> pa.Table:
    """select(cols).take(rows) without Table.take's concatenation of the whole
    chunked vector column (index.py:166; 0.75 s per 1M x 768 measured);
    ``values``: the vector column's rows, gathered on the device already."""
    arrays = []
    for c in cols:
        col = data.column(c)
        if c == column:
            null = None
            if (col.null_count if version is None else _resident.null_count(version, c, col)):
                null = (_resident.null_mask(version, c, col) if version is not None
                        else _null_mask(col))[rows]
            arrays.append(_gather_vectors(shards, rows, col.type, null, values))
        elif version is None:
            arrays.append(_take_chunked(col, rows))
        else:
            arrays.append(_resident.combined(version, c, col).take(pa.array(rows)))
    return pa.Table.from_arrays(arrays, schema=pa.schema([data.schema.field(c) for c in cols],
                                                         metadata=data.schema.metadata))


_register_lock = threading.Lock()


def register_distance(metric: str, type: pa.DataType) -> str:
    """Register (once) the pyarrow scalar UDF ``distance:{metric}:{T}:{D}``.

    The reference registers it lazily inside ``call`` (index.py:133-159):
    ``(x: fixed_size_list<T>[D] array, q: same-type scalar) -> T array``, one
    ``coder.distance`` per Arrow chunk.  ``call`` here does not need it (the
    scan fuses distance + top-k), but code that invokes the function through
    ``pc.call_function`` keeps working: each chunk is evaluated by the GPU
    distance kernel (fx_knn_distances).  Returns the function name.
    """
    coder.metric_id(metric)
    _engine.value_dtype(type)
    func = f"distance:{metric}:{type.value_type}:{type.list_size}"
    with _register_lock:
        if func in pc.list_functions():
            return func

        def dist(ctx: pc.UdfContext, x: pa.FixedSizeListArray,
                 q: pa.FixedSizeListScalar) -> pa.Array:
            from . import torch as io_torch

            xv = io_torch.from_arrow(x)
            qv = torch.from_numpy(_target_values(q, type))
            out = coder.distance(qv, xv, metric)[0]
            return pa.array(out.numpy(), type=type.value_type)

        pc.register_scalar_function(
            dist,
            func,
            {"summary": "fenix distance (GPU)", "description": "coder.py:38-50 on gfx950"},
            {"x": type, "q": type},
            type.value_type,
        )
    return func


def _index_path(root: str, name: str, source: str, column: str) -> str:
    return os.path.join(root, LOCATION, source, column, name + ".arrow")


def load(root: str, name: str, source: str | Sequence[str], column: str) -> pa.Table:
    """index.py:19-34: the source table(s) with their ``__CODED_ID__`` column."""
    if isinstance(source, str):
        coder.load(root, name)

        path = _index_path(root, name, source, column)

        return table.join(table.load(root, source), arrow.load(path), axis=1)

    assert isinstance(source, Sequence) and not isinstance(source, str)
    return table.join(*[load(root, name, s, column) for s in source])


def _encode(root: str, source: str, column: str, code: coder.Coding) -> tuple:
    """Composite code of every row of one source: fx_code_assign over its HBM
    shards.  -> (source table, int64 codes)."""
    _, t = _resident.load_table(table.path(root, source))
    parts = [(table.path(root, source), t)]
    out = np.zeros(t.num_rows, dtype=np.int64)
    m = coder.metric_id(code["config"]["metric"])
    for s, _, start in _resident.shards(parts, column, _engine.devices()):
        dev = s.data.device
        with torch.cuda.device(dev):
            # the shard brings its own quint8 map (sources may differ in scale)
            _, c, _ = _engine.Engine.get(dev).code_assign(s, code["tensor"], m)
            out[start : start + s.n] = c.cpu().numpy()
    return t, out


def make(root: str, name: str, source: str | Sequence[str], column: str) -> pa.Table:
    """index.py:37-65: encode the source(s) with the coding ``name`` and write
    the code column, one record batch per source batch."""
    if isinstance(source, str):
        path = _index_path(root, name, source, column)

        os.makedirs(os.path.dirname(path), exist_ok=True)

        code = coder.load(root, name)
        t, codes = _encode(root, source, column, code)

        def record_batch_generator():
            start = 0
            for batch in t.to_batches():
                n = batch.num_rows
                yield pa.record_batch([pa.array(codes[start : start + n])], names=[CODE_COL])
                start += n

        arrow.make(
            path,
            pa.RecordBatchReader.from_batches(
                pa.schema({CODE_COL: pa.int64()}),
                record_batch_generator(),
            ),
        )

        return load(root, name, source, column)

    assert isinstance(source, Sequence) and not isinstance(source, str)
    return table.join(*[make(root, name, s, column) for s in source])


def list(root: str) -> Iterator[str]:
    """index.py:68-71: index files as ``<source>/<column>/<name>``."""
    base = os.path.join(root, LOCATION)
    for dirpath, _, files in os.walk(base):
        for f in sorted(files):
            if f.endswith(".arrow"):
                rel = os.path.relpath(os.path.join(dirpath, f), base)
                yield rel.removesuffix(".arrow")


def drop(root: str, name: str, source: str, column: str) -> None:
    path = _index_path(root, name, source, column)

    if os.path.exists(path):
        os.unlink(path)


def _unpack(words: torch.Tensor, n: int) -> np.ndarray:
    w = words.cpu().numpy().view(np.uint8)
    return np.unpackbits(w, bitorder="little")[:n].astype(bool)


def _probe_masks(code: coder.Coding, q: np.ndarray, probes: int, shard_info, code_parts,
                 masks):
    """index.py:113-126 on the device: the ``probes`` composites nearest the
    target (with the coding's metric, as pc.call_function(coding, ...) does),
    then per shard bit r = code[r] in that set AND the filter bit.
    -> (per-shard masks, per-shard kept rows, kept-row total, lazy host mask)."""
    nb = int(code["config"]["num_codebooks"])
    ks = int(code["config"]["codebook_size"])
    total = ks**nb
    if probes > total:
        raise RuntimeError("selected index k out of range")  # torch.topk in coder.call
    dev0 = shard_info[0][0].data.device if shard_info else _engine.devices()[0]
    with torch.cuda.device(dev0):
        eng0 = _engine.Engine.get(dev0)
        cw = code["tensor"].to(dev0, torch.float32).contiguous()
        qd = torch.from_numpy(q).to(dev0)
        d = eng0.distances(_engine.Shard(cw.reshape(nb * ks, -1), 0), qd,
                           coder.metric_id(code["config"]["metric"]))
        _, _, sel = eng0.code_probe(d.reshape(1, nb, ks), int(probes), sel=True)
    out, counts = [], []
    for i, (s, src, start) in enumerate(shard_info):
        dev = s.data.device
        with torch.cuda.device(dev):
            key, t = code_parts[src]
            rc = _resident.code_column(key, t, CODE_COL, dev)[start : start + s.n]
            mk, cnt = _engine.Engine.get(dev).code_mask(
                rc, sel[0].to(dev), total, masks[i] if masks is not None else None)
        out.append(mk)
        counts.append(cnt)
    counts = [int(c.item()) for c in counts]
    n_rows = sum(counts)

    def host() -> np.ndarray:
        if not out:
            return np.zeros(0, dtype=bool)
        return np.concatenate([_unpack(mk, s.n) for mk, (s, _, _) in zip(out, shard_info)])

    return out, counts, n_rows, host


def _open_sources(root: str, coding: str | None, source, column: str):
    """The table ``call`` searches: -> (data, parts, version, code_parts).
    Named sources come from the resident cache; with ``coding`` each is joined
    with its ``__CODED_ID__`` column (``load``)."""
    if isinstance(source, pa.Table):
        return source, [(None, source)], None, None
    names = [source] if isinstance(source, str) else [*source]
    data, parts, version = _resident.sources(root, names)
    code_parts = None
    if coding is not None:
        coder.load(root, coding)
        code_parts = [_resident.load_table(_index_path(root, coding, s, column))
                      for s in names]
        data = table.join(*[table.join(t, it, axis=1)
                            for (_, t), (_, it) in zip(parts, code_parts)])
        version = version + tuple(k for k, _ in code_parts)
    return data, parts, version, code_parts


def _shared_filter(data: pa.Table, parts, version, filter, shard_info, want_counts: bool):
    """The row predicate of index.py:161, evaluated once: by the device program
    where ``predicate`` compiles it, else by pyarrow.  -> (program or None, host
    bool mask or None, per-shard device bitmaps or None, per-shard kept rows of
    a device evaluation when ``want_counts`` else None)."""
    program = _device_filter(data, parts, filter) if filter is not None else None
    fmask = _filter_mask(data, filter) if filter is not None and program is None else None
    masks, counts = None, None
    if program is not None:
        masks, counts = _device_masks(program, shard_info, parts, version, want_counts)
    if fmask is not None:
        masks = [_engine.device_mask(fmask[s.row_base : s.row_base + s.n], s.data.device)
                 for s, _, _ in shard_info]
    return program, fmask, masks, counts


def call(
    root: str,
    coding: str | None,
    source: str | Sequence[str] | pa.Table,
    column: str,
    target: pa.Array | pa.ChunkedArray | pa.FixedSizeListScalar | np.ndarray | Tensor,
    metric: str | None = None,
    select: Sequence[str] | None = None,
    filter: pc.Expression | None = None,
    maxval: int | None = None,
    probes: int | None = None,
) -> pa.Table:
    data, parts, version, code_parts = _open_sources(root, coding, source, column)

    type = data.schema.field(column).type
    q = _target_values(target, type)

    code = None
    if coding is not None and probes is not None:
        code = coder.load(root, coding)

        if metric is None:
            metric = code["config"]["metric"]

    select = [*select] if select is not None else data.column_names
    select = select + [DIST_COL]

    assert metric is not None

    m = coder.metric_id(metric)
    _engine.value_dtype(type)

    shard_info = _resident.shards(parts, column, _engine.devices())
    shards = [s for s, _, _ in shard_info]
    program, fmask, masks, counts = _shared_filter(data, parts, version, filter, shard_info,
                                                   code is None)
    if code is not None:
        if code_parts is None:
            raise ValueError("a probe search needs named sources with an index")
        masks, counts, n_rows, host_mask = _probe_masks(code, q, probes, shard_info, code_parts,
                                                         masks)
    elif program is not None:
        n_rows = sum(counts)

        def host_mask() -> np.ndarray:
            if not masks:
                return np.zeros(0, dtype=bool)
            return np.concatenate([_unpack(mk, s.n) for mk, s in zip(masks, shards)])
    else:
        n_rows = int(fmask.sum()) if fmask is not None else data.num_rows
        host_mask = (lambda: fmask) if fmask is not None else None
        counts = [int(fmask[s.row_base : s.row_base + s.n].sum()) for s in shards] \
            if fmask is not None else None

    qt = torch.from_numpy(q)
    base_cols = [c for c in dict.fromkeys(select) if c != DIST_COL]

    if maxval is not None and n_rows > maxval:
        # the k winning vectors are gathered on the device behind the scan and
        # come back with the distances (one synchronisation)
        dist, rows, vecs = _engine.search_host(shards, qt, m, int(maxval), masks, counts,
                                               gather=column in base_cols)
        dist, rows = dist[0], rows[0]
        keep = rows >= 0
        dist, rows = dist[keep], rows[keep]
        vecs = vecs[0][keep] if vecs is not None else None
        out = _take_columns(data, base_cols, rows, column, shards, version, vecs)
    else:
        dist = _engine.distances_all(shards, qt, m, masks)[0]
        out = data.select(base_cols)
        if host_mask is not None:
            hm = host_mask()
            out = out.filter(pa.array(hm))
            dist = dist[hm]
    dt = _dist_type(type)
    out = out.append_column(DIST_COL, pa.array(dist.astype(dt.to_pandas_dtype()), type=dt))
    return out.select(select).combine_chunks()


# ------------------------------------------------------------ many targets --
TARGET_COL: str = "__TARGET__"
# targets per engine call: the largest batch this project has measured (README);
# nothing bounds the workspace of a larger batch at large k
MANY_CHUNK: int = 256


def _targets_values(targets, type: pa.DataType) -> np.ndarray:
    """``_target_values`` for the nq >= 1 rows of ``targets`` -> [nq, D] f32.

    targets: a FixedSizeListArray / ListArray / ChunkedArray of nq rows, or a
    2-D ndarray / Tensor (quint8 columns: nq float rows of prod(shape) values).
    Each row is normalised and cast as ``_target_values`` does one target (the
    f16 cast, ``ArrowInvalid`` for a wrong length); rows that already have the
    column's value type and length are copied in one piece, which is the same
    thing."""
    if isinstance(targets, pa.ChunkedArray):
        targets = targets.combine_chunks()
    if isinstance(targets, Tensor):
        targets = targets.numpy()
    d = _engine.list_size(type)
    quint8 = isinstance(type, pa.ExtensionType)
    if isinstance(targets, np.ndarray):
        if targets.ndim != 2:
            raise ValueError(f"targets must be 2-D (one row per target), got {targets.ndim}-D")
        rows = [targets[i] for i in range(targets.shape[0])]
        if targets.shape[1] == d:
            if quint8:
                rows, out = None, np.array(targets, dtype=np.float32)
            elif pa.types.is_float16(type.value_type):
                rows, out = None, targets.astype(np.float16).astype(np.float32)
            elif targets.dtype == np.float32 and pa.types.is_float32(type.value_type):
                rows, out = None, np.array(targets, dtype=np.float32)
    elif isinstance(targets, pa.Array):
        if not (pa.types.is_fixed_size_list(targets.type) or pa.types.is_list(targets.type)
                or pa.types.is_large_list(targets.type)):
            raise TypeError(f"targets must hold one list per target, got {targets.type}")
        rows = [targets[i] for i in range(len(targets))]
        if (pa.types.is_fixed_size_list(targets.type) and targets.type.list_size == d
                and targets.null_count == 0 and targets.flatten().null_count == 0
                and (quint8 or targets.type == type)):
            flat = targets.flatten().to_numpy(zero_copy_only=False)
            rows, out = None, np.array(flat, dtype=np.float32).reshape(len(targets), d)
    else:
        raise TypeError(f"unsupported targets type {_type_name(targets)}")
    if rows is not None:
        if not rows:
            raise ValueError("targets holds no row")
        rows = [r.values.to_numpy(zero_copy_only=False) if isinstance(
            r, (pa.ListScalar, pa.LargeListScalar)) else r for r in rows]
        out = np.concatenate([_target_values(r, type) for r in rows])
    if out.shape[0] < 1:
        raise ValueError("targets holds no row")
    return np.ascontiguousarray(out, dtype=np.float32)


def _type_name(x) -> str:
    return f"{x.__class__.__module__}.{x.__class__.__qualname__}"


def _flatten_many(dist: np.ndarray, rows: np.ndarray):
    """[nq, k] results -> their valid slots (row >= 0; the NaN / -1 padding of
    a target with fewer than k admitted rows is dropped), target 0's first,
    each target's in the search's (distance, row) order.
    -> (dist, rows, target position int32, keep [nq, k] bool)."""
    keep = rows >= 0
    tidx = np.broadcast_to(np.arange(rows.shape[0], dtype=np.int32)[:, None], rows.shape)[keep]
    return dist[keep], rows[keep], np.ascontiguousarray(tidx), keep


def _many_table(out: pa.Table, dist: np.ndarray, tidx: np.ndarray, type: pa.DataType,
                select: Sequence[str]) -> pa.Table:
    """The taken columns of every target's rows plus ``__DISTANCE__`` (the
    column's value type) and ``__TARGET__`` (int32), in ``select`` order."""
    dt = _dist_type(type)
    out = out.append_column(DIST_COL, pa.array(dist.astype(dt.to_pandas_dtype()), type=dt))
    out = out.append_column(TARGET_COL, pa.array(tidx, type=pa.int32()))
    return out.select([*select]).combine_chunks()


def _probe_sel(code: coder.Coding, q: np.ndarray, probes: int, dev0) -> torch.Tensor:
    """One Engine.distances of all targets against the codewords and one
    fx_code_probe -> their selected-code bitmaps [nq, words] on ``dev0``."""
    nb = int(code["config"]["num_codebooks"])
    ks = int(code["config"]["codebook_size"])
    with torch.cuda.device(dev0):
        eng0 = _engine.Engine.get(dev0)
        cw = code["tensor"].to(dev0, torch.float32).contiguous()
        d = eng0.distances(_engine.Shard(cw.reshape(nb * ks, -1), 0), torch.from_numpy(q).to(dev0),
                           coder.metric_id(code["config"]["metric"]))
        _, _, sel = eng0.code_probe(d.reshape(q.shape[0], nb, ks), int(probes), sel=True)
    return sel


def _probe_qmasks(sel: torch.Tensor, ncodes: int, shard_info, code_parts, masks):
    """Per shard one Engine.code_qmask over its slice of the resident code
    column, the shared filter folded in; one D2H of the counts per device.
    -> (per-shard (bitmaps, packed), kept rows int64 [shards, nq])."""
    pairs, cnts = [], []
    for i, (s, src, start) in enumerate(shard_info):
        dev = s.data.device
        with torch.cuda.device(dev):
            key, t = code_parts[src]
            rc = _resident.code_column(key, t, CODE_COL, dev)[start : start + s.n]
            bm, pk, cnt = _engine.Engine.get(dev).code_qmask(
                rc, sel.to(dev), ncodes, masks[i] if masks is not None else None)
        pairs.append((bm, pk))
        cnts.append(cnt)
    counts = np.zeros((len(cnts), sel.shape[0]), dtype=np.int64)
    by_dev = {}
    for i, c in enumerate(cnts):
        by_dev.setdefault(c.device, []).append(i)
    for dev, idx in by_dev.items():
        with torch.cuda.device(dev):
            counts[idx] = torch.stack([cnts[i] for i in idx]).cpu().numpy()
    return pairs, counts


def _many_probe_chunk(code, q, probes, shard_info, code_parts, masks, m, k, gather):
    """One chunk of a probe search of many targets: the masks of all of them
    from one pass over the codes, then one per-query-mask search where
    ``qmask_batch_pays`` (as for coalesced batches), else target by target with
    its bitmap row and count (selective probe sets keep the row-list scan)."""
    shards = [s for s, _, _ in shard_info]
    nq = q.shape[0]
    nb = int(code["config"]["num_codebooks"])
    ks = int(code["config"]["codebook_size"])
    dev0 = shards[0].data.device
    if nq >= _engine.CODE_QMASK_MIN_NQ:
        try:
            sel = _probe_sel(code, q, probes, dev0)
            pairs, counts = _probe_qmasks(sel, ks**nb, shard_info, code_parts, masks)
        except NotImplementedError:  # FX_EUNSUPPORTED: the per-target masks
            pairs = None
    else:
        pairs = None
    if pairs is None:
        outs = []
        for j in range(nq):
            ms, cs, _, _ = _probe_masks(code, q[j : j + 1], probes, shard_info, code_parts, masks)
            outs.append(_engine.search_host(shards, torch.from_numpy(q[j : j + 1]), m, k, ms, cs,
                                            gather=gather))
        return outs
    served = k <= _lib.max_k() and all(
        s.n > 0 and _lib.get_option("filter_image") == 8
        and _lib.qmask_filter_used(s.n, s.d, s.dtype_id, nq, k, m) != 0 for s in shards)
    totals = [int(c) for c in counts.sum(axis=0)]
    if served and _engine.qmask_batch_pays(totals, sum(s.n for s in shards), shards[0].d,
                                           shards[0].data.element_size(), nq):
        return [_engine.search_host(shards, torch.from_numpy(q), m, k, gather=gather,
                                    qmasks=pairs)]
    outs = []
    for j in range(nq):
        ms = [bm[j].clone() for bm, _ in pairs]
        cs = [int(counts[i, j]) for i in range(len(pairs))]
        outs.append(_engine.search_host(shards, torch.from_numpy(q[j : j + 1]), m, k, ms, cs,
                                        gather=gather))
    return outs


def call_many(
    root: str,
    coding: str | None,
    source: str | Sequence[str] | pa.Table,
    column: str,
    targets: pa.Array | pa.ChunkedArray | np.ndarray | Tensor,
    metric: str | None = None,
    select: Sequence[str] | None = None,
    filter: pc.Expression | None = None,
    maxval: int | None = None,
    probes: int | None = None,
) -> pa.Table:
    """``call`` for nq >= 1 targets in one request (an extension: the reference
    has no such entry point).  The result holds the ``select`` columns, then
    ``__DISTANCE__``, then ``__TARGET__`` (int32, the target's position):
    target 0's rows first, each target's ascending by (distance, row).  For
    every i the rows with ``__TARGET__ == i`` are those of ``call(...,
    target=targets[i], ...)``: the same rows, order, distance bits and column
    values whenever that call keeps more than ``maxval`` rows, else the same
    rows sorted by (distance, row) (``call`` returns table order there).
    ``maxval`` is required.

    The filter is evaluated once.  Without probes all targets run as one
    batched search under the shared mask; with probes their masks come from
    one pass over the code column (fx_code_qmask) and the batch runs as one
    per-query-mask search where that pays, else target by target.  Targets are
    processed ``MANY_CHUNK`` at a time."""
    if maxval is None or int(maxval) < 1:
        raise ValueError("call_many: maxval is required (>= 1)")
    data, parts, version, code_parts = _open_sources(root, coding, source, column)

    type = data.schema.field(column).type
    q = _targets_values(targets, type)

    code = None
    if coding is not None and probes is not None:
        code = coder.load(root, coding)

        if metric is None:
            metric = code["config"]["metric"]

    select = [*select] if select is not None else data.column_names
    select = select + [DIST_COL, TARGET_COL]

    assert metric is not None

    m = coder.metric_id(metric)
    _engine.value_dtype(type)
    k = int(maxval)

    shard_info = _resident.shards(parts, column, _engine.devices())
    shards = [s for s, _, _ in shard_info]
    _, fmask, masks, counts = _shared_filter(data, parts, version, filter, shard_info,
                                             code is None)
    if code is not None:
        if code_parts is None:
            raise ValueError("a probe search needs named sources with an index")
        nb = int(code["config"]["num_codebooks"])
        ks = int(code["config"]["codebook_size"])
        if probes > ks**nb:
            raise RuntimeError("selected index k out of range")  # torch.topk in coder.call
    elif fmask is not None:
        counts = [int(fmask[s.row_base : s.row_base + s.n].sum()) for s in shards]

    base_cols = [c for c in dict.fromkeys(select) if c not in (DIST_COL, TARGET_COL)]
    gather = column in base_cols
    outs = []
    if data.num_rows > 0 and shards:
        for lo in range(0, q.shape[0], MANY_CHUNK):
            qc = q[lo : lo + MANY_CHUNK]
            if code is not None:
                outs += _many_probe_chunk(code, qc, probes, shard_info, code_parts, masks, m, k,
                                          gather)
            elif k > _lib.max_k():  # beyond the fused scan's k: target by target
                outs += [_engine.search_host(shards, torch.from_numpy(qc[j : j + 1]), m, k, masks,
                                             counts, gather=gather) for j in range(qc.shape[0])]
            else:
                outs.append(_engine.search_host(shards, torch.from_numpy(qc), m, k, masks, counts,
                                                gather=gather))
    if outs:
        dist = np.concatenate([o[0] for o in outs])
        rows = np.concatenate([o[1] for o in outs])
        vecs = np.concatenate([o[2] for o in outs]) if all(o[2] is not None for o in outs) else None
    else:
        dist = np.zeros((q.shape[0], 0), dtype=np.float32)
        rows = np.zeros((q.shape[0], 0), dtype=np.int64)
        vecs = None
    dist, rows, tidx, keep = _flatten_many(dist, rows)
    vecs = vecs[keep] if vecs is not None else None
    out = _take_columns(data, base_cols, rows, column, shards, version, vecs)
    return _many_table(out, dist, tidx, type, select)
