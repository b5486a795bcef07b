"""Many targets in one request: io.index.call_many and Flight.search_many
against per-target ``call`` / ``search`` (rows, order, distance bits, every
selected column) and against the float64 oracle.

40 003 rows of d = 128 in two sources (25 000 + 15 003: global rows, a ragged
last tile, two shards), k = 10, the library options of tests/test_gpu_qmask.py
(``BASE``), so batches run the int8 filter.  The probe cases use a small
trained coding (2 codebooks of 16) and probe sets small enough that, under a
shared filter, targets fall on both sides of ``maxval``; that is asserted from
fx_code_qmask's own counts, which are checked against numpy first.
"""

from __future__ import annotations

import functools
import socket

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest
import torch

import fenix_amd
from fenix_amd import _lib, engine
from fenix_amd.engine import Engine
from fenix_amd.ex.arrow import quint8 as Q
from fenix_amd.io import _resident, coder, index, table
from oracle import oracle as O
from tests import parity

pytestmark = pytest.mark.gpu

N, NA, D, K = 40_003, 25_000, 128, 10
BASE = {"filter_image": 8, "batch_cap": 4096, "qu8_batch_min_work": 0,
        "device_filter_min_rows": 0}
NQ_MAX = 65
FILTERS = {
    "none": None,
    "device": pc.field("a") > 30,          # the predicate compiler accepts it
    "host": (pc.field("a") + 1) > 31,      # ... and refuses this one: same rows
}
CODING = "c/l2"


def _sources(dtype):
    return [f"{dtype}/a", f"{dtype}/b"]


@functools.lru_cache(maxsize=None)
def _host(dtype):
    """(stored vector column, rows as float32, column a)."""
    x = O.fill_normal(N, D, seed=121)
    a = np.random.RandomState(122).randint(0, 100, N).astype(np.int32)
    if dtype == "f16":
        xs = x.astype(np.float16)
        return pa.FixedSizeListArray.from_arrays(pa.array(xs.ravel()), D), xs.astype(np.float32), a
    if dtype == "qu8":
        col = Q.from_numpy(x)
        return col, O.dequantize(col.codes(), col.type.scale, col.type.shift), a
    return pa.FixedSizeListArray.from_arrays(pa.array(x.ravel()), D), x, a


@functools.lru_cache(maxsize=None)
def _targets(dtype):
    t = O.fill_normal(NQ_MAX, D, seed=123)
    return t, (t.astype(np.float16).astype(np.float32) if dtype == "f16" else t)


@functools.lru_cache(maxsize=None)
def _oracle(dtype, metric, flt):
    """The float64 top-k of all NQ_MAX targets, computed once per case family."""
    _, xv, a = _host(dtype)
    mask = None if flt == "none" else a > 30
    return O.knn(xv, _targets(dtype)[1], metric, K, mask=mask)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = str(tmp_path_factory.mktemp("many"))
    for dtype in ("f32", "f16", "qu8"):
        col, _, a = _host(dtype)
        t = pa.table({"id": pa.array(np.arange(N, dtype=np.int64)), "a": pa.array(a),
                      "vector": col})
        for name, part in zip(_sources(dtype), (t.slice(0, NA), t.slice(NA))):
            table.make(root, name, part.combine_chunks().to_reader(max_chunksize=1000))
    np.random.seed(124)
    coder.make(root, CODING, _sources("f32"), "vector",
               {"metric": "l2", "codebook_size": 16, "num_codebooks": 2, "batch_size": 256,
                "num_epochs": 1})
    index.make(root, CODING, _sources("f32"), "vector")
    with _lib.options(**BASE):
        yield root
    engine.CACHE.clear()
    Engine.get(torch.device("cuda", 0)).clear_images()


def _bits(col):
    a = col.to_numpy(zero_copy_only=False)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _of_target(many, i):
    sub = many.filter(pc.field(index.TARGET_COL) == i)
    return sub.drop([index.TARGET_COL]).combine_chunks()


def _assert_same(sub, one, maxval, what, top=True):
    """The contract of call_many for one target: ``sub`` (its rows of the
    many-target table) against ``one`` (the single-target call).  ``top``: that
    call kept more than ``maxval`` rows, so it returned the nearest ``maxval``."""
    assert sub.schema == one.schema, what
    ids = sub.column("id").to_numpy()
    d = sub.column(index.DIST_COL).to_numpy(zero_copy_only=False)
    assert (np.diff(d.astype(np.float64)) >= 0).all(), f"{what}: distances not ascending"
    if d.dtype == np.float32:  # (a float16 column rounds the distances it was ordered by)
        order = np.lexsort((ids, d))
        np.testing.assert_array_equal(order, np.arange(len(ids)), err_msg=f"{what}: row order")
    if top:
        assert one.num_rows == maxval, what
        np.testing.assert_array_equal(ids, one.column("id").to_numpy(), err_msg=what)
        np.testing.assert_array_equal(_bits(sub.column(index.DIST_COL)),
                                      _bits(one.column(index.DIST_COL)), err_msg=what)
        assert sub.equals(one), what
        return
    # call kept at most maxval rows and returned them in table order with the
    # whole-table distance kernel's values: the same rows and column values,
    # here sorted by (distance, row).  Both kernels sum 128 float32 products:
    # each is within d * 2^-24 ~ 8e-6 of the exact value relative to the
    # accumulated magnitude, 1e-4 leaves an order of magnitude.
    assert one.num_rows <= maxval, what
    a, b = sub.sort_by("id"), one.sort_by("id")
    for name in one.column_names:
        if name == index.DIST_COL:
            da = a.column(name).to_numpy().astype(np.float64)
            db = b.column(name).to_numpy().astype(np.float64)
            assert da.shape == db.shape, what
            assert np.all(np.abs(da - db) <= 1e-4 * np.maximum(np.abs(db), 1.0)), what
        else:
            assert a.column(name).equals(b.column(name)), f"{what}: column {name}"


def _check_oracle(many, nq, dtype, metric, flt):
    _, xv, _ = _host(dtype)
    od, orow = _oracle(dtype, metric, flt)
    qh = _targets(dtype)[1]
    for i in range(nq):
        sub = _of_target(many, i)
        ids = sub.column("id").to_numpy()[None]
        dist = sub.column(index.DIST_COL).to_numpy(zero_copy_only=False)[None]
        if dtype == "f16":  # fp16 output distances: ids, and values at fp16 resolution
            np.testing.assert_array_equal(ids, orow[i:i + 1])
            assert np.all(np.abs(dist.astype(np.float64) - od[i:i + 1])
                          <= 2 ** -10 * np.abs(od[i:i + 1]))
        else:
            parity.check_topk(dist, ids, od[i:i + 1], orow[i:i + 1], xv, qh[i:i + 1], metric)


CASES = []
for mi, metric in enumerate(["l2", "inner_product", "cosine"]):
    for ni, nq in enumerate([1, 2, 33, 65]):
        flt = list(FILTERS)[(mi + ni) % 3]
        vec = (mi + ni) % 2 == 0
        CASES.append(pytest.param("f32", metric, nq, flt, vec,
                                  id=f"f32-{metric}-q{nq}-{flt}-{'vec' if vec else 'novec'}"))
CASES.append(pytest.param("f16", "inner_product", 33, "device", True, id="f16-ip-q33-device-vec"))
CASES.append(pytest.param("qu8", "l2", 33, "host", True, id="qu8-l2-q33-host-vec"))


@pytest.mark.parametrize("dtype,metric,nq,flt,vec", CASES)
def test_call_many_equals_per_target_calls(env, dtype, metric, nq, flt, vec):
    select = ["id", "vector", "a"] if vec else ["a", "id"]
    t = _targets(dtype)[0][:nq]
    kw = dict(metric=metric, select=select, filter=FILTERS[flt], maxval=K)
    before = index.filter_stats()
    many = index.call_many(env, None, _sources(dtype), "vector", t, **kw)
    after = index.filter_stats()
    # the filter is evaluated once for all targets, where the case says
    assert after["device"] - before["device"] == (1 if flt == "device" else 0)
    assert after["host"] - before["host"] == (1 if flt == "host" else 0)
    assert many.column_names == select + [index.DIST_COL, index.TARGET_COL]
    assert many.schema.field(index.TARGET_COL).type == pa.int32()
    assert many.num_rows == nq * K
    np.testing.assert_array_equal(many.column(index.TARGET_COL).to_numpy(),
                                  np.repeat(np.arange(nq, dtype=np.int32), K))
    for i in range(nq):
        one = index.call(env, None, _sources(dtype), "vector", target=t[i], **kw)
        _assert_same(_of_target(many, i), one, K, f"target {i}")
    _check_oracle(many, nq, dtype, metric, flt)
    # the accepted target types give the same table
    if nq == 2:
        fsl = pa.FixedSizeListArray.from_arrays(pa.array(t.ravel()), D)
        for other in (fsl, pa.chunked_array([fsl[:1], fsl[1:]]), torch.from_numpy(t)):
            assert index.call_many(env, None, _sources(dtype), "vector", other, **kw).equals(many)


def _kernel_counts(root, t, flt, probes):
    """fx_code_qmask's kept rows [shards, nq] through call_many's own helpers,
    and the same from numpy."""
    src = _sources("f32")
    data, parts, version, code_parts = index._open_sources(root, CODING, src, "vector")
    shard_info = _resident.shards(parts, "vector", engine.devices())
    _, _, masks, _ = index._shared_filter(data, parts, version, flt, shard_info, False)
    code = coder.load(root, CODING)
    q = index._targets_values(t, data.schema.field("vector").type)
    sel = index._probe_sel(code, q, probes, shard_info[0][0].data.device)
    pairs, counts = index._probe_qmasks(sel, 256, shard_info, code_parts, masks)
    torch.cuda.synchronize()
    codes = data.column(index.CODE_COL).to_numpy()
    selb = np.unpackbits(sel.cpu().numpy().view(np.uint8), axis=1, bitorder="little")[:, :256]
    assert (selb.sum(axis=1) == probes).all()
    member = selb.astype(bool)[:, codes] & (_host("f32")[2] < 12)[None, :]
    want = np.stack([member[:, s.row_base:s.row_base + s.n].sum(axis=1) for s, _, _ in shard_info])
    np.testing.assert_array_equal(counts, want)
    for (bm, pk), (s, _, _) in zip(pairs, shard_info):
        assert tuple(pk.shape) == (s.n, _lib.qmask_words(len(t)))
    return counts, len(shard_info)


def test_probe_targets_on_both_sides_of_maxval(env):
    nq, probes = 33, 1
    t = _targets("f32")[0][:nq]
    flt = pc.field("a") < 12
    counts, nshards = _kernel_counts(env, t, flt, probes)
    assert nshards == 2
    totals = counts.sum(axis=0)
    maxval = int(totals.min() + totals.max()) // 2
    print(f"kept rows per target {sorted(totals.tolist())}, maxval {maxval}")
    assert (totals > maxval).any() and (totals < maxval).any() and maxval >= 1
    kw = dict(select=["id", "a", "vector"], filter=flt, maxval=maxval, probes=probes)
    engs = list(Engine._instances.values())
    with _lib.options(qmask_batch_min_ratio=0):  # one per-query-mask search
        q0 = sum(e.qmask_searches for e in engs)
        low = index.call_many(env, CODING, _sources("f32"), "vector", t, **kw)
        assert sum(e.qmask_searches for e in engs) == q0 + nshards
    with _lib.options(qmask_batch_min_ratio=10**9):  # target by target
        q0 = sum(e.qmask_searches for e in engs)
        high = index.call_many(env, CODING, _sources("f32"), "vector", t, **kw)
        assert sum(e.qmask_searches for e in engs) == q0
    assert low.equals(high)
    got = np.bincount(low.column(index.TARGET_COL).to_numpy(), minlength=nq)
    np.testing.assert_array_equal(got, np.minimum(totals, maxval))
    for i in range(nq):
        one = index.call(env, CODING, _sources("f32"), "vector", target=t[i], **kw)
        assert one.num_rows == min(int(totals[i]), maxval)
        _assert_same(_of_target(low, i), one, maxval, f"target {i} ({totals[i]} rows kept)",
                     top=totals[i] > maxval)
    with pytest.raises(RuntimeError, match="out of range"):
        index.call_many(env, CODING, _sources("f32"), "vector", t, maxval=K, probes=257)


def test_probe_many_without_a_filter_and_a_single_target(env):
    t = _targets("f32")[0][:3]
    kw = dict(select=["id"], maxval=K, probes=40)
    many = index.call_many(env, CODING, _sources("f32"), "vector", t, **kw)
    for i in range(3):
        one = index.call(env, CODING, _sources("f32"), "vector", target=t[i], **kw)
        _assert_same(_of_target(many, i), one, K, f"target {i}")
    first = index.call_many(env, CODING, _sources("f32"), "vector", t[:1], **kw)
    assert first.equals(many.slice(0, first.num_rows))


def test_maxval_is_required_and_large_k_runs_target_by_target(env):
    t = _targets("f32")[0][:3]
    with pytest.raises(ValueError, match="maxval"):
        index.call_many(env, None, _sources("f32"), "vector", t, metric="l2")
    big = _lib.max_k() + 1
    kw = dict(metric="l2", select=["id"], maxval=big)
    many = index.call_many(env, None, _sources("f32"), "vector", t, **kw)
    assert many.num_rows == 3 * big
    for i in range(3):
        one = index.call(env, None, _sources("f32"), "vector", target=t[i], **kw)
        _assert_same(_of_target(many, i), one, big, f"target {i}")


def test_search_many_over_flight(env, tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    server = fenix_amd.Server(env, host="127.0.0.1", port=port)
    try:
        f = fenix_amd.Flight(host="127.0.0.1", port=port)
        t = _targets("f32")[0][:5]
        for kw in (dict(metric="cosine", select=["id", "vector"], maxval=K,
                        filter=pc.field("a") > 30),
                   dict(metric="l2", coding=CODING, select=["id", "a"], maxval=K, probes=40)):
            many = f.search_many(t, _sources("f32"), "vector", **kw)
            assert many.column_names[-2:] == [index.DIST_COL, index.TARGET_COL]
            assert many.num_rows == 5 * K
            for i in range(5):
                one = f.search(t[i], _sources("f32"), "vector", **kw)
                _assert_same(_of_target(many, i), one, K, f"target {i}")
            assert f.search_many(torch.from_numpy(t), _sources("f32"), "vector", **kw).equals(many)
        # the plain search of the same server is untouched
        one = f.search(t[0], _sources("f32"), "vector", "l2", select=["id"], maxval=K)
        assert one.column_names == ["id", index.DIST_COL] and one.num_rows == K
        with pytest.raises(Exception):
            f.search_many(t, _sources("f32"), "vector", "l2")  # maxval is required
    finally:
        server.shutdown()
