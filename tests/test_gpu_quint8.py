"""Search over a quint8 tensor column on the GPU (FX_DTYPE_QU8: 1-byte codes
dequantised in the scan's registers) against the oracle on the dequantised
values (oracle.dequantize = QUInt8NDArray.dequantize, quint8.py:53-54)."""

from __future__ import annotations

import functools
import socket

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest
import torch

import fenix_amd
from fenix_amd.ex.arrow import quint8 as Q
from fenix_amd.io import index, table
from oracle import oracle as O
from tests.parity import check_topk

pytestmark = pytest.mark.gpu

METRICS = ["l2", "inner_product", "cosine"]


@pytest.fixture(scope="module")
def qenv(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = str(tmp_path_factory.mktemp("q8"))
    n, d = 60_000, 128
    x = O.fill_normal(n, d, seed=71, cluster=1000)
    a = Q.from_numpy(x)
    src = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "vector": a})
    table.make(root, "q/t", src.to_reader(max_chunksize=1000))
    deq = O.dequantize(a.codes(), a.type.scale, a.type.shift)
    return dict(root=root, x=deq, codes=a.codes(), type=a.type, n=n, d=d)


@pytest.mark.parametrize("metric", METRICS)
def test_quint8_search_matches_oracle(qenv, metric):
    t = O.fill_normal(1, qenv["d"], seed=72)[0]
    r = index.call(qenv["root"], None, "q/t", "vector", target=t, metric=metric, maxval=20)
    assert r.schema.field("__DISTANCE__").type == pa.float32()
    assert Q.is_quint8(r.schema.field("vector").type)
    od, orow = O.knn(qenv["x"], t[None], metric, 20)
    check_topk(r.column("__DISTANCE__").to_numpy()[None], r.column("id").to_numpy()[None], od,
               orow, qenv["x"], t[None], metric)
    got = r.column("vector").chunk(0).codes()  # combine_chunks: one chunk
    np.testing.assert_array_equal(got, qenv["codes"][r.column("id").to_numpy()])


def test_quint8_whole_table_distances(qenv):
    t = O.fill_normal(1, qenv["d"], seed=73)[0]
    r = index.call(qenv["root"], None, "q/t", "vector", target=t, metric="l2", select=["id"])
    ref = O.distances(qenv["x"], t[None], "l2")[0]
    assert np.all(np.abs(r.column("__DISTANCE__").to_numpy() - ref) <= 1e-5 * np.abs(ref).max())


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_quint8_selective_filter_row_list(qenv, metric):
    """< 50 % kept: compacted row list through fx_knn_search_ex."""
    t = O.fill_normal(1, qenv["d"], seed=74)[0]
    expr = pc.field("id") < 9_000
    r = index.call(qenv["root"], None, "q/t", "vector", target=t, metric=metric,
                   select=["id"], filter=expr, maxval=15)
    mask = np.arange(qenv["n"]) < 9_000
    od, orow = O.knn(qenv["x"], t[None], metric, 15, mask=mask)
    check_topk(r.column("__DISTANCE__").to_numpy()[None], r.column("id").to_numpy()[None], od,
               orow, qenv["x"], t[None], metric)


def test_quint8_over_flight(qenv, tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    server = fenix_amd.Server(str(tmp_path), host="127.0.0.1", port=port)
    try:
        f = fenix_amd.Flight(host="127.0.0.1", port=port)
        f.make_table("q/f", table.load(qenv["root"], "q/t").to_reader())
        t = O.fill_normal(1, qenv["d"], seed=75)[0]
        r = f.search(target=t, source="q/f", column="vector", metric="dot", maxval=10)
        od, orow = O.knn(qenv["x"], t[None], "dot", 10)
        check_topk(r.column("__DISTANCE__").to_numpy()[None], r.column("id").to_numpy()[None],
                   od, orow, qenv["x"], t[None], "dot")
    finally:
        server.shutdown()


@pytest.mark.parametrize("metric", METRICS)
def test_quint8_dma_ring_equals_register_tiles(qenv, metric):
    """The LDS-DMA ring (unmasked scans) and the register tiles (masked scans,
    option "q8_dma" 0) compute the same distances bit for bit, top-k and all
    rows."""
    from fenix_amd import _lib
    from fenix_amd.engine import Engine, Shard

    eng = Engine.get(torch.device("cuda", 0))
    codes = torch.from_numpy(qenv["codes"].reshape(qenv["n"], qenv["d"])).to(eng.device)
    shard = Shard(codes, 0, float(qenv["type"].scale), int(qenv["type"].shift))
    q = torch.from_numpy(O.fill_normal(1, qenv["d"], seed=74))
    m = _lib.METRICS[metric]
    dd, dr = eng.search([shard], q, m, 50)
    da = eng.distances(shard, q, m)
    with _lib.options(q8_dma=0):
        rd, rr = eng.search([shard], q, m, 50)
        ra = eng.distances(shard, q, m)
    assert torch.equal(dr, rr)
    assert torch.equal(dd.view(torch.int32), rd.view(torch.int32))
    assert torch.equal(da.view(torch.int32), ra.view(torch.int32))


# The LDS-DMA ring ("q8_dma" 1) against the register tiles ("q8_dma" 0) at the
# shapes where a ring can go wrong.  A block step is 16 rows (4 waves x 4 lane
# groups x 1 row) and the ring is 3 tiles deep: n below, at and above one step
# and the ring's depth; a few steps per block; 70 001 rows leave uneven step
# counts and clamped tail rows over a full grid.  d runs over one to four
# slots per lane with a full and a partial last slot; 1040-d (six slots) has
# no DMA variant, so both settings run the tiles: the control.

RING_N, RING_DMAX = 70_001, 1040


@functools.lru_cache(maxsize=1)
def ring_base():
    """Seeded normal rows coded once at the widest d; a case takes the leading
    rows and columns, so every case shares one scale and zero point."""
    a = Q.from_numpy(O.fill_normal(RING_N, RING_DMAX, seed=81))
    codes = a.codes().copy()
    codes.setflags(write=False)
    return codes, float(a.type.scale), int(a.type.shift)


@functools.lru_cache(maxsize=2)
def ring_rows(n, d):
    codes, scale, shift = ring_base()
    c = np.ascontiguousarray(codes[:n, :d])
    c.setflags(write=False)
    return c, scale, shift


def ring_case(n, d, metric, k, plant=None, interleave=None):
    from fenix_amd import _lib
    from fenix_amd.engine import Engine, Shard

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    eng = Engine.get(torch.device("cuda", 0))
    codes, scale, shift = ring_rows(n, d)
    q = O.fill_normal(1, d, seed=82)
    if plant is not None:  # the true nearest neighbour at a chosen row
        codes = codes.copy()
        want = q[0] if metric == "l2" else 4.0 * q[0]
        codes[plant] = np.clip(np.rint(want / scale) + shift, 0, 127).astype(np.uint8)
    shard = Shard(torch.tensor(codes, device=eng.device), 0, scale, shift)
    qt = torch.from_numpy(q).to(eng.device)
    m = _lib.METRICS[metric]
    opts = {} if interleave is None else {"scan_interleave": interleave}
    out = {}
    for dma in (0, 1):
        with _lib.options(batched=0, single_query_image=0, q8_dma=dma, **opts):
            res = eng.search([shard], qt, m, k) + (eng.distances(shard, qt, m),)
            torch.cuda.synchronize()
        out[dma] = tuple(t.cpu().numpy() for t in res)
    for a, b in zip(out[0], out[1]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    x = O.dequantize(codes, scale, shift)
    od, orow = O.knn(x, q, metric, k)
    check_topk(out[1][0], out[1][1], od, orow, x, q, metric)
    return out[1]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 300, 5_003, 70_001])
def test_dma_ring_equals_tiles_768(n, metric):
    ring_case(n, 768, metric, min(100, n))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [16, 128, 256, 272, 1008, 1024, 1040])
def test_dma_ring_slot_classes(d, metric):
    ring_case(RING_N, d, metric, 100)


@pytest.mark.parametrize("k", [1, 512])
def test_dma_ring_k(k):
    ring_case(RING_N, 768, "l2", k)


@pytest.mark.parametrize("interleave", [0, 1])
def test_dma_ring_both_partitions(interleave):
    ring_case(RING_N, 1024, "l2", 100, interleave=interleave)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("where", ["first", "last"])
def test_dma_ring_keeps_first_and_last_row(where, metric):
    """A dropped first or last tile would lose the planted nearest neighbour."""
    row = 0 if where == "first" else RING_N - 1
    _, rows, _ = ring_case(RING_N, 768, metric, 100, plant=row)
    assert rows[0, 0] == row
