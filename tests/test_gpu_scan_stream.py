"""The streaming scan kernel ("scan_stream" 1: unconditional loads through a
register ring, counted waits) against the register-tile kernel ("scan_stream"
0): the same distances and rows byte for byte, and the oracle's top-k.

Shapes are the smallest at which a ring can go wrong.  At 768-d f32 a block
step is 32 rows (4 waves x 2 rows x 4 lane groups): n below, at and above one
step; 2 blocks; a few steps per block; one straggler tile on one block; and
256 blocks with uneven step counts, where prologue, steady state, ring drain
and clamped tail rows all occur.  Rows that do not fill their slots, masked
and row-list searches take the register tiles under either setting.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from fenix_amd import _lib
from fenix_amd.engine import Engine, Shard, device_mask
from oracle import oracle as O
from tests.parity import check_topk

pytestmark = pytest.mark.gpu

METRICS = ["l2", "inner_product", "cosine"]


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine.get(torch.device("cuda", 0))


@functools.lru_cache(maxsize=4)
def host_rows(n, d, seed, f16):
    x = O.fill_normal(n, d, seed, dtype=np.float16 if f16 else np.float32)
    x.setflags(write=False)
    return x


def device_rows(eng, n, d, seed, f16):
    x = torch.empty((n, d), dtype=torch.float16 if f16 else torch.float32, device=eng.device)
    eng.fill(x, seed)
    return x


def both(fn):
    """fn() under "scan_stream" 0 and 1 -> {0: arrays, 1: arrays} (host copies)."""
    out = {}
    for s in (0, 1):
        with _lib.options(batched=0, single_query_image=0, scan_stream=s):
            res = fn()
            torch.cuda.synchronize()
        out[s] = tuple(t.cpu().numpy() for t in res)
    return out


def assert_same_bytes(out):
    for a, b in zip(out[0], out[1]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


def search_case(eng, n, d, metric, k, f16=False, seed=31, plant=None):
    xh = host_rows(n, d, seed, f16)
    x = device_rows(eng, n, d, seed, f16)
    q = O.fill_normal(1, d, seed=seed + 1)
    if plant is not None:  # the true nearest neighbour at a chosen row
        xh = xh.copy()
        xh[plant] = q[0] if metric == "l2" else 4.0 * q[0]
        x[plant] = torch.from_numpy(xh[plant]).to(eng.device)
    qt = torch.from_numpy(q).to(eng.device)
    out = both(lambda: eng.search([Shard(x, 0)], qt, _lib.METRICS[metric], k))
    assert_same_bytes(out)
    xf = xh.astype(np.float32)
    od, orow = O.knn(xf, q, metric, k)
    check_topk(out[1][0], out[1][1], od, orow, xf, q, metric)
    return out[1]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 300, 5_000, 16_389, 70_001])
def test_stream_equals_tiles_768(eng, n, metric):
    search_case(eng, n, 768, metric, min(100, n))


@pytest.mark.parametrize("k", [1, 100, 1024])
def test_stream_k(eng, k):
    search_case(eng, 70_001, 768, "l2", k)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("where", ["first", "last"])
def test_stream_keeps_first_and_last_row(eng, where, metric):
    """A dropped first or last tile would lose the planted nearest neighbour."""
    n = 70_001
    row = 0 if where == "first" else n - 1
    _, rows = search_case(eng, n, 768, metric, 100, plant=row)
    assert rows[0, 0] == row


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,f16", [(1536, True), (256, False)])
def test_stream_other_row_classes(eng, d, f16, metric):
    """Another (slots, rows per group) class each: the query in LDS (f16
    1536-d) and a ring as deep as one row (f32 256-d)."""
    search_case(eng, 50_003, d, metric, 100, f16=f16)


def test_partial_slot_rows_take_the_tiles(eng):
    """764-d f32: 191 slots do not fill 16 x 12, so both settings run the
    register tiles."""
    search_case(eng, 50_003, 764, "l2", 100)


def test_multi_pass_rows(eng):
    """3072-d f32: two passes per row, the register tiles' pass loop."""
    search_case(eng, 20_001, 3072, "l2", 100)


@pytest.mark.parametrize("rowlist", [False, True])
def test_masked_searches_fall_back(eng, rowlist):
    n, d, k = 70_001, 768, 100
    xh = host_rows(n, d, 31, False)
    x = device_rows(eng, n, d, 31, False)
    q = O.fill_normal(1, d, seed=32)
    qt = torch.from_numpy(q).to(eng.device)
    keep = np.random.RandomState(5).rand(n) < 0.3
    m = device_mask(keep, eng.device)
    counts = [int(keep.sum())] if rowlist else None
    out = both(lambda: eng.search([Shard(x, 0)], qt, _lib.METRIC_L2, k, [m], counts))
    assert_same_bytes(out)
    od, orow = O.knn(xh, q, "l2", k, mask=keep)
    check_topk(out[1][0], out[1][1], od, orow, xh, q, "l2")


@pytest.mark.parametrize("metric", METRICS)
def test_stream_distance_mode(eng, metric):
    n, d = 70_001, 768
    x = device_rows(eng, n, d, 31, False)
    qt = torch.from_numpy(O.fill_normal(1, d, seed=32)).to(eng.device)
    out = both(lambda: (eng.distances(Shard(x, 0), qt, _lib.METRICS[metric]),))
    assert_same_bytes(out)
    assert not np.isnan(out[1][0]).any()
