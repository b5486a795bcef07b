"""The planner's gate for batches over quint8 codes (csrc/knn_plan.hip
use_batched_qu8), without a GPU: which shapes go through an int8 filter image
(fx_filter_image_used with FX_DTYPE_QU8) and what workspace they ask for."""

from __future__ import annotations

import pytest

from fenix_amd import _lib

QU8, F32, L2 = _lib.DTYPE_QU8, _lib.DTYPE_F32, _lib.METRIC_L2
N, D, NQ, K = 10_000_000, 768, 16, 100


def used(n=N, d=D, nq=NQ, k=K, metric=L2):
    return _lib.filter_image_used(n, d, QU8, nq, k, metric)


@pytest.mark.parametrize("metric", [_lib.METRIC_L2, _lib.METRIC_IP, _lib.METRIC_COS])
def test_a_quint8_batch_takes_the_image(metric):
    assert used(metric=metric)


def test_what_stays_on_the_exact_scan():
    assert not used(nq=1)                     # a single query
    with _lib.options(batch_min_queries=1):
        assert not used(nq=1)                 # (even where f32 single queries take the filter)
    assert not used(d=776)                    # d % 16 != 0: the scan's scalar variant
    assert used(d=784)
    with _lib.options(batched=0):
        assert not used()
    assert not used(k=_lib.get_option("i8_max_k") + 1)
    with _lib.options(i8_max_k=50):
        assert not used()
    with _lib.options(filter_image=16):       # no int8 image: nothing to filter codes with
        assert not used()
    with _lib.options(filter_image=0):
        assert not used()


def test_the_work_gate():
    work = _lib.get_option("qu8_batch_min_work")
    assert work > 0
    n = 100_000
    nq_below = max(2, work // (n * 128) - 1)
    assert nq_below * n * 128 < work and not used(n=n, d=128, nq=nq_below)
    assert used(n=n, d=128, nq=work // (n * 128) + 1)
    assert not used(n=1000, d=128, nq=2)
    with _lib.options(qu8_batch_min_work=0):
        assert used(n=1000, d=128, nq=2)
        assert not used(n=1000, d=128, nq=1)
    with _lib.options(qu8_batch_min_work=NQ * N * D):
        assert used()
    with _lib.options(qu8_batch_min_work=NQ * N * D + 1):
        assert not used()


def test_workspace_holds_the_batch_layout():
    """With an image the plan holds the int8 layout's candidate buffers (lower
    and upper bounds, 4x the f32 batch layout's 64 k slots per query) and the
    transformed queries; without one it is the exact scan's lists."""
    cap32 = max(64 * K, 16384)
    f32_buffers = 2 * NQ * cap32 * 8
    with_img = _lib.knn_workspace_bytes(N, D, QU8, NQ, K, img8=True)
    without = _lib.knn_workspace_bytes(N, D, QU8, NQ, K, img8=False)
    assert with_img >= f32_buffers
    assert with_img >= 2 * NQ * 4 * cap32 * 8 + NQ * D * 4
    assert with_img > without
    # the gate off: the same shape plans the exact scan either way
    with _lib.options(batched=0):
        assert _lib.knn_workspace_bytes(N, D, QU8, NQ, K, img8=True) == without


def test_other_dtypes_ignore_the_quint8_gate():
    before = _lib.filter_image_used(N, D, F32, NQ, K, L2)
    with _lib.options(qu8_batch_min_work=1 << 62):
        assert _lib.filter_image_used(N, D, F32, NQ, K, L2) == before
