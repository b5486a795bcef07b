"""Per-query row masks, the parts that need no GPU: the coalescer's request
payloads (fenix_amd/coalesce.py), the byte rule that decides whether a batch
of filtered searches runs as one per-query-mask pass (engine.qmask_batch_pays),
fx_qmask_words, and the planner's answer for which shapes run the int8 filter
with admission bits and which scan exactly (fx_qmask_filter_used)."""

from __future__ import annotations

import threading

import numpy as np
import pytest

from fenix_amd import _lib, coalesce

F32, F16, QU8, L2 = _lib.DTYPE_F32, _lib.DTYPE_F16, _lib.DTYPE_QU8, _lib.METRIC_L2


# ---------------------------------------------------------------- coalescer --
def _rows_run(calls):
    """run(queries, K[, extras]): distance j of query i is q[i, 0] + j, and a
    third array carries the payload seen for the query (-1: none)."""
    def run(queries, kk, *rest):
        calls.append((queries.shape[0], kk, rest))
        d = queries[:, :1] + np.arange(kk, dtype=np.float32)[None, :]
        r = np.tile(np.arange(kk, dtype=np.int64), (queries.shape[0], 1))
        tag = np.full((queries.shape[0], kk), -1, dtype=np.int64)
        if rest:
            for i, e in enumerate(rest[0]):
                if e is not None:
                    tag[i] = e
        return d, r, tag
    return run


def _queue_behind_a_leader(c, key, run, jobs):
    """Start a leader whose batch blocks, queue ``jobs`` [(value, k, extra)]
    behind it, release it, and return every job's result in order."""
    started, release = threading.Event(), threading.Event()

    def lead_run(queries, kk, *rest):
        started.set()
        release.wait(10)
        return run(queries, kk, *rest)

    out = [None] * len(jobs)
    err = [None] * len(jobs)
    lead = threading.Thread(target=lambda: c.search(key, lead_run, np.zeros(4, np.float32), 1))
    lead.start()
    assert started.wait(10)

    def one(i):
        v, k, extra = jobs[i]
        try:
            out[i] = c.search(key, run, np.full(4, v, np.float32), k, extra)
        except BaseException as e:  # noqa: BLE001 (reported to the test)
            err[i] = e

    threads = []
    for i in range(len(jobs)):
        t = threading.Thread(target=one, args=(i,))
        t.start()
        threads.append(t)
        # queue in order: until the request is queued (it then blocks behind the
        # leader), or its thread has ended (a request that was refused: err[i])
        while t.is_alive():
            with c._lock:
                if len(c._queues.get(key, [])) >= sum(x.is_alive() for x in threads):
                    break
    release.set()
    lead.join(10)
    for t in threads:
        t.join(10)
    return out, err


def test_a_mixed_batch_calls_run_with_the_payloads_and_slices_per_request():
    c, calls = coalesce.Coalescer(), []
    jobs = [(1.0, 3, None), (2.0, 5, 7), (3.0, 2, None), (4.0, 4, 9)]
    out, err = _queue_behind_a_leader(c, "k", _rows_run(calls), jobs)
    assert err == [None] * 4
    # the leader's own batch (plain, two arguments), then one batch of four
    assert [(n, k, len(rest)) for n, k, rest in calls] == [(1, 1, 0), (4, 5, 1)]
    assert calls[1][2][0] == [None, 7, None, 9]
    for (v, k, extra), (d, r, tag) in zip(jobs, out):
        assert d.shape == (1, k) and r.shape == (1, k)
        np.testing.assert_array_equal(d[0], v + np.arange(k, dtype=np.float32))
        assert (tag == (-1 if extra is None else extra)).all()
    assert c.requests == 5 and c.batches == 2


def test_a_plain_batch_calls_run_with_two_arguments():
    c, calls = coalesce.Coalescer(), []
    out, err = _queue_behind_a_leader(c, "k", _rows_run(calls), [(1.0, 2, None), (2.0, 3, None)])
    assert err == [None, None]
    assert [(n, k, rest) for n, k, rest in calls] == [(1, 1, ()), (2, 3, ())]
    assert out[1][0].shape == (1, 3)


def test_a_solo_request_with_a_payload_gets_it():
    c, calls = coalesce.Coalescer(), []
    d, r, tag = c.search("k", _rows_run(calls), np.ones(4, np.float32), 3, extra=5)
    assert calls[0][0] == 1 and calls[0][2] == ([5],) and (tag == 5).all()


def test_a_failing_masked_batch_fails_every_request_of_it():
    c = coalesce.Coalescer()

    def run(queries, kk, *rest):
        if rest:
            raise RuntimeError("boom")
        return (np.zeros((queries.shape[0], kk), np.float32),
                np.zeros((queries.shape[0], kk), np.int64))

    out, err = _queue_behind_a_leader(c, "k", run, [(1.0, 2, None), (2.0, 2, 1), (3.0, 2, None)])
    assert all(isinstance(e, RuntimeError) and "boom" in str(e) for e in err)
    # the key is free again
    assert c.search("k", run, np.ones(4, np.float32), 2)[0].shape == (1, 2)


def test_masked_batches_hold_at_most_128_requests():
    assert coalesce.MASKED_MAX == 128
    c, calls = coalesce.Coalescer(), []
    jobs = [(float(i), 1, i if i % 2 else None) for i in range(150)]
    out, err = _queue_behind_a_leader(c, "k", _rows_run(calls), jobs)
    assert err == [None] * 150
    assert [n for n, _, _ in calls] == [1, 128, 22]
    assert len(calls[1][2][0]) == 128 and len(calls[2][2][0]) == 22
    for (v, _, extra), (d, _, tag) in zip(jobs, out):
        assert d[0, 0] == v and tag[0, 0] == (-1 if extra is None else extra)
    # plain batches keep the coalescer's own limit
    c2, calls2 = coalesce.Coalescer(), []
    _queue_behind_a_leader(c2, "k", _rows_run(calls2), [(float(i), 1, None) for i in range(150)])
    assert [n for n, _, _ in calls2] == [1, 150]


# ---------------------------------------------------------------- byte rule --
def test_qmask_batch_pays_truth_table():
    from fenix_amd.engine import Engine, qmask_batch_pays

    n, d = 10_000_000, 768
    assert Engine.SPARSE == 0.5
    batch16 = n * (d + 16) + n * 4 * 4  # 16 queries: 4 words of admission bits per row

    def single(counts, itemsize=4):
        return sum((c if c < 0.5 * n else n) * d * itemsize for c in counts)

    # 16 requests keeping half the rows each walk the column 16 times
    assert qmask_batch_pays([n // 2] * 16, n, d, 4, 16, 1.0)
    assert single([n // 2] * 16) / batch16 > 30
    # the SPARSE switch: just under half reads the kept rows only
    lo, hi = [n // 2 - 1] * 2, [n // 2] * 2
    batch2 = n * (d + 16) + n * 16
    assert single(lo) == 2 * (n // 2 - 1) * d * 4 and single(hi) == 2 * n * d * 4
    for counts in (lo, hi):
        r = single(counts) / batch2
        assert qmask_batch_pays(counts, n, d, 4, 2, r * 0.999)
        assert not qmask_batch_pays(counts, n, d, 4, 2, r * 1.001)
    # very selective filters: the row-list scans read less than one image pass
    assert not qmask_batch_pays([1000] * 16, n, d, 4, 16, 1.0)
    assert single([1000] * 16) < batch16
    # a plain request (None) walks everything
    assert qmask_batch_pays([None, 10], n, d, 4, 2, 1.0)
    # one-byte codes: two requests read 2 n d against n (d + 16) + 16 n
    assert qmask_batch_pays([n, n], n, d, 1, 2, 1.0)
    assert not qmask_batch_pays([n, n], n, d, 1, 2, 2.0)
    # more queries, more admission words: 130 queries need 8 words
    assert not qmask_batch_pays([n] * 130, n, 16, 1, 130, 130 * 16 / (32 + 32) * 1.001)
    assert qmask_batch_pays([n] * 130, n, 16, 1, 130, 130 * 16 / (32 + 32) * 0.999)
    # ratio 0: always
    assert qmask_batch_pays([0, 0], n, d, 4, 2, 0.0)


def test_qmask_batch_min_ratio_is_a_library_option():
    from fenix_amd.engine import qmask_batch_pays

    assert "qmask_batch_min_ratio" in _lib.OPTIONS
    n, d = 1_000_000, 128
    counts = [1000, 1000]
    assert not qmask_batch_pays(counts, n, d, 4, 2)
    with _lib.options(qmask_batch_min_ratio=0):
        assert qmask_batch_pays(counts, n, d, 4, 2)


# ------------------------------------------------------------------ planner --
def test_qmask_words():
    for nq, want in [(1, 4), (31, 4), (32, 4), (33, 4), (128, 4), (129, 8), (130, 8), (256, 8),
                     (257, 12)]:
        assert _lib.qmask_words(nq) == want, nq
    assert _lib.qmask_words(0) == 0


N, D, K = 10_000_000, 768, 100


def used(n=N, d=D, dtype=F32, nq=16, k=K, metric=L2):
    return _lib.qmask_filter_used(n, d, dtype, nq, k, metric)


@pytest.mark.parametrize("metric", [_lib.METRIC_L2, _lib.METRIC_IP, _lib.METRIC_COS])
def test_which_slices_a_qmask_batch_takes(metric):
    assert used(nq=2, metric=metric) == 64
    assert used(nq=64, metric=metric) == 64
    assert used(nq=65, metric=metric) == 128     # q128 at 768-d stays under 160 KB
    assert used(nq=128, metric=metric) == 128
    assert used(nq=130, metric=metric) == 128    # two slices
    assert used(dtype=F16, nq=40, metric=metric) == 64
    assert used(dtype=QU8, nq=40, metric=metric) == 64


def test_what_a_qmask_search_scans_exactly():
    assert used(nq=1) == 0
    with _lib.options(batch_min_queries=1):
        assert used(nq=1) == 0
    assert used(d=772) == 0                       # f32 rows, d % 8 != 0: no image
    assert used(k=_lib.get_option("i8_max_k") + 1) == 0
    assert used(k=_lib.max_k() + 1) == 0
    with _lib.options(i8_max_k=50):
        assert used() == 0
    with _lib.options(filter_image=16):
        assert used() == 0
    with _lib.options(filter_image=0):
        assert used() == 0
    with _lib.options(batched=0):
        assert used() == 0
    assert used(dtype=QU8, d=776, nq=40) == 0     # quint8: d % 16


def test_row_lengths_the_slices_fit():
    """A q128 slice holds (160 KB - its tables and segments) / 128 B per 64
    components; past it a batch of more than 64 queries runs slices of 64, and
    past those the exact scan."""
    fits128 = [d for d in range(64, 4096, 64) if used(d=d, nq=100) == 128]
    fits64 = [d for d in range(64, 4096, 64) if used(d=d, nq=100) == 64]
    assert fits128 and fits64 and 768 in fits128
    d128, d64 = max(fits128), max(fits64)
    assert fits128 == list(range(64, d128 + 1, 64))
    assert fits64 == list(range(d128 + 64, d64 + 1, 64))
    assert used(d=d64 + 64, nq=100) == 0 and used(d=d64 + 64, nq=2) == 0
    assert used(d=d64, nq=2) == 64
    # the bytes behind it: queries x padded row bytes beside ~50 / ~27 KB of tables
    assert 100 * 1024 < 128 * d128 <= 160 * 1024 - 48 * 1024
    assert 128 * 1024 < 64 * d64 <= 160 * 1024 - 24 * 1024


def test_workspace_covers_both_plans():
    """A qmask search may plan exact where the plain search plans the filter:
    the one workspace size (fx_knn_workspace_bytes_img8) holds either."""
    for d in (768, 2048, 4096):
        both = _lib.knn_workspace_bytes(100_000, d, F32, 100, 10, img8=True)
        with _lib.options(batched=0):
            exact = _lib.knn_workspace_bytes(100_000, d, F32, 100, 10, img8=True)
        assert both >= exact
