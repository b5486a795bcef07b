"""Every kernel behind an int8-image search's selects and rescoring
(csrc/knn_select.hip, csrc/knn_exact.hip), each at the smallest shape that
reaches it: one table, one test.

A case runs ``scan`` and ``reduce`` apart, reads the candidate buffer's
capacity and the final counts in between (``Engine.filter_counts``), and
compares rows and distance bits with the same search under option "batched" 0
(per-query exact scans).  Before that it asserts what puts it on its path: the
int8 image served the search, the plan (``_plan``, the arithmetic of
csrc/knn_plan.hip plan_batched for an int8 image) has the phases, the prune
lists and the sort the case names, and no query left through the overflow
fallback unless the case forces all of them there.

Which launches a plan makes (capi.hip filter_phases_i8, reduce_impl), m phases:
  m >= 4: sample_threshold_kernel after phases 0 .. m-4;
  m >= 3: exact_threshold_kernel (resetting the counts) after phase m-3;
  m >= 2: after F1 exact_threshold_kernel with the overflow gate in its tail,
          then F2; m == 1: F1 reads every tile, no gate, no F2;
  more than 2 queries, or m == 1: exact_threshold_kernel once more;
  rescore_dense_kernel (<= 2 queries) or rescore_kernel; final_select_kernel,
  the wave sort for k <= 128, the LDS sort above.
With prune lists every select is preceded by prune_kernel, and the exact
threshold becomes select (rows out) + exact_kth_kernel + kth_max_kernel +
overflow_gate_kernel.  "force_fallback": the final select takes every query's
result from the fallback scan's lists.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from fenix_amd import _lib
from fenix_amd.engine import Engine, Shard
from oracle import oracle as O
from tests.test_gpu_quint8_batched import _codes, _queries

pytestmark = pytest.mark.gpu

METRICS = ["l2", "inner_product", "cosine"]
I8 = {"filter_image": 8, "batch_min_queries": 1, "qu8_batch_min_work": 0}
SELECT_ENTRIES = 16384  # kSelectEntries: the selects' LDS chunk and prune slice
QU8_SCALE, QU8_ZP = 1e-3, 64


def _plan(n, k, opts):
    """(cap, phases, prune lists) of plan_batched for an int8 image under the
    default sampling ratios (8, 16) or "batch_sample_ratio"."""
    cap = max(64 * k, 16384) * 4
    if opts.get("batch_cap", 0) >= 16 * k:
        cap = opts["batch_cap"]
    cap = -(-cap // 4096) * 4096
    rmax = cap // (4 * k)
    v = opts.get("batch_sample_ratio", 0)
    r1, r2 = (min(v, rmax),) * 2 if v >= 2 else (min(rmax, 8), min(rmax, 16))
    nums, r = [-(-n // 256)], r1
    while nums[-1] * 256 > cap:
        nums.append(-(-nums[-1] // r))
        r = r2
    o = opts.get("select_prune", 1)
    prune = 0 if o == 0 or (o == 1 and k < 512) or cap <= 2 * SELECT_ENTRIES else -(-cap // SELECT_ENTRIES)
    return cap, len(nums), prune


# (id, dtype, n, d, nq, k, metric, options, phases, prune lists, LDS sort)
CASES = [
    ("fused-gate", "f32", 40_000, 128, 3, 10, "l2", {"batch_cap": 4096}, 3, 0, False),
    ("sample-threshold", "f32", 40_000, 128, 3, 10, "cosine",
     {"batch_cap": 4096, "batch_sample_ratio": 2}, 5, 0, False),
    ("lds-sort", "f32", 40_000, 128, 3, 200, "inner_product", {"batch_cap": 16384}, 2, 0, True),
    ("one-phase", "f32", 10_000, 128, 3, 10, "cosine", {}, 1, 0, False),
    ("prune-k10", "f32", 40_000, 64, 3, 10, "l2", {"select_prune": 2, "batch_cap": 36864},
     2, 3, False),
    ("prune-k512", "f32", 140_000, 64, 1, 512, "inner_product", {}, 2, 8, True),
    ("fallback", "f32", 40_000, 128, 3, 10, "l2", {"batch_cap": 4096, "force_fallback": 1},
     3, 0, False),
    ("fallback-pruned", "f32", 40_000, 64, 3, 10, "l2",
     {"select_prune": 2, "batch_cap": 36864, "force_fallback": 1}, 2, 3, False),
]
# every <T, METRIC> of exact_threshold_kernel and of the two rescore kernels,
# which switch at kRescoreDenseMaxQ = 2 queries
CASES += [(f"{dt}-{m}-q{nq}", dt, 40_000, 128, nq, 10, m, {"batch_cap": 4096}, 3, 0, False)
          for dt in ("f32", "f16", "qu8") for m in METRICS for nq in (2, 3)]


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine.get(torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def _shard(dtype, n, d):
    """One corpus per (dtype, shape), left unchanged by every case."""
    e = Engine.get(torch.device("cuda", 0))
    if dtype == "qu8":
        codes = torch.from_numpy(_codes("wide", n, d, QU8_ZP)).to(e.device)
        return Shard(codes, 0, QU8_SCALE, QU8_ZP)
    x = torch.empty((n, d), dtype=torch.float16 if dtype == "f16" else torch.float32,
                    device=e.device)
    e.fill(x, 91)
    return Shard(x, 0)


@functools.lru_cache(maxsize=None)
def _exact(dtype, n, d, nq, k, metric):
    """(queries, distances, rows) of the per-query exact scans, computed once."""
    e = Engine.get(torch.device("cuda", 0))
    if dtype == "qu8":
        qh = _queries(nq, d, QU8_SCALE, 40.0)
    else:
        qh = O.fill_normal(nq, d, seed=95).astype(np.float32)
    q = torch.from_numpy(qh).to(e.device)
    with _lib.options(batched=0):
        dist, row = e.search([_shard(dtype, n, d)], q, _lib.METRICS[metric], k)
        torch.cuda.synchronize()
    return q, dist.cpu().numpy(), row.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_select_path_equals_exact_scans(eng, case):
    cid, dtype, n, d, nq, k, metric, opts, phases, prune, lds_sort = case
    m = _lib.METRICS[metric]
    shard = _shard(dtype, n, d)
    q, want_d, want_r = _exact(dtype, n, d, nq, k, metric)
    cap, got_phases, got_prune = _plan(n, k, opts)
    assert (got_phases, got_prune, k > 128) == (phases, prune, lds_sort)
    assert prune == 0 or cap > 2 * SELECT_ENTRIES
    eng.clear_images()
    with _lib.options(**I8, **opts):
        st = eng.scan(shard, q, m, k)
        count, got_cap = eng.filter_counts(shard, nq, m, k, st)
        assert st.bits == 8 and st.image is not None and count is not None, "no int8 image"
        assert got_cap == cap
        od = torch.empty((nq, k), dtype=torch.float32, device=eng.device)
        orow = torch.empty((nq, k), dtype=torch.int64, device=eng.device)
        eng.reduce(shard, q, m, k, st, od, orow)
        torch.cuda.synchronize()
    eng.clear_images()
    print(f"{cid}: cap {cap} counts {count.tolist()[:4]}")
    if not opts.get("force_fallback"):
        assert (count.astype(np.int64) <= cap).all(), f"overflowed: {count.max()} > {cap}"
    np.testing.assert_array_equal(orow.cpu().numpy(), want_r, err_msg=f"{cid}: rows")
    np.testing.assert_array_equal(od.cpu().numpy().view(np.uint32), want_d.view(np.uint32),
                                  err_msg=f"{cid}: distance bits")
