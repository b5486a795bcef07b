"""fx_topk_merge (Engine.merge) against the exact merge reference
(tests/topk_ref.py merge_ref: np.sort of the composites): rows and distance
bits equal, including duplicates, -1 rows and the NaN bit pattern.

Shapes (tests/topk_ref.py MERGE_SHAPES; tests/test_topk_host.py pins their
level counts to the planner): one level, the bitonic sort's width at a power
of two and one to either side, trees of two and three levels (among them the
ones plan_single builds for 512 scan blocks), the sort path above 1024, and
run_merge's split of the grid at 65 535 queries.  Content: where the winners
sit, unsorted lists, too few valid entries, equal composites across lists
(the only inputs for which block_keep_k's quota decides between real
entries), special distances and rows that encode to the empty composite.
"""

from __future__ import annotations

import time

import numpy as np
import pytest
import torch

from fenix_amd.engine import Engine
from tests import topk_ref as R

pytestmark = pytest.mark.gpu

NQ = R.MERGE_NQ


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine.get(torch.device("cuda", 0))


def _merge(eng, dist, row, k):
    od, orow = eng.merge(torch.from_numpy(dist).to(eng.device),
                         torch.from_numpy(row).to(eng.device), k)
    torch.cuda.synchronize()
    return od.cpu().numpy(), orow.cpu().numpy()


def _check(eng, dist, row, k, what):
    """dist, row [nq, parts, kin]: one merge, every query against the reference."""
    gd, gr = _merge(eng, dist, row, k)
    assert gd.shape == (dist.shape[0], k) and gr.shape == (dist.shape[0], k)
    for i in range(dist.shape[0]):
        R.check_merge(gd[i], gr[i], dist[i], row[i], k, f"{what} query {i}")


def _sorted_lists(dist, row):
    """Each list in (distance, row) order, as a search writes them."""
    comps = R.merge_comps(dist, row)
    order = np.argsort(comps, axis=-1, kind="stable")
    return np.take_along_axis(dist, order, -1), np.take_along_axis(row, order, -1)


def _filler(rng, parts, kin, lo=10.0, hi=20.0):
    dist = rng.uniform(lo, hi, size=(parts, kin)).astype(np.float32)
    row = rng.permutation(parts * kin).astype(np.int64).reshape(parts, kin) + 1000
    return dist, row


def _plant(rng, dist, row, where, lo=0.0, hi=1.0):
    """Winners (distances in [lo, hi)) at the flat positions ``where``."""
    dist.reshape(-1)[where] = rng.uniform(lo, hi, size=len(where)).astype(np.float32)


# -------------------------------------------------------------------- content


def mixed(rng, parts, kin, k):
    """Random lists with a little of everything: repeated distances, empty
    slots, a few equal composites."""
    dist = rng.randint(0, 4 * max(k, 8), size=(parts, kin)).astype(np.float32) / 4
    row = rng.randint(0, 1 << 20, size=(parts, kin)).astype(np.int64)
    row[rng.rand(parts, kin) < 0.1] = -1
    if parts * kin >= 8:
        src = rng.randint(0, parts * kin, size=4)
        dst = rng.randint(0, parts * kin, size=4)
        dist.reshape(-1)[dst] = dist.reshape(-1)[src]
        row.reshape(-1)[dst] = row.reshape(-1)[src]
    return _sorted_lists(dist, row)


def winners_last_list(rng, parts, kin, k):
    dist, row = _filler(rng, parts, kin)
    m = min(k, kin)
    _plant(rng, dist, row, (parts - 1) * kin + np.arange(m))
    return _sorted_lists(dist, row)


def winners_list0(rng, parts, kin, k):
    dist, row = _filler(rng, parts, kin)
    _plant(rng, dist, row, np.arange(min(k, kin)))
    return _sorted_lists(dist, row)


def two_per_list(rng, parts, kin, k):
    dist, row = _filler(rng, parts, kin)
    _plant(rng, dist, row, (np.arange(parts)[:, None] * kin + np.arange(min(2, kin))).ravel())
    return _sorted_lists(dist, row)


def descending_across_lists(rng, parts, kin, k):
    """Every list beats the one before it."""
    dist, row = _filler(rng, parts, kin, 0.0, 1.0)
    dist += (parts - 1 - np.arange(parts, dtype=np.float32))[:, None]
    return _sorted_lists(dist, row)


def unsorted_lists(rng, parts, kin, k):
    dist, row = _filler(rng, parts, kin, 0.0, 100.0)
    return dist, row  # as drawn


def too_few_valid(rng, parts, kin, k):
    """Only k-2 valid entries among all."""
    dist, row = _filler(rng, parts, kin)
    keep = rng.permutation(parts * kin)[: max(k - 2, 0)]
    valid = np.zeros(parts * kin, dtype=bool)
    valid[keep] = True
    row.reshape(-1)[~valid] = -1
    return dist, row


def all_equal(rng, parts, kin, k):
    return (np.full((parts, kin), 1.5, dtype=np.float32),
            np.full((parts, kin), 7, dtype=np.int64))


def kth_five_times(rng, parts, kin, k):
    """k-2 entries below the k-th composite, which occurs 5 times (2 of them
    inside the top k), everything else above."""
    assert parts * kin >= k + 3
    dist, row = _filler(rng, parts, kin)
    where = rng.permutation(parts * kin)[: k + 3]
    _plant(rng, dist, row, where[: k - 2])
    dist.reshape(-1)[where[k - 2:]] = 2.0
    row.reshape(-1)[where[k - 2:]] = 99
    return _sorted_lists(dist, row)


def duplicated_lists(rng, parts, kin, k):
    dist, row = _filler(rng, parts, kin, 0.0, 100.0)
    half = parts // 2
    dist[half: 2 * half], row[half: 2 * half] = dist[:half], row[:half]
    if parts % 2:
        dist[-1], row[-1] = dist[0], row[0]
    return _sorted_lists(dist, row)


def special_distances(rng, parts, kin, k):
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 1e-45, 3e38],
                        dtype=np.float32)
    dist = rng.choice(specials, size=(parts, kin))
    # (few real entries: the specials reach the top k)
    row = rng.randint(0, 1 << 16, size=(parts, kin)).astype(np.int64)
    row[rng.rand(parts, kin) < 1.0 - 1.5 * k / (parts * kin)] = -1
    return _sorted_lists(dist, row)


def empty_rows(rng, parts, kin, k):
    """Rows of -1 and 2^32-1 (both the empty composite) with the best
    distances, the row 2^32-2 (the largest real one) among the valid."""
    dist, row = _filler(rng, parts, kin, 0.0, 100.0)
    r = rng.rand(parts, kin)
    row[r < 0.3] = -1
    row[(r >= 0.3) & (r < 0.6)] = 0xFFFFFFFF
    dist[r < 0.6] = -5.0
    row.reshape(-1)[rng.randint(0, parts * kin)] = 0xFFFFFFFE
    return dist, row


PATTERNS = [winners_last_list, winners_list0, two_per_list, descending_across_lists,
            unsorted_lists, too_few_valid, all_equal, kth_five_times, duplicated_lists,
            special_distances, empty_rows]
PATTERN_SHAPES = [(512, 1000, 1000), (17, 1024, 1024)]


def _queries(fn, seed, parts, kin, k, nq=NQ):
    """nq queries of different content."""
    pairs = [fn(np.random.RandomState(1000 * seed + i), parts, kin, k) for i in range(nq)]
    return (np.ascontiguousarray(np.stack([p[0] for p in pairs]), dtype=np.float32),
            np.ascontiguousarray(np.stack([p[1] for p in pairs]), dtype=np.int64))


# ---------------------------------------------------------------------- tests


@pytest.mark.parametrize("shape", R.MERGE_SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_merge_shapes(eng, shape):
    parts, kin, k, levels = shape
    if levels:  # the table's claim, tied to the planner by tests/test_topk_host.py
        assert R.plan_merge(NQ, parts, kin, k)["levels"] == levels
    else:
        assert kin > R.MAX_K or k > R.MAX_K
    dist, row = _queries(mixed, parts + kin + k, parts, kin, k)
    _check(eng, dist, row, k, f"{shape}")


@pytest.mark.parametrize("shape", PATTERN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda f: f.__name__)
def test_merge_content(eng, pattern, shape):
    parts, kin, k = shape
    assert R.plan_merge(NQ, parts, kin, k)["levels"] >= 2
    dist, row = _queries(pattern, PATTERNS.index(pattern), parts, kin, k)
    _check(eng, dist, row, k, f"{pattern.__name__} {shape}")


def test_merge_kth_duplicates_small(eng):
    """One level, k = 10 of 6 lists of 8: the k-th composite 5 times over 4
    lists, 2 inside the top k (the host mutation test's pool)."""
    from tests.test_topk_host import _merge_pool

    dist, row, k = _merge_pool()
    _check(eng, dist[None], row[None], k, "kth duplicates")


@pytest.mark.parametrize("shape", R.MERGE_SPLIT_SHAPES, ids=lambda s: "x".join(map(str, s[:4])))
def test_merge_grid_split(eng, shape):
    """More than 65 535 queries: run_merge launches every level in two grids.
    The input comes from integer arithmetic on the device; one call must
    equal two half calls bit for bit, and the queries around the split are
    checked on the host."""
    nq, parts, kin, k, levels = shape
    assert nq > 65535 and R.plan_merge(nq, parts, kin, k)["levels"] == levels
    t0 = time.time()
    total = nq * parts * kin
    idx = torch.arange(total, dtype=torch.int64, device=eng.device)
    h = (idx * 2654435761) % 1000003
    dist = (h % 4099).to(torch.float32).view(nq, parts, kin)
    row = torch.where(h % 7 == 0, torch.full_like(h, -1), h).view(nq, parts, kin)
    del idx, h
    od, orow = eng.merge(dist, row, k)
    half = nq // 2
    for lo, hi in ((0, half), (half, nq)):
        pd, pr = eng.merge(dist[lo:hi], row[lo:hi], k)
        assert torch.equal(pd.view(torch.int32), od[lo:hi].view(torch.int32))
        assert torch.equal(pr, orow[lo:hi])
    torch.cuda.synchronize()
    qs = [0, 65534, 65535, 65536]
    gd, gr = od[qs].cpu().numpy(), orow[qs].cpu().numpy()
    hd, hr = dist[qs].cpu().numpy(), row[qs].cpu().numpy()
    for j, qi in enumerate(qs):
        R.check_merge(gd[j], gr[j], hd[j], hr[j], k, f"{shape} query {qi}")
    del dist, row, od, orow
    eng._ws = None  # (the 1.7 GB workspace of the larger case)
    torch.cuda.empty_cache()
    print(f"grid split {shape}: {time.time() - t0:.2f} s")
