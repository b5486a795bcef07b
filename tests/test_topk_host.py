"""Host checks of tests/topk_ref.py, the exact references the GPU selection
tests stand on (tests/test_gpu_topk_order.py, tests/test_gpu_merge_tree.py):
the plan model against the library's planner, the references against a
brute-force selection, the key encoders' exactness in f32, and that the two
comparison helpers reject six kinds of wrong selection."""

from __future__ import annotations

import math

import numpy as np
import pytest

from fenix_amd import _lib
from tests import parity
from tests import topk_ref as R


# ------------------------------------------------------------- 1. plan model


@pytest.mark.parametrize("shape", [(R.MERGE_NQ,) + s for s in R.MERGE_SHAPES]
                         + R.MERGE_SPLIT_SHAPES, ids=str)
def test_plan_model_equals_library(shape):
    """fx_topk_merge_workspace_bytes (no device needed) against the model, and
    the levels the shape table claims against the model's."""
    nq, parts, kin, k, levels = shape
    if kin > R.MAX_K or k > R.MAX_K:
        assert levels == 0, "the sort path has no merge tree"
        return
    plan = R.plan_merge(nq, parts, kin, k)
    assert plan["levels"] == levels, plan
    assert plan["lists"][0] == parts and plan["klen"][0] == kin
    assert all(kl == k for kl in plan["klen"][1:])
    want = R.align256(nq * parts * kin * 8) + plan["ws_bytes"]
    assert _lib.merge_workspace_bytes(nq, parts, kin, k) == want


def test_plan_model_lds_room():
    """k in 2049..4096 (the coded index's probe merge): the lists share the
    160 KB of LDS with a result area of 4096 slots, so a level folds less
    than 16 384 entries; the model and the library agree there too."""
    for k in (2049, 4096):
        plan = R.plan_merge(3, 64, 512, k)
        assert plan["group"][0] * 512 * 8 + R.MERGE_SHARED + 4096 * 8 <= R.MERGE_LDS
        assert plan["group"][0] * 512 < R.MERGE_ENTRIES


def test_scan_shape_model():
    """The kernel classes the GPU cases name."""
    S = R.scan_shape
    assert S("f32", 8) == {"W": 4, "L": 1, "U": 8, "nch": 1, "occ_cap": 2}
    assert S("f32", 768) == {"W": 4, "L": 12, "U": 2, "nch": 1, "occ_cap": 1}
    assert S("f16", 1536) == {"W": 8, "L": 12, "U": 2, "nch": 1, "occ_cap": 1}
    assert S("f32", 5) == {"W": 1, "L": 16, "U": 1, "nch": 1, "occ_cap": 1}
    assert S("f32", 8, aligned=False)["W"] == 1
    assert S("f32", 3072) == {"W": 4, "L": 24, "U": 1, "nch": 2, "occ_cap": 1}
    assert S("qu8", 64) == {"W": 16, "L": 1, "U": 8, "nch": 1, "occ_cap": 3}
    assert [R.scan_cap(k, 8) for k in (1, 10, 128, 224, 225, 1000, 1024)] == \
        [256, 256, 256, 512, 512, 2048, 2048]
    assert R.scan_cap(128, 1) == 256 and R.scan_cap(129, 1) == 512
    assert R.near_prime(4096) == 4099 and R.near_prime(13) == 13


# ------------------------------------------- 2. reference against brute force


def _less(a, b):
    """(distance, row) order written out: -0 == +0, NaN after +inf, then row."""
    (da, ra), (db, rb) = a, b
    na, nb = math.isnan(da), math.isnan(db)
    if na != nb:
        return nb
    if not na and da != db:
        return da < db
    return ra < rb


def _brute(entries, k):
    """k smallest (distance, row) pairs by repeated minimum; None row: empty."""
    pool = [e for e in entries if e[1] is not None]
    out = []
    while pool and len(out) < k:
        best = 0
        for i in range(1, len(pool)):
            if _less(pool[i], pool[best]):
                best = i
        out.append(pool.pop(best))
    return out


SPECIAL = [0.0, -0.0, 1.5, -1.5, float("inf"), float("-inf"), float("nan"), 1e-45, -1e-45,
           3.0, 3.0, 3.0, -7.25]


@pytest.mark.parametrize("seed", range(6))
def test_reference_equals_brute_force(seed):
    rng = np.random.RandomState(seed)
    n = 40
    dist = rng.choice(np.array(SPECIAL, dtype=np.float32), size=n)
    # search: masked rows are dropped
    mask = rng.rand(n) < 0.7
    base = 1000 * seed
    for k in (1, 5, int(mask.sum()), int(mask.sum()) + 3):
        gd, gr = R.search_ref(dist, mask, base, k)
        want = _brute([(float(dist[i]), base + i) for i in range(n) if mask[i]], k)
        assert gr.tolist() == [r for _, r in want] + [-1] * (k - len(want))
        for j, (dv, _) in enumerate(want):
            if math.isnan(dv):
                assert gd[j:j + 1].view(np.uint32)[0] == R.NAN_BITS
            else:  # -0 comes back as +0 (order_key folds them)
                assert gd[j] == dv and (dv != 0 or not np.signbit(gd[j]))
        assert (gd[len(want):].view(np.uint32) == R.NAN_BITS).all()
    # merge: duplicates kept as often as they occur, empty slots dropped
    rows = rng.choice(np.array([-1, -5, 0, 1, 2, 2, 7, 0xFFFFFFFE, 0xFFFFFFFF, 1 << 33]), size=n)
    for k in (1, 7, n + 2):
        gd, gr = R.merge_ref(dist.reshape(4, 10), rows.reshape(4, 10), k)
        want = _brute([(float(dist[i]), int(rows[i]) if 0 <= rows[i] < 0xFFFFFFFF else None)
                       for i in range(n)], k)
        assert gr.tolist() == [r for _, r in want] + [-1] * (k - len(want))
        wd = np.array([dv for dv, _ in want] + [np.nan] * (k - len(want)), dtype=np.float32)
        np.testing.assert_array_equal(parity.order_key(gd), parity.order_key(wd))


# ------------------------------------------------------------ 3. exact keys


def _lane_order_dot(x, q, slot):
    """f32 multiply-adds as the scan sums a row: lane jl of 16 takes the
    16-byte slots jl, jl + 16, ... in ascending element order, then the 16
    lane sums fold pairwise."""
    n, d = x.shape
    acc = np.zeros((n, 16), dtype=np.float32)
    for s in range(-(-d // slot)):
        for e in range(s * slot, min(d, (s + 1) * slot)):
            acc[:, s % 16] = acc[:, s % 16] + x[:, e].astype(np.float32) * q[e]
    w = 16
    while w > 1:
        w //= 2
        acc = acc[:, :w] + acc[:, w:2 * w]
    return acc[:, 0]


def _shuffled_dot(x, q, seed):
    acc = np.zeros(x.shape[0], dtype=np.float32)
    for e in np.random.RandomState(seed).permutation(x.shape[1]):
        acc = acc + x[:, e].astype(np.float32) * q[e]
    return acc


@pytest.mark.parametrize("dtype,d", [("f32", 8), ("f32", 5), ("f16", 24), ("f16", 1536),
                                     ("qu8", 64), ("qu8", 48)])
def test_key_encoders_are_exact(dtype, d):
    limit = R.ENCODING[dtype][2]
    keys = np.concatenate([[0, limit - 1, 1, limit // 2],
                           np.random.RandomState(5).randint(0, limit, size=10_000)])
    x = R.encode_rows(dtype, d, keys)
    q = R.key_query(dtype, d)
    assert x.dtype == R.NP_DTYPE[dtype] and q.dtype == np.float32
    cols = R.key_columns(dtype, d)
    slot = R.SLOT_ELEMS[dtype]
    if d >= slot * len(cols):  # the digit columns sit in different 16-byte slots
        assert len({c // slot for c in cols}) == len(cols)
    for got in (_lane_order_dot(x, q, slot), _shuffled_dot(x, q, 1), _shuffled_dot(x, q, 2)):
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.astype(np.int64), keys)
        # the search's distance -K, and its round trip through the composite
        dist = -got
        np.testing.assert_array_equal(parity.key_float(parity.order_key(dist)).astype(np.int64),
                                      -keys)


def test_l2_and_cosine_constructions():
    """L2: squares of levels up to 4095 are exact in f32, and so is their
    root.  Cosine: 64 levels are 100 near-tie widths apart."""
    x = np.arange(-4095, 4096, dtype=np.int64)
    sq = (x.astype(np.float32) * x.astype(np.float32))
    np.testing.assert_array_equal(sq.astype(np.int64), x * x)
    np.testing.assert_array_equal(np.sqrt(sq).astype(np.int64), np.abs(x))
    ref = R.cosine_ref(R.cosine_rows(np.arange(64), 64))
    assert np.diff(ref).min() >= 100 * parity.NEAR_RTOL


# --------------------------------------------- 4. wrong selections are rejected
#
# Each mutant is a selection over a pool of composites in arrival order
# (a search: row order; a merge: the lists back to back) with one defect.


def _mut_drop_tile(comps, k, at, width):
    """one tile of 4U rows never reaches the list"""
    return R.select(np.delete(comps, np.arange(at, at + width)), k)


def _mut_row_twice(comps, k):
    """a row kept twice: the second-best slot repeats the best"""
    out = R.select(comps, k)
    out[1] = out[0]
    return out


def _mut_highest_row(comps, k):
    """ties broken by the highest row"""
    key = parity.comp_key(comps).astype(np.int64)
    row = parity.comp_row(comps)
    order = np.lexsort((-row, key))[:k]
    return comps[order]


def _mut_le_threshold(comps, k):
    """a threshold compare of <= after compaction: a later entry whose
    distance equals the k-th kept one displaces it (running selection on the
    distance key; the kept set is then sorted as usual)"""
    kept = []
    for c in comps.tolist():
        if len(kept) < k:
            kept.append(c)
            continue
        worst = max(range(k), key=lambda i: (kept[i] >> 32, i))
        if (c >> 32) <= (kept[worst] >> 32):
            kept[worst] = c
    return R.select(np.array(kept, dtype=np.uint64), k)


def _mut_skip_last_list(comps, k, tail):
    """the last list of a level (a search: the last block's rows) skipped"""
    return R.select(comps[: len(comps) - tail], k)


def _mut_one_duplicate_short(comps, k):
    """one entry too few kept at the k-th composite: the next one fills in"""
    order = np.sort(comps)
    above = order[order > order[k - 1]]
    return np.concatenate([order[: k - 1], above[:1]])


def _search_pool():
    """96 rows, k = 8: ten rows tie at the smallest key, three of them in the
    last 16 rows; the rest descend."""
    n, k, base = 96, 8, 500
    keys = np.arange(n + 10, 10, -1).astype(np.int64)
    keys[[3, 40, 41, 42, 50, 60, 70, 85, 90, 93]] = 1
    # (the negated key query: distance = +K)
    dist = -_lane_order_dot(R.encode_rows("f16", 24, keys), -R.key_query("f16", 24), 8)
    return dist, base, k


def _merge_pool():
    """6 lists of 8, k = 10: the k-th composite occurs 5 times, 2 of them
    inside the top k, and once more at its distance with a higher row; the
    last list holds winners."""
    dist = np.full((6, 8), 9.0, dtype=np.float32)
    row = np.arange(48, dtype=np.int64).reshape(6, 8) + 100
    dist[0, :4] = [1, 1, 2, 2]
    dist[5, 4:8] = [0.5, 2, 2, 1]
    dist[5, 0] = 3.0
    for lst, slot in ((1, 0), (2, 3), (2, 4), (3, 7), (4, 1)):  # 5 copies of the k-th
        dist[lst, slot], row[lst, slot] = 3.0, 7
    return dist, row, 10


def _mutants(comps, k, tile_at, tile, tail):
    return {
        "tile dropped": _mut_drop_tile(comps, k, tile_at, tile),
        "row kept twice": _mut_row_twice(comps, k),
        "ties by highest row": _mut_highest_row(comps, k),
        "<= after compaction": _mut_le_threshold(comps, k),
        "last list skipped": _mut_skip_last_list(comps, k, tail),
        "one duplicate short": _mut_one_duplicate_short(comps, k),
    }


def test_search_comparison_rejects_wrong_selections():
    dist, base, k = _search_pool()
    comps = R.search_comps(dist, None, base)
    gd, gr = R.decode(R.select(comps, k))
    R.check_search(gd, gr, dist, None, base, k)  # the right answer passes
    assert gr.tolist() == [503, 540, 541, 542, 550, 560, 570, 585]
    muts = _mutants(comps, k, tile_at=32, tile=32, tail=16)  # one tile of 4U rows, U = 8
    assert len(muts) == 6
    for name, wrong in muts.items():
        wd, wr = R.decode(wrong)
        with pytest.raises(AssertionError):
            R.check_search(wd, wr, dist, None, base, k, name)
    # and a wrong distance bit alone
    gd2 = gd.copy()
    gd2.view(np.uint32)[k - 1] ^= 1
    with pytest.raises(AssertionError):
        R.check_search(gd2, gr, dist, None, base, k)


def test_merge_comparison_rejects_wrong_selections():
    dist, row, k = _merge_pool()
    comps = R.merge_comps(dist, row).ravel()
    gd, gr = R.decode(R.select(comps, k))
    R.check_merge(gd, gr, dist, row, k)
    assert gr.tolist() == [144, 100, 101, 147, 102, 103, 145, 146, 7, 7]
    muts = _mutants(comps, k, tile_at=0, tile=4, tail=8)
    assert len(muts) == 6
    for name, wrong in muts.items():
        wd, wr = R.decode(wrong)
        with pytest.raises(AssertionError):
            R.check_merge(wd, wr, dist, row, k, name)
    # an empty slot reported as row 0 instead of -1
    gd3, gr3 = R.merge_ref(dist[:1], row[:1], k)
    assert gr3[-1] == -1
    gr3 = np.where(gr3 < 0, 0, gr3)
    with pytest.raises(AssertionError):
        R.check_merge(gd3, gr3, dist[:1], row[:1], k)
