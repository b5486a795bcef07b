"""The exact scan's selection under adversarial row orders, against exact
references (tests/topk_ref.py): planted keys give every row a distance the
test chooses, so rows and distance bits must simply be equal.

Every other bit-identity test of the batched paths compares with the exact
scan; this file pins the exact scan's own selection: the per-wave candidate
lists and their overflow path (tile_finish -> wave_select -> wave_compact in
csrc/knn_scan.hip), the block fold (scan_end -> block_keep_k), the merge tree
behind it, and above k = 1024 the radix sort (csrc/knn_large.hip).

A wave's list overflows only when enough rows beat its threshold, which
random data never does after the first few hundred rows.  Each case therefore
asserts its own precondition before it searches: with the device's CU count
and the plan rules restated in topk_ref, the scanned rows are at least
8 * cap * CUs * (workgroups per CU), so every wave scans at least 2 * cap rows
whatever occupancy the runtime reports, and the "descending" sequences make
every one of them enter.  Corpora are zeros plus the key columns, built on
the device; the host keeps only the keys.

Queries: a case searches with the key query negated (distance = +K: a
descending key sequence is a descending distance sequence, maximal churn),
the key query itself (distance = -K: the mirrored sequence) and, where three
queries run, twice the negated one (distance = 2K).
"""

from __future__ import annotations

import gc

import numpy as np
import pytest
import torch

from fenix_amd import _lib
from fenix_amd.engine import Engine, Shard, device_mask
from tests import parity
from tests import topk_ref as R

pytestmark = pytest.mark.gpu

EXACT = {"batched": 0, "single_query_image": 0}
TORCH = {"f32": torch.float32, "f16": torch.float16, "qu8": torch.uint8}
IP = _lib.METRICS["inner_product"]
EXTRA = 37  # rows beyond the precondition: the last block step is partial


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine.get(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def cus(eng):
    return int(torch.cuda.get_device_properties(eng.device).multi_processor_count)


@pytest.fixture(autouse=True)
def _release():
    """The large corpora (6.4 GB at d = 3072) go back to the device after each case."""
    yield
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ helpers


def _rows_for(dtype, d, k, cus, aligned=True, live=1):
    """(n, shape): the smallest n whose every ``live``-th row alone meets the
    overflow precondition, plus EXTRA rows so that n is no multiple of the
    block step 16 U."""
    shape = R.scan_shape(dtype, d, aligned)
    n = live * R.overflow_rows(k, shape, cus) + EXTRA
    assert n % (16 * shape["U"]) != 0
    return n, shape


def _assert_overflows(scanned, k, shape, cus):
    """At most cus * occ_cap workgroups of 4 waves: every wave scans at least
    2 cap rows, so a sequence whose rows all enter overflows its list."""
    cap = R.scan_cap(k, shape["U"])
    assert cap >= 2 * k and cap - 4 * shape["U"] >= k
    assert scanned >= 8 * cap * cus * shape["occ_cap"], (scanned, cap, cus, shape)
    assert scanned // (4 * cus * shape["occ_cap"]) >= 2 * cap


def _zeros(eng, dtype, n, d, unaligned=False):
    if not unaligned:
        return torch.zeros((n, d), dtype=TORCH[dtype], device=eng.device)
    flat = torch.zeros(n * d + 4, dtype=TORCH[dtype], device=eng.device)
    x = flat[1: 1 + n * d].view(n, d)  # rows 4 bytes off the 16-byte grid: scalar loads
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    return x


def _set_columns(x, cols, values):
    for j, c in enumerate(cols):
        x[:, c] = torch.from_numpy(np.ascontiguousarray(values[:, j])).to(x.device)


def _key_corpus(eng, dtype, n, d, keys, nan=None, unaligned=False):
    """Zeros (quint8: the zero-point code 0) plus the digit columns of ``keys``."""
    x = _zeros(eng, dtype, n, d, unaligned)
    cols = R.key_columns(dtype, d)
    _set_columns(x, cols, R.key_digits(dtype, keys))
    if nan is not None:
        x[torch.from_numpy(nan).to(x.device), cols[0]] = float("nan")
    return x


def _key_queries(eng, dtype, d, signs):
    """distance = sign * K: the query is -sign times the key query."""
    q = np.stack([-float(s) * R.key_query(dtype, d) for s in signs]).astype(np.float32)
    return torch.from_numpy(q).to(eng.device)


def _search(eng, shard, q, metric, k, opts=None, mask=None, count=None):
    with _lib.options(**EXACT, **(opts or {})):
        gd, gr = eng.search([shard], q, metric, k, [mask], [count])
        torch.cuda.synchronize()
    return gd.cpu().numpy(), gr.cpu().numpy()


def _check_keys(got, keys, signs, k, nan=None, mask=None, row_base=0, what=""):
    gd, gr = got
    assert gd.shape == (len(signs), k) and gr.shape == (len(signs), k)
    for i, s in enumerate(signs):
        dist = (np.float32(s) * keys.astype(np.float32)).astype(np.float32)
        assert np.array_equal(dist.astype(np.int64), s * keys), "keys not exact in f32"
        if nan is not None:
            dist[nan] = np.nan
        R.check_search(gd[i], gr[i], dist, mask, row_base, k, f"{what} sign {s}")


def _sequence(name, n, k, shape, cus, kmax=1 << 24):
    """(keys, nan rows or None) of a named sequence."""
    cap = R.scan_cap(k, shape["U"])
    if name == "descending":
        return R.descending(n, k, kmax), None
    if name == "ascending":
        return R.ascending(n, k, kmax), None
    if name == "sawtooth-64":
        return R.sawtooth(n, 64, kmax), None
    if name == "sawtooth-4cap":
        return R.sawtooth(n, 4 * cap, kmax), None
    if name == "sawtooth-prime":
        rpb = R.scan_rows_per_block(n, k, shape["U"], cus * shape["occ_cap"])
        return R.sawtooth(n, R.near_prime(rpb), kmax), None
    if name == "winners-in-tail":
        return R.winners_in_tail(n, k, kmax), None
    if name == "winners-in-one-wave":
        return R.winners_in_one_wave(n, k, kmax), None
    if name == "one-per-block":
        return R.one_per_block(n, k, kmax), None
    if name == "tie-group":
        return R.tie_group(n, min(k, n // 3), kmax), None
    if name == "mostly-nan":
        return R.mostly_nan(n, min(k, n), kmax)
    raise KeyError(name)


ALL_SEQUENCES = ["descending", "ascending", "sawtooth-64", "sawtooth-4cap", "sawtooth-prime",
                 "winners-in-tail", "winners-in-one-wave", "one-per-block", "tie-group",
                 "mostly-nan"]


def _key_case(eng, cus, dtype, d, k, seq, signs, opts=None, unaligned=False, option_sets=None):
    """One corpus, one search per option set (all byte-equal), exact compare."""
    n, shape = _rows_for(dtype, d, k, cus, aligned=not unaligned)
    _assert_overflows(n, k, shape, cus)
    keys, nan = _sequence(seq, n, k, shape, cus, R.ENCODING[dtype][2])
    shard = Shard(_key_corpus(eng, dtype, n, d, keys, nan, unaligned), 0)
    q = _key_queries(eng, dtype, d, signs)
    first = None
    for o in option_sets or [opts or {}]:
        got = _search(eng, shard, q, IP, k, o)
        _check_keys(got, keys, signs, k, nan, what=f"{dtype} d={d} k={k} {seq} {o}")
        if first is None:
            first = got
        else:
            assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes()
    return shape


# ------------------------------------------------- register tiles, L = 1, U = 8

D8_CASES = [(10, s) for s in ALL_SEQUENCES] + [(k, s) for k in (1, 1000, 1024)
                                               for s in ("descending", "tie-group")]


@pytest.mark.parametrize("k,seq", D8_CASES, ids=[f"k{k}-{s}" for k, s in D8_CASES])
def test_f32_d8(eng, cus, k, seq):
    """f32 d = 8: register tiles, one slot per lane, 8 rows per lane group
    (32 appends per wave and tile); at k = 1000 and 1024 the lists hold 2048
    slots and the corpus 8.4M rows."""
    shape = _key_case(eng, cus, "f32", 8, k, seq, (1, -1, 2) if k <= 10 else (1, -1))
    assert (shape["W"], shape["L"], shape["U"]) == (4, 1, 8)


@pytest.mark.parametrize("seq", ["descending", "winners-in-tail"])
@pytest.mark.parametrize("interleave", [0, 1])
def test_f32_d8_partitions(eng, cus, interleave, seq):
    """Both row partitions: a contiguous range per workgroup, and block steps
    dealt round-robin (where the winners of the tail meet one workgroup)."""
    _key_case(eng, cus, "f32", 8, 10, seq, (1, -1), {"scan_interleave": interleave})


# ---------------------------------------------------- L = 12: tiles and stream


@pytest.mark.parametrize("seq", ["descending", "sawtooth-64", "winners-in-tail"])
def test_f32_d768_tiles_and_stream(eng, cus, seq):
    """768-d f32 rows fill their 16 x 12 slots exactly: the register tiles
    ("scan_stream" 0) and the stream ring (1), which must also be byte-equal."""
    shape = _key_case(eng, cus, "f32", 768, 10, seq, (1, -1),
                      option_sets=[{"scan_stream": 0}, {"scan_stream": 1}])
    assert (shape["L"], shape["U"], shape["occ_cap"]) == (12, 2, 1)


@pytest.mark.parametrize("seq", ["descending", "one-per-block"])
def test_f16_d1536(eng, cus, seq):
    """16-bit rows of 12 slots per lane: the tiles without the software pipeline."""
    shape = _key_case(eng, cus, "f16", 1536, 10, seq, (1, -1), {"scan_stream": 0})
    assert (shape["W"], shape["L"], shape["U"]) == (8, 12, 2)


@pytest.mark.parametrize("seq", ["descending", "winners-in-tail"])
@pytest.mark.parametrize("form", ["d5", "d8-offset"])
def test_f32_scalar_loads(eng, cus, form, seq):
    """W = 1: d = 5 (no 16-byte slots), and d = 8 rows 4 bytes off the grid."""
    d, unaligned = (5, False) if form == "d5" else (8, True)
    shape = _key_case(eng, cus, "f32", d, 10, seq, (1, -1), unaligned=unaligned)
    assert (shape["W"], shape["L"], shape["U"]) == (1, 16, 1)


def test_f32_d3072_two_passes(eng, cus):
    """Rows longer than 16 x 24 slots: two passes per row (nch = 2)."""
    shape = _key_case(eng, cus, "f32", 3072, 10, "descending", (1, -1))
    assert (shape["L"], shape["nch"]) == (24, 2)


# ------------------------------------------------------------------- quint8


@pytest.mark.parametrize("seq", ["descending", "tie-group", "winners-in-one-wave"])
@pytest.mark.parametrize("k", [10, 100])
def test_qu8_d64_dma_ring_and_tiles(eng, cus, k, seq):
    """quint8 codes (scale 1, zero point 0), three base-256 digits: the DMA
    ring ("q8_dma" 1) and the register tiles (0), byte-equal."""
    shape = _key_case(eng, cus, "qu8", 64, k, seq, (1, -1),
                      option_sets=[{"q8_dma": 1}, {"q8_dma": 0}])
    assert (shape["W"], shape["L"], shape["U"], shape["occ_cap"]) == (16, 1, 8, 3)


# -------------------------------------------------------- masks and row lists


def test_shared_mask_every_second_row(eng, cus):
    """Descending keys behind a mask that keeps every 2nd row: the kept rows
    alone meet the precondition."""
    k = 10
    n, shape = _rows_for("f32", 8, k, cus, live=2)
    mask = np.arange(n) % 2 == 0
    _assert_overflows(int(mask.sum()), k, shape, cus)
    keys = R.descending(n)
    shard = Shard(_key_corpus(eng, "f32", n, 8, keys), 0)
    got = _search(eng, shard, _key_queries(eng, "f32", 8, (1, -1)), IP, k,
                  mask=device_mask(mask, eng.device))
    _check_keys(got, keys, (1, -1), k, mask=mask, what="every 2nd row")


@pytest.mark.parametrize("live", [-1, 0, 1], ids=["k-1", "k", "k+1"])
def test_shared_mask_about_k_rows(eng, cus, live):
    """A mask keeping exactly k-1, k and k+1 of the descending rows, one of
    them in the last partial tile: fewer than k live rows end in (-1, NaN)."""
    k = 10
    n, shape = _rows_for("f32", 8, k, cus)
    _assert_overflows(n, k, shape, cus)
    mask = np.zeros(n, dtype=bool)
    at = np.random.RandomState(3).permutation(n - 1)[: k + live - 1]
    mask[at] = True
    mask[n - 1] = True
    assert int(mask.sum()) == k + live
    keys = R.descending(n)
    shard = Shard(_key_corpus(eng, "f32", n, 8, keys), 0)
    got = _search(eng, shard, _key_queries(eng, "f32", 8, (1, -1)), IP, k,
                  mask=device_mask(mask, eng.device))
    _check_keys(got, keys, (1, -1), k, mask=mask, what=f"{k + live} live rows")
    assert (got[1][:, k + live:] == -1).all()


@pytest.mark.parametrize("seq", ["descending", "sawtooth-64"])
def test_row_list(eng, cus, seq):
    """The same corpus through ``masks`` / ``counts`` with a third of the rows
    kept: below Engine.SPARSE the mask is compacted and the scan reads the
    row list, whose rows alone meet the precondition."""
    k = 10
    n, shape = _rows_for("f32", 8, k, cus, live=3)
    mask = np.arange(n) % 3 == 1
    count = int(mask.sum())
    assert count < Engine.SPARSE * n
    _assert_overflows(count, k, shape, cus)
    keys, _ = _sequence(seq, n, k, shape, cus)
    shard = Shard(_key_corpus(eng, "f32", n, 8, keys), 0)
    got = _search(eng, shard, _key_queries(eng, "f32", 8, (1, -1)), IP, k,
                  mask=device_mask(mask, eng.device), count=count)
    _check_keys(got, keys, (1, -1), k, mask=mask, what=f"row list {seq}")


# --------------------------------------------------------- k > 1024: the sort

LARGE_N = 20_000


@pytest.mark.parametrize("seq", ["descending", "tie-group", "mostly-nan"])
@pytest.mark.parametrize("k", [1025, 4096, LARGE_N + 5])
def test_large_k_sort(eng, cus, k, seq):
    """Above the fused scan's k: every distance, then the radix sort of the
    composites; k above n ends in (-1, NaN)."""
    n = LARGE_N
    assert k > _lib.max_k()
    keys, nan = _sequence(seq, n, k, R.scan_shape("f32", 8), cus)
    shard = Shard(_key_corpus(eng, "f32", n, 8, keys, nan), 0)
    got = _search(eng, shard, _key_queries(eng, "f32", 8, (1, -1)), IP, k)
    _check_keys(got, keys, (1, -1), k, nan, what=f"sort k={k} {seq}")
    if k > n:
        assert (got[1][:, n:] == -1).all()


def test_large_k_sort_masked(eng, cus):
    n, k = LARGE_N, 4096
    keys, nan = R.mostly_nan(n, k)
    mask = np.random.RandomState(8).rand(n) < 0.7
    shard = Shard(_key_corpus(eng, "f32", n, 8, keys, nan), 0)
    got = _search(eng, shard, _key_queries(eng, "f32", 8, (1, -1)), IP, k,
                  mask=device_mask(mask, eng.device))
    _check_keys(got, keys, (1, -1), k, nan, mask=mask, what="sort masked")


# ------------------------------------------------------------- L2 and cosine
#
# The overflow path is instantiated per metric (tile_finish<METRIC>).  L2:
# query 0 and one column of signed integer levels x, |x| <= 4095 (quint8:
# codes, <= 255): the distance is the root of the exact square, so rows AND
# distance bits are exact.  Cosine: query (1, 0), rows (cos t, sin t) over 64
# levels; the float64 reference comes from the rounded rows, its distinct
# levels are asserted to lie 100 near-tie widths apart, then rows are exact
# and distances within parity.DIST_RTOL * max(|ref|, 1).

METRIC_CASES = [("f32", 8, {}), ("f32", 768, {"scan_stream": 1}), ("qu8", 64, {})]
COS_LEVELS = 64


@pytest.mark.parametrize("seq", ["sawtooth-64", "one-per-block"])
@pytest.mark.parametrize("dtype,d,opts", METRIC_CASES, ids=["f32-d8", "f32-d768-stream", "qu8-d64"])
def test_l2_levels(eng, cus, dtype, d, opts, seq):
    k = 10
    n, shape = _rows_for(dtype, d, k, cus)
    _assert_overflows(n, k, shape, cus)
    levels, _ = _sequence(seq, n, k, shape, cus, kmax=256 if dtype == "qu8" else 4096)
    assert levels.max() <= (255 if dtype == "qu8" else 4095)
    x = levels.copy()
    if dtype != "qu8":
        x[1::2] *= -1  # signed levels: the square is what counts
    corpus = _zeros(eng, dtype, n, d)
    _set_columns(corpus, [d // 2], x.astype(R.NP_DTYPE[dtype])[:, None])
    q = torch.zeros((1, d), dtype=torch.float32, device=eng.device)
    gd, gr = _search(eng, Shard(corpus, 0), q, _lib.METRICS["l2"], k, opts)
    dist = np.sqrt((x * x).astype(np.float32))
    assert np.array_equal(dist.astype(np.int64), np.abs(x))
    R.check_search(gd[0], gr[0], dist, None, 0, k, f"l2 {dtype} d={d} {seq}")


@pytest.mark.parametrize("seq", ["sawtooth-64", "one-per-block"])
@pytest.mark.parametrize("dtype,d,opts", METRIC_CASES[:2], ids=["f32-d8", "f32-d768-stream"])
def test_cosine_levels(eng, cus, dtype, d, opts, seq):
    k = 10
    n, shape = _rows_for(dtype, d, k, cus)
    _assert_overflows(n, k, shape, cus)
    levels, _ = _sequence(seq, n, k, shape, cus, kmax=COS_LEVELS)
    rows2 = R.cosine_rows(levels, COS_LEVELS)
    ref = R.cosine_ref(rows2)
    distinct = np.unique(ref)
    assert len(distinct) <= 4096
    assert np.diff(distinct).min() >= 100 * parity.NEAR_RTOL, "a near tie in the reference"
    corpus = _zeros(eng, dtype, n, d)
    _set_columns(corpus, [0, d - 1], rows2)
    q = torch.zeros((1, d), dtype=torch.float32, device=eng.device)
    q[0, 0] = 1.0
    gd, gr = _search(eng, Shard(corpus, 0), q, _lib.METRICS["cosine"], k, opts)
    order = np.lexsort((np.arange(n), ref))[:k]  # (float64 distance, row)
    np.testing.assert_array_equal(gr[0], order)
    err = np.abs(gd[0].astype(np.float64) - ref[order])
    assert (err <= parity.DIST_RTOL * np.maximum(np.abs(ref[order]), 1.0)).all(), err.max()


# ------------------------------------------------- the top of the row space


def test_row_base_at_top_of_row_space(eng, cus):
    """row_base = 2^32 - 2 - n: the last row is 2^32 - 3, the largest rows a
    composite can carry beside the empty one."""
    k = 10
    n, shape = _rows_for("f32", 8, k, cus)
    _assert_overflows(n, k, shape, cus)
    base = (1 << 32) - 2 - n
    keys = R.descending(n)
    shard = Shard(_key_corpus(eng, "f32", n, 8, keys), base)
    signs = (1, -1, 2)
    got = _search(eng, shard, _key_queries(eng, "f32", 8, signs), IP, k)
    _check_keys(got, keys, signs, k, row_base=base, what="row_base top")
    assert got[1][0, 0] == (1 << 32) - 3
