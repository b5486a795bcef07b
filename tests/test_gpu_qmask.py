"""Per-query row masks in the int8 filter (fx_qmask_pack, fx_knn_search_qmask_ex,
csrc/filter/img6.inc filter_img6_kernel<., true>): a batch whose every query
brings its own row bitmap runs in one pass over the filter image.

* pack: the bit matrix against a numpy transpose;
* bits: rows and distance bits equal per-query masked exact scans (option
  "batched" 0) and the float64 oracle, on every slice build a batch size
  reaches, every metric and row type, and through the exact plans;
* equivalence: for queries that share a mask, the filter state (counts,
  thresholds, candidate sets, held bounds) equals the shared-mask batch's:
  the filter ran, and appended exactly what the existing path appends;
* bounds: B1-B5 and D1-D3 of tests/test_gpu_filter_bounds.py (its checkers)
  with each query's own mask as the admissible set;
* forced rows, repetition, no host synchronisation, and concurrent Flight
  clients with filters and probe sets sharing batches.

Shapes follow test_gpu_filter_bounds.py: 40 003 rows (a ragged tile, a
non-trivial permutation) of d = 128, k = 10, "batch_cap" 4096: three phases.
"""

from __future__ import annotations

import functools
import socket
import threading
import types

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest
import torch

import fenix_amd
from fenix_amd import _lib, coalesce
from fenix_amd.engine import Engine, Shard, bitmap, device_mask
from oracle import oracle as O
from tests import parity
from tests.test_gpu_filter_bounds import _check_default, _check_held

pytestmark = pytest.mark.gpu

METRICS = ["l2", "inner_product", "cosine"]
N, D, K, CAP = 40_003, 128, 10, 4096
BASE = {"filter_image": 8, "batch_cap": CAP, "qu8_batch_min_work": 0}


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine.get(torch.device("cuda", 0))


# ------------------------------------------------------------------ inputs --
@functools.lru_cache(maxsize=8)
def _host_rows(n, d, dtype):
    """(rows as stored, rows as float32, scale, zero point), one generation per shape."""
    x = O.fill_normal(n, d, seed=91)
    if dtype == "f16":
        xs = x.astype(np.float16)
        return xs, xs.astype(np.float32), 1.0, 0
    if dtype == "qu8":
        codes = np.clip(np.rint(64 + 40.0 * x), 0, 255).astype(np.uint8)
        return codes, O.dequantize(codes, 1e-3, 64), 1e-3, 64
    return x, x, 1.0, 0


def _shard(eng, n, d, dtype, row_base=0):
    xs, xv, scale, zp = _host_rows(n, d, dtype)
    return Shard(torch.from_numpy(xs).to(eng.device), row_base, float(scale), int(zp)), xv


def _queries(nq, d, dtype, seed=95):
    q = O.fill_normal(nq, d, seed=seed)
    if dtype == "qu8":
        q = (np.float32(1e-3 * 40.0) * q).astype(np.float32)
    return q


def _mask_set(n, nq, seed=96):
    """bool [nq, n]: by query i % 7 a random keep of 0.9 / 0.3, all rows, no
    row, 5 rows (fewer than k), query 0's mask again, the rows r % nq == i."""
    rs = np.random.RandomState(seed)
    m = np.zeros((nq, n), dtype=bool)
    for i in range(nq):
        kind = i % 7
        if kind == 0:
            m[i] = rs.rand(n) < 0.9
        elif kind == 1:
            m[i] = rs.rand(n) < 0.3
        elif kind == 2:
            m[i] = True
        elif kind == 4:
            m[i, rs.choice(n, 5, replace=False)] = True
        elif kind == 5:
            m[i] = m[0]
        elif kind == 6:
            m[i] = np.arange(n) % nq == i
    return m


def _bitmaps(masks, pad=0):
    """bool [nq, n] -> uint32 [nq, ceil(n / 32) + pad] (garbage in the padding)."""
    words = np.stack([bitmap(r) for r in masks])
    if pad:
        words = np.concatenate([words, np.full((len(masks), pad), 0xDEADBEEF, np.uint32)], axis=1)
    return np.ascontiguousarray(words)


def _qm(eng, masks, pad=0):
    return torch.from_numpy(_bitmaps(masks, pad).view(np.int32)).to(eng.device)


def _per_query(eng, shard, q, m, k, masks):
    """nq masked single-query exact searches."""
    ds, rs = [], []
    with _lib.options(batched=0):
        for i in range(q.shape[0]):
            d, r = eng.search([shard], q[i:i + 1], m, k, [device_mask(masks[i], eng.device)])
            ds.append(d)
            rs.append(r)
        torch.cuda.synchronize()
    return torch.cat(ds).cpu().numpy(), torch.cat(rs).cpu().numpy()


def _assert_bits(got, want, what):
    (gd, gr), (wd, wr) = got, want
    np.testing.assert_array_equal(gr, wr, err_msg=f"{what}: rows")
    np.testing.assert_array_equal(gd.view(np.uint32), wd.view(np.uint32),
                                  err_msg=f"{what}: distance bits")


def _host(*ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


# -------------------------------------------------------------------- pack --
@pytest.mark.parametrize("n", [1, 31, 32, 40_003])
@pytest.mark.parametrize("nq", [1, 31, 32, 33, 128, 130])
def test_pack_is_the_bit_transpose(eng, nq, n):
    rs = np.random.RandomState(nq * 7 + n)
    masks = rs.rand(nq, n) < 0.5
    pad = 3
    words = _bitmaps(masks, pad)
    # bits of rows >= n inside the last word are ignored
    if n % 32:
        words[:, (n - 1) // 32] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    qw = _lib.qmask_words(nq)
    src = torch.from_numpy(words.view(np.int32)).to(eng.device)
    out = torch.full((n + 2, qw), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    _lib.check(_lib.load().fx_qmask_pack(src.data_ptr(), words.shape[1], nq, n, out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream))
    got = _host(out)[0].view(np.uint32)
    assert (got[n:] == 0x5A5A5A5A).all(), "rows past n were written"
    want = np.zeros((n, qw * 32), dtype=bool)
    want[:, :nq] = masks.T
    want = np.packbits(want, axis=1, bitorder="little").view("<u4").reshape(n, qw)
    np.testing.assert_array_equal(got[:n], want)  # (padding bits zero included)


def test_pack_rejects_a_short_stride(eng):
    src = torch.zeros((2, 4), dtype=torch.int32, device=eng.device)
    out = torch.zeros((1000, 4), dtype=torch.int32, device=eng.device)
    rc = _lib.load().fx_qmask_pack(src.data_ptr(), 4, 2, 1000, out.data_ptr(), None)
    assert rc == -1


# -------------------------------------------------------------------- bits --
@functools.lru_cache(maxsize=1)
def _slice_limits():
    """(largest d a 128-query slice fits, the next: slices of 64)."""
    d128 = max(d for d in range(64, 4096, 64)
               if _lib.qmask_filter_used(N, d, _lib.DTYPE_F32, 65, K, _lib.METRIC_L2) == 128)
    assert _lib.qmask_filter_used(N, d128 + 64, _lib.DTYPE_F32, 65, K, _lib.METRIC_L2) == 64
    return d128, d128 + 64


# (id, nq, row type, metrics, options, shape overrides, expected slice width or
# 0 = exact plan)
BITS = [
    ("q2", 2, "f32", ["l2"], {}, {}, 64),
    ("q33", 33, "f32", METRICS, {}, {}, 64),           # the second query tile live
    ("q64", 64, "f32", ["l2"], {}, {}, 64),
    ("q65", 65, "f32", METRICS, {}, {}, 128),
    ("q128", 128, "f32", ["l2"], {}, {}, 128),
    ("q130", 130, "f32", ["l2"], {}, {}, 128),         # two slices
    ("q40-f16", 40, "f16", ["cosine"], {}, {}, 64),
    ("q40-qu8", 40, "qu8", ["l2"], {}, {}, 64),
    ("q65-d768", 65, "f32", ["l2"], {}, {"d": 768}, 128),
    ("q65-dmax128", 65, "f32", ["inner_product"], {}, {"d": "d128"}, 128),
    ("q65-dmin64", 65, "f32", ["l2"], {}, {"d": "d64"}, 64),   # q64i slices
    ("q33-rowbase", 33, "f32", ["l2"], {}, {"row_base": 1_000_000}, 64),
    ("q65-shared", 65, "f32", ["cosine"], {}, {"shared": True}, 128),
    ("q33-fallback", 33, "f32", ["l2"], {"force_fallback": 1}, {}, 64),
    ("q33-noimage", 33, "f32", ["l2"], {"filter_image": 0}, {}, 0),
]
BIT_CASES = [pytest.param(b, metric, id=f"{b[0]}-{metric}") for b in BITS for metric in b[3]]


@pytest.mark.parametrize("case,metric", BIT_CASES)
def test_qmask_batch_equals_per_query_masked_scans(eng, case, metric):
    cid, nq, dtype, _, opts, shape, kind = case
    d = shape.get("d", D)
    if isinstance(d, str):
        d = _slice_limits()[0 if d == "d128" else 1]
    m = _lib.METRICS[metric]
    shard, xv = _shard(eng, N, d, dtype, shape.get("row_base", 0))
    qh = _queries(nq, d, dtype)
    q = torch.from_numpy(qh).to(eng.device)
    masks = _mask_set(N, nq)
    shared, dm = None, None
    if shape.get("shared"):
        shared = np.random.RandomState(97).rand(N) < 0.7
        dm = device_mask(shared, eng.device)
    eff = masks if shared is None else masks & shared[None, :]
    eng.clear_images()
    want = _per_query(eng, shard, q, m, K, eff)
    qm = _qm(eng, masks, pad=2)
    with _lib.options(**{**BASE, **opts}):
        assert _lib.qmask_filter_used(N, d, shard.dtype_id, nq, K, m) == kind
        before = eng.qmask_searches
        gd, gr = eng.search([shard], q, m, K, [dm] if dm is not None else None, qmasks=[qm])
        assert eng.qmask_searches == before + 1
        st = eng.scan(shard, q, m, K, dm, qmasks=qm)
        count, cap = eng.filter_counts(shard, nq, m, K, st)
        od = torch.empty((nq, K), dtype=torch.float32, device=eng.device)
        orow = torch.empty((nq, K), dtype=torch.int64, device=eng.device)
        eng.reduce(shard, q, m, K, st, od, orow)
        got, got2 = _host(gd, gr), _host(od, orow)
    if kind:
        assert count is not None and cap == CAP and st.image is not None and st.packed is not None
        kept = eff.sum(axis=1)
        print(f"{cid}-{metric}: count/cap max {count.max() / cap:.3f}, "
              f"over cap {(count.astype(np.int64) > cap).sum()} of {nq}")
        assert (count[kept == 0] == 0).all(), "a query with an empty mask got candidates"
        ok = count.astype(np.int64) <= cap
        assert (count[ok] <= kept[ok]).all(), "more candidates than admitted rows"
    else:
        assert count is None and st.image is None
    _assert_bits(got, want, "search")
    _assert_bits(got2, want, "scan + reduce")
    # fewer than k admitted rows: NaN / -1 padding
    short = eff.sum(axis=1) < K
    for i in np.nonzero(short)[0]:
        keep = int(eff[i].sum())
        assert (got[1][i, keep:] == -1).all() and np.isnan(got[0][i, keep:]).all()
        assert (got[1][i, :keep] >= 0).all()
    # the float64 oracle, each query under its own mask
    for i in range(nq):
        odist, orows = O.knn(xv, qh[i:i + 1], metric, K, mask=eff[i], row_base=shard.row_base)
        parity.check_topk(got[0][i:i + 1], got[1][i:i + 1], odist, orows, xv, qh[i:i + 1], metric)
    eng.clear_images()


# ------------------------------------------- equivalence with a shared mask --
def _state(eng, shard, q, m, mask=None, qmasks=None):
    """(count, thr, cand) of the default path and (count, cand lb, cand ub) held."""
    nq = q.shape[0]
    st = eng.scan(shard, q, m, K, mask, qmasks=qmasks)
    count, cap = eng.filter_counts(shard, nq, m, K, st)
    assert count is not None and cap == CAP
    thr, cand, _ = eng.filter_state(shard, nq, m, K, st, cap)
    held = eng.filter_bounds(shard, q, m, K, mask, qmasks=qmasks)
    assert held is not None and held["bits"] == 8
    return count.astype(np.int64), thr, cand, held


@pytest.mark.parametrize("nq", [33, 100])
def test_filter_state_equals_the_shared_mask_batch(eng, nq):
    m = _lib.METRIC_L2
    shard, _ = _shard(eng, N, D, "f32")
    q = torch.from_numpy(_queries(nq, D, "f32", seed=98)).to(eng.device)
    rs = np.random.RandomState(99)
    three = np.stack([rs.rand(N) < keep for keep in (0.9, 0.5, 0.2)])
    masks = three[np.arange(nq) % 3]
    eng.clear_images()
    with _lib.options(**BASE):
        assert _lib.qmask_filter_used(N, D, _lib.DTYPE_F32, nq, K, m) == (64 if nq <= 64 else 128)
        count, thr, cand, held = _state(eng, shard, q, m, qmasks=_qm(eng, masks))
        for j in range(3):
            c1, t1, k1, h1 = _state(eng, shard, q, m, mask=device_mask(three[j], eng.device))
            for qi in range(j, nq, 3):
                assert count[qi] == c1[qi], f"q{qi}: count {count[qi]} != shared-mask {c1[qi]}"
                assert thr[qi] == t1[qi], f"q{qi}: threshold"
                cq = min(int(count[qi]), CAP)
                np.testing.assert_array_equal(np.sort(cand[qi, :cq]), np.sort(k1[qi, :cq]),
                                              err_msg=f"q{qi}: candidate composites")
                hq = int(held["count"][qi])
                assert hq == int(h1["count"][qi]) and held["thr"][qi] == h1["thr"][qi]
                hq = min(hq, CAP)
                for key in ("cand", "cand_ub"):
                    np.testing.assert_array_equal(np.sort(held[key][qi, :hq]),
                                                  np.sort(h1[key][qi, :hq]),
                                                  err_msg=f"q{qi}: held {key}")
                # (lb, ub) pairs, not only the two sets
                a = np.lexsort((held["cand_ub"][qi, :hq], held["cand"][qi, :hq]))
                b = np.lexsort((h1["cand_ub"][qi, :hq], h1["cand"][qi, :hq]))
                np.testing.assert_array_equal(held["cand_ub"][qi, :hq][a], h1["cand_ub"][qi, :hq][b])
    assert (count > 0).all() and (count <= CAP).any()
    eng.clear_images()


# ------------------------------------------------------------------ bounds --
class _QueryView:
    """One query of a qmask batch, as test_gpu_filter_bounds' checkers see an
    engine: the batch ran once (held and default), and each view hands out its
    query's slice of that state.  D3's reference search is the real engine's,
    under the query's own mask."""

    def __init__(self, eng, full, qi):
        self.eng, self.full, self.qi, self.device = eng, full, qi, eng.device

    def _s(self, a):
        return a[self.qi:self.qi + 1]

    def filter_bounds(self, shard, q, m, k, dm):
        h = self.full.held
        return {"count": self._s(h["count"]), "cap": h["cap"], "thr": self._s(h["thr"]),
                "cand": self._s(h["cand"]), "cand_ub": self._s(h["cand_ub"]), "bits": h["bits"]}

    def scan(self, shard, q, m, k, dm):
        return self.full.st

    def filter_counts(self, shard, nq, m, k, st):
        return self._s(self.full.count), self.full.cap

    def filter_state(self, shard, nq, m, k, st, cap):
        return tuple(self._s(a) for a in self.full.state)

    def reduce(self, shard, q, m, k, st, od, orow, dm):
        od.copy_(self._s(self.full.od))
        orow.copy_(self._s(self.full.orow))

    def search(self, shards, q, m, k, msk):
        return self.eng.search(shards, q, m, k, msk)


@pytest.mark.parametrize("nq,metric", [(40, "l2"), (100, "cosine"), (40, "inner_product")])
def test_filter_bounds_with_per_query_masks(eng, nq, metric):
    m = _lib.METRICS[metric]
    shard, xv = _shard(eng, N, D, "f32", 1_000_000 if nq == 100 else 0)
    qh = _queries(nq, D, "f32", seed=101)
    q = torch.from_numpy(qh).to(eng.device)
    rs = np.random.RandomState(102)
    masks = np.stack([rs.rand(N) < (0.9, 0.3, 0.6)[i % 3] for i in range(nq)])
    qm = _qm(eng, masks)
    eng.clear_images()
    full = types.SimpleNamespace()
    with _lib.options(**BASE):
        full.held = eng.filter_bounds(shard, q, m, K, qmasks=qm)
        assert full.held is not None
        full.st = eng.scan(shard, q, m, K, qmasks=qm)
        full.count, full.cap = eng.filter_counts(shard, nq, m, K, full.st)
        full.state = eng.filter_state(shard, nq, m, K, full.st, full.cap)
        full.od = torch.empty((nq, K), dtype=torch.float32, device=eng.device)
        full.orow = torch.empty((nq, K), dtype=torch.int64, device=eng.device)
        eng.reduce(shard, q, m, K, full.st, full.od, full.orow)
        ds = eng.distances(shard, q, m)
        torch.cuda.synchronize()
    d_scan = ds.cpu().numpy()
    keys = parity.order_key(d_scan)
    grow = np.arange(N, dtype=np.uint64) + np.uint64(shard.row_base)
    comp = (keys.astype(np.uint64) << np.uint64(32)) | grow[None, :]
    top = int(np.argmax(np.einsum("ij,ij->i", xv, xv, dtype=np.float64)))
    scale = parity.scale_of(xv[top:top + 1], qh, metric)
    failures = []
    for qi in range(nq):
        c = types.SimpleNamespace(
            id=f"qmask-q{qi}", fam="i8", nq=1, metric=metric, m=m, n=N, cap=CAP, d=D,
            row_base=shard.row_base, opts=dict(BASE), xv=xv, qh=qh[qi:qi + 1], q=q[qi:qi + 1],
            mask=masks[qi], dm=device_mask(masks[qi], eng.device), altered=[], shard=shard,
            live=masks[qi], d_scan=d_scan[qi:qi + 1], keys=keys[qi:qi + 1], comp=comp[qi:qi + 1],
            bad_rows=np.zeros(N, dtype=bool), scale=scale[qi:qi + 1], kind="normal")
        view = _QueryView(eng, full, qi)
        for name, run in (("held", lambda: _check_held(view, c, {})),
                          ("default", lambda: _check_default(view, c))):
            try:
                run()
            except AssertionError as e:
                failures.append(f"[q{qi} {name}] {e}")
    eng.clear_images()
    assert not failures, "\n".join(failures[:10])


# ------------------------------------------------------------- forced rows --
def test_a_forced_row_obeys_each_query_mask(eng):
    """Rows with a non-finite component are forced through the pass test; a
    query whose mask excludes such a row never sees it as a candidate, and a
    non-finite query (every row forced) still gets only its own rows."""
    nq, m = 40, _lib.METRIC_L2
    x = _host_rows(N, D, "f32")[0].copy()
    bad = np.random.RandomState(103).choice(N, 24, replace=False)
    x[bad[:8], 3] = np.inf
    x[bad[8:16], 5] = np.nan
    x[bad[16:], 0] = -np.inf
    shard = Shard(torch.from_numpy(x).to(eng.device), 0)
    qh = _queries(nq, D, "f32", seed=104)
    qh[7, 2] = np.nan
    q = torch.from_numpy(qh).to(eng.device)
    rs = np.random.RandomState(105)
    masks = rs.rand(nq, N) < 0.6
    masks[::2, bad] = False   # even queries exclude every forced row
    masks[1::2, bad] = True   # odd ones admit them all
    qm = _qm(eng, masks)
    eng.clear_images()
    want = _per_query(eng, shard, q, m, K, masks)
    with _lib.options(**BASE):
        gd, gr = eng.search([shard], q, m, K, qmasks=[qm])
        got = _host(gd, gr)
        held = eng.filter_bounds(shard, q, m, K, qmasks=qm)
    _assert_bits(got, want, "forced rows")
    assert held is not None
    seen_forced = 0
    for qi in range(nq):
        rows = got[1][qi]
        assert masks[qi, rows[rows >= 0]].all(), f"q{qi}: a returned row is masked out"
        cq = int(held["count"][qi])
        if cq > held["cap"]:
            continue
        cr = parity.comp_row(held["cand"][qi, :cq])
        assert masks[qi, cr].all(), f"q{qi}: candidate rows {cr[~masks[qi, cr]][:5]} are masked out"
        hit = np.isin(bad, cr)
        if qi % 2:
            assert hit.all(), f"q{qi}: admitted forced rows {bad[~hit][:5]} were not appended"
            seen_forced += int(hit.sum())
        else:
            assert not hit.any()
    assert seen_forced > 0
    assert int(held["count"][7]) > held["cap"], "the non-finite query did not overflow"
    eng.clear_images()


# --------------------------------------------------- repetition, no syncs --
@pytest.mark.parametrize("nq", [33, 64, 65])
def test_repeated_qmask_scans_append_the_same_counts(eng, nq):
    m = _lib.METRIC_L2
    shard, _ = _shard(eng, N, D, "f32")
    q = torch.from_numpy(_queries(nq, D, "f32", seed=106)).to(eng.device)
    qm = _qm(eng, _mask_set(N, nq, seed=107))
    eng.clear_images()
    with _lib.options(**BASE):
        first = None
        for rep in range(8):
            st = eng.scan(shard, q, m, K, qmasks=qm)
            count, cap = eng.filter_counts(shard, nq, m, K, st)
            assert count is not None
            if first is None:
                first = count.copy()
            np.testing.assert_array_equal(count, first, err_msg=f"repetition {rep}")
    eng.clear_images()


def test_a_qmask_search_does_not_synchronise(eng):
    nq = 65
    shard, _ = _shard(eng, N, D, "f32")
    q = torch.from_numpy(_queries(nq, D, "f32", seed=108)).to(eng.device)
    qm = _qm(eng, _mask_set(N, nq, seed=109))
    eng.clear_images()
    with _lib.options(**BASE):
        eng.search([shard], q, _lib.METRIC_L2, K, qmasks=[qm])  # (builds the image)
        before = _lib.host_sync_count()
        for metric in METRICS:
            eng.search([shard], q, _lib.METRICS[metric], K, qmasks=[qm])
        assert _lib.host_sync_count() == before
        torch.cuda.synchronize()
    eng.clear_images()


# ------------------------------------------------------------------ served --
def test_concurrent_flight_clients_with_filters_share_qmask_batches(tmp_path):
    """8 Flight clients on one table: two with filters, two probe searches,
    two plain, one whose filter keeps 3 rows (maxval 2, so that it is searched
    at all), one more filter.  Each gets the
    answer of the same search run alone; they share batches, and at least one
    batch went through the per-query-mask entry point."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fenix_amd import engine

    n, d, clients, rounds = 200_000, 128, 8, 3
    x = O.fill_normal(n, d, seed=110, cluster=1000)
    vec = pa.FixedSizeListArray.from_arrays(pa.array(x.ravel()), d)
    src = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "vector": vec})
    targets = O.fill_normal(clients * rounds, d, seed=111)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    server = fenix_amd.Server(str(tmp_path), host="127.0.0.1", port=port)
    try:
        f0 = fenix_amd.Flight(host="127.0.0.1", port=port)
        f0.make_table("m/served", src.to_reader())
        f0.make_index(name="m/code", source="m/served", column="vector",
                      config={"metric": "l2", "codebook_size": 8, "num_codebooks": 2,
                              "batch_size": 2560, "num_epochs": 2})
        kinds = [
            dict(filter=pc.field("id") >= 50_000),
            dict(filter=(pc.field("id") >= 20_000) & (pc.field("id") < 150_000)),
            dict(coding="m/code", probes=12),
            dict(coding="m/code", probes=30),
            dict(),
            dict(),
            dict(filter=pc.field("id").isin([5, 77_777, 199_999]), maxval=2),  # keeps 3 rows
            dict(filter=pc.field("id") < 120_000),
        ]

        def one(f, i):
            r = f.search(target=targets[i], source="m/served", column="vector", metric="l2",
                         select=["id"], **{"maxval": 10, **kinds[i % clients]})
            return r.column("id").to_numpy(), r.column("__DISTANCE__").to_numpy()

        with _lib.options(filter_image=8, qmask_batch_min_ratio=0):
            seq = [one(f0, i) for i in range(clients * rounds)]
            assert len(seq[6][0]) == 2
            co = coalesce.default()
            b0, r0 = co.batches, co.requests
            q0 = sum(e.qmask_searches for e in Engine._instances.values())
            par = [None] * (clients * rounds)
            gate = threading.Barrier(clients)

            def client(c):
                f = fenix_amd.Flight(host="127.0.0.1", port=port)
                for r in range(rounds):
                    gate.wait()
                    par[r * clients + c] = one(f, r * clients + c)

            threads = [threading.Thread(target=client, args=(c,)) for c in range(clients)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert co.requests - r0 == clients * rounds
            assert co.batches - b0 < co.requests - r0, "no two requests shared a batch"
            q1 = sum(e.qmask_searches for e in Engine._instances.values())
            assert q1 > q0, "no batch went through the per-query-mask entry point"
        for (a, da), (b, db) in zip(seq, par):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(da.view(np.uint32), db.view(np.uint32))
    finally:
        server.shutdown()
        engine.CACHE.clear()
        Engine.get(torch.device("cuda", 0)).clear_images()
