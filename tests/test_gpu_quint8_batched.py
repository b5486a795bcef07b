"""Batches over quint8 codes through the int8 filter image
(fx_knn_search_img8_ex): the int8-MFMA filter runs over an image of the
dequantised rows (csrc/knn_filter.hip image8_qu8_kernel) and the candidates
are rescored from the codes in the quint8 scan's own arithmetic
(csrc/fx_exact.h exact_distance16_qu8).

* bits: rows and distance bits equal per-query exact scans (option "batched"
  0) on every kernel a batch size reaches, for every metric;
* bounds: B1-B5 and D1-D3 of tests/test_gpu_filter_bounds.py (its checkers,
  its JSON record) for the quint8 family, against the quint8 scan's own
  distances.  The inputs that load what is particular to codes: "near"
  (queries that are dequantised rows, or one code step away in a few
  components: the L2 scan compares codes with q' = fl(zp + q / scale), and the
  filter must bound THAT distance), "offset" (zp = 255 with codes in 200..255,
  zp = 0 with codes in 0..55: the zero point far from the data, where
  scale * zp * sqrt(d) dwarfs the distances) and "aligned" (queries along a
  row's own int8 residual);
* oracle, lifecycle (a torch write to the codes), a non-finite query, no host
  synchronisation, and concurrent Flight clients whose coalesced batches take
  the image.

Shapes follow test_gpu_filter_bounds.py: 40 000 rows (+3: a ragged tile) of
d = 128, k = 10, "batch_cap" 4096: three phases; the clustered corpus 160 000
rows / 16 384.  The work gate (option "qu8_batch_min_work") is 0 throughout.
"""

from __future__ import annotations

import functools
import socket
import threading

import numpy as np
import pyarrow as pa
import pytest
import torch

import fenix_amd
from fenix_amd import _lib, coalesce
from fenix_amd.engine import Engine, Shard, device_mask
from fenix_amd.ex.arrow import quint8 as Q
from oracle import oracle as O
from tests import parity
from tests.test_gpu_filter_bounds import _check_default, _check_held, _record

pytestmark = pytest.mark.gpu

METRICS = ["l2", "inner_product", "cosine"]
K = 10
BASE = {"filter_image": 8, "qu8_batch_min_work": 0}


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine.get(torch.device("cuda", 0))


# ------------------------------------------------------------------ inputs --
@functools.lru_cache(maxsize=4)
def _codes(kind, n, d, zp):
    """uint8 codes [n, d] of an input kind (one generation per shape).
    wide: zp + 40 N(0, 1), clipped (zp 0 / 255: half the components sit on the
    zero point); full: uniform over 0..255; clustered: the suite's clustered
    corpus (x + 10 x0 per 1 000 rows) on a grid of 128 steps around zp;
    hi / lo: uniform over 200..255 / 0..55."""
    rs = np.random.RandomState(1000 + zp)
    if kind == "full":
        return rs.randint(0, 256, (n, d)).astype(np.uint8)
    if kind == "hi":
        return rs.randint(200, 256, (n, d)).astype(np.uint8)
    if kind == "lo":
        return rs.randint(0, 56, (n, d)).astype(np.uint8)
    if kind == "clustered":
        x = O.fill_normal(n, d, seed=92, cluster=1000)
        return np.clip(np.rint(zp + x * (127.0 / np.abs(x).max())), 0, 255).astype(np.uint8)
    x = O.fill_normal(n, d, seed=91)
    return np.clip(np.rint(zp + 40.0 * x), 0, 255).astype(np.uint8)


def _shard(eng, codes, row_base, scale, zp):
    return Shard(torch.from_numpy(codes).to(eng.device), row_base, float(scale), int(zp))


def _queries(nq, d, scale, spread, seed=95):
    """Queries at the rows' own magnitude: scale * spread * N(0, 1)."""
    return (np.float32(scale * spread) * O.fill_normal(nq, d, seed=seed)).astype(np.float32)


def _exact(eng, shard, q, m, k, masks=None):
    with _lib.options(batched=0):
        d, r = eng.search([shard], q, m, k, masks)
        torch.cuda.synchronize()
    return d.cpu().numpy(), r.cpu().numpy()


def _assert_bits(got, want, what):
    (gd, gr), (wd, wr) = got, want
    np.testing.assert_array_equal(gr, wr, err_msg=f"{what}: rows")
    np.testing.assert_array_equal(gd.view(np.uint32), wd.view(np.uint32),
                                  err_msg=f"{what}: distance bits")


# -------------------------------------------------------------------- bits --
# (id, nq, codes, zero point, scale, options, shape overrides); the kernel each
# batch size reaches: launch_filter (csrc/knn_filter.hip)
BITS = [
    ("q2", 2, "wide", 64, 1e-3, {}, {}),                       # the dense rescore
    ("q40", 40, "full", 0, 7.5, {}, {"mask": True}),           # q64i img6
    ("q100", 100, "wide", 255, 1e-3, {}, {"n": 3}),            # q128 img6
    ("q200", 200, "wide", 64, 7.5, {}, {"row_base": 1_000_000}),   # filter_img8_kernel
    ("q200-d768", 200, "full", 255, 7.5, {}, {"d": 768}),      # img8: six ring chunks
    ("q200-d784", 200, "wide", 0, 1e-3, {}, {"d": 784}),       # past 768: img3 by shape
    ("q40-stream", 40, "wide", 64, 1e-3, {"img6": 0}, {"n": 3, "mask": True}),
    # k = 600 over a buffer of more than two select slices: the pruned selects
    ("q40-k600", 40, "wide", 64, 7.5, {}, {"n": 120_000, "k": 600, "cap": 36_864}),
]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", BITS, ids=[c[0] for c in BITS])
def test_batch_equals_per_query_scans(eng, case, metric):
    cid, nq, kind, zp, scale, opts, shape = case
    n, d = 40_000 + shape.get("n", 0), shape.get("d", 128)
    k, cap = shape.get("k", K), shape.get("cap", 4096)
    m = _lib.METRICS[metric]
    shard = _shard(eng, _codes(kind, n, d, zp), shape.get("row_base", 0), scale, zp)
    q = torch.from_numpy(_queries(nq, d, scale, 40.0)).to(eng.device)
    masks = None
    if shape.get("mask"):
        masks = [device_mask(np.random.RandomState(96).rand(n) < 0.6, eng.device)]
    eng.clear_images()
    want = _exact(eng, shard, q, m, k, masks)
    with _lib.options(**BASE, batch_cap=cap, **opts):
        assert _lib.filter_image_used(n, d, _lib.DTYPE_QU8, nq, k, m)
        gd, gr = eng.search([shard], q, m, k, masks)
        torch.cuda.synchronize()
        assert id(shard.data) in eng._images, "no image was built for the shard"
        # the same batch, its halves apart: it ran the filter against a
        # threshold (more rows than the buffer holds), and no query fell back
        # to the exact scan
        st = eng.scan(shard, q, m, k, masks[0] if masks else None)
        count, got_cap = eng.filter_counts(shard, nq, m, k, st)
        assert st.bits == 8 and got_cap == cap and n > 4 * cap
        od = torch.empty((nq, k), dtype=torch.float32, device=eng.device)
        orow = torch.empty((nq, k), dtype=torch.int64, device=eng.device)
        eng.reduce(shard, q, m, k, st, od, orow, masks[0] if masks else None)
        torch.cuda.synchronize()
    print(f"{cid}-{metric}: count/cap max {count.max() / cap:.3f}")
    assert (count.astype(np.int64) <= cap).all(), f"queries overflowed: {count.max()} > {cap}"
    _assert_bits((gd.cpu().numpy(), gr.cpu().numpy()), want, "search")
    _assert_bits((od.cpu().numpy(), orow.cpu().numpy()), want, "scan + reduce")
    eng.clear_images()


# ------------------------------------------------------------------ bounds --
def _near_queries(codes, nq, scale, zp):
    """Even queries: the dequantised values of a row; odd ones: that row moved
    by one code step in three components."""
    n, d = codes.shape
    rs = np.random.RandomState(97)
    q = np.empty((nq, d), dtype=np.float32)
    for i in range(nq):
        c = codes[rs.randint(n)].astype(np.int64)
        if i % 2:
            j = rs.choice(d, 3, replace=False)
            c[j] += np.where(c[j] >= 255, -1, 1)
        q[i] = O.dequantize(c, scale, zp)
    return q


def _offset_queries(codes, nq, scale, zp):
    """Within the rows' narrow range, far from the zero point: every second
    one a dequantised row plus noise of a tenth of a code step."""
    n, d = codes.shape
    rs = np.random.RandomState(98)
    lo, hi = int(codes.min()), int(codes.max())
    q = O.dequantize(rs.randint(lo, hi + 1, (nq, d)), scale, zp)
    for i in range(0, nq, 2):
        q[i] = O.dequantize(codes[rs.randint(n)], scale, zp)
    return (q + np.float32(0.1 * scale) * O.fill_normal(nq, d, seed=99)).astype(np.float32)


def _aligned_queries(codes, nq, scale, zp, spread):
    """Along +- a row's own int8 residual x - s rint(x / s), with
    image8_qu8_kernel's scale (in code units: t)."""
    n, d = codes.shape
    rs = np.random.RandomState(97)
    q = _queries(nq, d, scale, spread)
    for i in range(nq):
        y = codes[rs.randint(n)].astype(np.float64) - zp
        t = max(np.abs(y).max() / 127.0, np.sqrt((y * y).sum()) / (2046.0 - 0.5 * np.sqrt(d)))
        if t == 0:
            continue
        rho = y - t * np.clip(np.rint(y / t), -127, 127)
        if rho.any():
            sign = 1.0 if i % 4 < 2 else -1.0
            q[i] = (sign * rho / np.sqrt((rho * rho).sum()) * np.sqrt(d) * scale * spread
                    ).astype(np.float32)
    return q


# (id, nq, input, codes, zero point, scale, metrics, shape overrides)
BOUNDS = [
    ("qu8-q2", 2, "normal", "wide", 64, 1e-3, METRICS, {}),
    ("qu8-q40", 40, "normal", "full", 0, 7.5, METRICS, {}),
    ("qu8-q100", 100, "normal", "wide", 255, 7.5, METRICS, {"n": 3}),
    ("qu8-q200", 200, "normal", "wide", 64, 1e-3, METRICS, {"row_base": 1_000_000}),
    ("qu8-q100", 100, "clustered", "clustered", 128, 1e-3, METRICS, {}),
    ("qu8-q40", 40, "near", "wide", 64, 7.5, METRICS, {}),
    ("qu8-q200", 200, "near", "full", 0, 1e-3, METRICS, {"n": 3}),
    ("qu8-q40", 40, "offset-zp255", "hi", 255, 1e-3, ["l2"], {}),
    ("qu8-q100", 100, "offset-zp0", "lo", 0, 7.5, ["l2"], {}),
    ("qu8-q100", 100, "aligned", "full", 64, 7.5, METRICS, {}),
    ("qu8-q200", 200, "aligned", "wide", 0, 1e-3, METRICS, {}),
]
BOUND_CASES = [pytest.param(b, metric, id=f"{b[0]}-{metric}-{b[2]}")
               for b in BOUNDS for metric in b[6]]


class _QCase:
    """What test_gpu_filter_bounds._check_held / _check_default read of a
    case (its _Case), for a quint8 shard: the references are the quint8
    scan's own distances of the same shard."""

    fam = "i8"  # an int8 image: bits 8, the exact thresholds of D2

    def __init__(self, eng, bound, metric):
        self.id, self.nq, self.kind, ckind, zp, scale, _, shape = bound
        clustered = self.kind == "clustered"
        self.metric, self.m = metric, _lib.METRICS[metric]
        self.n = (160_000 if clustered else 40_000) + shape.get("n", 0)
        self.cap = 16_384 if clustered else 4096
        self.d, self.row_base = 128, shape.get("row_base", 0)
        self.opts = {**BASE, "batch_cap": self.cap}
        codes = _codes(ckind, self.n, self.d, zp)
        self.xv = O.dequantize(codes, scale, zp)
        spread = {"full": 74.0, "clustered": 20.0}.get(ckind, 40.0)
        if self.kind == "near":
            self.qh = _near_queries(codes, self.nq, scale, zp)
        elif self.kind.startswith("offset"):
            self.qh = _offset_queries(codes, self.nq, scale, zp)
        elif self.kind == "aligned":
            self.qh = _aligned_queries(codes, self.nq, scale, zp, spread)
        else:
            self.qh = _queries(self.nq, self.d, scale, spread)
        self.mask, self.dm, self.altered = None, None, []
        self.q = torch.from_numpy(self.qh).to(eng.device)
        self.shard = _shard(eng, codes, self.row_base, scale, zp)
        self.live = np.ones(self.n, dtype=bool)
        ds = eng.distances(self.shard, self.q, self.m)
        torch.cuda.synchronize()
        self.d_scan = ds.cpu().numpy()
        self.keys = parity.order_key(self.d_scan)
        grow = np.arange(self.n, dtype=np.uint64) + np.uint64(self.row_base)
        self.comp = (self.keys.astype(np.uint64) << np.uint64(32)) | grow[None, :]
        self.bad_rows = np.zeros(self.n, dtype=bool)  # every quint8 row is representable
        ss = np.einsum("ij,ij->i", self.xv, self.xv, dtype=np.float64)
        top = int(np.argmax(ss))
        self.scale = parity.scale_of(self.xv[top:top + 1], self.qh, metric)


@pytest.mark.parametrize("bound,metric", BOUND_CASES)
def test_filter_bounds_quint8(eng, bound, metric):
    """B1-B5 on the held state and D1-D3 on the default path (the checkers and
    their meaning: tests/test_gpu_filter_bounds.py).  No query is altered, so
    B2 allows no forced pair and B5 no query left out by count > cap."""
    eng.clear_images()
    c = _QCase(eng, bound, metric)
    stats = {"n": c.n, "d": c.d, "nq": c.nq, "metric": metric, "input": c.kind}
    failures = []
    for name, run in (("held", lambda: _check_held(eng, c, stats)),
                      ("default", lambda: _check_default(eng, c))):
        try:
            run()
        except AssertionError as e:
            failures.append(f"[{name}] {e}")
    print(f"{c.id}-{metric}-{c.kind}: {stats}")
    _record(f"{c.id}-{metric}-{c.kind}", stats)
    eng.clear_images()
    assert not failures, "\n".join(failures)


# ------------------------------------------------------- oracle, lifecycle --
@pytest.mark.parametrize("metric", METRICS)
def test_batch_matches_the_float64_oracle(eng, metric):
    n, d, nq, zp, scale = 40_003, 128, 16, 64, 1e-3
    codes = _codes("wide", n, d, zp)
    shard = _shard(eng, codes, 0, scale, zp)
    qh = _queries(nq, d, scale, 40.0, seed=101)
    eng.clear_images()
    with _lib.options(**BASE, batch_cap=4096):
        gd, gr = eng.search([shard], torch.from_numpy(qh), _lib.METRICS[metric], K)
        torch.cuda.synchronize()
        assert id(shard.data) in eng._images
    x = O.dequantize(codes, scale, zp)
    od, orow = O.knn(x, qh, metric, K)
    parity.check_topk(gd.cpu().numpy(), gr.cpu().numpy(), od, orow, x, qh, metric)
    eng.clear_images()


def test_a_write_to_the_codes_rebuilds_the_image(eng):
    n, d, nq, zp, scale = 40_000, 128, 40, 64, 7.5
    shard = _shard(eng, _codes("wide", n, d, zp).copy(), 0, scale, zp)
    q = torch.from_numpy(_queries(nq, d, scale, 40.0, seed=102)).to(eng.device)
    m = _lib.METRIC_L2
    eng.clear_images()
    with _lib.options(**BASE, batch_cap=4096):
        first = eng.search([shard], q, m, K)
        torch.cuda.synchronize()
        old = eng._images[id(shard.data)][1]
        # the nearest rows of every query change: the winners' codes are inverted
        rows = first[1].reshape(-1)
        shard.data[rows] = 255 - shard.data[rows]
        gd, gr = eng.search([shard], q, m, K)
        torch.cuda.synchronize()
        assert eng._images[id(shard.data)][1] is not old, "the stale image was kept"
    _assert_bits((gd.cpu().numpy(), gr.cpu().numpy()), _exact(eng, shard, q, m, K), "after a write")
    assert not np.array_equal(gr.cpu().numpy(), first[1].cpu().numpy())
    eng.clear_images()


@pytest.mark.parametrize("metric", METRICS)
def test_a_non_finite_query_overflows_into_the_exact_scan(eng, metric):
    n, d, nq, zp, scale = 40_000, 128, 40, 64, 1e-3
    shard = _shard(eng, _codes("wide", n, d, zp), 0, scale, zp)
    qh = _queries(nq, d, scale, 40.0, seed=103)
    qh[3, 5], qh[17, 0], qh[30] = np.inf, np.nan, qh[30] * np.float32(2.0 ** 100)
    q = torch.from_numpy(qh).to(eng.device)
    m = _lib.METRICS[metric]
    eng.clear_images()
    with _lib.options(**BASE, batch_cap=4096):
        gd, gr = eng.search([shard], q, m, K)
        st = eng.scan(shard, q, m, K)
        count, cap = eng.filter_counts(shard, nq, m, K, st)
        torch.cuda.synchronize()
    over = set(np.nonzero(count.astype(np.int64) > cap)[0].tolist())
    assert {3, 17} <= over <= {3, 17, 30}, over
    _assert_bits((gd.cpu().numpy(), gr.cpu().numpy()), _exact(eng, shard, q, m, K), metric)
    eng.clear_images()


def test_a_batched_search_does_not_synchronise(eng):
    n, d, nq, zp, scale = 40_000, 128, 40, 64, 1e-3
    shard = _shard(eng, _codes("wide", n, d, zp), 0, scale, zp)
    q = torch.from_numpy(_queries(nq, d, scale, 40.0, seed=104)).to(eng.device)
    eng.clear_images()
    with _lib.options(**BASE, batch_cap=4096):
        eng.search([shard], q, _lib.METRIC_L2, K)  # (builds the image)
        before = _lib.host_sync_count()
        for metric in METRICS:
            eng.search([shard], q, _lib.METRICS[metric], K)
        assert _lib.host_sync_count() == before
        torch.cuda.synchronize()
    eng.clear_images()


# ------------------------------------------------------------------ served --
def test_concurrent_flight_clients_share_image_batches(tmp_path):
    """8 Flight clients searching a quint8 table together: the coalescer
    (fenix_amd/coalesce.py) turns them into batches, a batch of >= 2 takes the
    int8 image, and every client gets its sequential single-query answer."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fenix_amd import engine

    n, d, clients, rounds = 40_000, 128, 8, 4
    x = O.fill_normal(n, d, seed=105, cluster=1000)
    src = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "vector": Q.from_numpy(x)})
    targets = O.fill_normal(clients * rounds, d, seed=106)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    server = fenix_amd.Server(str(tmp_path), host="127.0.0.1", port=port)
    try:
        fenix_amd.Flight(host="127.0.0.1", port=port).make_table("q/served", src.to_reader())

        def one(f, i):
            r = f.search(target=targets[i], source="q/served", column="vector", metric="l2",
                         select=["id"], maxval=20)
            return r.column("id").to_numpy(), r.column("__DISTANCE__").to_numpy()

        with _lib.options(**BASE, batch_cap=4096):
            f0 = fenix_amd.Flight(host="127.0.0.1", port=port)
            seq = [one(f0, i) for i in range(clients * rounds)]
            (entry,) = [e for e in engine.CACHE._entries.values() if "served" in e.key[0]]
            piece = entry.pieces[0]
            eng = Engine.get(piece.device)
            assert id(piece.data) not in eng._images  # single queries: the exact scan
            co = coalesce.default()
            b0, r0 = co.batches, co.requests
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
            assert id(piece.data) in eng._images, "no batch went through an image"
        for (a, da), (b, db) in zip(seq, par):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(da.view(np.uint32), db.view(np.uint32))
    finally:
        server.shutdown()
        engine.CACHE.clear()
        Engine.get(torch.device("cuda", 0)).clear_images()
