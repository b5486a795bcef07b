"""The batched filter's bounds and pass test, looked at directly.

Every other filter test compares the final top-k with the exact scan.  A
result depends only on rows at or below the final k-th distance, far inside
the thresholds the passes test against, so a bound or pass test that is
unsound by a few ulps, or an epilogue that pairs the wrong row terms with an
accumulator, moves none of them.  Here the filter's own output is read back
(library option "filter_hold": the phases stop after their last filter pass,
``Engine.filter_bounds``) and checked per (row, query) pair against the scan's
own f32 distances ``d_scan`` (``Engine.distances``), in ``order_key`` space:

* B1  the lb and ub lists hold the same rows in the same slots; rows lie in
      [row_base, row_base + n), none twice, none masked out;
* B2  key(lb) <= key(d_scan) <= key(ub) for every slot, no tolerance (the
      contract of the derivations in csrc/filter/tiled.inc and
      csrc/knn_filter.hip); a forced pair (lb = -inf) only for rows the
      filter cannot represent or for the queries the case altered;
* B3  lb <= d64 + tol and ub >= d64 - tol against the float64 oracle with the
      scan's own tolerance (parity.DIST_RTOL), over the pairs whose f32 scan
      distance and float64 distance are finite (the scan's parity rule says
      nothing where f32 overflows): implied by B2 and scan parity, so it fails
      only if B2's reference is itself wrong;
* B4  every live row with comp(d_scan, row) <= thr[q] is a candidate (the
      packed pass test loses nothing), for every query with count <= cap;
* B5  the queries B1-B4 leave out (count > cap: overflowed, or marked by the
      overflow gate, whose slots past the first pass's are not written) are a
      subset of the queries the case altered; none for the other inputs.

and on the default path (same inputs, no hold, state read between scan and
reduce):

* D1  a kept slot holds exactly make_comp(d_scan, row); a slot the rescoring
      emptied has comp(d_scan, row) > thr[q];
* D2  thr[q] >= the k-th smallest live comp(d_scan, .); with an int8 image it
      is the exact composite of a candidate row, on the fp16 paths (whose
      final threshold is the k-th upper bound, capi.hip filter_phases) it is
      the k-th smallest ub composite of the candidates;
* D3  after the reduce, rows and distance bits equal the unbatched search.

How tight the bounds are (count / cap, count / rows under the threshold,
(ub - lb) / scale) is recorded in filter_bounds.json, in the directory of the
suite's other recorded results (tests/test_gpu_fullsize.OUT), not asserted.

What these checks can and cannot see is in DESIGN.md 3.6, item 6: the u-sized
slacks of the int8 bounds are 1e-4 of the bracket's width (no input makes them
bind); the "aligned" input exists to load the quantisation term E itself.
"""

from __future__ import annotations

import functools
import json
import os

import numpy as np
import pytest
import torch

from fenix_amd import _lib
from fenix_amd.engine import Engine, Shard, device_mask
from oracle import oracle as O
from tests import parity
from tests.test_gpu_fullsize import OUT  # where the suite records measured numbers
from tests.test_gpu_kernels import _extreme_rows

pytestmark = pytest.mark.gpu

METRICS = ["l2", "inner_product", "cosine"]
INPUTS = ["normal", "clustered", "extreme"]
K = 10
# rows and candidate buffer ("batch_cap") per input.  40 000 rows are 157 tiles
# of 256: the int8 plan's samples are 2 and 20 tiles (all-pass, F1) and F2 the
# other 137; "batch_sample_ratio" 8 gives the fp16 paths 3, 20, 157.  Against a
# corpus in clusters of 1 000 rows the candidates come in whole clusters (the
# fp16 paths' strided samples can miss the best one; an inner product or cosine
# hardly tells the rows of a cluster apart), several thousand per query: those
# cases take 4x the buffer and 4x the rows, which keeps three phases (more than
# 8 x cap rows): 625 tiles, samples of 5 and 79 (int8) or 10 and 79 (fp16).
SHAPE = {"normal": (40_000, 4096), "extreme": (40_000, 4096), "clustered": (160_000, 16_384),
         "aligned": (40_000, 4096)}
KEY_NEG_INF = 0x007FFFFF  # order_key(-inf): a forced pair's lb

I8 = {"filter_image": 8, "batch_min_queries": 1}
F16IMG = {"filter_image": 16, "batch_sample_ratio": 8}
NOIMG = {"filter_image": 0, "batch_sample_ratio": 8}

# (id, family, nq, corpus dtype, options, shape overrides: "n" is added to the
# input's row count); the kernel each batch size reaches: launch_filter
# (csrc/knn_filter.hip).
VARIANTS = [
    # int8 image of f32 rows: q64i img6 (1, 2: the rescore-all path), q128 img6,
    # filter_img8_kernel; with img6 / img8 off the streamed filter_img3_kernel<., true>
    ("i8-q1", "i8", 1, "f32", I8, {}),
    ("i8-q2", "i8", 2, "f32", I8, {}),
    ("i8-q40", "i8", 40, "f32", I8, {}),
    ("i8-q100", "i8", 100, "f32", I8, {"n": 3}),
    ("i8-q200", "i8", 200, "f32", I8, {"row_base": 1_000_000}),
    ("i8-q40-stream", "i8", 40, "f32", {**I8, "img6": 0}, {}),
    ("i8-q100-stream", "i8", 100, "f32", {**I8, "img6": 0}, {}),
    ("i8-q200-stream", "i8", 200, "f32", {**I8, "img8": 0}, {"n": 3}),
    ("i8-q200-d768", "i8", 200, "f32", I8, {"d": 768}),   # img8: six ring chunks
    ("i8-q200-d776", "i8", 200, "f32", I8, {"d": 776}),   # past 768: img3 by shape
    # fp16 image of f32 rows: q64, q128, q256 filter_img3_kernel<., false>
    ("h16-q40", "h16", 40, "f32", F16IMG, {}),
    ("h16-q100", "h16", 100, "f32", F16IMG, {"n": 3}),
    ("h16-q200", "h16", 200, "f32", F16IMG, {}),
    # f32 rows, no image: the register-staged kernels
    ("f32-q40", "f32", 40, "f32", NOIMG, {}),
    ("f32-q100", "f32", 100, "f32", NOIMG, {"n": 3}),
    ("f32-q200", "f32", 200, "f32", NOIMG, {}),
    # f16 corpus, no image: q64, q128, h256
    ("f16-q40", "f16", 40, "f16", NOIMG, {}),
    ("f16-q100", "f16", 100, "f16", NOIMG, {"n": 3}),
    ("f16-q200", "f16", 200, "f16", NOIMG, {}),
    # f16 corpus, int8 image
    ("f16i8-q40", "f16i8", 40, "f16", I8, {"n": 3}),
]

# every variant with every metric; the input rotates, so that every family
# meets every metric and every input (checked below).  The two d >= 768
# variants meet the clustered corpus under L2, where that input has its point
# (distances near 0: the expansion cancels and lb clamps): at that width the
# int8 bounds on an inner product or cosine span most of the spread between the
# cluster centres, so a fifth of a corpus of 40 to 160 clusters stays candidate
# -- more than any buffer that still leaves three phases (cap < n / 8).
CASES = []
for _vi, _v in enumerate(VARIANTS):
    for _mi, _metric in enumerate(METRICS):
        _inp = INPUTS[(_vi + _mi) % 3]
        if "d" in _v[5]:
            _inp = {"l2": "clustered", "inner_product": INPUTS[_vi % 2 * 2],
                    "cosine": INPUTS[2 - _vi % 2 * 2]}[_metric]
        CASES.append(pytest.param(_v, _metric, _inp, id=f"{_v[0]}-{_metric}-{_inp}"))
# and per family one variant with the fourth input, "aligned": normal rows,
# queries built so that the filter's own rounding errors add up instead of
# averaging out (_aligned_queries) -- on random data the observed error is a
# fraction 1 / sqrt(d) of what the bounds allow
for _v in VARIANTS:
    if _v[0] in ("i8-q100", "i8-q200", "h16-q100", "f32-q100", "f16-q100", "f16i8-q40"):
        for _metric in METRICS:
            CASES.append(pytest.param(_v, _metric, "aligned", id=f"{_v[0]}-{_metric}-aligned"))


def test_every_family_meets_every_metric_and_input():
    fams = {v[1] for v in VARIANTS}
    seen_m = {(c.values[0][1], c.values[1]) for c in CASES}
    seen_i = {(c.values[0][1], c.values[2]) for c in CASES}
    assert seen_m == {(f, m) for f in fams for m in METRICS}
    assert seen_i == {(f, i) for f in fams for i in INPUTS + ["aligned"]}


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine.get(torch.device("cuda", 0))


@functools.lru_cache(maxsize=2)
def _extreme(n, d):
    """_extreme_rows plus rows with one component 1e4 times the rest (a coarse
    int8 scale, a large omega); one generation per shape."""
    xh = _extreme_rows(n, d, 93)
    spike = np.random.RandomState(94).choice(n, 16, replace=False)
    xh[spike, spike % d] *= 1e4
    return xh


def _corpus(eng, kind, n, d, dtype, row_base):
    """(device rows, host copy) of an input kind in the corpus dtype."""
    tdt = torch.float16 if dtype == "f16" else torch.float32
    if kind == "extreme":
        xh = _extreme(n, d)
        if dtype == "f16":
            with np.errstate(over="ignore"):
                xh = xh.astype(np.float16)  # (|x| >= 65520: an f16 infinity)
        return torch.from_numpy(xh).to(eng.device), xh
    # the portable generator (bit-identical to oracle.fill_normal: test_fill_bit_exact)
    x = torch.empty((n, d), dtype=tdt, device=eng.device)
    eng.fill(x, 92 if kind == "clustered" else 91, row_base, 1000 if kind == "clustered" else 0)
    xh = x.cpu().numpy()
    if kind == "aligned":
        # rows whose int8 image keeps one component only (127 at component 0, the
        # others, below half a step, round to 0): the smallest w = |x~| against
        # the largest residual, so the residual term of omega is nearly all of it
        rs = np.random.RandomState(98)
        spike = _spike_rows(n)
        tail = (rs.rand(len(spike), d) - 0.5) * (0.98 * 8.0 / 127.0)
        tail[:, 0] = 8.0
        xh[spike] = tail.astype(xh.dtype)
        x = torch.from_numpy(xh).to(eng.device)
    return x, xh


def _spike_rows(n):
    return np.random.RandomState(99).choice(n, 64, replace=False)


def _aligned_queries(xv, nq, fam):
    """Queries against which one row's filter error is as large as the
    derivation allows for: along +- the row's own quantisation residual (int8
    image: x - s rint(x / s) with launch_image8's scale; fp16 image or f32 rows
    converted in registers: x - fp16(x)), or, every second query of the fp16
    filters and all of an f16 corpus (whose rows are exact), a query whose own
    fp16 rounding errors (0.49 ulp each, at qprep_kernel's scale) all carry the
    sign of that row's components."""
    n, d = xv.shape
    q = O.fill_normal(nq, d, seed=95)
    rs = np.random.RandomState(97)
    spike = _spike_rows(n)
    for i in range(nq):
        # (the first 64 queries: against the one-component rows, the nearest
        # rows of their queries under L2)
        x = xv[spike[i] if i < len(spike) else rs.randint(n)].astype(np.float64)
        sign = 1.0 if i % 4 < 2 else -1.0
        rho = None
        if fam in ("i8", "f16i8"):
            sc = max(np.abs(x).max() / 127.0, np.sqrt((x * x).sum()) / (2046.0 - 0.5 * np.sqrt(d)))
            rho = x - sc * np.clip(np.rint(x / sc), -127, 127)
        elif fam in ("h16", "f32") and i % 2 == 0:
            rho = x - x.astype(np.float16).astype(np.float64)
        if rho is not None and rho.any():
            q[i] = (sign * rho / np.sqrt((rho * rho).sum()) * np.sqrt(d)).astype(np.float32)
        elif rho is None:
            scale = 2.0 ** (15 - np.frexp(float(np.abs(q[i]).max()))[1])
            h = (q[i].astype(np.float64) * scale).astype(np.float16)
            ulp = np.spacing(np.abs(h)).astype(np.float64)
            q[i] = ((h.astype(np.float64) + sign * np.sign(x) * 0.49 * ulp) / scale).astype(np.float32)
    return q


def _queries(kind, xv, nq, dtype, fam):
    """(f32 queries, mask or None, altered queries) for rows xv (as f32)."""
    n, d = xv.shape
    if kind == "aligned":
        return _aligned_queries(xv, nq, fam), None, []
    q = O.fill_normal(nq, d, seed=95)
    if dtype == "f16":
        q = q.astype(np.float16).astype(np.float32)
    mask, altered = None, []
    rs = np.random.RandomState(96)
    if kind == "clustered":
        # every second query: a corpus row plus 1e-3 noise (L2 distance near 0,
        # where n^2 + q^2 - 2 x.q cancels and lb must clamp)
        for i in range(0, nq, 2):
            q[i] = xv[rs.randint(n)] + np.float32(1e-3) * O.fill_normal(1, d, seed=200 + i)[0]
    elif kind == "extreme":
        mask = rs.rand(n) < 0.8
        sel = np.random.RandomState(93).choice(n, 48, replace=False)  # _extreme_rows' picks
        # query 0 stays as generated; then x 2^60, x 2^-60, a huge row (of an f16
        # corpus: with infinities), a tiny row, zero, and an infinite and a NaN
        # component (a non-finite query is forced through every filter)
        def put(v, j, val):
            v = v.copy()
            v[j] = val
            return v
        edits = [lambda v: v * np.float32(2.0 ** 60), lambda v: v * np.float32(2.0 ** -60),
                 lambda v: xv[sel[0]], lambda v: xv[sel[8]], lambda v: np.zeros_like(v),
                 lambda v: put(v, 3, np.inf), lambda v: put(v, 7, np.nan)]
        for i, f in zip(range(1, nq), edits):
            with np.errstate(over="ignore", invalid="ignore"):
                q[i] = f(q[i])
            altered.append(i)
    return q, mask, altered


def _unrepresentable(xv, fam):
    """Rows the family's filter forces through: non-finite ones; on the fp16
    filters of f32 rows also a component that rounds to an fp16 infinity or a
    sum of squares past f32 (csrc/knn_filter.hip); with an int8 image also a
    row too small to scale (image8_kernel: tiny)."""
    with np.errstate(over="ignore", invalid="ignore"):
        bad = ~np.isfinite(xv).all(axis=1)
        amax = np.nanmax(np.abs(xv), axis=1).astype(np.float64)
        ss = np.einsum("ij,ij->i", xv, xv, dtype=np.float64)
        if fam in ("h16", "f32"):
            bad |= (amax >= 65520.0) | ~(ss <= 3.4e38)
        if fam in ("i8", "f16i8"):
            bad |= (amax != 0) & ~(np.maximum(amax / 127.0, np.sqrt(ss) / 2000.0) > 1e-30)
            bad |= ~(ss <= 3.4e38)
    return bad


_STATS = {}


def _record(case_id, stats):
    _STATS[case_id] = stats
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "filter_bounds.json"), "w") as f:
        json.dump(_STATS, f, indent=1, sort_keys=True)


class _Case:
    """One case's inputs on the device and its references: d_scan keys and
    composites [nq, n] (computed once, read by both halves)."""

    def __init__(self, eng, variant, metric, kind):
        self.id, self.fam, self.nq, self.dtype, self.opts, shape = variant
        self.metric, self.kind, self.m = metric, kind, _lib.METRICS[metric]
        self.n, self.cap = SHAPE[kind][0] + shape.get("n", 0), SHAPE[kind][1]
        self.d, self.row_base = shape.get("d", 136), shape.get("row_base", 0)
        self.opts = {**self.opts, "batch_cap": self.cap}
        self.x, self.xh = _corpus(eng, kind, self.n, self.d, self.dtype, self.row_base)
        self.xv = self.xh if self.xh.dtype == np.float32 else self.xh.astype(np.float32)
        self.qh, self.mask, self.altered = _queries(kind, self.xv, self.nq, self.dtype, self.fam)
        self.q = torch.from_numpy(self.qh).to(eng.device)
        self.dm = device_mask(self.mask, eng.device) if self.mask is not None else None
        self.shard = Shard(self.x, self.row_base)
        self.live = self.mask if self.mask is not None else np.ones(self.n, dtype=bool)
        with _lib.options(batched=0):
            ds = eng.distances(self.shard, self.q, self.m)
            torch.cuda.synchronize()
        self.d_scan = ds.cpu().numpy()
        self.keys = parity.order_key(self.d_scan)                     # [nq, n] uint32
        grow = np.arange(self.n, dtype=np.uint64) + np.uint64(self.row_base)
        self.comp = (self.keys.astype(np.uint64) << np.uint64(32)) | grow[None, :]
        if kind == "extreme":
            self.bad_rows = _unrepresentable(self.xv, self.fam)
        else:
            self.bad_rows = np.zeros(self.n, dtype=bool)
        # parity.scale_of reads the rows' largest norm only: hand it that row
        with np.errstate(over="ignore", invalid="ignore"):
            ss = np.einsum("ij,ij->i", self.xv, self.xv, dtype=np.float64)
        top = int(np.argmax(np.where(np.isfinite(ss), ss, -1.0)))
        self.scale = parity.scale_of(self.xv[top:top + 1], self.qh, metric)  # [nq]


def _check_held(eng, c, stats):
    with _lib.options(**c.opts):
        st = eng.filter_bounds(c.shard, c.q, c.m, K, c.dm)
    assert st is not None, "the search did not run the filter"
    assert st["bits"] == {"i8": 8, "f16i8": 8, "h16": 16}.get(c.fam, 0), st["bits"]
    cap, count, thr = st["cap"], st["count"].astype(np.int64), st["thr"]
    # the phase structure: more rows than the buffer holds, so the last pass
    # ran against a threshold
    assert cap == c.cap and c.n > 8 * cap
    normal = np.array([i not in c.altered for i in range(c.nq)])
    assert (thr[normal] != parity.EMPTY).all(), "a query reached the last pass without a threshold"
    # B5
    over = np.nonzero(count > cap)[0]
    assert set(over.tolist()) <= set(c.altered), (
        f"B5: queries {over.tolist()} overflowed (counts {count[over].tolist()}, cap {cap})")
    forced = 0
    ratio_cap, ratio_need, width, margin = [], [], [], []
    for qi in range(c.nq):
        cq = int(count[qi])
        if cq > cap:
            continue
        lbc, ubc = st["cand"][qi, :cq], st["cand_ub"][qi, :cq]
        rows = parity.comp_row(lbc) - c.row_base
        # B1
        assert np.array_equal(parity.comp_row(ubc) - c.row_base, rows), f"B1 q{qi}: lb / ub rows differ"
        assert ((rows >= 0) & (rows < c.n)).all(), f"B1 q{qi}: rows out of range"
        assert len(np.unique(rows)) == cq, f"B1 q{qi}: a row appended twice"
        assert c.live[rows].all(), f"B1 q{qi}: masked-out rows {rows[~c.live[rows]][:5]}"
        # B2
        klb, kub, ks = parity.comp_key(lbc), parity.comp_key(ubc), c.keys[qi, rows]
        lo, hi = np.nonzero(klb > ks)[0], np.nonzero(kub < ks)[0]
        lb, ub = parity.key_float(klb), parity.key_float(kub)
        assert len(lo) == 0, (f"B2 q{qi}: lb above the scan's distance at rows {rows[lo][:5]}: "
                              f"lb {lb[lo][:5]!r} d_scan {c.d_scan[qi, rows[lo]][:5]!r}")
        assert len(hi) == 0, (f"B2 q{qi}: ub below the scan's distance at rows {rows[hi][:5]}: "
                              f"ub {ub[hi][:5]!r} d_scan {c.d_scan[qi, rows[hi]][:5]!r}")
        with np.errstate(invalid="ignore", over="ignore"):
            wd = ub.astype(np.float64) - lb
            pos = (c.d_scan[qi, rows] - lb.astype(np.float64)) / wd
            pos = pos[np.isfinite(pos) & (wd > 0)]
        if len(pos):
            margin.append((float(pos.min()), float((1.0 - pos).min())))
        f = klb == KEY_NEG_INF
        forced += int(f.sum())
        if qi not in c.altered:
            assert c.bad_rows[rows[f]].all(), (
                f"B2 q{qi}: representable rows {rows[f][~c.bad_rows[rows[f]]][:5]} forced through")
        # B3
        if cq:
            with np.errstate(invalid="ignore", over="ignore"):
                d64 = O.distance_f64(c.xv[rows], c.qh[qi], c.metric)[0]
                ok = np.isfinite(d64) & np.isfinite(c.d_scan[qi, rows])
                tol = parity.DIST_RTOL * np.fmax(np.abs(d64), c.scale[qi])
                lb64 = lb.astype(np.float64)
                ub64 = np.where(np.isnan(ub), np.inf, ub.astype(np.float64))  # NaN: above every key
                bad = ok & ~((lb64 <= d64 + tol) & (ub64 >= d64 - tol))
            assert not bad.any(), (f"B3 q{qi}: rows {rows[bad][:5]} lb {lb[bad][:5]!r} "
                                   f"ub {ub[bad][:5]!r} d64 {d64[bad][:5]!r}")
            fin = ok & np.isfinite(lb64) & np.isfinite(ub64)
            if fin.any() and np.isfinite(c.scale[qi]):
                width.append((ub64[fin] - lb64[fin]) / c.scale[qi])
        # B4
        need = c.live & (c.comp[qi] <= thr[qi])
        present = np.zeros(c.n, dtype=bool)
        present[rows] = True
        miss = np.nonzero(need & ~present)[0]
        assert len(miss) == 0, (
            f"B4 q{qi}: {len(miss)} rows under the threshold "
            f"{parity.key_float(parity.comp_key(thr[qi:qi + 1]))[0]!r} were dropped: rows "
            f"{miss[:5]} d_scan {c.d_scan[qi, miss[:5]]!r}")
        ratio_cap.append(cq / cap)
        ratio_need.append(cq / max(int(need.sum()), 1))
    w = np.concatenate(width) if width else np.zeros(1)
    stats.update({"count_over_cap_median": float(np.median(ratio_cap)) if ratio_cap else None,
                  "count_over_cap_max": float(np.max(ratio_cap)) if ratio_cap else None,
                  "count_over_needed_median": float(np.median(ratio_need)) if ratio_need else None,
                  "count_over_needed_max": float(np.max(ratio_need)) if ratio_need else None,
                  "width_over_scale_median": float(np.median(w)),
                  "width_over_scale_max": float(np.max(w)),
                  # where in its bracket the scan's distance sits, nearest to either
                  # end, as a fraction of the width (0: on the bound)
                  "margin_to_lb_min": min(m[0] for m in margin) if margin else None,
                  "margin_to_ub_min": min(m[1] for m in margin) if margin else None,
                  "forced_pairs": forced, "queries_over_cap": over.tolist()})


def _check_default(eng, c):
    with _lib.options(**c.opts):
        st = eng.scan(c.shard, c.q, c.m, K, c.dm)
        count, cap = eng.filter_counts(c.shard, c.nq, c.m, K, st)
        assert count is not None
        thr, cand, cub = eng.filter_state(c.shard, c.nq, c.m, K, st, cap)
        od = torch.empty((c.nq, K), dtype=torch.float32, device=eng.device)
        orow = torch.empty((c.nq, K), dtype=torch.int64, device=eng.device)
        eng.reduce(c.shard, c.q, c.m, K, st, od, orow, c.dm)
        torch.cuda.synchronize()
    count = count.astype(np.int64)
    over = np.nonzero(count > cap)[0]
    assert set(over.tolist()) <= set(c.altered), f"queries {over.tolist()} overflowed"
    for qi in range(c.nq):
        cq = int(count[qi])
        if cq > cap:
            continue
        got, rows = cand[qi, :cq], parity.comp_row(cub[qi, :cq]) - c.row_base
        assert ((rows >= 0) & (rows < c.n)).all()
        want = c.comp[qi, rows]
        kept = got != parity.EMPTY
        # D1
        bad = np.nonzero(kept & (got != want))[0]
        assert len(bad) == 0, (f"D1 q{qi}: slots {bad[:5]} hold {got[bad][:5]} for rows "
                               f"{rows[bad][:5]}, the scan's composites are {want[bad][:5]}")
        bad = np.nonzero(~kept & (want <= thr[qi]))[0]
        assert len(bad) == 0, f"D1 q{qi}: rows {rows[bad][:5]} under the threshold were emptied"
        # D2
        kth = np.partition(c.comp[qi, c.live], K - 1)[K - 1]
        assert thr[qi] != parity.EMPTY and thr[qi] >= kth, (
            f"D2 q{qi}: threshold {thr[qi]} below the k-th composite {kth}")
        if c.fam in ("i8", "f16i8"):
            assert (want == thr[qi]).any(), f"D2 q{qi}: the threshold is no candidate's composite"
        else:
            assert cq >= K and thr[qi] == np.sort(cub[qi, :cq])[K - 1], (
                f"D2 q{qi}: the threshold is not the k-th upper bound")
    # D3
    msk = [c.dm] if c.dm is not None else None
    with _lib.options(batched=0):
        sd, sr = eng.search([c.shard], c.q, c.m, K, msk)
        torch.cuda.synchronize()
    np.testing.assert_array_equal(orow.cpu().numpy(), sr.cpu().numpy(), err_msg="D3 rows")
    np.testing.assert_array_equal(od.cpu().numpy().view(np.uint32),
                                  sd.cpu().numpy().view(np.uint32), err_msg="D3 distance bits")


@pytest.mark.parametrize("variant,metric,kind", CASES)
def test_filter_bounds(eng, variant, metric, kind):
    """B1-B5 on the held state and D1-D3 on the default path of one case (see
    the module's docstring); both halves run, and every failure is reported."""
    eng.clear_images()
    c = _Case(eng, variant, metric, kind)
    stats = {"n": c.n, "d": c.d, "nq": c.nq, "metric": metric, "input": kind}
    failures = []
    for name, run in (("held", lambda: _check_held(eng, c, stats)),
                      ("default", lambda: _check_default(eng, c))):
        try:
            run()
        except AssertionError as e:
            failures.append(f"[{name}] {e}")
    _record(f"{c.id}-{metric}-{kind}", stats)
    eng.clear_images()
    assert not failures, "\n".join(failures)
