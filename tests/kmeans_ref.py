"""References for the k-means step (fx_kmeans_step / fx_kmeans_step_ex,
fenix_amd/csrc/knn_code.hip) — helpers only, no tests.

* ``planted``     codewords and sample rows around planted centres, with the
                  planned cluster of every row;
* ``check_plan``  the precondition that makes a comparison unambiguous: the
                  float64 argmin of every row is its planned cluster, by a
                  clear gap, so the kernel's f32 argmin is the plan too;
* ``step_f32``    update_kernel's documented order in np.float32 (L2, inner
                  product): the bits the kernel must return;
* ``step_f64``    oracle.coder.update_all;
* ``bound``       the acceptance against float64, in multiples of u = 2^-24;
* ``CASES``       the shapes tests/test_gpu_kmeans.py runs, with the host-side
                  consistency and sensitivity checks of
                  tests/test_kmeans_host.py over the same list.

``corruptions`` restates the step with one deliberate mistake each (a row
dropped, a row added twice, the slice boundary off by one, a codebook's rows
read from one row early, the codeword left out of its mean): what the GPU
acceptance has to reject.
"""

from __future__ import annotations

import functools
import math
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np

from oracle import coder as OC
from oracle import oracle as O

U = 2.0 ** -24          # unit roundoff of f32
SLICE = 1024            # update_kernel: assignments are compacted 1024 at a time
METRICS = ["l2", "inner_product", "cosine"]


def _cos(metric: str) -> bool:
    return O.METRIC_IDS[metric] == 2


def gamma(k) -> float:
    """k roundings: |prod (1 + d_i) - 1| <= k u / (1 - k u), |d_i| <= u."""
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------ inputs


def planted(nb: int, ks: int, bs: int, d: int, seed: int, plan=None, noise: float = 0.05
            ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(q [nb, ks, d] f32, v [nb, bs, d] f32, a [nb, bs] int32): every codebook
    has its own centres; row i of codebook j is centre a[j, i] plus noise, the
    codewords are the centres plus noise.  ``plan`` ([bs] or [nb, bs]) fixes a,
    otherwise it is drawn from RandomState(seed)."""
    centres = O.fill_normal(nb * ks, d, seed).reshape(nb, ks, d).astype(np.float64)
    if plan is None:
        a = np.random.RandomState(seed).randint(0, ks, size=(nb, bs))
    else:
        a = np.broadcast_to(np.asarray(plan), (nb, bs)).copy()
    assert a.min() >= 0 and a.max() < ks
    nv = O.fill_normal(nb * bs, d, seed + 1).reshape(nb, bs, d)
    nq = O.fill_normal(nb * ks, d, seed + 2).reshape(nb, ks, d)
    v = centres[np.arange(nb)[:, None], a] + noise * nv
    q = centres + noise * nq
    return q.astype(np.float32), v.astype(np.float32), a.astype(np.int32)


def check_plan(q: np.ndarray, v: np.ndarray, a: np.ndarray, metric: str) -> float:
    """Asserts, in float64, that every row's nearest codeword is its planned
    one and that the runner-up is at least 1e-3 * max(|best|, 1) further
    (1e-3 * max(|best|, 1e-3) for cosine).  A property of the inputs, not a
    tolerance on the kernel.  Returns the smallest relative gap (inf, ks = 1)."""
    floor = 1e-3 if _cos(metric) else 1.0
    worst = math.inf
    for j in range(q.shape[0]):
        qq, vv = (OC.normalize(q[j]), OC.normalize(v[j])) if _cos(metric) else (q[j], v[j])
        dist = OC.distance(vv, qq, metric)
        assert np.array_equal(np.argmin(dist, axis=1), a[j]), f"codebook {j}: argmin != plan"
        if dist.shape[1] == 1:
            continue
        two = np.partition(dist, 1, axis=1)[:, :2]
        rel = (two[:, 1] - two[:, 0]) / np.maximum(np.abs(two[:, 0]), floor)
        assert rel.min() >= 1e-3, f"codebook {j}: gap {rel.min():.3g}"
        worst = min(worst, float(rel.min()))
    return worst


def quantize(v: np.ndarray) -> Tuple[np.ndarray, float, int]:
    """uint8 codes of v under a scale covering its range and the (non-zero)
    zero point that puts its minimum at code 0."""
    lo, hi = float(v.min()), float(v.max())
    scale = float(np.float32((hi - lo) / 255.0))
    zp = int(round(-lo / scale))
    assert 0 < zp < 255
    codes = np.clip(np.rint(v.astype(np.float64) / scale) + zp, 0, 255).astype(np.uint8)
    return codes, scale, zp


# --------------------------------------------------------------- the step


def _rows(nb: int, bs: int, src) -> np.ndarray:
    return np.arange(nb * bs).reshape(nb, bs) if src is None else np.asarray(src)


def step_f32(q: np.ndarray, v: np.ndarray, a: np.ndarray, metric: str, src=None,
             dup: Iterable[Tuple[int, int]] = (), include_self: bool = True) -> np.ndarray:
    """update_kernel's sum in np.float32, L2 and inner product: acc = w
    (knn_code.hip "include_self"), then the member rows one at a time in
    ascending row index (slices ascending, the compacted list ascending inside
    a slice, the groups of four as t = 0..3), count = 1 + members,
    acc / float(count).  Only IEEE f32 adds and one divide, no multiply: the
    bits of the kernel.  v is what the kernel reads as f32: f16 rows widened,
    quint8 rows dequantised (oracle.dequantize, one rounding).

    The keyword arguments restate it with a mistake: ``a[j, i] < 0`` skips a
    row, ``src[j, i]`` is the flat row read for (j, i), ``dup`` rows are added
    twice, ``include_self=False`` starts from 0 with count = members."""
    assert not _cos(metric)
    nb, ks, d = q.shape
    bs = a.shape[1]
    flat = np.ascontiguousarray(v, dtype=np.float32).reshape(nb * bs, d)
    src = _rows(nb, bs, src)
    dup = set(dup)
    out = np.empty((nb, ks, d), np.float32)
    for j in range(nb):
        acc = q[j].astype(np.float32).copy() if include_self else np.zeros((ks, d), np.float32)
        count = np.full(ks, 1 if include_self else 0, np.int64)
        for i in range(bs):
            c = a[j, i]
            if c < 0:
                continue
            for _ in range(2 if (j, i) in dup else 1):
                acc[c] += flat[src[j, i]]
                count[c] += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            out[j] = acc / count.astype(np.float32)[:, None]
    return out


def step_f64(q: np.ndarray, v: np.ndarray, metric: str) -> np.ndarray:
    return OC.update_all(q, v, metric)


def step_f64_planned(q: np.ndarray, v: np.ndarray, a: np.ndarray, metric: str, src=None,
                     dup: Iterable[Tuple[int, int]] = (), include_self: bool = True
                     ) -> np.ndarray:
    """oracle.coder.update with the argmin replaced by the assignment a (equal
    to step_f64 wherever check_plan holds), and the mistakes of step_f32."""
    nb, ks, d = q.shape
    bs = a.shape[1]
    flat = np.asarray(v, dtype=np.float64).reshape(nb * bs, d)
    src = _rows(nb, bs, src)
    out = np.empty((nb, ks, d))
    for j in range(nb):
        qq, vv = np.asarray(q[j], np.float64), flat[src[j]]
        if _cos(metric):
            qq, vv = OC.normalize(qq), OC.normalize(vv)
        s = qq.copy() if include_self else np.zeros_like(qq)
        c = np.full(ks, 1.0 if include_self else 0.0)
        keep = a[j] >= 0
        np.add.at(s, a[j][keep], vv[keep])
        np.add.at(c, a[j][keep], 1.0)
        for jj, i in dup:
            if jj == j:
                s[a[j, i]] += vv[i]
                c[a[j, i]] += 1.0
        with np.errstate(invalid="ignore", divide="ignore"):
            m = s / c[:, None]
        out[j] = OC.normalize(m) if _cos(metric) else m
    return out


def bound(q: np.ndarray, v: np.ndarray, a: np.ndarray, metric: str) -> np.ndarray:
    """How far update_kernel's f32 result may lie from the float64 step, in
    multiples of u = 2^-24 only (correctly rounded add, fma, divide and sqrt:
    the library is built without fast-math).

    L2 and inner product — per element, [nb, ks, d]:

        |got - ref| <= count * u * (|w| + sum_members |v|) / count + u * |ref|

    The first term is the sequential sum of count terms (``acc[u] += v[t]``,
    count - 1 adds, each off by at most u times the partial sum, which the sum
    of magnitudes bounds); the second is ``acc[u] / (float)count``.  count is
    below 2^24, so (float)count is exact.

    Cosine — norm-wise per codeword, [nb, ks].  With m = ceil(d / 64) and
    p = ceil(d / 1024):

    * a normalised term t = x / max(|x|, 1e-12) (normalize_kernel for the
      codeword, rownorm_kernel mode 1 and ``v[t] / sc[t]`` for a row) comes
      with relative error gamma(kn), kn = (m + 6) / 2 + 2: the sum of squares
      takes m fmas per lane and 6 butterfly adds, all terms positive, so it
      is off by at most (m + 6) u relative; the square root halves that and
      rounds once; the divide rounds once.  (The issue's (m + 9) u counts the
      sum's error in full; the root halves it, so the derivation is used.)
    * the sum and the division by count add count more roundings to every
      term, so per element
          delta <= gamma(kn + count) * (|w^| + sum_members |v^|) / count
      with w^, v^ the exactly normalised codeword and rows;
    * the final ``acc[u] / nrm``: nrm takes p fmas per thread, 6 butterfly
      adds and 16 adds over ``red[]`` (p + 22 roundings of a positive sum),
      a root and the divide: e_f = gamma((p + 22) / 2 + 2).  Normalising
      y + delta instead of y moves the unit vector by at most
      2 |delta|_2 / |y|_2, so

          |got - ref|_2 <= 2 |delta|_2 / |y|_2 * (1 + e_f) + e_f.

      (The issue adds "one more normalisation term" (m + 9) u here; the last
      norm is reduced over 1024 threads, not 64 lanes, hence p and ``red``.)
      A codeword whose mean is exactly 0 (a zero codeword with zero members)
      stays 0: bound 0."""
    nb, ks, d = q.shape
    cos = _cos(metric)
    out = np.empty((nb, ks) if cos else (nb, ks, d))
    for j in range(nb):
        qq, vv = np.asarray(q[j], np.float64), np.asarray(v[j], np.float64)
        if cos:
            qq, vv = OC.normalize(qq), OC.normalize(vv)
        mag = np.abs(qq)
        s = qq.copy()
        count = np.ones(ks)
        np.add.at(mag, a[j], np.abs(vv))
        np.add.at(s, a[j], vv)
        np.add.at(count, a[j], 1.0)
        y = s / count[:, None]
        if not cos:
            out[j] = count[:, None] * U * mag / count[:, None] + U * np.abs(y)
            continue
        kn = (math.ceil(d / 64) + 6) / 2 + 2
        e_f = gamma((math.ceil(d / 1024) + 22) / 2 + 2)
        delta = gamma(kn + count)[:, None] * mag / count[:, None]
        dn, yn = np.sqrt((delta * delta).sum(1)), np.sqrt((y * y).sum(1))
        zero = yn == 0
        assert np.all(dn[zero] == 0)
        out[j] = np.where(zero, 0.0, 2 * dn / np.where(zero, 1.0, yn) * (1 + e_f) + e_f)
    return out


def error(got: np.ndarray, ref: np.ndarray, metric: str) -> np.ndarray:
    """What ``bound`` bounds: |got - ref| per element, per codeword's 2-norm
    for cosine.  NaN stays NaN."""
    diff = np.asarray(got, np.float64) - ref
    return np.sqrt((diff * diff).sum(-1)) if _cos(metric) else np.abs(diff)


def ratio(got: np.ndarray, ref: np.ndarray, bnd: np.ndarray, metric: str) -> float:
    """Largest error / bound (0 / 0 = 0; NaN or anything over a 0 bound = inf)."""
    err = error(got, ref, metric)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bnd)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


# ------------------------------------------------------------------ cases


def slice_plan(ks: int, bs: int) -> np.ndarray:
    """[bs] assignment that puts exact member counts into exact 1024-row
    slices (ks >= 14):

    cluster 0        empty;
    cluster 1        members only in the last slice (when there are two);
    cluster 2        rows 1023 and 1024 only: the two sides of a boundary;
    clusters 3..7    (1,2,3), (4,5,0), (5,1,4), (2,3,1), (3,4,2) members in
                     slices 0, 1, 2: with clusters 0 and 1 every slice sees
                     totals 0..5, every total % 4, scattered over the waves;
    clusters 8..     the remaining rows, round robin."""
    assert ks >= 14
    a = np.full(bs, -1, np.int64)

    def put(rows, c):
        for r in rows:
            if 0 <= r < bs and a[r] < 0:
                a[r] = c

    nslices = (bs + SLICE - 1) // SLICE
    put([1023, 1024], 2)
    if nslices > 1:
        put(range(max((nslices - 1) * SLICE, bs - 3), bs), 1)
    counts = {3: (1, 2, 3), 4: (4, 5, 0), 5: (5, 1, 4), 6: (2, 3, 1), 7: (3, 4, 2)}
    offs = {3: (7, 300, 650), 4: (1, 64, 65, 511, 1000), 5: (2, 63, 128, 640, 1022),
            6: (5, 129, 900), 7: (66, 67, 68, 1021)}
    for c, per in counts.items():
        for s, k in enumerate(per):
            put([s * SLICE + o for o in offs[c][:k]], c)
    free = np.nonzero(a < 0)[0]
    a[free] = 8 + np.arange(free.size) % (ks - 8)
    return a


class Case:
    """One GPU case: shape, plan, sample type and how it is handed over."""

    def __init__(self, name: str, nb: int, ks: int, bs: int, d: int, plan: str = "random",
                 dtype: str = "f32", form: str = "tensor", noise: float = 0.05,
                 cos_noise: float = 0.25):
        self.name, self.nb, self.ks, self.bs, self.d = name, nb, ks, bs, d
        self.plan, self.dtype, self.form = plan, dtype, form
        self.noise, self.cos_noise = noise, cos_noise

    def __repr__(self) -> str:
        return self.name


def _cases() -> List[Case]:
    c: List[Case] = []
    # d classes: update_kernel's register slots, the 64-lane strides of
    # rownorm_kernel / normalize_kernel; odd d: the assign kernel's scalar staging
    c.append(Case("d8", 2, 5, 70, 8))
    for d in (63, 64, 65):
        c.append(Case(f"d{d}", 2, 5, 70, d))
    for d in (1023, 1024):  # slot u = 0 full / u = 1 first used
        c.append(Case(f"d{d}", 1, 6, 40, d))
    c.append(Case("d1025_two_slices", 1, 6, 1100, 1025))
    c.append(Case("d2049", 1, 5, 40, 2049))  # slot u = 2 holds one dimension
    c.append(Case("d16384_cap", 1, 4, 64, 16384))  # all 16 slots
    # slices
    for d in (37, 64):
        for bs in (1, 3, 1023, 1024, 1025, 2050):
            c.append(Case(f"slices_d{d}_bs{bs}", 2, 14, bs, d, plan="slice"))
    # codebook sizes.  ks = 1: one sum of 1501 terms over two slices; its cosine
    # bound is 5.5e-4, and one row out of 1501 moves the unit mean by 4x that
    # only if the rows point well apart, hence the wide noise (with a single
    # codeword every row's argmin is the plan whatever the noise)
    c.append(Case("ks1_bs1500", 1, 1, 1500, 96, cos_noise=4.0))
    c.append(Case("ks260_d136", 2, 260, 150, 136))  # two 256-slot blocks of the assign kernel
    c.append(Case("nb3_bs1025_d37", 3, 5, 1025, 37))
    # types
    c.append(Case("f16_small", 2, 5, 70, 64, dtype="f16"))
    c.append(Case("f16_d1025_two_slices", 1, 6, 1100, 1025, dtype="f16"))
    for form in ("scale", "shard"):
        c.append(Case(f"qu8_small_{form}", 2, 5, 70, 64, dtype="qu8", form=form))
        c.append(Case(f"qu8_d1025_two_slices_{form}", 1, 6, 1100, 1025, dtype="qu8", form=form))
    return c


CASES: List[Case] = _cases()
CASE = {c.name: c for c in CASES}


class Data:
    """Inputs and references of one (case, metric), computed once.

    q, a       codewords f32, plan
    sample     what the engine gets: f32 / f16 values or uint8 codes (+ scale, zp)
    v          the rows as the kernel reads them, f32
    f64        step_f64; f32: step_f32 (None for cosine); bound"""

    def __init__(self, case: Case, metric: str):
        self.case, self.metric = case, metric
        cos = _cos(metric)
        seed = 1000 + 7 * CASES.index(case)
        plan = slice_plan(case.ks, case.bs) if case.plan == "slice" else None
        q, v, a = planted(case.nb, case.ks, case.bs, case.d, seed, plan,
                          case.cos_noise if cos else case.noise)
        self.q, self.a = q, a
        self.scale, self.zp = 1.0, 0
        if case.dtype == "f16":
            self.sample = v.astype(np.float16)
            self.v = self.sample.astype(np.float32)
        elif case.dtype == "qu8":
            self.sample, self.scale, self.zp = quantize(v)
            self.v = O.dequantize(self.sample, self.scale, self.zp)
            assert self.v.dtype == np.float32
        else:
            self.sample = self.v = v
        self.gap = check_plan(self.q, self.v, self.a, metric)
        self.f64 = step_f64(self.q, self.v, metric)
        self.f32 = None if cos else step_f32(self.q, self.v, self.a, metric)
        self.bound = bound(self.q, self.v, self.a, metric)

    def members(self, j: int) -> np.ndarray:
        return np.bincount(self.a[j], minlength=self.case.ks)


@functools.lru_cache(maxsize=None)
def data(name: str, metric: str) -> Data:
    return Data(CASE[name], metric)


FLOOR_ZERO_ROW, FLOOR_ZERO_WORD = 5, 2


def floor_case(metric: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray, List[int]]:
    """The 1e-12 floor (d = 16, ks = 3, bs = 8, nb = 1): sample row 5 and
    codeword 2 are all zeros.  Returns (q, v, a, tied): a holds the plan of
    the other rows (clusters 0 and 1; check_plan covers them) and, for the
    zero row, the first of ``tied``, the clusters at its float64 minimum.

    What oracle.coder.update does with the zeros, as the project's model:
    x / max(|x|, 1e-12) of a zero vector is 0, so the cosine distance between
    a zero vector and anything is 0.5 - 0.5 * 0 = 0.5: the zero row ties over
    all three codewords, every other row is nearer to its own centre
    (distance < 0.5), and the zero codeword, gaining at most the zero row,
    stays 0 (0 / 1e-12).  The zero row's inner products are all 0 as well: the
    same tie.  Under L2 the zero row belongs to the zero codeword alone."""
    nb, ks, bs, d = 1, 3, 8, 16
    plan = np.array([0, 1, 1, 0, 1, 0, 0, 1])
    q, v, a = planted(nb, ks, bs, d, 4242, plan, 0.25 if _cos(metric) else 0.05)
    q[0, FLOOR_ZERO_WORD] = 0
    v[0, FLOOR_ZERO_ROW] = 0
    qq, vv = (OC.normalize(q[0]), OC.normalize(v[0])) if _cos(metric) else (q[0], v[0])
    dz = OC.distance(vv[FLOOR_ZERO_ROW:FLOOR_ZERO_ROW + 1], qq, metric)[0]
    tied = [int(c) for c in np.nonzero(dz == dz.min())[0]]
    a[0, FLOOR_ZERO_ROW] = tied[0]
    return q, v, a, tied


def corruptions(dt: Data) -> Dict[str, dict]:
    """Keyword arguments of step_f32 / step_f64_planned for every mistake that
    applies to the case.  Rows are taken from the largest cluster of the last
    codebook, where one row weighs least."""
    case, a = dt.case, dt.a
    nb, bs, ks = case.nb, case.bs, case.ks
    j = nb - 1
    big = int(np.argmax(dt.members(j)))
    row = int(np.nonzero(a[j] == big)[0][-1])
    out: Dict[str, dict] = {}
    dropped = a.copy()
    dropped[j, row] = -1
    out["row_dropped"] = dict(a=dropped)
    out["row_twice"] = dict(a=a, dup=[(j, row)])
    if bs > SLICE:
        skipped = a.copy()
        skipped[j, SLICE] = -1
        out["boundary_row_skipped"] = dict(a=skipped)
        if ks > 1:
            moved = a.copy()
            moved[j, SLICE] = (a[j, SLICE] + 1) % ks
            out["boundary_row_in_wrong_cluster"] = dict(a=moved)
    if nb > 1:  # codebook j >= 1 reads from row j * bs - 1 on
        src = np.arange(nb * bs).reshape(nb, bs).copy()
        src[1:] -= 1
        out["codebook_offset_minus_one"] = dict(a=a, src=src)
    out["include_self_forgotten"] = dict(a=a, include_self=False)
    return out
