"""The k-means step (fx_kmeans_step / fx_kmeans_step_ex: normalize_kernel,
rownorm_kernel, the grouped assign_kernel, finalize_kernel, update_kernel of
fenix_amd/csrc/knn_code.hip) and fx_row_sqnorms against independent
references (tests/kmeans_ref.py), through Engine.kmeans_step.

Acceptance.  L2 and inner product: the codewords equal ``step_f32`` — the
kernel's documented summation order in np.float32 — bit for bit, and
``step_f32`` lies within ``bound`` of the float64 step.  Cosine: the codewords
lie within ``bound`` (norm-wise, multiples of 2^-24 only) of the float64 step.
Every sample is planted (``check_plan``: the float64 argmin of every row is
its planned cluster by a clear gap), so no row is left out of a comparison.
tests/test_kmeans_host.py shows on the CPU that this acceptance rejects a
step that drops or repeats one row, moves a slice boundary, reads a codebook
one row early or forgets the codeword itself.

The largest error / bound of every case goes to kmeans_parity.json in the
suite's output folder (``OUT`` of tests/test_gpu_fullsize.py).
"""

from __future__ import annotations

import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from fenix_amd import _lib
from fenix_amd.engine import Engine, Shard
from fenix_amd.io import coder
from oracle import coder as OC
from oracle import oracle as O
from tests import kmeans_ref as R
from tests.test_gpu_fullsize import OUT

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine.get(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def parity():
    """{case: {metric: largest error / bound}}, written when the module is done."""
    rec = {}
    yield rec
    worst = {m: max((c[m] for c in rec.values() if m in c), default=None) for m in R.METRICS}
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "kmeans_parity.json"), "w") as f:
        json.dump({"what": "largest |got - step_f64| / bound per case (L2, inner product: "
                           "got == step_f32 bit for bit)", "worst": worst, "cases": rec}, f,
                  indent=1)
        f.write("\n")


def _bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _step(eng, dt: R.Data, q: np.ndarray = None) -> np.ndarray:
    """One Engine.kmeans_step over the case's sample in its own type and form."""
    case = dt.case
    cw = torch.from_numpy((dt.q if q is None else q).copy()).to(eng.device)
    s = torch.from_numpy(dt.sample).to(eng.device)
    m = _lib.METRICS[dt.metric]
    if case.dtype == "qu8" and case.form == "shard":
        eng.kmeans_step(Shard(s.view(case.nb * case.bs, case.d), 0, dt.scale, dt.zp), cw, m)
    elif case.dtype == "qu8":
        eng.kmeans_step(s, cw, m, scale=dt.scale, zero_point=dt.zp)
    else:
        assert s.dtype == (torch.float16 if case.dtype == "f16" else torch.float32)
        eng.kmeans_step(s, cw, m)
    torch.cuda.synchronize()
    return cw.cpu().numpy()


def _accept(got, q, f32, f64, bnd, metric, members):
    """The acceptance of the module docstring; returns the largest error / bound."""
    assert np.all(np.isfinite(got))
    if metric == "cosine":
        r = R.ratio(got, f64, bnd, metric)
        print(f"cosine: {r:.3f} of the bound")
        assert r <= 1.0
        for j in range(q.shape[0]):  # an empty cluster's codeword: its normalised self
            empty = members[j] == 0
            assert np.all(R.error(got[j][empty], OC.normalize(q[j][empty]), metric)
                          <= bnd[j][empty])
        return r
    r = R.ratio(f32, f64, bnd, metric)
    print(f"{metric}: step_f32 at {r:.3f} of the bound")
    np.testing.assert_array_equal(_bits(got), _bits(f32))
    assert r <= 1.0
    for j in range(q.shape[0]):  # an empty cluster's codeword comes back untouched
        empty = members[j] == 0
        np.testing.assert_array_equal(_bits(got[j][empty]), _bits(q[j][empty]))
    return r


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_kmeans_step_matches_reference(eng, parity, case, metric):
    dt = R.data(case.name, metric)
    got = _step(eng, dt)
    members = [dt.members(j) for j in range(case.nb)]
    try:
        r = _accept(got, dt.q, dt.f32, dt.f64, dt.bound, metric, members)
    except AssertionError:
        parity.setdefault(case.name, {})[metric] = R.ratio(got, dt.f64, dt.bound, metric)
        raise
    parity.setdefault(case.name, {})[metric] = r
    if case.plan == "slice":
        assert members[0][0] == 0  # the plan's empty cluster was in the comparison


@pytest.mark.parametrize("metric", R.METRICS)
def test_each_codebook_alone_equals_its_slice(eng, metric):
    """nb = 3 (bs = 1025, d = 37: no group starts 16-byte aligned): codebook j
    through the single-codebook form equals slice j of the grouped step."""
    dt = R.data("nb3_bs1025_d37", metric)
    got = _step(eng, dt)
    for j in range(dt.case.nb):
        one = coder.update(torch.from_numpy(dt.q[j]), torch.from_numpy(dt.v[j]), metric).numpy()
        np.testing.assert_array_equal(_bits(one), _bits(got[j]), err_msg=f"codebook {j}")


@pytest.mark.parametrize("metric", R.METRICS)
def test_kmeans_step_repeats_bit_exactly(eng, metric):
    """update_kernel promises a fixed order of its sum: the same bits each time."""
    dt = R.data("slices_d64_bs2050", metric)
    first = _bits(_step(eng, dt))
    for _ in range(2):
        np.testing.assert_array_equal(_bits(_step(eng, dt)), first)


@pytest.mark.parametrize("metric", R.METRICS)
def test_zero_row_and_zero_codeword(eng, parity, metric):
    """The 1e-12 floor: an all-zero sample row and an all-zero codeword
    (R.floor_case states what the reference does with them).  The zero row is
    the one row outside check_plan; where its float64 assignment is a tie the
    result may follow either tied cluster, and is compared with the reference
    recomputed under that assignment.  No NaN, no inf."""
    q, v, a, tied = R.floor_case(metric)
    cw = torch.from_numpy(q.copy()).to(eng.device)
    eng.kmeans_step(torch.from_numpy(v).to(eng.device), cw, _lib.METRICS[metric])
    torch.cuda.synchronize()
    got = cw.cpu().numpy()
    assert np.all(np.isfinite(got))
    assert not got[0, R.FLOOR_ZERO_WORD].any()  # 0 / max(0, 1e-12): stays 0 under every metric
    failures = []
    for c in tied:
        a[0, R.FLOOR_ZERO_ROW] = c
        f64 = R.step_f64_planned(q, v, a, metric)
        f32 = None if metric == "cosine" else R.step_f32(q, v, a, metric)
        members = [np.bincount(a[0], minlength=q.shape[1])]
        try:
            r = _accept(got, q, f32, f64, R.bound(q, v, a, metric), metric, members)
        except AssertionError as e:
            failures.append(e)
            continue
        parity.setdefault("zero_row_zero_codeword", {})[metric] = r
        return
    raise failures[0]


# ---------------------------------------------------------------- refusals


def _unchanged(cw: torch.Tensor, cw0: torch.Tensor) -> bool:
    torch.cuda.synchronize()
    return torch.equal(cw.view(torch.int32), cw0.view(torch.int32))


@pytest.mark.parametrize("metric", R.METRICS)
def test_refusals_leave_the_codewords_alone(eng, metric):
    """Every refusal comes before normalize_kernel: the (unnormalised)
    codewords keep their bits, cosine included."""
    L = _lib.load()
    m = _lib.METRICS[metric]
    nb, ks, bs, d = 2, 4, 8, 16
    dev = eng.device

    def words(dd):
        return torch.from_numpy(3.0 * O.fill_normal(nb * ks, dd, seed=77).reshape(nb, ks, dd)
                                ).to(dev)

    def space(dd, rows=bs):
        return torch.empty(_lib.kmeans_workspace_bytes(nb, rows, dd, ks), dtype=torch.uint8,
                           device=dev)

    x = torch.from_numpy(O.fill_normal(nb * bs, d, seed=78)).to(dev)
    cw0 = words(d)
    cw, ws = cw0.clone(), space(d)
    # the control: the same call with nothing wrong moves the codewords
    assert L.fx_kmeans_step(x.data_ptr(), _lib.DTYPE_F32, nb, bs, d, cw.data_ptr(), ks, m,
                            ws.data_ptr(), ws.numel(), None) == 0
    assert not _unchanged(cw, cw0)
    cw = cw0.clone()
    # bs = 0
    assert L.fx_kmeans_step(x.data_ptr(), _lib.DTYPE_F32, nb, 0, d, cw.data_ptr(), ks, m,
                            ws.data_ptr(), ws.numel(), None) == EINVAL
    assert _unchanged(cw, cw0)
    # a workspace one byte short
    assert L.fx_kmeans_step(x.data_ptr(), _lib.DTYPE_F32, nb, bs, d, cw.data_ptr(), ks, m,
                            ws.data_ptr(), ws.numel() - 1, None) == EINVAL
    assert _unchanged(cw, cw0)
    # fx_kmeans_step_ex: rows that do not split into nb slices
    codes = torch.full((nb * bs + 1, d), 60, dtype=torch.uint8, device=dev)
    wsx = space(d, bs + 1)
    c = _lib.Corpus(codes.data_ptr(), _lib.DTYPE_QU8, nb * bs + 1, d, 0, 0.04, 56)
    assert L.fx_kmeans_step_ex(ctypes.byref(c), nb, cw.data_ptr(), ks, m, wsx.data_ptr(),
                               wsx.numel(), None) == EINVAL
    assert _unchanged(cw, cw0)
    # d above update_kernel's 16 x 1024 register slots
    big = 16385
    xb = torch.zeros((nb * bs, big), dtype=torch.float32, device=dev)
    cwb0 = words(big)
    cwb, wsb = cwb0.clone(), space(big)
    assert L.fx_kmeans_step(xb.data_ptr(), _lib.DTYPE_F32, nb, bs, big, cwb.data_ptr(), ks, m,
                            wsb.data_ptr(), wsb.numel(), None) == EUNSUPPORTED
    assert _unchanged(cwb, cwb0)


# ---------------------------------------------------------- fx_row_sqnorms

SQ_NS = [1, 3, 4, 5, 1001]  # four rows per block
SQ_DS = [1, 63, 64, 65, 1000, 16384]
BIG = 300.0  # 300^2 overflows f16, not the f32 sum


@pytest.fixture(scope="module")
def sq_pool():
    x = O.fill_normal(max(SQ_NS), max(SQ_DS), seed=79)
    x[1] = 0  # a row of zeros
    x[2] *= np.float32(BIG)  # squares beyond f16's range
    return x


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("d", SQ_DS)
def test_row_sqnorms_match_float64(eng, sq_pool, d, dtype):
    """rownorm_kernel mode 0: m = ceil(d / 64) fmas per lane and 6 butterfly
    adds of non-negative terms, so |got - ref| <= (m + 6) u sum(v^2)."""
    for n in SQ_NS:
        x = np.ascontiguousarray(sq_pool[:n, :d]).astype(dtype)
        v = x.astype(np.float64)
        ref = (v * v).sum(1)
        assert np.all(np.isfinite(v))
        if n >= 3:
            assert ref[1] == 0
            assert d == 1 or (v[2] ** 2).max() > 65504  # past f16's largest finite value
        got = eng.row_sqnorms(torch.from_numpy(x).to(eng.device))
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (n,)
        got = got.cpu().numpy().astype(np.float64)
        bnd = (math.ceil(d / 64) + 6) * R.U * ref
        assert np.all(np.abs(got - ref) <= bnd), (n, d, np.abs(got - ref).max())


def test_row_sqnorms_no_rows_and_quint8(eng):
    L = _lib.load()
    d = 64
    x = torch.ones((4, d), dtype=torch.float32, device=eng.device)
    out = torch.full((4,), 12345.0, dtype=torch.float32, device=eng.device)
    assert L.fx_row_sqnorms(x.data_ptr(), _lib.DTYPE_F32, 0, d, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.all(out == 12345.0)  # n = 0: nothing is launched
    codes = torch.zeros((4, d), dtype=torch.uint8, device=eng.device)
    assert L.fx_row_sqnorms(codes.data_ptr(), _lib.DTYPE_QU8, 4, d, out.data_ptr(),
                            None) == EINVAL
    torch.cuda.synchronize()
    assert torch.all(out == 12345.0)
    with pytest.raises(TypeError):
        eng.row_sqnorms(codes)
    # the control: the same buffers, float32, four rows
    assert L.fx_row_sqnorms(x.data_ptr(), _lib.DTYPE_F32, 4, d, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.all(out == float(d))
