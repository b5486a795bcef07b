"""Host side of tests/test_gpu_kmeans.py (CPU): for every GPU case the
reference is consistent on its own (the plan is the float64 argmin by a clear
gap; the f32 restatement of update_kernel's sum lies within ``bound`` of the
float64 step), and the acceptance the GPU tests use — bit equality with
``step_f32`` for L2 and inner product, ``bound`` around ``step_f64`` for
cosine — rejects a step with one row dropped, one row added twice, the slice
boundary off by one, a codebook's rows read one row early, or the codeword
left out of its mean; by a factor of 4 or more for cosine."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from fenix_amd.engine import Engine
from tests import kmeans_ref as R

COS_MARGIN = 4.0


def _bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_reference_is_consistent(case, metric):
    dt = R.data(case.name, metric)
    gap = R.check_plan(dt.q, dt.v, dt.a, metric)
    assert gap >= 1e-3
    # the plan is the oracle's argmin, so the oracle's step is the planned mean
    np.testing.assert_array_equal(R.step_f64_planned(dt.q, dt.v, dt.a, metric), dt.f64)
    assert np.all(np.isfinite(dt.f64)) and np.all(np.isfinite(dt.bound))
    if metric == "cosine":
        assert dt.f32 is None
        np.testing.assert_allclose(np.linalg.norm(dt.f64, axis=-1), 1.0, rtol=0, atol=1e-12)
        assert dt.bound.shape == (case.nb, case.ks) and dt.bound.max() < 1e-3
        return
    r = R.ratio(dt.f32, dt.f64, dt.bound, metric)
    print(f"{case.name} {metric}: step_f32 at {r:.3f} of its bound, plan gap {gap:.3g}")
    assert r <= 1.0
    # an empty cluster's codeword is its input, bit for bit
    for j in range(case.nb):
        empty = dt.members(j) == 0
        np.testing.assert_array_equal(_bits(dt.f32[j][empty]), _bits(dt.q[j][empty]))


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_acceptance_rejects_a_wrong_step(case, metric):
    dt = R.data(case.name, metric)
    wrong = R.corruptions(dt)
    assert {"row_dropped", "row_twice", "include_self_forgotten"} <= set(wrong)
    assert ("boundary_row_skipped" in wrong) == (case.bs > R.SLICE)
    assert ("codebook_offset_minus_one" in wrong) == (case.nb > 1)
    for name, kw in wrong.items():
        if metric == "cosine":
            bad = R.step_f64_planned(dt.q, dt.v, metric=metric, **kw)
            r = R.ratio(bad, dt.f64, dt.bound, metric)
            assert r >= COS_MARGIN, f"{name}: only {r:.2f} of the bound"
        else:
            bad = R.step_f32(dt.q, dt.v, metric=metric, **kw)
            assert not np.array_equal(_bits(bad), _bits(dt.f32)), name


def test_uncorrupted_step_passes_its_own_acceptance():
    """The two restatements with no mistake in them are the references."""
    for name in ("slices_d37_bs2050", "nb3_bs1025_d37"):
        for metric in R.METRICS:
            dt = R.data(name, metric)
            if metric == "cosine":
                same = R.step_f64_planned(dt.q, dt.v, dt.a, metric)
                assert R.ratio(same, dt.f64, dt.bound, metric) == 0.0
            else:
                np.testing.assert_array_equal(_bits(R.step_f32(dt.q, dt.v, dt.a, metric)),
                                              _bits(dt.f32))


@pytest.mark.parametrize("bs", [1, 3, 1023, 1024, 1025, 2050])
def test_slice_plan_places_what_it_promises(bs):
    ks = 14
    a = R.slice_plan(ks, bs)
    assert a.shape == (bs,) and a.min() >= 0 and a.max() < ks
    assert not np.any(a == 0)  # the empty cluster
    per = np.stack([np.bincount(a[s:s + R.SLICE], minlength=ks)
                    for s in range(0, bs, R.SLICE)])
    if bs >= R.SLICE:
        # every total 0..5 (so every total % 4) occurs in the first slice
        assert set(range(6)) <= set(per[0].tolist())
    if bs > R.SLICE:
        assert per[:-1, 1].sum() == 0  # members in the last slice only ...
        assert np.array_equal(np.nonzero(a == 2)[0], [1023, 1024])  # ... and across a boundary
    if bs == 2050:
        assert per[-1, 1] == 2 and set(range(6)) <= set(per[1].tolist())
    assert per[:, 8:].max() <= 400  # the large clusters stay at a few hundred rows


@pytest.mark.parametrize("metric", R.METRICS)
def test_floor_case_reference(metric):
    """The zero row is the one row outside check_plan; its rule is the tie set."""
    q, v, a, tied = R.floor_case(metric)
    keep = np.arange(v.shape[1]) != R.FLOOR_ZERO_ROW
    R.check_plan(q, v[:, keep], a[:, keep], metric)
    assert tied == ([R.FLOOR_ZERO_WORD] if metric == "l2" else [0, 1, 2])
    ref = R.step_f64(q, v, metric)  # np.argmin takes the first of the tie
    np.testing.assert_array_equal(ref, R.step_f64_planned(q, v, a, metric))
    assert np.all(np.isfinite(ref)) and not ref[0, R.FLOOR_ZERO_WORD].any()
    bnd = R.bound(q, v, a, metric)
    assert np.all(np.isfinite(bnd)) and not np.any(bnd[0, R.FLOOR_ZERO_WORD])


def test_quantize_covers_the_range_with_a_nonzero_zero_point():
    dt = R.data("qu8_small_scale", "l2")
    assert dt.sample.dtype == np.uint8 and dt.zp != 0
    assert dt.sample.min() == 0 and dt.sample.max() == 255
    np.testing.assert_array_equal(
        dt.v, np.float32(dt.scale) * (dt.sample.astype(np.float32) - np.float32(dt.zp)))


def test_row_sqnorms_rejects_other_dtypes():
    """Engine.row_sqnorms used to hand every non-f32 tensor over as f16."""
    eng = Engine(torch.device("cpu"))
    for dtype in (torch.uint8, torch.int32, torch.float64, torch.bfloat16):
        with pytest.raises(TypeError):
            eng.row_sqnorms(torch.zeros((4, 8), dtype=dtype))
