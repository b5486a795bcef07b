"""The GPU-free parts of the many-target search (io.index.call_many,
Flight.search_many): target normalisation, the assembly of the result table
and the descriptor."""

from __future__ import annotations

import pickle

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest
import torch

from fenix_amd import flight
from fenix_amd.ex.arrow import quint8 as Q
from fenix_amd.io import index

D = 8


def _rows(nq, seed=0):
    return np.random.RandomState(seed).randn(nq, D).astype(np.float32)


def test_targets_of_every_accepted_type_equal_the_single_target_rows():
    t = pa.list_(pa.float32(), D)
    x = _rows(5)
    fsl = pa.FixedSizeListArray.from_arrays(pa.array(x.ravel()), D)
    f64 = pa.FixedSizeListArray.from_arrays(pa.array(x.ravel().astype(np.float64)), D)
    var = pa.array([r.tolist() for r in x], type=pa.list_(pa.float32()))
    for targets in (x, torch.from_numpy(x), fsl, pa.chunked_array([fsl[:2], fsl[2:]]),
                    x.astype(np.float64), f64, var):
        got = index._targets_values(targets, t)
        assert got.dtype == np.float32 and got.shape == (5, D) and got.flags.writeable
        for i in range(5):
            np.testing.assert_array_equal(got[i], index._target_values(x[i], t)[0])
    assert index._targets_values(x[:1], t).shape == (1, D)


def test_targets_are_cast_to_float16_like_a_single_target():
    t16 = pa.list_(pa.float16(), D)
    x = _rows(4, seed=1) / 3
    fsl16 = pa.FixedSizeListArray.from_arrays(pa.array(x.ravel().astype(np.float16)), D)
    for targets in (x, x.astype(np.float64), fsl16):
        got = index._targets_values(targets, t16)
        want = np.concatenate([index._target_values(r, t16) for r in x])
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, x.astype(np.float16).astype(np.float32))
    assert not np.array_equal(index._targets_values(x, t16), x)


def test_quint8_columns_take_float_rows():
    a = Q.from_numpy(_rows(3, seed=2))
    x = _rows(4, seed=3)
    fsl = pa.FixedSizeListArray.from_arrays(pa.array(x.ravel()), D)
    for targets in (x, fsl, x.astype(np.float64)):
        np.testing.assert_array_equal(index._targets_values(targets, a.type), x)
    with pytest.raises(pa.ArrowInvalid):
        index._targets_values(np.zeros((2, D + 1), np.float32), a.type)


def test_a_wrong_length_or_shape_is_refused():
    t = pa.list_(pa.float32(), D)
    with pytest.raises(pa.ArrowInvalid):
        index._targets_values(np.zeros((3, D + 1), np.float32), t)
    with pytest.raises(pa.ArrowInvalid):
        index._targets_values(np.zeros((3, D - 1), np.float64), pa.list_(pa.float16(), D))
    with pytest.raises(pa.ArrowInvalid):
        short = pa.FixedSizeListArray.from_arrays(pa.array(np.zeros(6, np.float32)), 3)
        index._targets_values(short, t)
    with pytest.raises(ValueError):
        index._targets_values(np.zeros(D, np.float32), t)  # one target: use call
    with pytest.raises(ValueError):
        index._targets_values(np.zeros((0, D), np.float32), t)
    with pytest.raises(TypeError):
        index._targets_values(pa.array(np.zeros(D, np.float32)), t)
    with pytest.raises(TypeError):
        index._targets_values([[0.0] * D], t)


def test_result_assembly_drops_the_empty_slots_and_numbers_the_targets():
    nan = np.float32(np.nan)
    dist = np.array([[0.5, 1.5, 2.5], [0.25, nan, nan], [nan, nan, nan], [3.0, 4.0, nan]],
                    dtype=np.float32)
    rows = np.array([[7, 2, 9], [4, -1, -1], [-1, -1, -1], [0, 7, -1]], dtype=np.int64)
    d, r, tidx, keep = index._flatten_many(dist, rows)
    np.testing.assert_array_equal(r, [7, 2, 9, 4, 0, 7])
    np.testing.assert_array_equal(d, np.array([0.5, 1.5, 2.5, 0.25, 3.0, 4.0], np.float32))
    np.testing.assert_array_equal(tidx, [0, 0, 0, 1, 3, 3])
    assert tidx.dtype == np.int32 and keep.shape == rows.shape and keep.sum() == 6
    # the columns are taken once for all targets, then the two columns appended
    data = pa.table({"id": pa.array(np.arange(10, dtype=np.int64) * 10),
                     "tag": pa.array([f"t{i}" for i in range(10)])})
    taken = index.take_rows(data, r)
    t = pa.list_(pa.float32(), D)
    out = index._many_table(taken, d, tidx, t, ["tag", "id", index.DIST_COL, index.TARGET_COL])
    assert out.column_names == ["tag", "id", "__DISTANCE__", "__TARGET__"]
    assert out.schema.field("__TARGET__").type == pa.int32()
    assert out.schema.field("__DISTANCE__").type == pa.float32()
    assert out.column("id").to_pylist() == [70, 20, 90, 40, 0, 70]
    assert out.column("__TARGET__").to_pylist() == [0, 0, 0, 1, 3, 3]
    assert all(c.num_chunks == 1 for c in out.columns)
    # float16 columns: the distance takes the column's value type
    out16 = index._many_table(taken, d, tidx, pa.list_(pa.float16(), D),
                              ["id", index.DIST_COL, index.TARGET_COL])
    assert out16.schema.field("__DISTANCE__").type == pa.float16()
    # no target kept a row
    d0, r0, t0, _ = index._flatten_many(dist[2:3], rows[2:3])
    empty = index._many_table(index.take_rows(data, r0), d0, t0, t,
                              ["id", index.DIST_COL, index.TARGET_COL])
    assert empty.num_rows == 0 and empty.column_names == ["id", "__DISTANCE__", "__TARGET__"]


def test_the_descriptor_gains_one_key_only_for_many():
    expr = pc.field("id") > 3
    args = ("c", ["a", "b"], "vector", "l2", ["id"], expr, 10, 4)
    one = flight.search_command(*args)
    assert list(one) == ["coding", "source", "column", "metric", "select", "filter", "maxval",
                         "probes"]
    assert "many" not in one and pickle.loads(one["filter"]).equals(expr)
    many = flight.search_command(*args, many=True)
    assert many.pop("many") is True and many == one
    # the client sends one list per target
    x = _rows(3)
    col = flight.target_rows(x)
    assert col.type == pa.list_(pa.float32(), D) and len(col) == 3
    np.testing.assert_array_equal(col.flatten().to_numpy(), x.ravel())
    assert flight.target_rows(torch.from_numpy(x)).equals(col)
    assert flight.target_rows(col) is col
    with pytest.raises(ValueError):
        flight.target_rows(x[0])


def test_maxval_is_required():
    data = pa.table({"vector": pa.FixedSizeListArray.from_arrays(pa.array(_rows(4).ravel()), D)})
    for bad in (None, 0, -3):
        with pytest.raises(ValueError, match="maxval"):
            index.call_many("/nonexistent", None, data, "vector", _rows(2), metric="l2",
                            maxval=bad)
