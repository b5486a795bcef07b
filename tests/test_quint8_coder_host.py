"""Host side of the coded index over quint8 tensor columns (CPU, library
stubbed): the coding file keeps the extension type with its parameters, and
``coder.call`` hands a quint8 array to the engine as its codes plus its own
map while float targets stay float (queries are never coded)."""

from __future__ import annotations

import os

import numpy as np
import pyarrow as pa
import pytest
import torch

from fenix_amd import _lib, engine
from fenix_amd.ex.arrow import quint8 as Q
from fenix_amd.io import coder

D = 12


def _array(n=7, seed=3, mul=1.0):
    rs = np.random.RandomState(seed)
    return Q.from_numpy((mul * rs.randn(n, D)).astype(np.float32))


def test_coding_file_round_trips_the_quint8_type(tmp_path):
    t = Q.QUInt8TensorType((3, 4), 0.0375, 61)
    path = coder._path(str(tmp_path), "c/q8")
    os.makedirs(os.path.dirname(path))
    cfg = {"metric": "l2", "codebook_size": 4, "num_codebooks": 2, "batch_size": 8,
           "num_epochs": 1}
    tensor = torch.arange(2 * 4 * D, dtype=torch.float32).reshape(2, 4, D)
    with open(path, "wb") as f:
        torch.save({"tensor": tensor, "column": coder._type_bytes(t), "config": cfg}, f)
    with open(path, "rb") as f:  # what load() does: no arbitrary unpickling
        raw = torch.load(f, map_location="cpu", weights_only=True)
    assert isinstance(raw["column"], bytes)
    got = coder.load(str(tmp_path), "c/q8")
    col = got["column"]
    assert isinstance(col, Q.QUInt8TensorType)
    assert (col.shape, col.scale, col.shift) == ((3, 4), 0.0375, 61)
    assert col.storage_type == pa.list_(pa.uint8(), D)
    assert torch.equal(got["tensor"], tensor) and got["config"] == cfg
    # load() registered the UDF on the extension type: it takes a quint8 array
    import pyarrow.compute as pc

    fn = pc.get_function("c/q8")
    assert fn.arity == 2


def test_target_rows_quint8_array_yields_codes_and_its_map():
    a = _array()
    rows, qmap = coder.target_rows(a, a.type)
    assert rows.dtype == torch.uint8 and tuple(rows.shape) == (7, D)
    np.testing.assert_array_equal(rows.numpy(), a.codes())
    assert qmap == (float(a.type.scale), int(a.type.shift))
    # chunked, sliced (offset-aware), and as the coding's column of a table
    sl = a.slice(2, 4)
    rows2, qmap2 = coder.target_rows(pa.chunked_array([a.slice(0, 2), sl]), a.type)
    np.testing.assert_array_equal(rows2.numpy(), a.codes()[:6])
    assert qmap2 == qmap
    t = pa.table({"id": pa.array(np.arange(7)), "vector": a})
    rows3, qmap3 = coder.target_rows(t, a.type)
    np.testing.assert_array_equal(rows3.numpy(), a.codes())
    assert qmap3 == qmap


def test_target_rows_uses_the_targets_own_map():
    """The coding's column type names the column; the codes are read under the
    map of the array that holds them."""
    a, b = _array(seed=3), _array(seed=4, mul=5.0)
    assert a.type.scale != b.type.scale
    _, qmap = coder.target_rows(b, a.type)
    assert qmap == (float(b.type.scale), int(b.type.shift))


def test_target_rows_float_targets_stay_float():
    x = np.random.RandomState(5).randn(4, D).astype(np.float32)
    for target in (x, torch.from_numpy(x),
                   pa.FixedSizeListArray.from_arrays(pa.array(x.ravel()), D)):
        rows, qmap = coder.target_rows(target, pa.list_(pa.float32(), D))
        assert qmap is None and rows.dtype == torch.float32
        np.testing.assert_array_equal(rows.numpy().reshape(4, D), x)
    with pytest.raises(KeyError):
        coder.target_rows(pa.table({"id": pa.array([1])}), pa.list_(pa.float32(), D))


class _FakeEngine:
    """Engine.code_assign over numpy: records what it was handed."""

    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def code_assign(self, x, codewords, metric, index=False, code=True, dist=False,
                    scale=1.0, zero_point=0):
        self.calls.append((x.dtype, scale, zero_point))
        v = x.to(torch.float32)
        if x.dtype == torch.uint8:
            v = torch.tensor(scale, dtype=torch.float32) * (v - zero_point)
        nb, ks, _ = codewords.shape
        d2 = torch.cdist(v[None].double(), codewords.double()).permute(1, 0, 2)  # [n, nb, ks]
        idx = d2.argmin(dim=2)
        out = torch.zeros(v.shape[0], dtype=torch.int64)
        for j in range(nb):
            out = out * ks + idx[:, j]
        return None, out, None


def test_call_codes_a_quint8_array_and_leaves_floats_float(monkeypatch):
    fake = _FakeEngine()
    monkeypatch.setattr(engine.Engine, "get", classmethod(lambda cls, dev=None: fake))
    a = _array(n=9)
    deq = a.to_numpy().dequantize().reshape(9, D).astype(np.float32)
    cw = torch.from_numpy(np.random.RandomState(6).randn(2, 4, D).astype(np.float32))
    coding = {"tensor": cw, "column": a.type,
              "config": {"metric": "l2", "codebook_size": 4, "num_codebooks": 2,
                         "batch_size": 1, "num_epochs": 1}}
    got = coder.call(a, coding, 1)
    assert got.type == pa.list_(pa.int64()) and len(got) == 9
    assert fake.calls == [(torch.uint8, float(a.type.scale), int(a.type.shift))]
    same = coder.call(deq, coding, 1)  # ndarray in, ndarray out, float rows
    assert isinstance(same, np.ndarray)
    assert fake.calls[1] == (torch.float32, 1.0, 0)
    np.testing.assert_array_equal(same[:, 0], [v[0] for v in got.to_pylist()])


def test_engine_rows_reject_other_dtypes():
    rows = engine.Engine._code_rows
    x = torch.zeros((4, 8), dtype=torch.uint8)
    assert rows(x, 0.5, 3)[0] is x and rows(x, 0.5, 3)[1:] == (_lib.DTYPE_QU8, 0.5, 3)
    s = engine.Shard(x, 100, 0.25, 7)  # a Shard brings its own map
    assert rows(s, 1.0, 0)[0] is x and rows(s, 1.0, 0)[1:] == (_lib.DTYPE_QU8, 0.25, 7)
    assert rows(x.float(), 9.0, 9)[1:] == (_lib.DTYPE_F32, 1.0, 0)
    assert rows(x.half(), 9.0, 9)[1:] == (_lib.DTYPE_F16, 1.0, 0)
    for bad in (torch.int32, torch.int8, torch.float64, torch.bfloat16):
        with pytest.raises(TypeError):
            rows(torch.zeros((4, 8), dtype=bad), 1.0, 0)
