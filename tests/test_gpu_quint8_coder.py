"""The coded index over quint8 tensor columns (fx_code_assign_ex /
fx_kmeans_step_ex, FX_DTYPE_QU8): rows are read as their 1-byte codes and
dequantised in the kernels, scale * (float)(code - zero_point) with one
rounding, so every result must equal, bit for bit, the float32 entry points
over the dequantised rows.  Then the CPU oracle (oracle/coder.py), a seeded
``coder.make`` / ``index.make`` against the float32 column of the same rows,
and the probe search end to end over Flight.

Shapes are the smallest that cross the assign kernel's seams: the 128-row
tile (n = 1, 127, 128, 129, 300), the 32-wide K chunk and the 4-code vector
load (d = 16, 32, 36, 100; 37 takes the scalar loads and has padding up to
d4 = 40; a base pointer 1 byte off 4-B alignment takes them with d % 4 == 0),
codebook segments below and above 32 lanes (ks = 8, 37, 64, 100) and two
256-slot tiles ((nb, ks) = (3, 100): 384 slots)."""

from __future__ import annotations

import socket

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest
import torch

import fenix_amd
from fenix_amd import _lib
from fenix_amd.engine import Engine, Shard, device_mask
from fenix_amd.ex.arrow import quint8 as Q
from fenix_amd.io import coder, index, table
from oracle import coder as OC
from oracle import oracle as O
from tests.parity import check_topk
from tests.test_gpu_coder import _assign_ok

pytestmark = pytest.mark.gpu

METRICS = ["l2", "inner_product", "cosine"]
NS = [1, 127, 128, 129, 300]
DS = [16, 32, 36, 100, 37]
CODINGS = [(2, 8), (2, 37), (1, 64), (3, 100)]
MAPS = [(0.04, 56), (1e-3, 0), (7.5, 127)]


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine.get(torch.device("cuda", 0))


def _deq(codes: torch.Tensor, scale: float, zp: int) -> torch.Tensor:
    """QUInt8NDArray.dequantize in f32 on the device: f32(scale) * (code - zp)."""
    s = torch.tensor(scale, dtype=torch.float32, device=codes.device)
    return (s * (codes.to(torch.float32) - zp)).contiguous()


def _codewords(nb, ks, d, scale, seed):
    """Codewords on the scale of the dequantised rows (codes spread ~ +-60)."""
    return torch.from_numpy(O.fill_normal(nb * ks, d, seed=seed).reshape(nb, ks, d)
                            * np.float32(20.0 * scale))


def _same_assign(eng, codes, scale, zp, cw, m):
    got = eng.code_assign(codes, cw, m, index=True, code=True, dist=True, scale=scale,
                          zero_point=zp)
    ref = eng.code_assign(_deq(codes, scale, zp), cw, m, index=True, code=True, dist=True)
    assert torch.equal(got[0], ref[0]), "index"
    assert torch.equal(got[1], ref[1]), "code"
    assert torch.equal(got[2].view(torch.int32), ref[2].view(torch.int32)), "distance bits"
    return got


# ------------------------------------------------------------------ 1. assign


@pytest.fixture(scope="module")
def code_pool(eng):
    """Quantiser-range codes (0..127) for the widest case, drawn once."""
    rs = np.random.RandomState(91)
    return torch.from_numpy(rs.randint(0, 128, size=(max(NS), max(DS)), dtype=np.uint8)
                            ).to(eng.device)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nb,ks", CODINGS)
def test_assign_equals_f32_assign(eng, code_pool, metric, nb, ks):
    m = _lib.METRICS[metric]
    for d in DS:
        for scale, zp in MAPS:
            cw = _codewords(nb, ks, d, scale, seed=92 + d)
            for n in NS:
                codes = code_pool[:n, :d].contiguous()
                try:
                    _same_assign(eng, codes, scale, zp, cw, m)
                except AssertionError as e:
                    raise AssertionError(f"n={n} d={d} scale={scale} zp={zp}: {e}") from None


@pytest.mark.parametrize("metric", METRICS)
def test_assign_unaligned_base_pointer(eng, metric):
    """d % 4 == 0 but the rows start 1 byte off 4-B alignment: scalar loads."""
    n, d, nb, ks = 300, 36, 2, 37
    rs = np.random.RandomState(93)
    buf = torch.from_numpy(rs.randint(0, 128, size=n * d + 8, dtype=np.uint8)).to(eng.device)
    codes = buf[1 : 1 + n * d].view(n, d)
    assert codes.data_ptr() % 4 == 1 and codes.is_contiguous()
    _same_assign(eng, codes, 0.04, 56, _codewords(nb, ks, d, 0.04, seed=94),
                 _lib.METRICS[metric])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [36, 37])
def test_assign_full_code_range(eng, metric, d):
    """Any uint8 code is valid, not only the quantiser's 0..127."""
    n, nb, ks = 300, 3, 100
    rs = np.random.RandomState(95)
    codes = torch.from_numpy(rs.randint(0, 256, size=(n, d), dtype=np.uint8)).to(eng.device)
    assert int(codes.max()) > 127
    _same_assign(eng, codes, 0.04, 56, _codewords(nb, ks, d, 0.04, seed=96),
                 _lib.METRICS[metric])


def test_plain_entry_points_refuse_quint8(eng):
    """fx_code_assign / fx_kmeans_step carry no map: FX_DTYPE_QU8 stays FX_EINVAL."""
    n, d, nb, ks = 16, 16, 1, 4
    x = torch.zeros((n, d), dtype=torch.uint8, device=eng.device)
    cw = torch.zeros((nb, ks, d), dtype=torch.float32, device=eng.device)
    ws = torch.empty(_lib.code_assign_workspace_bytes(n, d, nb, ks), dtype=torch.uint8,
                     device=eng.device)
    oc = torch.empty(n, dtype=torch.int64, device=eng.device)
    L = _lib.load()
    assert L.fx_code_assign(x.data_ptr(), _lib.DTYPE_QU8, n, d, cw.data_ptr(), nb, ks,
                            _lib.METRIC_L2, ws.data_ptr(), ws.numel(), None, oc.data_ptr(),
                            None, None) == -1
    ws = torch.empty(_lib.kmeans_workspace_bytes(nb, n, d, ks), dtype=torch.uint8,
                     device=eng.device)
    assert L.fx_kmeans_step(x.data_ptr(), _lib.DTYPE_QU8, nb, n, d, cw.data_ptr(), ks,
                            _lib.METRIC_L2, ws.data_ptr(), ws.numel(), None) == -1


# ----------------------------------------------------------------- 2. k-means


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("bs", [129, 1100])  # 1100: two 1024-entry slices in update_kernel
@pytest.mark.parametrize("d", [32, 37])
def test_kmeans_step_equals_f32_step(eng, metric, nb, bs, d):
    ks, scale, zp = 8, 0.04, 56
    rs = np.random.RandomState(97)
    codes = torch.from_numpy(rs.randint(0, 128, size=(nb, bs, d), dtype=np.uint8)).to(eng.device)
    cw0 = _codewords(nb, ks, d, scale, seed=98).to(eng.device)
    m = _lib.METRICS[metric]
    got, ref = cw0.clone(), cw0.clone()
    eng.kmeans_step(codes, got, m, scale=scale, zero_point=zp)
    eng.kmeans_step(_deq(codes, scale, zp), ref, m)
    assert not torch.equal(ref, cw0)  # the step moved the codewords
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    # a Shard brings its map
    again = cw0.clone()
    eng.kmeans_step(Shard(codes.view(nb * bs, d), 0, scale, zp), again, m)
    assert torch.equal(again, got)


# ------------------------------------------------------------------ 3. oracle


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nb,ks,d", [(2, 37, 37), (3, 100, 36)])
def test_assign_matches_oracle(eng, metric, nb, ks, d):
    n = 3000
    a = Q.from_numpy(O.fill_normal(n, d, seed=101, cluster=100))
    scale, zp = float(a.type.scale), int(a.type.shift)
    x = O.dequantize(a.codes(), scale, zp)
    cw = O.fill_normal(nb * ks, d, seed=102).reshape(nb, ks, d)
    shard = Shard(torch.from_numpy(a.codes().copy()).to(eng.device), 0, scale, zp)
    idx, code, dist = eng.code_assign(shard, torch.from_numpy(cw), _lib.METRICS[metric],
                                      index=True, code=True, dist=True)
    idx, code, dist = idx.cpu().numpy(), code.cpu().numpy(), dist.cpu().numpy()
    _assign_ok(x, cw, metric, idx, dist)
    expect = np.zeros(n, np.int64)
    for j in range(nb):
        expect = expect * ks + idx[:, j]
    np.testing.assert_array_equal(code, expect)


# ---------------------------------------------------- 4. coder.make, index.make

MAKE_N, MAKE_D = 20_000, 32
MAKE_CFG = {"codebook_size": 8, "num_codebooks": 2, "batch_size": 2560, "num_epochs": 2}


@pytest.fixture(scope="module")
def make_env(eng, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("q8coder"))
    a = Q.from_numpy(O.fill_normal(MAKE_N, MAKE_D, seed=103, cluster=200))
    deq = O.dequantize(a.codes(), a.type.scale, a.type.shift)
    ids = pa.array(np.arange(MAKE_N, dtype=np.int64))
    table.make(root, "m/q8", pa.table({"id": ids, "vector": a}).to_reader(max_chunksize=1000))
    f = pa.FixedSizeListArray.from_arrays(pa.array(deq.ravel()), MAKE_D)
    table.make(root, "m/f32", pa.table({"id": ids, "vector": f}).to_reader(max_chunksize=1000))
    return dict(root=root, type=a.type, x=deq)


@pytest.mark.parametrize("metric", ["l2", "cosine", "dot"])
def test_seeded_make_equals_f32_make(make_env, metric):
    root = make_env["root"]
    cfg = {"metric": metric, **MAKE_CFG}
    np.random.seed(7)
    cq = coder.make(root, f"q8/{metric}", "m/q8", "vector", cfg)
    np.random.seed(7)
    cf = coder.make(root, f"f32/{metric}", "m/f32", "vector", cfg)
    assert cq["tensor"].dtype == torch.float32
    assert torch.equal(cq["tensor"].view(torch.int32), cf["tensor"].view(torch.int32))
    # the coding file keeps the extension type with its parameters
    t = coder.load(root, f"q8/{metric}")["column"]
    assert Q.is_quint8(t) and t == make_env["type"]
    assert (t.shape, t.scale, t.shift) == (make_env["type"].shape, make_env["type"].scale,
                                           make_env["type"].shift)
    # index.make over a copy of the float coding under the quint8 table's name
    iq = index.make(root, f"q8/{metric}", "m/q8", "vector")
    jf = index.make(root, f"f32/{metric}", "m/f32", "vector")
    got = iq.column(index.CODE_COL).to_numpy()
    np.testing.assert_array_equal(got, jf.column(index.CODE_COL).to_numpy())
    assert len(np.unique(got)) > 8  # both codebooks are in use
    # coder.call on the quint8 array: its codes under its own map
    col = table.load(root, "m/q8").column("vector")
    via_call = coder.call(col, cq, 1)
    np.testing.assert_array_equal(np.array([v[0] for v in via_call.to_pylist()]), got)
    # ... and a float target stays float: the same rows dequantised, the same codes
    np.testing.assert_array_equal(coder.call(make_env["x"], cq, 1)[:, 0], got)


# ------------------------------------------------------------------ 5. Flight

FL_N, FL_D = 20_000, 64
FL_CFG = {"codebook_size": 8, "num_codebooks": 2, "batch_size": 2560, "num_epochs": 2}


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def fl_env(eng, tmp_path_factory):
    r = str(tmp_path_factory.mktemp("q8index"))
    port = _port()
    server = fenix_amd.Server(r, host="127.0.0.1", port=port)
    flight = fenix_amd.Flight(host="127.0.0.1", port=port)
    parts = {}
    # "a" and "b" are quantised on their own: two scales (b's rows are 3x wider)
    for name, seed, mul in (("a", 111, 1.0), ("b", 112, 3.0)):
        arr = Q.from_numpy(O.fill_normal(FL_N, FL_D, seed=seed, cluster=500) * np.float32(mul))
        base = 0 if name == "a" else FL_N
        src = pa.table({"id": pa.array(np.arange(base, base + FL_N, dtype=np.int64)),
                        "vector": arr})
        flight.make_table(f"q/{name}", src.to_reader(max_chunksize=1000))
        parts[name] = dict(codes=arr.codes().copy(), type=arr.type, source=src,
                           x=O.dequantize(arr.codes(), arr.type.scale, arr.type.shift))
    assert parts["a"]["type"].scale != parts["b"]["type"].scale
    yield dict(root=r, flight=flight, eng=eng, **parts)
    server.shutdown()


def _check_probe_search(env, names, coding, metric, result, target, k, extra=None,
                        select=None):
    """result == the exact top-k over the rows whose stored code is in the
    oracle's probe set: Engine.search bits, then the f64 oracle's rows."""
    eng = env["eng"]
    code = coder.load(env["root"], coding)
    probe = OC.call(target[None], code["tensor"].numpy(), code["config"]["metric"], 16)[0]
    src = [f"q/{n}" for n in names] if len(names) > 1 else f"q/{names[0]}"
    stored = index.load(env["root"], coding, src, "vector").column("__CODED_ID__").to_numpy()
    mask = np.isin(stored, probe)
    if extra is not None:
        mask &= extra
    x = np.concatenate([env[n]["x"] for n in names])
    ids = result.column("id").to_numpy()
    assert result.num_rows == k
    if select is None or "__CODED_ID__" in select:
        assert np.all(np.isin(result.column("__CODED_ID__").to_numpy(), probe))
    # the same code shards, the host-built mask
    shards, masks, base = [], [], 0
    for n in names:
        t = env[n]["type"]
        c = torch.from_numpy(env[n]["codes"]).to(eng.device)
        shards.append(Shard(c, base, float(t.scale), int(t.shift)))
        masks.append(device_mask(mask[base : base + c.shape[0]], eng.device))
        base += c.shape[0]
    q = torch.from_numpy(target[None].astype(np.float32))
    gd, gr = eng.search(shards, q, _lib.METRICS[metric], k, masks=masks)
    np.testing.assert_array_equal(ids, gr.cpu().numpy()[0])
    np.testing.assert_array_equal(result.column("__DISTANCE__").to_numpy().view(np.uint32),
                                  gd.cpu().numpy()[0].view(np.uint32))
    od, orow = O.knn(x, target[None], metric, k, mask=mask)
    check_topk(result.column("__DISTANCE__").to_numpy()[None], ids[None], od, orow, x,
               target[None], metric)


@pytest.mark.parametrize("metric", ["l2", "cosine", "dot"])
def test_flight_index_and_probe_search(fl_env, metric):
    flight = fl_env["flight"]
    coding = f"q8/{metric}"
    flight.make_index(name=coding, source="q/a", column="vector",
                      config={"metric": metric, **FL_CFG})
    t = flight.read_table("q/a", coding, "vector").read_all()
    src = fl_env["a"]["source"]
    assert t.schema == pa.schema([*src.schema, pa.field("__CODED_ID__", pa.int64())])
    assert t.drop(["__CODED_ID__"]) == src
    # every stored code is the composite argmin of the dequantised row
    code = coder.load(fl_env["root"], coding)
    ref = OC.call(fl_env["a"]["x"], code["tensor"].numpy(), metric, 1)[:, 0]
    assert (t.column("__CODED_ID__").to_numpy() != ref).mean() < 1e-3
    # sync_index rewrites the same codes
    flight.sync_index(coding, "q/a", "vector")
    again = flight.read_table("q/a", coding, "vector").read_all()
    assert again.column("__CODED_ID__") == t.column("__CODED_ID__")

    target = O.fill_normal(1, FL_D, seed=113)[0]
    result = flight.search(target=target, source="q/a", column="vector", metric=metric,
                           coding=coding, maxval=10, probes=16)
    assert result.schema == pa.schema([*src.schema, pa.field("__CODED_ID__", pa.int64()),
                                       pa.field("__DISTANCE__", pa.float32())])
    _check_probe_search(fl_env, ["a"], coding, metric, result, target, 10)


def test_flight_probe_search_filter_and_select(fl_env):
    flight = fl_env["flight"]
    coding = "q8/fs"
    flight.make_index(name=coding, source="q/a", column="vector",
                      config={"metric": "l2", **FL_CFG})
    target = O.fill_normal(1, FL_D, seed=114)[0]
    select = ["id", "__CODED_ID__"]
    result = flight.search(target=target, source="q/a", column="vector", metric="l2",
                           coding=coding, select=select, filter=pc.field("id") >= 8_000,
                           maxval=10, probes=16)
    assert result.schema == pa.schema({"id": pa.int64(), "__CODED_ID__": pa.int64(),
                                       "__DISTANCE__": pa.float32()})
    _check_probe_search(fl_env, ["a"], coding, "l2", result, target, 10,
                        extra=np.arange(FL_N) >= 8_000, select=select)


def test_flight_two_sources_with_different_scales(fl_env):
    """Joined sources whose quint8 maps differ: coder.make trains through the
    f32 step over per-shard dequantised gathers, index.make encodes each
    source's shards under that source's own map."""
    flight = fl_env["flight"]
    coding = "q8/two"
    names = ["q/a", "q/b"]
    flight.make_index(name=coding, source=names, column="vector",
                      config={"metric": "l2", **FL_CFG})
    code = coder.load(fl_env["root"], coding)
    for n in ("a", "b"):
        stored = index.load(fl_env["root"], coding, f"q/{n}", "vector") \
            .column("__CODED_ID__").to_numpy()
        ref = OC.call(fl_env[n]["x"], code["tensor"].numpy(), "l2", 1)[:, 0]
        assert (stored != ref).mean() < 1e-3
    target = O.fill_normal(1, FL_D, seed=115)[0] * np.float32(2.0)
    result = flight.search(target=target, source=names, column="vector", metric="l2",
                           coding=coding, select=["id", "__CODED_ID__"], maxval=10, probes=16)
    _check_probe_search(fl_env, ["a", "b"], coding, "l2", result, target, 10,
                        select=["id", "__CODED_ID__"])


# ------------------------------------------------------------- 6. dtype check


def test_coded_index_rejects_other_dtypes(eng):
    x = torch.zeros((8, 16), dtype=torch.int32, device=eng.device)
    cw = torch.zeros((1, 4, 16), dtype=torch.float32, device=eng.device)
    with pytest.raises(TypeError):
        eng.code_assign(x, cw, _lib.METRIC_L2)
    with pytest.raises(TypeError):
        eng.kmeans_step(x.view(1, 8, 16), cw, _lib.METRIC_L2)
