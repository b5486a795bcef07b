"""fx_pred_eval (csrc/knn_pred.hip) and the device filter path of io.index.call.

The kernel's bitmap must equal, word for word, both pyarrow's evaluation of
the expression (io.index._filter_mask, the host path it replaces) and the
numpy interpreter of the same program (io.predicate.evaluate_host); end to
end, every search must return the table the host path returns."""

from __future__ import annotations

import ctypes

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest
import torch

import fenix_amd.io.table
from fenix_amd import _lib, engine
from fenix_amd.engine import Engine, PredColumn
from fenix_amd.io import coder, index
from fenix_amd.io import predicate as P
from oracle import oracle as O

pytestmark = pytest.mark.gpu

f = pc.field
SIZES = (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 100_003)
ROW0 = (0, 1, 31, 33)
ROWS = max(SIZES) + max(ROW0)
POISON = -0x21524111  # 0xDEADBEEF as int32
BIG = 2**53


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine.get(torch.device("cuda", 0))


def _nulls(rng, values, type):
    return pa.array(values, type=type, mask=rng.random(len(values)) < 0.1)


def _kernel_table() -> pa.Table:
    rng = np.random.default_rng(11)
    cols = {}
    for name, t, np_t in (("i8", pa.int8(), np.int8), ("i16", pa.int16(), np.int16),
                          ("i32", pa.int32(), np.int32), ("u8", pa.uint8(), np.uint8),
                          ("u16", pa.uint16(), np.uint16), ("u32", pa.uint32(), np.uint32)):
        info = np.iinfo(np_t)
        v = rng.integers(max(info.min, -40), min(info.max, 40) + 1, ROWS).astype(np_t)
        v[:2] = [info.min, info.max]
        cols[name] = _nulls(rng, v, t)
    v = (BIG + 1 + rng.integers(-3, 4, ROWS)).astype(np.int64)
    v[::2] *= -1
    cols["i64"] = _nulls(rng, v, pa.int64())
    cols["key"] = pa.array(rng.integers(0, 10_000, ROWS).astype(np.int64))  # no nulls
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 0.1, 0.5, 1e-320])
    x = np.where(rng.random(ROWS) < 0.5, rng.choice(special, ROWS), rng.normal(size=ROWS))
    cols["f64"] = _nulls(rng, x, pa.float64())
    cols["f32"] = _nulls(rng, x.astype(np.float32), pa.float32())
    cols["g32"] = pa.array(x.astype(np.float32)[::-1].copy())  # no nulls
    words = np.array(["", "a", "b", "it's", 'q"', "zz"], dtype=object)
    cols["s"] = _nulls(rng, rng.choice(words, ROWS), pa.string())
    cols["ds"] = pa.array(rng.choice(words, ROWS)).dictionary_encode()  # no nulls
    return pa.table(cols)


def _cap_expression():
    e = f("i32") > -100  # 16 leaves + 15 ands + 1 invert = the 32-instruction cap
    for i in range(15):
        e = e & (f("i16") != i) if i % 2 else e & (f("i32") != i)
    return ~e


EXPRESSIONS = {
    "ints": ((f("i8") > 0) | (f("i16") <= 3)) & ~((f("i32") == 2) | (f("u8") >= 30))
    | (f("u16") < 5) & (f("u32") != 7) & (f("i64") > BIG + 1) | (f("i64") <= -(BIG + 2)),
    "floats": (f("f32") == 0.1) | (f("f64") < 0.0) & ~(f("g32") >= -0.0)
    | (f("f64") != float("nan")) & f("f32").is_null(nan_is_null=True)
    | f("g32").is_null(nan_is_null=True) | (f("f64") == float(np.float32(0.1))),
    "no_validity": (f("key") < 5000) & (f("g32") > 0.25) | (f("ds") == "zz"),
    "strings": (f("s") == "it's") | ~f("ds").isin(["a", "nope", 'q"']) & (f("s") != "nope")
    | f("s").is_null() & f("i8").is_valid(),
    "set_1": ~f("i32").isin([3]) & (f("u8") > 10),
    "set_2": f("i64").isin([BIG + 2, -(BIG + 1)]) | f("u8").isin([1, 39]),
    "set_4096": f("key").isin(list(range(1, 8192, 2))) & ~f("i16").isin([0, 1, 2]),
    "cap": _cap_expression(),
}


class Staged:
    """The table's columns on the device, each expression's program, and the
    two references over all ROWS rows, computed once and left unchanged."""

    def __init__(self, device) -> None:
        self.table = _kernel_table()
        self.cols, self.prog, self.want = {}, {}, {}
        for name, expr in EXPRESSIONS.items():
            prog, why = P.explain(expr, self.table.schema)
            assert prog is not None, (name, why)
            host = P.host_columns(prog, self.table)
            want = index._filter_mask(self.table, expr)
            assert np.array_equal(P.evaluate_host(prog, host), want), name
            assert 0.02 * ROWS < want.sum() < 0.98 * ROWS, (name, want.sum())
            for c, (values, valid, dictionary) in zip(prog.columns, host):
                if c.name not in self.cols:
                    signed = {"u": "i"}.get(values.dtype.kind, values.dtype.kind)
                    self.cols[c.name] = PredColumn(
                        torch.from_numpy(values.view(f"{signed}{values.dtype.itemsize}")).to(device),
                        None if valid is None else torch.from_numpy(
                            P.pack_validity(valid).view(np.int32)).to(device),
                        dictionary, c.dtype)
            self.prog[name], self.want[name] = prog, want
        assert len(self.prog["cap"].instructions) == P.MAX_OPS
        assert self.cols["key"].valid is None and self.cols["i32"].valid is not None

    def columns(self, name):
        return [self.cols[c.name] for c in self.prog[name].columns]


@pytest.fixture(scope="module")
def staged(eng):
    return Staged(eng.device)


def test_limits_match_the_compiler(eng):
    assert _lib.pred_limits() == {"columns": P.MAX_COLUMNS, "ops": P.MAX_OPS, "set": P.MAX_SET,
                                  "pool": P.MAX_POOL}
    assert ctypes.sizeof(_lib.PredOp) == P.OP_DTYPE.itemsize == 24
    assert ctypes.sizeof(_lib.PredColumn) == 24


@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_host_path(eng, staged, n):
    rng = np.random.default_rng(n)
    for name in EXPRESSIONS:
        for row0 in ROW0:
            want = staged.want[name][row0 : row0 + n]
            keep = rng.random(n) < 0.7
            am = engine.device_mask(keep, eng.device)
            for and_mask, ref in ((None, want), (am, want & keep)):
                mk, cnt = eng.pred_eval(staged.prog[name], staged.columns(name), n, row0, and_mask)
                got = mk.cpu().numpy().view(np.uint32)
                assert got.shape == ((n + 31) // 32,)
                assert np.array_equal(got, engine.bitmap(ref)), (name, row0, and_mask is not None)
                assert int(cnt.item()) == int(ref.sum()), (name, row0)


def _raw_eval(eng, cols, ops, pool, n, row0=0, ncols=None, nops=None):
    """fx_pred_eval into ceil(n/32) + 2 poisoned words and a poisoned count."""
    words = (n + 31) // 32
    out = torch.full((words + 2,), POISON, dtype=torch.int32, device=eng.device)
    cnt = torch.full((1,), POISON, dtype=torch.int64, device=eng.device)
    carr = (_lib.PredColumn * max(1, len(cols)))(
        *[_lib.PredColumn(c.values.data_ptr(), c.valid.data_ptr() if c.valid is not None else None,
                          c.dtype, 0) for c in cols])
    ops = np.ascontiguousarray(ops)
    pool = np.ascontiguousarray(pool, dtype=np.int64)
    rc = _lib.load().fx_pred_eval(
        carr, len(cols) if ncols is None else ncols,
        ops.ctypes.data_as(ctypes.POINTER(_lib.PredOp)), len(ops) if nops is None else nops,
        pool.ctypes.data if pool.size else None, n, row0, None, out.data_ptr(), cnt.data_ptr(),
        torch.cuda.current_stream(eng.device).cuda_stream)
    torch.cuda.synchronize(eng.device)
    return rc, out.cpu().numpy(), int(cnt.item())


def _ops(*rows):
    ops = np.zeros(len(rows), dtype=P.OP_DTYPE)
    for i, r in enumerate(rows):
        for k, v in r.items():
            ops[i][k] = v
    return ops


def test_output_words_and_tail_bits(eng, staged):
    prog = staged.prog["set_2"]
    ops, pool = prog.encode([c.dictionary for c in staged.columns("set_2")])
    for n in (1, 33, 2049):
        rc, out, cnt = _raw_eval(eng, staged.columns("set_2"), ops, pool, n, row0=33)
        words = (n + 31) // 32
        assert rc == 0
        assert np.all(out[words:] == POISON)  # nothing past ceil(n/32) words
        want = staged.want["set_2"][33 : 33 + n]
        assert np.array_equal(out[:words].view(np.uint32), engine.bitmap(want))  # tail bits zero
        assert cnt == want.sum()


def test_refusals_leave_the_output_untouched(eng, staged):
    i32, f32 = staged.cols["i32"], staged.cols["f32"]
    leaf = {"op": P.GT, "column": 0, "imm": 1}
    isin = {"op": P.IS_IN, "column": 0, "set_offset": 0, "set_length": 3}
    bad_dtype = PredColumn(i32.values, None, None, 9)
    cases = {
        "stack underflow": ([i32], _ops({"op": P.AND}), []),
        "underflow behind a leaf": ([i32], _ops(leaf, {"op": P.OR}), []),
        "final depth 2": ([i32], _ops(leaf, leaf), []),
        "column index": ([i32], _ops({**leaf, "column": 1}), []),
        "negative column": ([i32], _ops({**leaf, "column": -1}), []),
        "unknown instruction": ([i32], _ops({**leaf, "op": 12}), []),
        "unsorted set": ([i32], _ops(isin), [1, 3, 2]),
        "repeated set entry": ([i32], _ops(isin), [1, 2, 2]),
        "set past the pool": ([i32], _ops({**isin, "set_offset": P.MAX_POOL - 2}), [1, 2, 3]),
        "negative set offset": ([i32], _ops({**isin, "set_offset": -1}), [1, 2, 3]),
        "empty set": ([i32], _ops({**isin, "set_length": 0}), [1, 2, 3]),
        "set too long": ([i32], _ops({**isin, "set_length": P.MAX_SET + 1}),
                         np.arange(P.MAX_SET + 1)),
        "set without a pool": ([i32], _ops(isin), []),
        "is_in on floats": ([f32], _ops(isin), [1, 2, 3]),
        "is_null flag": ([f32], _ops({"op": P.IS_NULL, "column": 0, "imm": 2}), []),
        "dtype": ([bad_dtype], _ops(leaf), []),
    }
    for name, (cols, ops, pool) in cases.items():
        rc, out, cnt = _raw_eval(eng, cols, ops, pool, 100)
        assert rc == -1, name
        assert _lib.load().fx_last_error().startswith(b"fx_pred_eval"), name
        assert np.all(out == POISON) and cnt == POISON, name
    nine = [i32] * 9
    for name, kw in {"no instructions": dict(nops=0), "33 instructions": dict(nops=33),
                     "nine columns": dict(ncols=9)}.items():
        cols = nine if name == "nine columns" else [i32]
        rc, out, cnt = _raw_eval(eng, cols, _ops(*[leaf] * 33), [], 100, **kw)
        assert rc == -1 and np.all(out == POISON) and cnt == POISON, name
    with pytest.raises(ValueError):  # Engine.pred_eval: a column shorter than row0 + n
        eng.pred_eval(staged.prog["set_1"], staged.columns("set_1"), ROWS, 1)


def test_repeats_are_identical(eng, staged):
    n, row0 = 100_003, 31
    runs = [eng.pred_eval(staged.prog["strings"], staged.columns("strings"), n, row0)
            for _ in range(3)]
    first = runs[0][0].cpu().numpy()
    for mk, cnt in runs[1:]:
        assert np.array_equal(mk.cpu().numpy(), first)
        assert int(cnt.item()) == int(runs[0][1].item())


# -------------------------------------------------------------- end to end --
N, D = 20_000, 32


def _source(seed: int) -> pa.Table:
    rng = np.random.default_rng(seed)
    x = O.fill_normal(N, D, seed=71)
    vec = pa.FixedSizeListArray.from_arrays(pa.array(x.ravel()), list_size=D)
    return pa.table({
        "id": pa.array(np.arange(N, dtype=np.int64)),
        "a": _nulls(rng, rng.integers(0, 100, N).astype(np.int32), pa.int32()),
        "x": _nulls(rng, rng.normal(size=N).astype(np.float32), pa.float32()),
        "s": _nulls(rng, rng.choice(np.array(["red", "green", "blue"], dtype=object), N),
                    pa.string()),
        "vector": vec,
    })


FILTERS = {
    "compare": f("a") > 90,
    "compare_and_set": (f("a") > 30) & f("a").isin([31, 47, 50, 99]) | (f("x") < -1.5),
    "string": (f("s") == "green") & ~(f("x") >= 0.0),
    "nulls": f("s").is_null() | f("a").is_null() & f("x").is_valid(),
}
UNSUPPORTED = (f("a") + 1) > 91


@pytest.fixture(scope="module")
def root(eng, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("pred"))
    fenix_amd.io.table.make(root, "p/src", _source(5).to_reader(max_chunksize=1000))
    np.random.seed(72)
    coder.make(root, "p/l2", "p/src", "vector",
               {"metric": "l2", "codebook_size": 16, "num_codebooks": 2, "batch_size": 256,
                "num_epochs": 1})
    index.make(root, "p/l2", "p/src", "vector")
    return root


def _calls(root, flt):
    target = O.fill_normal(1, D, seed=73)[0]
    return [
        lambda: index.call(root, None, "p/src", "vector", target=target, metric="l2",
                           filter=flt, maxval=10),
        lambda: index.call(root, None, "p/src", "vector", target=target, metric="l2",
                           select=["id", "a", "s"], filter=flt, maxval=None),
        lambda: index.call(root, "p/l2", "p/src", "vector", target=target, filter=flt,
                           maxval=10, probes=64, select=["id", "x"]),
    ]


def _check_end_to_end(root, monkeypatch):
    with _lib.options(device_filter_min_rows=0):
        for name, flt in FILTERS.items():
            for i, call in enumerate(_calls(root, flt)):
                before = index.filter_stats()
                got = call()
                after = index.filter_stats()
                # through the kernel, not through the fallback
                assert after["device"] == before["device"] + 1, (name, i, after)
                assert after["host"] == before["host"], (name, i, after)
                monkeypatch.setenv("FENIX_AMD_DEVICE_FILTER", "0")
                want = call()
                monkeypatch.delenv("FENIX_AMD_DEVICE_FILTER")
                off = index.filter_stats()
                assert off["device"] == after["device"] and off["host"] == after["host"] + 1
                assert off["reasons"].get("switched off", 0) >= 1
                assert got.equals(want), (name, i)
                assert got.num_rows > 0, (name, i)
        for i, call in enumerate(_calls(root, UNSUPPORTED)):
            before = index.filter_stats()
            got = call()
            after = index.filter_stats()
            assert after["device"] == before["device"] and after["host"] == before["host"] + 1
            reason = [k for k in after["reasons"]
                      if after["reasons"][k] != before["reasons"].get(k, 0)]
            assert len(reason) == 1 and reason[0].startswith("expression: "), reason
            monkeypatch.setenv("FENIX_AMD_DEVICE_FILTER", "0")
            want = call()
            monkeypatch.delenv("FENIX_AMD_DEVICE_FILTER")
            assert got.equals(want), i


def test_end_to_end_equals_the_host_path(root, monkeypatch):
    _check_end_to_end(root, monkeypatch)


def test_end_to_end_sharded_in_two(root, monkeypatch):
    """Two shards on one device: the second starts at source row 10 000, which
    is not a multiple of 32, and reads the full staged columns from there."""
    from fenix_amd.distributed import shard_rows

    monkeypatch.setenv("FENIX_AMD_DEVICES", "0,0")
    assert shard_rows(N, 2, 1)[0] % 32 != 0
    _check_end_to_end(root, monkeypatch)


def test_min_rows_option_keeps_small_tables_on_the_host(root):
    target = O.fill_normal(1, D, seed=73)[0]
    with _lib.options(device_filter_min_rows=N + 1):
        before = index.filter_stats()
        index.call(root, None, "p/src", "vector", target=target, metric="l2",
                   filter=FILTERS["compare"], maxval=10)
        after = index.filter_stats()
    assert after["host"] == before["host"] + 1 and after["device"] == before["device"]
    assert after["reasons"]["below device_filter_min_rows"] == \
        before["reasons"].get("below device_filter_min_rows", 0) + 1


def test_rewritten_source_is_restaged(eng, tmp_path, monkeypatch):
    root = str(tmp_path)
    target = O.fill_normal(1, D, seed=73)[0]
    flt = (f("a") > 90) & (f("s") == "red")

    def call():
        return index.call(root, None, "r/src", "vector", target=target, metric="l2",
                          select=["id", "a", "s"], filter=flt, maxval=None)

    results = []
    with _lib.options(device_filter_min_rows=0):
        for seed in (5, 6):
            fenix_amd.io.table.make(root, "r/src", _source(seed).to_reader(max_chunksize=1000))
            before = index.filter_stats()["device"]
            got = call()
            assert index.filter_stats()["device"] == before + 1
            monkeypatch.setenv("FENIX_AMD_DEVICE_FILTER", "0")
            assert got.equals(call())
            monkeypatch.delenv("FENIX_AMD_DEVICE_FILTER")
            results.append(got)
    assert not results[0].column("id").equals(results[1].column("id"))
