"""io.predicate on the CPU: which expressions compile, which are refused and
by what, and the numpy interpreter of the program against pyarrow's own
evaluation (io.index._filter_mask, the host path of index.py:161)."""

import datetime
import pickle

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from fenix_amd.io import predicate as P
from fenix_amd.io.index import _filter_mask

f = pc.field

SCHEMA = pa.schema([
    ("a", pa.int32()), ("b", pa.int64()), ("c", pa.int8()), ("x", pa.float64()),
    ("y", pa.float32()), ("s", pa.string()), ("u", pa.uint64()), ("t", pa.timestamp("us")),
    ("flag", pa.bool_()), ("a > 3", pa.int64()), ("and", pa.int64()), ('q"r', pa.int64()),
    ("p(r", pa.int64()),
] + [(f"k{i}", pa.int16()) for i in range(9)])


def _deep(depth: int) -> pc.Expression:
    e = f("a") > 0
    for i in range(depth):
        e = ~(e & (f("b") < i)) if i % 2 else (e | (f("x") >= float(i)))
    return e


ACCEPTED = {
    "eq": f("a") == 1, "ne": f("a") != -5, "lt": f("a") < 3, "le": f("a") <= 3,
    "gt": f("a") > 30, "ge": f("a") >= 3,
    "and": (f("a") > 30) & f("b").isin([1, 2, 3]),
    "or": (f("a") > 30) | (f("b") == 2),
    "invert": ~(f("a") == 1),
    "literal_left": pc.scalar(3) < f("a"),
    "literal_left_eq": pc.scalar(2.5) == f("x"),
    "negative": f("b") > -(2**62),
    "exponent": f("x") < -1.5e-7,
    "big_exponent": f("x") == 1e22,
    "float_integral": f("x") == 1.0,
    "nan": f("x") == float("nan"),
    "inf": f("x") > -float("inf"),
    "f32_column": f("y") == 0.1,
    "quotes": f("s") == 'it\'s "q" \\ x',
    "operator_in_string": f("s") != "a > 3 == 1",
    "paren_in_string": f("s") == ") or (",
    "unicode": f("s") == "日本",
    "string_set": f("s").isin(["a", "b'c", 'd"e']),
    "is_null": f("a").is_null(),
    "is_null_nan": f("x").is_null(nan_is_null=True),
    "is_valid": f("s").is_valid(),
    "depth5": _deep(5),
    "set_1": f("c").isin([7]),
    "set_unsorted_dupes": f("a").isin([3, 1, 2, 1]),
    "set_4096": f("b").isin(list(range(0, 8192, 2))),
    "eight_columns": (f("k0") > 0) & (f("k1") > 0) & (f("k2") > 0) & (f("k3") > 0)
    & (f("k4") > 0) & (f("k5") > 0) & (f("k6") > 0) & (f("k7") > 0),
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_accepted(name):
    expr = ACCEPTED[name]
    prog, why = P.explain(expr, SCHEMA)
    assert prog is not None, why
    again = pickle.loads(pickle.dumps(expr))
    assert prog.rebuilt.equals(again) and again.equals(prog.rebuilt)
    assert P.compile(again, SCHEMA).instructions == prog.instructions or name == "nan"
    ops, pool = prog.encode([pa.array(["a", "b"]) if c.kind == "string" else None
                             for c in prog.columns])
    assert ops.dtype == P.OP_DTYPE and len(ops) <= P.MAX_OPS and pool.dtype == np.int64
    assert len(prog.columns) <= P.MAX_COLUMNS
    for op in ops[ops["op"] == P.IS_IN]:
        s = pool[op["set_offset"] : op["set_offset"] + op["set_length"]]
        assert len(s) >= 1 and np.all(np.diff(s) > 0)


def test_accepted_shapes():
    p = P.compile(ACCEPTED["set_4096"], SCHEMA)
    assert p.encode()[1].size == 4096
    p = P.compile(ACCEPTED["literal_left"], SCHEMA)
    assert p.instructions == ((P.GT, 0, 3),)  # 3 < a  ==  a > 3
    p = P.compile(ACCEPTED["and"], SCHEMA)
    assert [c.name for c in p.columns] == ["a", "b"]
    assert [i[0] for i in p.instructions] == [P.GT, P.IS_IN, P.AND]
    # a literal absent from the dictionary: a code no row has
    p = P.compile(f("s") == "zzz", SCHEMA)
    assert p.encode([pa.array(["a", "b"])])[0]["imm"][0] == -1
    assert P.compile(f("s") == "b", SCHEMA).encode([pa.array(["a", "b"])])[0]["imm"][0] == 1


def _cap_program():
    e = f("a") > 0
    for i in range(15):  # 16 leaves + 15 operators + 1 invert = 32 instructions
        e = e & (f("a") != i)
    return ~e


def test_instruction_cap():
    assert len(P.compile(_cap_program(), SCHEMA).instructions) == 32
    assert P.compile(~_cap_program(), SCHEMA) is None


REFUSED = {
    "int8_literal": f("a") >= pa.scalar(3, pa.int8()),
    "uint16_literal": f("a") == pa.scalar(3, pa.uint16()),
    "float32_literal": f("x") < pa.scalar(0.5, pa.float32()),
    "int32_value_set": f("a").isin(pa.array([1, 2], pa.int32())),
    "field_field": f("a") > f("b"),
    "add_checked": (f("a") + 1) > 2,
    "cast": f("a").cast(pa.int64()) > 2,
    "timestamp": f("t") > datetime.datetime(2020, 1, 1),
    "timestamp_on_int": f("b") > datetime.datetime(2020, 1, 1),
    "ambiguous_name": f("a > 3") == 1,
    "field_named_and": f("and") == 1,
    "field_with_quote": f('q"r') == 1,
    "field_with_paren": f("p(r") == 1,
    "set_4097": f("b").isin(list(range(4097))),
    "nine_columns": (f("k0") > 0) & (f("k1") > 0) & (f("k2") > 0) & (f("k3") > 0)
    & (f("k4") > 0) & (f("k5") > 0) & (f("k6") > 0) & (f("k7") > 0) & (f("k8") > 0),
    "empty_set": f("a").isin([]),
    "float_literal_on_int": f("a") > 1.5,
    "int_literal_on_float": f("x") > 1,
    "uint64": f("u") > 3,
    "bare_bool": f("flag"),
    "bool_literal": f("a") == True,  # noqa: E712
    "null_in_set": f("a").isin([1, None]),
    "skip_nulls_set": pc.is_in(f("a"), options=pc.SetLookupOptions(value_set=pa.array([1, 2]),
                                                                    skip_nulls=True)),
    "float_set": f("x").isin([1.0, 2.0]),
    "string_ordered": f("s") < "m",
    "nested_ref": pc.field("a", "b") == 1,
    "non_kleene_and": pc.Expression._call("and", [f("a") > 1, f("b") > 2]),
    "unknown_column": f("nope") == 1,
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused(name):
    prog, why = P.explain(REFUSED[name], SCHEMA)
    assert prog is None and why, name
    assert P.compile(pickle.loads(pickle.dumps(REFUSED[name])), SCHEMA) is None


@pytest.mark.parametrize("name", ["ambiguous_name", "int8_literal", "uint16_literal",
                                  "float32_literal", "int32_value_set"])
def test_refused_by_the_equals_check(name, monkeypatch):
    """These parse (the field named ``a > 3`` as ``a > <literal 1>``, the typed
    literals as Python's): only rebuilt.equals(expr) stands between them and
    a wrong program."""
    seen = []
    real = P._verified

    def spy(rebuilt, expr):
        seen.append(real(rebuilt, expr))
        return seen[-1]

    monkeypatch.setattr(P, "_verified", spy)
    assert P.compile(REFUSED[name], SCHEMA) is None
    assert seen == [False]
    # and with the check disabled the parse does produce a (wrong) program
    monkeypatch.setattr(P, "_verified", lambda rebuilt, expr: True)
    assert P.compile(REFUSED[name], SCHEMA) is not None


def test_serialised_literals_layout():
    """The literal values come from the record batch behind the expression's
    pickle support.  If a pyarrow release changes that layout every filter
    would quietly keep the host path: this fails instead."""
    e = (f("a") > 30) & f("b").isin([3, 1, 2]) | f("x").is_null(nan_is_null=True) \
        & (pc.scalar(2.5) <= f("x")) & f("s").is_valid() & (f("s") == "q")
    cols = P._serialised_columns(e)
    assert [len(c) for c in cols] == [1] * 5
    assert cols[0].type == pa.int64() and cols[0][0].as_py() == 30
    assert pa.types.is_struct(cols[1].type)
    assert cols[1][0]["value_set"].as_py() == [3, 1, 2]
    assert cols[1].type.field("value_set").type == pa.list_(pa.int64())
    assert cols[2][0]["nan_is_null"].as_py() is True
    assert cols[3].type == pa.float64() and cols[3][0].as_py() == 2.5
    assert cols[4].type == pa.string() and cols[4][0].as_py() == "q"
    prog, why = P.explain(e, SCHEMA)
    assert prog is not None and why == ""
    # no accepted or refused case may end in the catch-all: a refusal is the
    # grammar's or the equals check's, never an exception inside the compiler
    for name, expr in {**ACCEPTED, **REFUSED}.items():
        assert not P.explain(expr, SCHEMA)[1].startswith("error:"), name


# ---------------------------------------------------------- interpreter --
N = 1000
BIG = 2**53


def _with_nulls(rng, values, type):
    return pa.array(values, type=type, mask=rng.random(len(values)) < 0.1)


def _table() -> pa.Table:
    rng = np.random.default_rng(7)
    cols = {}
    for name, t, np_t in (("i8", pa.int8(), np.int8), ("i16", pa.int16(), np.int16),
                          ("i32", pa.int32(), np.int32), ("u8", pa.uint8(), np.uint8),
                          ("u16", pa.uint16(), np.uint16), ("u32", pa.uint32(), np.uint32)):
        info = np.iinfo(np_t)
        v = rng.integers(max(info.min, -40), min(info.max, 40) + 1, N).astype(np_t)
        v[:4] = [info.min, info.max, 0, 3]
        cols[name] = _with_nulls(rng, v, t)
    # int64 around 2^53 + 1: a double compare cannot tell these apart
    v = (BIG + 1 + rng.integers(-3, 4, N)).astype(np.int64)
    v[N // 2:] *= -1
    cols["i64"] = _with_nulls(rng, v, pa.int64())
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 0.1, 0.5, 1e-320])
    x = np.where(rng.random(N) < 0.5, rng.choice(special, N), rng.normal(size=N))
    cols["f64"] = _with_nulls(rng, x, pa.float64())
    cols["f32"] = _with_nulls(rng, x.astype(np.float32), pa.float32())
    cols["f32_nonull"] = pa.array(x.astype(np.float32)[::-1].copy(), type=pa.float32())
    words = np.array(["", "a", "b", "it's", 'q"', "日本", "zz"], dtype=object)
    s = rng.choice(words, N)
    cols["s"] = _with_nulls(rng, s, pa.string())
    cols["ls"] = _with_nulls(rng, s[::-1].copy(), pa.large_string())
    cols["ds"] = _with_nulls(rng, rng.choice(words, N), pa.string()).dictionary_encode()
    return pa.table(cols)


TABLE = _table()

INTERPRETED = {
    **{f"{c}_{op}": getattr(f(c), op)(3) for c in ("i8", "i16", "i32", "u8", "u16", "u32")
       for op in ("__eq__", "__ne__", "__lt__", "__le__", "__gt__", "__ge__")},
    "i8_beyond_range": f("i8") < 1000,
    "u32_negative": f("u32") > -1,
    "i64_above": f("i64") > BIG + 1, "i64_eq": f("i64") == BIG + 1, "i64_le": f("i64") <= BIG + 2,
    "i64_below": f("i64") < -(BIG + 1), "i64_ne": f("i64") != -(BIG + 1),
    "i64_set": f("i64").isin([BIG, BIG + 2, -(BIG + 1)]),
    "f32_tenth": f("f32") == 0.1, "f32_tenth_ne": f("f32") != 0.1, "f32_tenth_le": f("f32") <= 0.1,
    "f32_exact_tenth": f("f32") == float(np.float32(0.1)),
    "f64_tenth": f("f64") == 0.1,
    "f64_nan_eq": f("f64") == float("nan"), "f64_nan_ne": f("f64") != float("nan"),
    "f64_nan_lt": f("f64") < float("nan"), "f64_nan_ge": f("f64") >= float("nan"),
    "zero": f("f64") == 0.0, "neg_zero": f("f32") >= -0.0, "zero_lt": f("f64") < 0.0,
    "inf": f("f32_nonull") < float("inf"), "denormal": f("f64") >= 1e-320,
    "is_null": f("f64").is_null(), "is_null_nan": f("f64").is_null(nan_is_null=True),
    "is_null_nan_f32": f("f32_nonull").is_null(nan_is_null=True),
    "is_null_nan_int": f("i32").is_null(nan_is_null=True), "is_valid": f("s").is_valid(),
    "s_eq": f("s") == "it's", "s_ne": f("s") != 'q"', "s_missing": f("s") == "nope",
    "s_missing_ne": f("s") != "nope", "s_empty": f("s") == "",
    "s_set": f("s").isin(["a", "nope", "日本"]), "s_set_missing": f("s").isin(["x", "y"]),
    "ls_eq": f("ls") == "b", "ds_eq": f("ds") == "zz", "ds_set": ~f("ds").isin(["a", "b"]),
    "set_not": ~f("i32").isin([1, 2, 3]),
    "set_null_or": f("i32").isin([5]) | (f("i16") > 0),
    "kleene_or": (f("i32") > 0) | (f("i16") > 0),
    "kleene_and": (f("i32") > 0) & (f("i16") > 0),
    "kleene_not": ~(f("i32") > 0),
    "kleene_mix": ~((f("i32") > 0) & ~(f("f64") < 0.5)) | (f("s") == "a") & f("u8").is_valid(),
    "literal_left": pc.scalar(3) < f("i16"),
    "depth": ~(~(~(((f("i8") > 0) | (f("f32") < 0.0)) & (f("s") != "a")) | f("i64").isin([BIG]))
               & (f("u16") <= 20)),
}


@pytest.mark.parametrize("name", sorted(INTERPRETED))
def test_interpreter_equals_pyarrow(name):
    expr = INTERPRETED[name]
    prog, why = P.explain(expr, TABLE.schema)
    assert prog is not None, why
    got = P.evaluate_host(prog, P.host_columns(prog, TABLE))
    want = _filter_mask(TABLE, expr)
    assert got.dtype == bool and np.array_equal(got, want)
    assert 0 < want.sum() < N or name in ("f64_nan_eq", "f64_nan_lt", "f64_nan_ge", "s_missing",
                                          "s_set_missing", "i8_beyond_range", "u32_negative",
                                          "is_null_nan_int", "f32_tenth")


def test_kleene_truth_table():
    """null / true / false against each other, spelled out, through pyarrow and
    through the interpreter."""
    T, F_, U = 1, 0, None
    vals = [T, F_, U]
    p = pa.array([a for a in vals for _ in vals], type=pa.int8())
    q = pa.array([b for _ in vals for b in vals], type=pa.int8())
    t = pa.table({"p": p, "q": q})
    pe, qe = f("p") == 1, f("q") == 1
    #           TT TF TU FT FF FU UT UF UU   (kept rows: result true; null drops)
    table = {
        "and": (pe & qe, [1, 0, 0, 0, 0, 0, 0, 0, 0]),
        "or": (pe | qe, [1, 1, 1, 1, 0, 0, 1, 0, 0]),
        "not_p": (~pe, [0, 0, 0, 1, 1, 1, 0, 0, 0]),
        # not (p and q): known false and anything is false, so its negation keeps
        "not_and": (~(pe & qe), [0, 1, 0, 1, 1, 1, 0, 1, 0]),
        "not_or": (~(pe | qe), [0, 0, 0, 0, 1, 0, 0, 0, 0]),
        "not_not": (~~pe, [1, 1, 1, 0, 0, 0, 0, 0, 0]),
    }
    for name, (expr, want) in table.items():
        prog = P.compile(expr, t.schema)
        got = P.evaluate_host(prog, P.host_columns(prog, t))
        assert got.tolist() == [bool(w) for w in want], name
        assert _filter_mask(t, expr).tolist() == got.tolist(), name


def _mismatch(expr) -> bool:
    prog = P.compile(expr, TABLE.schema)
    got = P.evaluate_host(prog, P.host_columns(prog, TABLE))
    return not np.array_equal(got, _filter_mask(TABLE, expr))


def test_teeth_is_in_of_null(monkeypatch):
    expr = ~f("i32").isin([1, 2, 3])
    assert not _mismatch(expr)
    monkeypatch.setattr(P, "_leaf_is_in", lambda x, s, valid: (np.isin(x, s) & valid,
                                                               valid.copy()))
    assert _mismatch(expr)


def test_teeth_non_kleene_or(monkeypatch):
    expr = (f("i32") > 0) | (f("i16") > 0)
    assert not _mismatch(expr)
    monkeypatch.setattr(P, "_or", lambda a, b: (a[0] | b[0], a[1] & b[1]))
    assert _mismatch(expr)


def test_teeth_invert_drops_known(monkeypatch):
    expr = ~(f("i32") > 0)
    assert not _mismatch(expr)
    monkeypatch.setattr(P, "_not", lambda a: (~a[0], np.ones_like(a[1])))
    assert _mismatch(expr)


def test_teeth_f32_compare(monkeypatch):
    expr = f("f32") == 0.1
    assert not _mismatch(expr)
    real = P._leaf_compare

    def narrow(op, x, lit, valid):
        if x.dtype.kind == "f":
            x, lit = x.astype(np.float32), np.float32(lit)
        return real(op, x, lit, valid)

    monkeypatch.setattr(P, "_leaf_compare", narrow)
    assert _mismatch(expr)


def test_pack_validity():
    v = np.array([1, 0, 1] + [1] * 30 + [0], dtype=bool)
    w = P.pack_validity(v)
    assert w.dtype == np.uint32 and w.tolist() == [0xFFFFFFFD, 0x1]
