"""Filter expressions as verified postfix programs (torch-free).

``io.index.call`` takes its row filter as a ``pc.Expression`` (index.py:161).
pyarrow offers no way to walk one, and its ``str()`` is ambiguous: a field
named ``a > 3`` compared with 1 prints ``(a > 3 == 1)``, ``(a > 3)`` prints the
same for an int8 and an int64 literal, and a value set of more than 20 entries
prints with an ellipsis.  So ``compile`` parses, and never trusts the parse:

1. ``str(expr)`` is parsed with a strict grammar for the *structure*: the
   operators, the field names (plain identifiers of the schema) and where the
   literals sit.  Literal text is skipped, not interpreted;
2. the literal *values* and value sets are read from the expression's own
   serialisation (the record batch behind its pickle support,
   ``Expression.__reduce__``), in the tree's order;
3. a ``pc.Expression`` is rebuilt from the AST through the public pyarrow API,
   with plain Python literals (so int64 / double / string), and the program is
   accepted only if ``rebuilt.equals(expr)``.  ``equals`` tells ``int8(3)``
   from ``int64(3)`` and an int32 value set from an int64 one, and survives a
   pickle round trip.

Anything else returns ``None`` and the caller keeps the host path: a misparse
can cost speed, never correctness.

The program is a postfix instruction list over (value, known) pairs
(``include/fenix_knn.h``, fx_pred_eval): leaf compares, set membership, null
tests, Kleene ``and`` / ``or`` and ``not``; an unknown result drops the row,
as ``_filter_mask``'s ``fill_null(False)`` does.  ``evaluate_host`` interprets
the same encoded program in numpy and pins its semantics without a GPU.
"""

from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

# the limits of fx_pred_eval (fx_pred_limits; tests/test_gpu_predicate.py compares)
MAX_COLUMNS = 8
MAX_OPS = 32
MAX_SET = 4096
MAX_POOL = 8192

# FX_PRED_* dtypes and instructions (include/fenix_knn.h)
I8, I16, I32, I64, U8, U16, U32, F32, F64 = range(9)
EQ, NE, LT, LE, GT, GE, IS_IN, IS_NULL, IS_VALID, AND, OR, NOT = range(12)

# struct fx_pred_op, as the C ABI takes it
OP_DTYPE = np.dtype([("op", "<i4"), ("column", "<i4"), ("imm", "<i8"), ("set_offset", "<i4"),
                     ("set_length", "<i4")])
assert OP_DTYPE.itemsize == 24

NP_DTYPES = {I8: np.int8, I16: np.int16, I32: np.int32, I64: np.int64, U8: np.uint8,
             U16: np.uint16, U32: np.uint32, F32: np.float32, F64: np.float64}

_COMPARE = {"==": EQ, "!=": NE, "<": LT, "<=": LE, ">": GT, ">=": GE}
_FLIP = {EQ: EQ, NE: NE, LT: GT, LE: GE, GT: LT, GE: LE}  # literal OP field -> field OP' literal
_IDENT = re.compile(r"[A-Za-z_][A-Za-z0-9_]*\Z")
_RESERVED = {"and", "or", "invert", "is_in", "is_null", "is_valid", "nan", "inf", "true", "false",
             "null"}
_CALLS = ("invert(", "is_in(", "is_null(", "is_valid(")
_SET_END = "\n], null_matching_behavior=MATCH})"


def _column_kind(t: pa.DataType) -> Optional[Tuple[str, int]]:
    """-> ("int" | "float" | "string", staged FX_PRED dtype) of a column type
    the kernel serves; string columns are staged as int32 dictionary codes."""
    ints = {pa.int8(): I8, pa.int16(): I16, pa.int32(): I32, pa.int64(): I64, pa.uint8(): U8,
            pa.uint16(): U16, pa.uint32(): U32}
    if t in ints:
        return "int", ints[t]
    if t == pa.float32():
        return "float", F32
    if t == pa.float64():
        return "float", F64
    if t in (pa.string(), pa.large_string()):
        return "string", I32
    if pa.types.is_dictionary(t) and t.value_type == pa.string():
        return "string", I32
    return None


@dataclass(frozen=True)
class Column:
    """One entry of a program's column table."""
    name: str    # source column
    kind: str    # "int", "float" or "string"
    dtype: int   # FX_PRED_* of the staged values (string: I32 codes)


@dataclass(frozen=True)
class Program:
    """Postfix instructions over ``columns``.  Each is a tuple: (EQ..GE, column,
    literal), (IS_IN, column, values), (IS_NULL, column, nan_is_null),
    (IS_VALID, column), (AND,), (OR,), (NOT,).  Literals of string columns stay
    strings here; ``encode`` translates them with a file version's dictionary."""
    columns: Tuple[Column, ...]
    instructions: Tuple[tuple, ...]
    rebuilt: pc.Expression

    def encode(self, dictionaries: Optional[Sequence[Optional[pa.Array]]] = None
               ) -> Tuple[np.ndarray, np.ndarray]:
        """-> (fx_pred_op records, sorted int64 set pool).  ``dictionaries``:
        per column, the distinct strings of a string column (None otherwise);
        a literal absent from it gets code -1, which no row has."""
        ops = np.zeros(len(self.instructions), dtype=OP_DTYPE)
        pool: List[np.ndarray] = []
        used = 0
        for i, ins in enumerate(self.instructions):
            ops[i]["op"] = ins[0]
            if ins[0] > IS_VALID:
                continue
            c = ins[1]
            col = self.columns[c]
            ops[i]["column"] = c
            if ins[0] <= GE:
                if col.kind == "float":
                    ops[i]["imm"] = np.array(ins[2], dtype=np.float64).view(np.int64)
                elif col.kind == "string":
                    ops[i]["imm"] = _codes(dictionaries[c], [ins[2]])[0]
                else:
                    ops[i]["imm"] = ins[2]
            elif ins[0] == IS_IN:
                vals = _codes(dictionaries[c], ins[2]) if col.kind == "string" else ins[2]
                s = np.unique(np.asarray(vals, dtype=np.int64))
                ops[i]["set_offset"], ops[i]["set_length"] = used, s.size
                pool.append(s)
                used += s.size
            elif ins[0] == IS_NULL:
                ops[i]["imm"] = int(ins[2])
        return ops, (np.concatenate(pool) if pool else np.zeros(0, dtype=np.int64))


def _codes(dictionary: pa.Array, literals: Sequence[str]) -> np.ndarray:
    got = pc.index_in(pa.array(literals, type=dictionary.type), value_set=dictionary)
    return got.fill_null(-1).to_numpy(zero_copy_only=False).astype(np.int64)


class _Refused(Exception):
    pass


class _Parser:
    """Recursive descent over ``str(expr)``.  AST nodes: ("and" | "or", l, r),
    ("not", e), ("cmp", op text, field, literal_left), ("in", field),
    ("null", field, nan_is_null), ("valid", field)."""

    def __init__(self, text: str, schema: pa.Schema) -> None:
        self.s, self.i, self.schema = text, 0, schema

    def expect(self, lit: str) -> None:
        if not self.s.startswith(lit, self.i):
            raise _Refused(f"expected {lit!r} at {self.i}")
        self.i += len(lit)

    def field(self, name: str) -> str:
        if not _IDENT.match(name) or name in _RESERVED:
            raise _Refused(f"not a plain field name: {name!r}")
        if self.schema.get_field_index(name) < 0:
            raise _Refused(f"no such column: {name!r}")
        return name

    def ident(self) -> str:
        m = re.compile(r"[A-Za-z_][A-Za-z0-9_]*").match(self.s, self.i)
        if m is None:
            raise _Refused(f"field name expected at {self.i}")
        self.i = m.end()
        return self.field(m.group())

    def parse(self):
        e = self.expr()
        if self.i != len(self.s):
            raise _Refused("trailing text")
        return e

    def expr(self):
        s = self.s
        if s.startswith("invert(", self.i):
            self.i += 7
            e = self.expr()
            self.expect(")")
            return ("not", e)
        if s.startswith("is_valid(", self.i):
            self.i += 9
            f = self.ident()
            self.expect(")")
            return ("valid", f)
        if s.startswith("is_null(", self.i):
            self.i += 8
            f = self.ident()
            self.expect(", {nan_is_null=")
            nan = s.startswith("true", self.i)
            self.expect("true" if nan else "false")
            self.expect("})")
            return ("null", f, nan)
        if s.startswith("is_in(", self.i):
            self.i += 6
            f = self.ident()
            self.expect(", {value_set=")
            m = re.compile(r"[a-z_0-9]+:\[\n").match(s, self.i)
            if m is None:
                raise _Refused("value set")
            end = s.find(_SET_END, m.end() - 1)
            if end < 0:
                raise _Refused("value set end")
            self.i = end + len(_SET_END)
            return ("in", f)
        self.expect("(")
        if s.startswith("(", self.i) or s.startswith(_CALLS, self.i):
            left = self.expr()
            kind = "and" if s.startswith(" and ", self.i) else "or"
            self.expect(f" {kind} ")
            right = self.expr()
            self.expect(")")
            return (kind, left, right)
        return self.compare()

    def compare(self):
        """``FIELD OP LITERAL)`` or ``LITERAL OP FIELD)``: split at the first
        operator outside a quoted string; the literal's text is opaque."""
        s, start = self.s, self.i
        j, quoted, split = start, False, None
        while j < len(s):
            ch = s[j]
            if quoted:
                if ch == "\\":
                    j += 1
                elif ch == '"':
                    quoted = False
            elif ch == '"':
                quoted = True
            elif ch == "(":
                raise _Refused("nested call in a comparison")
            elif ch == ")":
                break
            elif split is None and ch == " ":
                m = re.compile(r" (==|!=|<=|>=|<|>) ").match(s, j)
                if m is not None:
                    split = (j, m.end(), m.group(1))
                    j = m.end() - 1
            j += 1
        if j >= len(s) or split is None:
            raise _Refused("comparison")
        left, right = s[start : split[0]], s[split[1] : j]
        self.i = j + 1
        if not left or not right:
            raise _Refused("comparison operand")
        left_is_field = bool(_IDENT.match(left)) and left not in _RESERVED
        if left_is_field:
            return ("cmp", split[2], self.field(left), False)
        return ("cmp", split[2], self.field(right), True)


def _serialised_columns(expr: pc.Expression) -> List[pa.Array]:
    """The literals and function options of ``expr`` in tree order: the record
    batch of its serialisation (what its pickle support stores)."""
    _, args = expr.__reduce__()
    table = pa.ipc.open_file(args[0]).read_all()
    return [c.combine_chunks() for c in table.columns]


class _Builder:
    """AST -> (rebuilt expression, postfix instructions), consuming the
    serialised literals in the tree's order."""

    def __init__(self, values: List[pa.Array], schema: pa.Schema) -> None:
        self.values, self.next, self.schema = values, 0, schema
        self.columns: List[Column] = []
        self.out: List[tuple] = []

    def take(self) -> pa.Array:
        if self.next >= len(self.values):
            raise _Refused("fewer literals than the parse expects")
        v = self.values[self.next]
        self.next += 1
        if len(v) != 1:
            raise _Refused("literal column")
        return v

    def column(self, name: str) -> int:
        kind = _column_kind(self.schema.field(name).type)
        if kind is None:
            raise _Refused(f"column type {self.schema.field(name).type}")
        col = Column(name, kind[0], kind[1])
        if col not in self.columns:
            if len(self.columns) == MAX_COLUMNS:
                raise _Refused("too many columns")
            self.columns.append(col)
        return self.columns.index(col)

    def literal(self, c: int, v) -> None:
        kind = self.columns[c].kind
        ok = {"int": type(v) is int, "float": type(v) is float, "string": type(v) is str}[kind]
        if not ok:
            raise _Refused(f"{type(v).__name__} literal on a {kind} column")

    def build(self, node) -> pc.Expression:
        tag = node[0]
        if tag in ("and", "or"):
            left, right = self.build(node[1]), self.build(node[2])
            self.out.append((AND,) if tag == "and" else (OR,))
            return (left & right) if tag == "and" else (left | right)
        if tag == "not":
            e = self.build(node[1])
            self.out.append((NOT,))
            return ~e
        c = self.column(node[-2] if tag == "cmp" else node[1])
        f = pc.field(self.columns[c].name)
        if tag == "valid":
            self.out.append((IS_VALID, c))
            return f.is_valid()
        if tag == "null":
            self.take()  # the options record; the flag is in the text and in equals
            self.out.append((IS_NULL, c, bool(node[2])))
            return f.is_null(nan_is_null=bool(node[2]))
        if tag == "in":
            opts = self.take()
            if not pa.types.is_struct(opts.type) or opts.type.get_field_index("value_set") < 0:
                raise _Refused("is_in options")
            values = opts[0]["value_set"].as_py()
            if not values or len(values) > MAX_SET or any(v is None for v in values):
                raise _Refused("value set size or nulls")
            if self.columns[c].kind == "float":
                raise _Refused("is_in on a float column")
            for v in values:
                self.literal(c, v)
            self.out.append((IS_IN, c, tuple(values)))
            return f.isin(values)
        op, left = node[1], node[3]
        v = self.take()[0].as_py()
        self.literal(c, v)
        if self.columns[c].kind == "string" and op not in ("==", "!="):
            raise _Refused("ordered comparison of strings")
        code = _COMPARE[op]
        self.out.append((_FLIP[code] if left else code, c, v))
        a, b = (pc.scalar(v), f) if left else (f, pc.scalar(v))
        return {"==": a == b, "!=": a != b, "<": a < b, "<=": a <= b, ">": a > b,
                ">=": a >= b}[op]


def _verified(rebuilt: pc.Expression, expr: pc.Expression) -> bool:
    """The one test a parse has to pass."""
    return bool(rebuilt.equals(expr))


def compile(expr: pc.Expression, schema: pa.Schema) -> Optional[Program]:
    """-> the program of ``expr`` over ``schema``'s columns, or None when the
    expression is outside the accepted grammar (module docstring)."""
    return explain(expr, schema)[0]


def explain(expr: pc.Expression, schema: pa.Schema) -> Tuple[Optional[Program], str]:
    """``compile`` with the reason of a refusal ("" when accepted)."""
    try:
        ast = _Parser(str(expr), schema).parse()
        b = _Builder(_serialised_columns(expr), schema)
        rebuilt = b.build(ast)
        if b.next != len(b.values):
            raise _Refused("more literals than the parse expects")
        if len(b.out) > MAX_OPS:
            raise _Refused("too many instructions")
        if sum(len(set(i[2])) for i in b.out if i[0] == IS_IN) > MAX_POOL:
            raise _Refused("value sets exceed the pool")
    except _Refused as e:
        return None, f"grammar: {e}"
    except Exception as e:  # a pyarrow this module does not know: keep the host path
        return None, f"error: {type(e).__name__}: {e}"
    if not _verified(rebuilt, expr):
        return None, "rebuilt expression differs"
    return Program(tuple(b.columns), tuple(b.out), rebuilt), ""


# ------------------------------------------------------------ host columns --
def host_column(col: "pa.ChunkedArray | pa.Array"
                ) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[pa.Array]]:
    """A scalar column as the kernel reads it: (values in the staged dtype,
    validity bool[n] or None when it has no nulls, the distinct strings of a
    string column or None).  String values are int32 codes into the distinct
    strings; the value of a null slot is unspecified (0 here)."""
    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks() if col.num_chunks != 1 else col.chunk(0)
    kind = _column_kind(col.type)
    if kind is None:
        raise TypeError(f"unsupported predicate column type {col.type}")
    valid = None
    if col.null_count:
        valid = pc.is_valid(col).to_numpy(zero_copy_only=False).astype(bool)
    dictionary = None
    if kind[0] == "string":
        if col.type != pa.large_string():
            col = col.cast(pa.string())
        dictionary = pc.unique(col.drop_null())
        dictionary = dictionary.take(pc.array_sort_indices(dictionary))
        col = pc.index_in(col, value_set=dictionary).cast(pa.int32())
    zero = pa.scalar(0, type=col.type)
    values = col.fill_null(zero).to_numpy(zero_copy_only=False) if col.null_count else \
        col.to_numpy(zero_copy_only=False)
    # (a writable copy: the Arrow buffer is not, and the caller hands it to torch)
    return np.array(values, dtype=NP_DTYPES[kind[1]]), valid, dictionary


def host_columns(program: Program, table: pa.Table) -> List[tuple]:
    """``host_column`` of every column of the program, in its order."""
    return [host_column(table.column(c.name)) for c in program.columns]


def pack_validity(valid: np.ndarray) -> np.ndarray:
    """bool[n] -> uint32 validity words starting at bit 0 of row 0."""
    n = valid.size
    padded = np.zeros((n + 31) // 32 * 32, dtype=bool)
    padded[:n] = valid
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


# -------------------------------------------------------- host interpreter --
def _widen(values: np.ndarray) -> np.ndarray:
    """Integers compare in int64, floats in double (a float32 0.1 is not == 0.1)."""
    return values.astype(np.float64 if values.dtype.kind == "f" else np.int64)


def _leaf_compare(op: int, x: np.ndarray, lit, valid: np.ndarray):
    with np.errstate(invalid="ignore"):
        v = {EQ: x == lit, NE: x != lit, LT: x < lit, LE: x <= lit, GT: x > lit,
             GE: x >= lit}[op]
    return v & valid, valid.copy()  # a compare of a null is unknown


def _leaf_is_in(x: np.ndarray, values: np.ndarray, valid: np.ndarray):
    return np.isin(x, values) & valid, np.ones_like(valid)  # is_in of a null is false


def _leaf_is_null(x: np.ndarray, nan_is_null: bool, valid: np.ndarray):
    v = ~valid
    if nan_is_null and x.dtype.kind == "f":
        v = v | (valid & np.isnan(x))
    return v, np.ones_like(valid)


def _and(a, b):
    (va, ka), (vb, kb) = a, b
    return va & vb, (ka & kb) | (ka & ~va) | (kb & ~vb)  # false and anything is false


def _or(a, b):
    (va, ka), (vb, kb) = a, b
    return va | vb, (ka & kb) | va | vb  # true or anything is true


def _not(a):
    va, ka = a
    return ~va & ka, ka


def evaluate_host(program: "Program | tuple", columns: Sequence[tuple]) -> np.ndarray:
    """bool[n]: the program over ``columns`` (per program column (values,
    validity bool[n] or None, distinct strings or None), ``host_column``'s
    triples).  ``program``: a Program, or already encoded (ops, pool).  An
    entry is a (value, known) pair whose value is False while unknown."""
    if isinstance(program, Program):
        program = program.encode([c[2] for c in columns])
    ops, pool = program
    n = len(columns[0][0]) if columns else 0
    stack: List[tuple] = []
    for op in ops:
        code = int(op["op"])
        if code <= IS_VALID:
            values, valid, _ = columns[int(op["column"])]
            valid = np.ones(n, dtype=bool) if valid is None else valid
            if code == IS_VALID:
                stack.append((valid.copy(), np.ones(n, dtype=bool)))
            elif code == IS_NULL:
                stack.append(_leaf_is_null(values, bool(op["imm"]), valid))
            elif code == IS_IN:
                s = pool[int(op["set_offset"]) : int(op["set_offset"]) + int(op["set_length"])]
                stack.append(_leaf_is_in(_widen(values), s, valid))
            else:
                x = _widen(values)
                imm = np.int64(op["imm"])
                lit = imm.view(np.float64) if x.dtype.kind == "f" else imm
                stack.append(_leaf_compare(code, x, lit, valid))
        elif code == NOT:
            stack.append(_not(stack.pop()))
        else:
            b, a = stack.pop(), stack.pop()
            stack.append(_and(a, b) if code == AND else _or(a, b))
    (value, known), = stack
    return value & known  # a null result drops the row
