"""tests/parity.py's key helpers against fx_common.h: ``order_key`` is checked
against a scalar transcription of the C definition and against the order of
the floats themselves, ``key_float`` as its inverse, bit for bit."""

from __future__ import annotations

import struct

import numpy as np

from tests import parity


def _bits(f: float) -> int:
    return struct.unpack("<I", struct.pack("<f", f))[0]


def _order_key_c(u: int) -> int:
    """fx_common.h order_key, line by line, on the float's bits."""
    if (u & 0x7FFFFFFF) == 0:
        u = 0
    if (u & 0x7FFFFFFF) > 0x7F800000:
        return 0xFFFFFFFF
    return (~u & 0xFFFFFFFF) if (u & 0x80000000) else (u | 0x80000000)


def _specials() -> np.ndarray:
    bits = [
        0x00000000, 0x80000000,              # +-0
        0x7F800000, 0xFF800000,              # +-inf
        0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF,  # NaNs, both signs
        0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,  # subnormals
        0x00800000, 0x80800000,              # smallest normals
        0x7F7FFFFF, 0xFF7FFFFF,              # largest finite
        0x3F800000, 0xBF800000, 0x3F7FFFFF, 0x3F800001,
        0x4B400000,                          # 1.5 * 2^23 (the int8 accumulator's start)
    ]
    rs = np.random.RandomState(3)
    rnd = rs.randint(0, 1 << 32, size=20_000, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([np.array(bits, dtype=np.uint32), rnd])


def test_order_key_matches_the_c_definition():
    u = _specials()
    got = parity.order_key(u.view(np.float32))
    want = np.array([_order_key_c(int(b)) for b in u], dtype=np.uint32)
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, want)


def test_order_key_orders_like_the_floats():
    f = _specials().view(np.float32)
    key = parity.order_key(f)
    nan = np.isnan(f)
    assert (key[nan] == parity.KEY_NAN).all() and (key[~nan] < parity.KEY_NAN).all()
    assert parity.order_key(np.float32(-0.0)) == parity.order_key(np.float32(0.0))
    v, kv = f[~nan].astype(np.float64), key[~nan].astype(np.int64)
    o = np.argsort(v, kind="stable")
    v, kv = v[o], kv[o]
    # equal floats (+-0 included) share a key; a larger float has a larger key
    assert ((np.diff(v) > 0) == (np.diff(kv) > 0)).all() and (np.diff(kv) >= 0).all()
    assert parity.order_key(np.float32(-np.inf)) == 0x007FFFFF
    assert parity.order_key(np.float32(np.inf)) == 0xFF800000


def test_key_float_inverts_order_key_bit_for_bit():
    u = _specials()
    f = u.view(np.float32)
    back = parity.key_float(parity.order_key(f)).view(np.uint32)
    mag = u & np.uint32(0x7FFFFFFF)
    want = np.where(mag == 0, np.uint32(0), u)                      # -0 -> +0
    want = np.where(mag > 0x7F800000, np.uint32(0x7FC00000), want)  # NaN -> the quiet NaN
    np.testing.assert_array_equal(back, want)
    # and the other way round, on every key a float can have
    keys = parity.order_key(f)
    np.testing.assert_array_equal(parity.order_key(parity.key_float(keys)), keys)


def test_composites_split_and_compare_by_distance_then_row():
    d = np.array([1.0, 1.0, -2.0, np.nan, 0.0, -0.0], dtype=np.float32)
    r = np.array([7, 3, 1_000_000, 0, 0xFFFFFFFE, 5], dtype=np.int64)
    c = parity.make_comp(d, r)
    assert c.dtype == np.uint64
    np.testing.assert_array_equal(parity.comp_row(c), r)
    np.testing.assert_array_equal(parity.comp_key(c), parity.order_key(d))
    assert [int(i) for i in np.argsort(c)] == [2, 5, 4, 1, 0, 3]
    assert (c < parity.EMPTY).all()
