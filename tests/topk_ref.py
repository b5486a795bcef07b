"""Exact references for the selection pipeline (host only, numpy).

Selection does not care how a distance was computed, so the tests built on
this module give every row a distance they choose exactly ("planted keys"):

* inner product: row r holds the base-B digits of an integer key K_r in a few
  columns, the query the powers of B in the same columns, everything else is
  zero.  Every product and partial sum is an integer below 2^24, so
  ``distance(r) == -K_r`` in f32 on every scan kernel, whatever its summation
  order: f32 one column (K < 2^24), f16 B = 2048 over two columns
  (K < 2^22), quint8 (scale 1, zero point 0) B = 256 over three columns.
  The negated query gives ``distance(r) == +K_r``; the GPU tests search with
  both, so a sequence named for its keys ("descending": every row beats
  every threshold) runs as that order of distances and as its mirror.
* L2: query 0, one column of integer levels x: the distance is the square
  root of the exact square x * x.
* cosine: query (1, 0) and rows (cos t_j, sin t_j) rounded to f32; the float64
  reference is computed from the rounded rows.

The expected result of a search or merge is then ``np.sort`` of the
composites (tests/parity.py make_comp), decoded; no tolerance is involved.

Also here: the key sequences that drive the scan's candidate lists through
their overflow path, and restatements of ``plan_merge`` (csrc/knn_merge.hip)
and of ``plan_scan``'s shape rules (csrc/knn_scan.hip) as they are used.
"""

from __future__ import annotations

import math

import numpy as np

from tests import parity

EMPTY = parity.EMPTY
NAN_BITS = np.uint32(0x7FC00000)  # the NaN of an empty slot and of key_float(KEY_NAN)

# ------------------------------------------------------------- key encoders

# dtype -> (base, digits, exclusive key limit)
ENCODING = {
    "f32": (1 << 24, 1, 1 << 24),
    "f16": (2048, 2, 1 << 22),
    "qu8": (256, 3, 1 << 24),
}
NP_DTYPE = {"f32": np.float32, "f16": np.float16, "qu8": np.uint8}
SLOT_ELEMS = {"f32": 4, "f16": 8, "qu8": 16}  # elements per 16-byte slot


def key_columns(dtype: str, d: int):
    """Columns of the digits, most significant first: the first, middle and
    last column of the row as far as the dtype needs them (one digit: the
    middle), each in a 16-byte slot of its own where the row has as many."""
    nd = ENCODING[dtype][1]
    return {1: [d // 2], 2: [0, d - 1], 3: [0, d // 2, d - 1]}[nd]


def key_digits(dtype: str, keys) -> np.ndarray:
    """[n, digits] array in the corpus dtype: the base-B digits of ``keys``,
    most significant first."""
    base, nd, limit = ENCODING[dtype]
    keys = np.asarray(keys, dtype=np.int64)
    assert keys.size == 0 or (keys.min() >= 0 and keys.max() < limit), "key out of range"
    out = np.empty(keys.shape + (nd,), dtype=NP_DTYPE[dtype])
    rest = keys.copy()
    for j in range(nd - 1, -1, -1):
        out[..., j] = (rest % base).astype(NP_DTYPE[dtype])
        rest //= base
    return out


def key_query(dtype: str, d: int) -> np.ndarray:
    """[d] f32 query: B^(digits-1-j) in digit column j, zeros elsewhere."""
    base, nd, _ = ENCODING[dtype]
    q = np.zeros(d, dtype=np.float32)
    for j, c in enumerate(key_columns(dtype, d)):
        q[c] = float(base ** (nd - 1 - j))
    return q


def encode_rows(dtype: str, d: int, keys) -> np.ndarray:
    """[n, d] host corpus of the keys (small n: the host tests)."""
    keys = np.asarray(keys, dtype=np.int64)
    x = np.zeros((len(keys), d), dtype=NP_DTYPE[dtype])
    x[:, key_columns(dtype, d)] = key_digits(dtype, keys)
    return x


def cosine_rows(levels, nlevels: int) -> np.ndarray:
    """[n, 2] f32 (cos t, sin t), t = level * pi / nlevels."""
    t = np.asarray(levels, dtype=np.float64) * (math.pi / nlevels)
    return np.stack([np.cos(t), np.sin(t)], axis=1).astype(np.float32)


def cosine_ref(rows2: np.ndarray) -> np.ndarray:
    """float64 cosine distance 0.5 - 0.5 cos(q, x) of query (1, 0) to the
    ROUNDED rows (cos, sin)."""
    x = rows2.astype(np.float64)
    return 0.5 - 0.5 * x[:, 0] / np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2)


# ---------------------------------------------------------------- references


def decode(comps: np.ndarray):
    """(distance f32, row i64) of sorted composites: the empty composite
    becomes (NaN, -1), a NaN key the NaN 0x7FC00000."""
    comps = np.asarray(comps, dtype=np.uint64)
    empty = comps == EMPTY
    dist = parity.key_float(parity.comp_key(comps))
    row = np.where(empty, np.int64(-1), parity.comp_row(comps))
    return dist, row


def select(comps: np.ndarray, k: int) -> np.ndarray:
    """The k smallest composites in order, padded with the empty composite;
    equal composites are kept as often as they occur."""
    comps = np.asarray(comps, dtype=np.uint64).ravel()
    if len(comps) > k:
        comps = np.partition(comps, k - 1)[:k]
    out = np.full(k, EMPTY, dtype=np.uint64)
    out[: len(comps)] = np.sort(comps)
    return out


def search_comps(dist, mask, row_base: int) -> np.ndarray:
    """Composites of the live rows of one query: ``dist`` [n] f32."""
    dist = np.asarray(dist, dtype=np.float32)
    rows = np.arange(len(dist), dtype=np.uint64) + np.uint64(row_base)
    comps = parity.make_comp(dist, rows)
    return comps if mask is None else comps[np.asarray(mask, dtype=bool)]


def search_ref(dist, mask, row_base: int, k: int):
    """Exact (distance f32 [k], row i64 [k]) of one query over rows whose f32
    distances are ``dist``; masked rows dropped, fewer than k live rows: rows
    of -1 and NaN."""
    return decode(select(search_comps(dist, mask, row_base), k))


def merge_comps(dist, row) -> np.ndarray:
    """encode_kernel: a row < 0 or >= 0xffffffff is the empty composite."""
    row = np.asarray(row, dtype=np.int64)
    comps = parity.make_comp(np.asarray(dist, dtype=np.float32), row & np.int64(0xFFFFFFFF))
    return np.where((row < 0) | (row >= 0xFFFFFFFF), EMPTY, comps)


def merge_ref(dist, row, k: int):
    """Exact result of fx_topk_merge for one query: lists of any shape."""
    return decode(select(merge_comps(dist, row), k))


def assert_same(got_dist, got_row, want_dist, want_row, what: str = "") -> None:
    """Rows and distance bits equal, nothing else accepted."""
    got_row = np.asarray(got_row)
    want_row = np.asarray(want_row)
    gb = np.ascontiguousarray(got_dist, dtype=np.float32).view(np.uint32)
    wb = np.ascontiguousarray(want_dist, dtype=np.float32).view(np.uint32)
    assert got_row.shape == want_row.shape and gb.shape == wb.shape, f"{what}: shapes differ"
    bad = np.nonzero(got_row != want_row)
    assert len(bad[0]) == 0, (
        f"{what}: rows differ at {[b[:5].tolist() for b in bad]}: got {got_row[bad][:5].tolist()} "
        f"want {want_row[bad][:5].tolist()}")
    bad = np.nonzero(gb != wb)
    assert len(bad[0]) == 0, (
        f"{what}: distance bits differ at {[b[:5].tolist() for b in bad]}: "
        f"got {gb[bad][:5].tolist()} want {wb[bad][:5].tolist()}")


def check_search(got_dist, got_row, dist, mask, row_base: int, k: int, what: str = "") -> None:
    """The search comparison: one query's result against ``search_ref``."""
    wd, wr = search_ref(dist, mask, row_base, k)
    assert_same(got_dist, got_row, wd, wr, what)


def check_merge(got_dist, got_row, dist, row, k: int, what: str = "") -> None:
    """The merge comparison: one query's result against ``merge_ref``."""
    wd, wr = merge_ref(dist, row, k)
    assert_same(got_dist, got_row, wd, wr, what)


# ------------------------------------------------------------ key sequences
#
# Each returns int64 keys [n] in [0, kmax); smaller key = closer row under
# every construction above.  "Large" keys are drawn from [kmax / 2, kmax).


def _large(n: int, kmax: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(kmax // 2, kmax, size=n).astype(np.int64)


def descending(n: int, k: int = 0, kmax: int = 1 << 24) -> np.ndarray:
    """K_r = n-1-r: every row beats every threshold, maximal churn."""
    assert n <= kmax
    return np.arange(n - 1, -1, -1, dtype=np.int64)


def ascending(n: int, k: int = 0, kmax: int = 1 << 24) -> np.ndarray:
    assert n <= kmax
    return np.arange(n, dtype=np.int64)


def sawtooth(n: int, period: int, kmax: int = 1 << 24) -> np.ndarray:
    """Descending within periods of ``period`` rows."""
    assert period <= kmax
    return (period - 1 - np.arange(n, dtype=np.int64) % period).astype(np.int64)


def winners_in_tail(n: int, k: int, kmax: int = 1 << 24, seed: int = 11) -> np.ndarray:
    """Large keys; the k smallest keys on the last k rows."""
    assert 2 * k <= kmax and k <= n
    keys = _large(n, kmax, seed)
    keys[n - k:] = np.random.RandomState(seed + 1).permutation(k)
    return keys


def winners_in_one_wave(n: int, k: int, kmax: int = 1 << 24, seed: int = 12) -> np.ndarray:
    """Large keys; the k smallest keys in k consecutive rows in the middle."""
    assert 2 * k <= kmax and k <= n
    keys = _large(n, kmax, seed)
    at = (n - k) // 2
    keys[at: at + k] = np.random.RandomState(seed + 1).permutation(k)
    return keys


def one_per_block(n: int, k: int, kmax: int = 1 << 24, seed: int = 13) -> np.ndarray:
    """Large keys; the k smallest keys spaced n / k rows apart."""
    assert 2 * k <= kmax and k <= n
    keys = _large(n, kmax, seed)
    keys[(np.arange(k, dtype=np.int64) * n) // k + (n // k) // 2] = \
        np.random.RandomState(seed + 1).permutation(k)
    return keys


def tie_group(n: int, k: int, kmax: int = 1 << 24, seed: int = 14) -> np.ndarray:
    """3k rows share the smallest key, scattered by a fixed permutation: the
    answer is the k lowest row numbers among them."""
    assert 3 * k <= n and kmax >= 4
    keys = _large(n, kmax, seed)
    keys[np.random.RandomState(seed + 1).permutation(n)[: 3 * k]] = 0
    return keys


def mostly_nan(n: int, k: int, kmax: int = 1 << 24, seed: int = 15):
    """(keys, nan) for f32 corpora: all but k-3 rows have a NaN key column
    (``nan`` True), so the result ends with the three lowest NaN rows."""
    assert k >= 3 and n >= k
    keys = _large(n, kmax, seed)
    nan = np.ones(n, dtype=bool)
    nan[np.random.RandomState(seed + 1).permutation(n)[: k - 3]] = False
    return keys, nan


def near_prime(v: int) -> int:
    """The smallest prime >= v."""
    v = max(v, 2)
    while any(v % p == 0 for p in range(2, int(math.isqrt(v)) + 1)):
        v += 1
    return v


# ------------------------------------------------------------ plan_merge

MERGE_ENTRIES = 16384          # kMergeEntries
MERGE_LDS = 160 * 1024         # kMergeLdsBudget
MERGE_SHARED = 256 * 4 + 4 * 4 + 2 * 4 + 3 * 8  # sizeof(MergeShared)
MAX_K = 1024                   # kMaxK: lists or k above it take the sort


def align256(v: int) -> int:
    return (v + 255) // 256 * 256


def next_pow2(v: int) -> int:
    p = 1
    while p < v:
        p <<= 1
    return p


def plan_merge(nq: int, nlists: int, kin: int, k: int) -> dict:
    """csrc/knn_merge.hip plan_merge for kin, k <= kMergeEntries / 2:
    {"group": [G per level], "lists": [...], "klen": [...], "levels",
    "ws_bytes"}."""
    assert kin <= MERGE_ENTRIES // 2 and k <= MERGE_ENTRIES // 2
    fixed = MERGE_SHARED + max(next_pow2(k), k) * 8
    group, nlist, klens = [], [], []
    lists, klen, scratch = nlists, kin, 0
    while True:
        target = max(8 * klen, 3200)
        g = -(-target // klen)
        if g * klen > MERGE_ENTRIES:
            g = MERGE_ENTRIES // klen
        room = (MERGE_LDS - fixed) // 8
        if g * klen > room:
            g = room // klen
        g = min(max(g, 2), lists)
        assert fixed + max(g * klen, k) * 8 <= MERGE_LDS
        nxt = -(-lists // g)
        group.append(g)
        nlist.append(lists)
        klens.append(klen)
        if nxt > 1:
            scratch = max(scratch, nq * nxt * k * 8)
        lists, klen = nxt, k
        if lists == 1:
            break
    return {"group": group, "lists": nlist, "klen": klens, "levels": len(group),
            "ws_bytes": 2 * align256(scratch)}


def merge_workspace_bytes(nq: int, parts: int, kin: int, k: int) -> int:
    """fx_topk_merge_workspace_bytes on the merge-kernel path."""
    return align256(nq * parts * kin * 8) + plan_merge(nq, parts, kin, k)["ws_bytes"]


# ------------------------------------------------------------- plan_scan

SLOT_COUNTS = (1, 2, 3, 4, 6, 8, 12, 16, 24)        # kSlotCounts
ROWS = dict(zip(SLOT_COUNTS, (8, 2, 2, 1, 1, 1, 2, 1, 1)))     # kRows (f32, f16)
ROWS_Q8 = dict(zip(SLOT_COUNTS, (8, 2, 1, 1, 1, 1, 1, 1, 1)))  # kRowsQ8


def scan_shape(dtype: str, d: int, aligned: bool = True) -> dict:
    """plan_scan's kernel class: W elements per load (1: scalar loads), L
    slots per lane, U rows per lane group, nch passes per row, and the cap on
    workgroups per CU."""
    vecw = SLOT_ELEMS[dtype]
    w = vecw if aligned and d % vecw == 0 else 1
    s = d // w
    if w == 1:
        slots = 16
    else:
        need = -(-s // 16)
        slots = next((c for c in SLOT_COUNTS if c >= need), SLOT_COUNTS[-1])
    u = 1 if w == 1 else (ROWS_Q8 if dtype == "qu8" else ROWS)[slots]
    nch = -(-s // (16 * slots))
    occ = 3 if dtype == "qu8" else 1 if slots >= 12 else 2
    return {"W": w, "L": slots, "U": u, "nch": nch, "occ_cap": occ}


def scan_cap(k: int, u: int) -> int:
    """Slots of a wave's candidate list: from 256, doubled while it holds
    fewer than 2k or, after a full tile of 4U appends, fewer than k."""
    cap = 256
    while cap < 2 * k or cap - 4 * u < k:
        cap *= 2
    return cap


def scan_rows_per_block(n: int, k: int, u: int, max_blocks: int) -> int:
    min_rows = max(16 * u * 4, 2 * k, 256)
    blocks = max(1, min(-(-n // min_rows), max_blocks))
    step = 16 * u
    return -(-(-(-n // blocks)) // step) * step


def overflow_rows(k: int, shape: dict, cus: int) -> int:
    """Rows from which every wave of the exact scan scans at least 2 cap
    rows: at most cus * occ_cap workgroups of 4 waves share them."""
    return 8 * scan_cap(k, shape["U"]) * cus * shape["occ_cap"]


# ------------------------------------------------------------ merge shapes
#
# (parts, kin, k, levels of the merge tree; 0: the sort path) of the GPU
# merge tests (tests/test_gpu_merge_tree.py), at MERGE_NQ queries.
MERGE_NQ = 3
MERGE_SHAPES = [
    # one workgroup per query at the first level
    (1, 1, 1, 1), (1, 1000, 1000, 1), (2, 5, 40, 1), (8, 1024, 1024, 1),
    # 16 lists of 1000 fold 8 at a time
    (16, 1000, 10, 2),
    # the bitonic sort's width P2 at a power of two and one to either side
    (9, 1024, 127, 2), (9, 1024, 128, 2), (9, 1024, 129, 2), (9, 1024, 1023, 2),
    (9, 1024, 1024, 2),
    # two and three levels; the last two are plan_single's trees for 512 scan blocks
    (3201, 1, 1, 2), (3201, 1, 1024, 2), (17, 1024, 1024, 2), (512, 1000, 1000, 3),
    (512, 10, 10, 2),
    # the sort path: kin or k above 1024, k above parts * kin
    (3, 3000, 2500, 0), (5000, 1, 1025, 0), (2, 1025, 1, 0), (4, 300, 1300, 0),
]
# (nq, parts, kin, k, levels): run_merge's split at 65 535 queries
MERGE_SPLIT_SHAPES = [(65537, 2, 2, 2, 1), (65537, 3201, 1, 1, 2)]
