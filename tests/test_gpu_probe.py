"""The row-selection kernels of the coded index (fenix_amd/csrc/knn_code.hip)
at the shapes where they take another path: ``fx_code_probe`` (composite
lists, then the merge tree of knn_merge.hip up to 4 096 probes or the
segmented sort above), ``fx_code_mask`` and ``fx_mask_compact``.  A wrong
probe set or row bitmap loses neighbours silently (nothing downstream
recomputes it), so every case is compared bit for bit with a host oracle.

The probe oracle: the score of composite ``c`` is the float32 sum of its digit
terms, left to right from 0.0f, most significant digit first
(``oracle.coder.digits``) — numpy float32 adds give the same bits — and the
expected order is ascending ``parity.make_comp(score, code)`` (-0 == +0, NaN
last, ties by code).  The float32 sums are tied to ``oracle.coder.composite``
in float64 by the standard bound of a length-nb sum,
(nb-1) * 2^-24 * sum_j |term_j|."""

from __future__ import annotations

import numpy as np
import pyarrow as pa
import pytest
import torch

import fenix_amd
from fenix_amd import _lib
from fenix_amd.engine import Engine, bitmap
from fenix_amd.io import coder, index
from oracle import coder as OC
from oracle import oracle as O
from tests import parity

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A  # int32 fill of output buffers: an untouched word keeps it
POISON64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine.get(torch.device("cuda", 0))


# ------------------------------------------------------------------ oracle

_DIGITS = {}


def _digits(nb, ks):
    if (nb, ks) not in _DIGITS:
        _DIGITS[nb, ks] = OC.digits(nb, ks)
    return _DIGITS[nb, ks]


def f32_scores(cw, nb, ks):
    """[nq, ks^nb] float32: s = 0.0f; s = s + d[j, digit_j] for j = 0..nb-1."""
    cw = np.ascontiguousarray(cw, dtype=np.float32)
    dg = _digits(nb, ks)
    s = np.zeros((cw.shape[0], ks**nb), dtype=np.float32)
    for j in range(nb):
        s = s + cw[:, j, dg[j]]
    assert s.dtype == np.float32
    return s


def probe_oracle(cw, nb, ks, probes):
    """(codes [nq, probes] int64, score bits [nq, probes] uint32) in ascending
    (order_key(score), code) order; the score bits are those of
    key_float(order_key(score)), what the kernels decode a key to."""
    s = f32_scores(cw, nb, ks)
    comp = parity.make_comp(s, np.arange(ks**nb, dtype=np.uint64)[None, :])
    order = np.argsort(comp, axis=1, kind="stable")[:, :probes]  # composites are unique
    best = np.take_along_axis(comp, order, axis=1)
    np.testing.assert_array_equal(parity.comp_row(best), order)
    return order.astype(np.int64), parity.key_float(parity.comp_key(best)).view(np.uint32)


def unpack(words, nbits=None):
    """int32 / uint32 words [..., w] -> bool [..., 32 w] (bit r of word r >> 5)."""
    w = np.ascontiguousarray(words).view(np.uint32).astype("<u4")
    bits = np.unpackbits(w.view(np.uint8).reshape(*w.shape[:-1], -1), axis=-1, bitorder="little")
    return bits.astype(bool) if nbits is None else bits[..., :nbits].astype(bool)


def run_probe(eng, cw, probes):
    """Engine.code_probe on the host -> (codes, score bits, sel bits [nq, 32 words])."""
    codes, scores, sel = eng.code_probe(torch.from_numpy(np.ascontiguousarray(cw)), probes)
    torch.cuda.synchronize()
    return (codes.cpu().numpy(), scores.cpu().numpy().view(np.uint32), unpack(sel.cpu().numpy()))


def check_probe(eng, cw, nb, ks, probes):
    nq, C = cw.shape[0], ks**nb
    codes, bits, sel = run_probe(eng, cw, probes)
    ecodes, ebits = probe_oracle(cw, nb, ks, probes)
    assert codes.shape == (nq, probes) and sel.shape == (nq, (C + 31) // 32 * 32)
    # a code outside [0, C) would also be a bit of another query, or past C
    assert codes.min() >= 0 and codes.max() < C
    np.testing.assert_array_equal(codes, ecodes)
    np.testing.assert_array_equal(bits, ebits)
    # each query's bitmap is exactly its own probe set: nothing at or above C,
    # nothing of another query's
    expect = np.zeros(sel.shape, dtype=bool)
    np.put_along_axis(expect, ecodes, True, axis=1)
    np.testing.assert_array_equal(sel, expect)
    return codes, bits


def normal_terms(nq, nb, ks, seed):
    """Terms of both signs (inner-product distances are negative)."""
    return np.random.RandomState(seed).randn(nq, nb, ks).astype(np.float32)


# ------------------------------------------------------------------- cases

#  nb, ks, nq, probes               what it reaches
PROBE_CASES = [
    (1, 5, 1, 1),                 # one sel word
    (1, 5, 1, 5),                 # m == k: copy and sort
    (2, 6, 3, 7),                 # several queries, word stride 2
    (3, 5, 4, 125),               # the golden call case, with the bitmap
    (2, 64, 2, 1),                # exactly one full list
    (2, 64, 2, 4096),             # probes == C == kProbeMerge
    (2, 100, 3, 100),             # 3 lists, the last padded with empty slots
    (2, 100, 3, 4096),            # last probe count of the merge path
    (2, 100, 3, 4097),            # first of the segmented sort
    (2, 100, 3, 10000),           # full sort
    (2, 111, 2, 2048),            # 4 lists in one level (148 528 B of LDS)
    (2, 111, 2, 2049),            # 4 lists + a 4 096-slot result area: 3 + 1 lists; C % 32 != 0
    (2, 256, 2, 2048),            # 2-level tree
    (2, 256, 2, 2049),
    (2, 256, 2, 3000),
    (2, 256, 2, 4096),
    (2, 256, 2, 65536),           # full segmented sort
    (3, 64, 2, 100),              # 64 lists
    (3, 64, 2, 4096),             # the deepest tree
    (4, 16, 1, 300),              # nb = 4 digits
]


@pytest.mark.parametrize("nb,ks,nq,probes", PROBE_CASES)
def test_probe_matches_f32_oracle(eng, nb, ks, nq, probes):
    cw = normal_terms(nq, nb, ks, seed=1000 * nb + ks)
    check_probe(eng, cw, nb, ks, probes)


@pytest.mark.parametrize("nb,ks,nq", sorted({c[:3] for c in PROBE_CASES}))
def test_probe_scores_within_f64_bound(eng, nb, ks, nq):
    """The kernel's (and the oracle's) float32 composite scores against
    oracle.coder.composite in float64: |s32 - s64| <= (nb-1) 2^-24 sum_j |term_j|."""
    C = ks**nb
    cw = normal_terms(nq, nb, ks, seed=1000 * nb + ks)
    codes, bits, _ = run_probe(eng, cw, C)
    got = np.empty((nq, C), dtype=np.float64)
    np.put_along_axis(got, codes, bits.view(np.float32).astype(np.float64), axis=1)
    s64 = OC.composite(cw.reshape(nq, -1).astype(np.float64), nb, ks)
    mag = OC.composite(np.abs(cw).reshape(nq, -1).astype(np.float64), nb, ks)
    bound = (nb - 1) * 2.0**-24 * mag
    assert np.all(np.abs(got - s64) <= bound), float((np.abs(got - s64) - bound).max())
    assert np.all(np.abs(f32_scores(cw, nb, ks).astype(np.float64) - s64) <= bound)


def _edge_terms(kind, nq, nb, ks):
    rs = np.random.RandomState(7)
    if kind == "few_values":  # thousands of exactly equal scores: code order decides
        return rs.choice(np.array([0, 0.25, 0.5, 1], np.float32), size=(nq, nb, ks))
    if kind == "all_equal":
        return np.full((nq, nb, ks), 0.375, dtype=np.float32)
    if kind == "nan_query":  # query 0 all NaN, the others ordinary
        cw = rs.randn(nq, nb, ks).astype(np.float32)
        cw[0] = np.nan
        return cw
    assert kind == "signed_zero"
    return rs.choice(np.array([-0.0, 0.0, -0.0, 0.5, -0.5], np.float32), size=(nq, nb, ks))


@pytest.mark.parametrize("probes", [3000, 4097])  # merge tree / segmented sort
@pytest.mark.parametrize("nb,ks", [(2, 100), (2, 256)])
@pytest.mark.parametrize("kind", ["few_values", "all_equal", "nan_query", "signed_zero"])
def test_probe_ties_nan_and_signed_zero(eng, kind, nb, ks, probes):
    nq = 2
    cw = _edge_terms(kind, nq, nb, ks)
    codes, bits = check_probe(eng, cw, nb, ks, probes)
    first = np.arange(probes, dtype=np.int64)
    if kind == "all_equal":
        np.testing.assert_array_equal(codes, np.broadcast_to(first, codes.shape))
    if kind == "nan_query":
        np.testing.assert_array_equal(codes[0], first)
        assert np.all(bits[0] == 0x7FC00000)
    if kind == "few_values":  # the case is about ties: there are some inside the probe set
        assert len(np.unique(bits[0])) < probes // 100


def _raw_probe(eng, cw, probes, ws_bytes):
    """fx_code_probe on poisoned output buffers -> (rc, every output untouched)."""
    nq, nb, ks = cw.shape
    dev = eng.device
    cd = torch.from_numpy(cw).to(dev)
    codes = torch.full((4096,), POISON64, dtype=torch.int64, device=dev)
    scores = torch.full((4096,), POISON, dtype=torch.int32, device=dev)
    sel = torch.full((4096,), POISON, dtype=torch.int32, device=dev)
    ws = torch.zeros(max(ws_bytes, 1 << 20), dtype=torch.uint8, device=dev)
    with eng.lock:
        rc = _lib.load().fx_code_probe(cd.data_ptr(), nq, nb, ks, probes, ws.data_ptr(), ws.numel(),
                                       codes.data_ptr(), scores.data_ptr(), sel.data_ptr(),
                                       eng._stream())
    torch.cuda.synchronize()
    clean = (bool((codes == POISON64).all()) and bool((scores == POISON).all())
             and bool((sel == POISON).all()))
    return rc, clean


@pytest.mark.parametrize("nb,ks,nq,probes", [
    (2, 6, 2, 0),                # probes = 0
    (2, 6, 2, 37),               # probes = C + 1
    (4, 256, 1, 1),              # C = 2^32
    (2, 32768, 2, 1),            # C = 2^30, nq * C = 2^31
])
def test_probe_errors_launch_nothing(eng, nb, ks, nq, probes):
    cw = normal_terms(nq, nb, ks, seed=5)
    C = ks**nb
    if nq * C < 2**31:
        ws_bytes = _lib.code_probe_workspace_bytes(nq, nb, ks)
    else:
        ws_bytes = 0
        with pytest.raises(NotImplementedError):
            _lib.code_probe_workspace_bytes(nq, nb, ks)
    rc, clean = _raw_probe(eng, cw, probes, ws_bytes)
    assert rc != 0 and clean
    with pytest.raises((ValueError, NotImplementedError)):
        _lib.check(rc)


# ------------------------------------------------------------ fx_code_mask

MASK_N = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 5000, "grid"]


def _mask_inputs(n, ncodes, with_filter, seed):
    rs = np.random.RandomState(seed)
    member = rs.rand(ncodes) < 0.3
    member[[0, ncodes - 1]] = True
    row_code = rs.randint(0, ncodes, size=n).astype(np.int64)
    odd = rs.rand(n) < 0.1  # out-of-range codes: never selected, never read from sel
    row_code[odd] = rs.choice(np.array([-1, ncodes, ncodes + 40], np.int64), size=int(odd.sum()))
    row_code[-1] = ncodes - 1  # the last valid row is selected (unless filtered out)
    filt = rs.rand(n) < 0.5 if with_filter else None
    expect = member[np.clip(row_code, 0, ncodes - 1)] & (row_code >= 0) & (row_code < ncodes)
    np.testing.assert_array_equal(expect, np.isin(row_code, np.nonzero(member)[0]))
    if filt is not None:
        expect = expect & filt
    return member, row_code, filt, expect


def _raw_mask(eng, member, row_code, filt, ncodes):
    """fx_code_mask into words + 2 poisoned int32 -> (that buffer on the host, count)."""
    n = row_code.size
    dev = eng.device
    words = (n + 31) // 32
    out = torch.full((words + 2,), POISON, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), -1, dtype=torch.int64, device=dev)
    rc_t = torch.from_numpy(row_code).to(dev)
    sel_t = torch.from_numpy(bitmap(member).view(np.int32)).to(dev)
    f_t = fenix_amd.engine.device_mask(filt, dev)
    with eng.lock:
        _lib.check(_lib.load().fx_code_mask(
            rc_t.data_ptr(), n, sel_t.data_ptr(), ncodes,
            None if f_t is None else f_t.data_ptr(), out.data_ptr(), cnt.data_ptr(),
            eng._stream()))
    torch.cuda.synchronize()
    return out, int(cnt.item())


@pytest.mark.parametrize("with_filter", [False, True], ids=["nofilter", "filter"])
@pytest.mark.parametrize("ncodes", [36, 12321])
@pytest.mark.parametrize("n", MASK_N)
def test_code_mask_bits_tail_and_count(eng, n, ncodes, with_filter):
    if n == "grid":
        # more rows than the grid holds (8 blocks of 256 per CU): blocks loop,
        # and the last wave of the last pass is partial
        n = 8 * torch.cuda.get_device_properties(eng.device).multi_processor_count * 256 + 257
    member, row_code, filt, expect = _mask_inputs(n, ncodes, with_filter, seed=n % 9973 + ncodes)
    out, cnt = _raw_mask(eng, member, row_code, filt, ncodes)
    out = out.cpu().numpy()
    words = (n + 31) // 32
    assert np.all(out[words:].view(np.uint32) == POISON), "wrote past the bitmap"
    full = np.zeros(words * 32, dtype=bool)  # bits n .. 32 * words are 0
    full[:n] = expect
    np.testing.assert_array_equal(unpack(out[:words]), full)
    assert cnt == int(expect.sum())


@pytest.mark.parametrize("n", [70001, 5000 + 13])  # n % 32 != 0; two compact blocks / one
def test_code_mask_feeds_compact(eng, n):
    """fx_mask_compact never looks at n (compact_write_kernel lists every set
    bit of the last word): the producer's zeroed tail bits are the contract."""
    ncodes = 12321
    member, row_code, filt, expect = _mask_inputs(n, ncodes, True, seed=n)
    out, cnt = _raw_mask(eng, member, row_code, filt, ncodes)
    with eng.lock:
        rows, count = eng.compact(out[: (n + 31) // 32], n)
    torch.cuda.synchronize()
    want = np.nonzero(expect)[0]
    assert int(count.item()) == want.size == cnt
    np.testing.assert_array_equal(rows[: want.size].cpu().numpy(), want)


# --------------------------------------------------------- fx_mask_compact


def test_mask_compact_above_1024_blocks(eng):
    """1 026 blocks of 65 536 rows: compact_scan_kernel scans the block counts
    1 024 at a time and carries the running total into the second round."""
    block = 65536
    n = 1025 * block + 17
    words = (n + 31) // 32
    rs = np.random.RandomState(11)
    rows = np.concatenate([
        rs.randint(0, n, size=3000),
        [0, 1, 31, 32, n - 1, n - 2, n - 17, n - 18],            # first / last valid rows
        [1023 * block - 1, 1023 * block, 1024 * block - 1, 1024 * block,  # blocks 1023 | 1024
         1024 * block + 1, 1025 * block - 1, 1025 * block],      # ... and the partial last block
        np.arange(1024 * block + 4096, 1024 * block + 4096 + 200),  # dense words in round two
    ]).astype(np.int64)
    want = np.unique(rows)
    host = np.zeros(words, dtype=np.uint32)
    np.bitwise_or.at(host, want >> 5, (np.uint32(1) << (want & 31).astype(np.uint32)))
    assert (words + 2047) // 2048 == 1026
    mask = torch.from_numpy(host.view(np.int32)).to(eng.device)
    with eng.lock:
        out, count = eng.compact(mask, n)
    torch.cuda.synchronize()
    assert int(count.item()) == want.size
    np.testing.assert_array_equal(out[: want.size].cpu().numpy(), want)


# -------------------------------------------------------------- end to end


def test_probe_search_3000_probes_over_128x128_codes(eng, tmp_path):
    """io.index.call with probes = 3000 over a 128 x 128 code space: four key
    lists of 4 096 and a 4 096-slot result area, the merge level that asked
    for more LDS than a workgroup can have.  The result is the brute-force
    top-k over the rows whose code is in the oracle's probe set."""
    n, d, ks, nb, probes, k = 4000, 32, 128, 2, 3000, 10
    root = str(tmp_path)
    x = O.fill_normal(n, d, seed=61, cluster=50)
    arr = pa.FixedSizeListArray.from_arrays(pa.array(x.ravel()), list_size=d)
    t = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "vector": arr})
    fenix_amd.io.table.make(root, "p/src", t.to_reader(max_chunksize=1000))
    np.random.seed(62)
    code = coder.make(root, "p/l2", "p/src", "vector",
                      {"metric": "l2", "codebook_size": ks, "num_codebooks": nb,
                       "batch_size": 256, "num_epochs": 1})
    rows_code = index.make(root, "p/l2", "p/src", "vector").column("__CODED_ID__").to_numpy()
    target = O.fill_normal(1, d, seed=63, cluster=50)[0]

    # the oracle's probe set, and that float32 cannot move its boundary: the
    # gap between the last probed and the first unprobed score is far above
    # the rounding of a float32 distance
    cw = code["tensor"].numpy()
    s = OC.composite(OC.distance(target[None], cw.reshape(nb * ks, -1), "l2"), nb, ks)[0]
    order = np.argsort(s, kind="stable")
    gap = s[order[probes]] - s[order[probes - 1]]
    assert gap > 1e-5 * s[order[probes]], gap
    probe = order[:probes]
    np.testing.assert_array_equal(probe, OC.call(target[None], cw, "l2", probes)[0])
    keep = np.isin(rows_code, probe)
    assert keep.sum() > k

    r = index.call(root, "p/l2", "p/src", "vector", target=target, maxval=k, probes=probes)
    od, orow = O.knn(x, target[None], "l2", k, mask=keep)
    gr = r.column("id").to_numpy()
    gd = r.column("__DISTANCE__").to_numpy()
    parity.check_topk(gd[None], gr[None], od, orow, x, target[None], "l2", allow_near_ties=False)
    assert np.all(np.isin(r.column("__CODED_ID__").to_numpy(), probe))
