"""fx_code_qmask (csrc/knn_qmask.hip code_qmask_kernel): the row bitmaps, the
packed admission matrix and the kept-row counts of a batch of probe searches,
built in one pass over the row codes.

* bits: out_masks equals nq fx_code_mask calls and a numpy membership test,
  out_qmask equals fx_qmask_pack of them, the counts equal numpy popcounts;
  padding words, sentinel rows and tail bits are as the header says.  Shapes:
  one row, the edges of a 32-row word and of the 1 024-row tile, several
  workgroups with a ragged last tile; one query, the edges of a 32-query word,
  a full 128-query group and a second, nearly empty one; a code space inside
  one selection word's reach and one of several hundred words;
* each output may be null without changing the others; two runs give the same
  bytes; the call does not synchronise the host; every refusal leaves the
  outputs untouched.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from fenix_amd import _lib
from fenix_amd.engine import Engine, bitmap

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A
PAD = 3


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine.get(torch.device("cuda", 0))


def _case(n, nq, ncodes, filt, seed=0):
    """Host inputs: (codes int64 [n], sel bool [nq, ncodes], sel words uint32
    [nq, cw + PAD] with garbage padding, filter bool [n] or None)."""
    rs = np.random.RandomState(1000 * seed + 7 * n + 13 * nq + ncodes % 97 + int(filt))
    sel = rs.rand(nq, ncodes) < 0.1
    if nq >= 3:
        sel[1] = False
        sel[2] = True
    codes = rs.randint(0, ncodes, size=n).astype(np.int64)
    if n >= 8:
        at = rs.choice(n, 6, replace=False)
        codes[at[:3]] = -1
        codes[at[3:]] = ncodes
    cw = (ncodes + 31) // 32
    words = np.stack([bitmap(r) for r in sel])
    if ncodes % 32:  # bits of codes >= ncodes in the last word are garbage
        words[:, cw - 1] |= np.uint32((0xFFFFFFFF << (ncodes % 32)) & 0xFFFFFFFF)
    words = np.concatenate([words, np.full((nq, PAD), 0xDEADBEEF, np.uint32)], axis=1)
    keep = (rs.rand(n) < 0.7) if filt else None
    return codes, sel, np.ascontiguousarray(words), keep


def _want(codes, sel, keep, ncodes):
    """numpy membership: bool [nq, n]."""
    ok = (codes >= 0) & (codes < ncodes)
    m = sel[:, np.clip(codes, 0, ncodes - 1)] & ok[None, :]
    return m if keep is None else m & keep[None, :]


class _Run:
    """One fx_code_qmask call over sentinel-filled outputs."""

    def __init__(self, eng, codes, words, keep, ncodes, masks=True, packed=True, counts=True):
        dev = eng.device
        n, nq = codes.shape[0], words.shape[0]
        self.n, self.nq, self.mw, self.qw = n, nq, (n + 31) // 32, _lib.qmask_words(nq)
        self.rc_t = torch.from_numpy(codes).to(dev)
        self.sel_t = torch.from_numpy(words.view(np.int32)).to(dev)
        self.filt_t = (torch.from_numpy(bitmap(keep).view(np.int32)).to(dev)
                       if keep is not None else None)
        self.ws = torch.empty(_lib.code_qmask_workspace_bytes(nq, ncodes), dtype=torch.uint8,
                              device=dev)
        self.masks = torch.full((nq, self.mw + PAD), SENT, dtype=torch.int32, device=dev)
        self.packed = torch.full((n + 2, self.qw), SENT, dtype=torch.int32, device=dev)
        self.counts = torch.full((nq,), -7, dtype=torch.int64, device=dev)
        self.ncodes = ncodes
        self.want = (masks, packed, counts)

    def call(self, **over):
        a = dict(row_code=self.rc_t.data_ptr(), n=self.n, sel=self.sel_t.data_ptr(),
                 sel_stride=self.sel_t.shape[1], nq=self.nq, ncodes=self.ncodes,
                 filter=self.filt_t.data_ptr() if self.filt_t is not None else None,
                 ws=self.ws.data_ptr(), ws_bytes=self.ws.numel(),
                 out_masks=self.masks.data_ptr() if self.want[0] else None,
                 mask_stride=self.masks.shape[1],
                 out_qmask=self.packed.data_ptr() if self.want[1] else None,
                 out_counts=self.counts.data_ptr() if self.want[2] else None)
        a.update(over)
        return _lib.load().fx_code_qmask(
            a["row_code"], a["n"], a["sel"], a["sel_stride"], a["nq"], a["ncodes"], a["filter"],
            a["ws"], a["ws_bytes"], a["out_masks"], a["mask_stride"], a["out_qmask"],
            a["out_counts"], torch.cuda.current_stream().cuda_stream)

    def host(self):
        torch.cuda.synchronize()
        return (self.masks.cpu().numpy().view(np.uint32), self.packed.cpu().numpy().view(np.uint32),
                self.counts.cpu().numpy())

    def untouched(self):
        m, p, c = self.host()
        return (m == SENT).all() and (p == SENT).all() and (c == -7).all()


@pytest.mark.parametrize("filt", [False, True], ids=["nofilter", "filter"])
@pytest.mark.parametrize("ncodes", [36, 12_321])
@pytest.mark.parametrize("nq", [1, 31, 33, 128, 130])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1_023, 1_025, 40_003])
def test_masks_matrix_and_counts(eng, n, nq, ncodes, filt):
    codes, sel, words, keep = _case(n, nq, ncodes, filt)
    run = _Run(eng, codes, words, keep, ncodes)
    before = _lib.host_sync_count()
    assert run.call() == 0, _lib.load().fx_last_error()
    assert _lib.host_sync_count() == before
    masks, packed, counts = run.host()
    mw, qw = run.mw, run.qw
    member = _want(codes, sel, keep, ncodes)
    want_words = np.stack([bitmap(r) for r in member])
    # nq fx_code_mask calls, bit for bit
    for q in range(nq):
        mk, cnt = eng.code_mask(run.rc_t, run.sel_t[q], ncodes, run.filt_t)
        np.testing.assert_array_equal(masks[q, :mw], mk.cpu().numpy().view(np.uint32)[:mw],
                                      err_msg=f"target {q}: fx_code_mask")
        assert int(cnt.item()) == counts[q]
    np.testing.assert_array_equal(masks[:, :mw], want_words)  # (zero tail bits included)
    if n % 32:
        assert (masks[:, mw - 1] >> np.uint32(n % 32) == 0).all(), "tail bits set"
    assert (masks[:, mw:] == SENT).all(), "words past ceil(n / 32) were written"
    np.testing.assert_array_equal(counts, member.sum(axis=1))
    # the packed matrix is fx_qmask_pack of the bitmaps
    pk = torch.full((n + 2, qw), SENT, dtype=torch.int32, device=eng.device)
    _lib.check(_lib.load().fx_qmask_pack(run.masks.data_ptr(), run.masks.shape[1], nq, n,
                                         pk.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(packed, pk.cpu().numpy().view(np.uint32))
    assert (packed[n:] == SENT).all(), "rows past n were written"
    bits = np.zeros((n, qw * 32), dtype=bool)
    bits[:, :nq] = member.T
    np.testing.assert_array_equal(
        packed[:n], np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(n, qw))


@pytest.mark.parametrize("n,nq,ncodes", [(33, 33, 36), (40_003, 130, 12_321), (1_025, 128, 36)])
def test_a_null_output_leaves_the_others_identical(eng, n, nq, ncodes):
    codes, sel, words, keep = _case(n, nq, ncodes, True, seed=1)
    full = _Run(eng, codes, words, keep, ncodes)
    assert full.call() == 0
    ref = full.host()
    for drop in range(3):
        want = [True] * 3
        want[drop] = False
        run = _Run(eng, codes, words, keep, ncodes, *want)
        assert run.call() == 0, _lib.load().fx_last_error()
        got = run.host()
        for i in range(3):
            if i == drop:
                assert (got[i] == (SENT if i < 2 else -7)).all(), "a null output's twin was written"
            else:
                np.testing.assert_array_equal(got[i], ref[i])


def test_two_runs_give_the_same_bytes(eng):
    codes, sel, words, keep = _case(40_003, 130, 12_321, True, seed=2)
    outs = []
    for _ in range(2):
        run = _Run(eng, codes, words, keep, 12_321)
        assert run.call() == 0
        outs.append(run.host())
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


def test_no_rows_zeroes_the_counts(eng):
    codes, sel, words, keep = _case(0, 5, 36, False)
    run = _Run(eng, codes, words, keep, 36)
    assert run.call(row_code=None) == 0
    masks, packed, counts = run.host()
    assert (counts == 0).all() and (masks == SENT).all() and (packed == SENT).all()


def test_refusals_leave_the_outputs_untouched(eng):
    n, nq, ncodes = 1_025, 33, 36
    codes, sel, words, keep = _case(n, nq, ncodes, True, seed=3)
    run = _Run(eng, codes, words, keep, ncodes)
    cw, mw = (ncodes + 31) // 32, (n + 31) // 32
    invalid = [
        dict(row_code=None), dict(sel=None), dict(ws=None),
        dict(nq=0), dict(ncodes=0), dict(n=-1),
        dict(sel_stride=cw - 1), dict(mask_stride=mw - 1),
        dict(ws_bytes=run.ws.numel() - 1), dict(ws_bytes=0),
        dict(out_masks=None, out_qmask=None, out_counts=None),
        dict(out_qmask=run.packed.data_ptr() + 4),
    ]
    for over in invalid:
        assert run.call(**over) == -1, over
        assert _lib.load().fx_last_error()
    # a code-major table above 1 GiB: the caller masks target by target
    assert run.call(ncodes=1 << 28, sel_stride=1 << 23) == -2
    out = ctypes.c_size_t(0)
    L = _lib.load()
    assert L.fx_code_qmask_workspace_bytes(33, 1 << 28, ctypes.byref(out)) == -2
    assert L.fx_code_qmask_workspace_bytes(0, 36, ctypes.byref(out)) == -1
    assert L.fx_code_qmask_workspace_bytes(33, 0, ctypes.byref(out)) == -1
    assert L.fx_code_qmask_workspace_bytes(33, 36, None) == -1
    assert run.untouched()
    assert run.call() == 0 and not run.untouched()
