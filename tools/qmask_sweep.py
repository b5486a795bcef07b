"""Concurrent filtered searches as one per-query-mask batch
(fx_knn_search_qmask_ex) against the same requests run one by one, through
Engine.search.

    python tools/qmask_sweep.py --json profiles/qmask_batch_sweep.json
    python tools/qmask_sweep.py --rows 1000000 --nq 16 --keep 0.5 --reps 5

Per (nq, keep fraction): every request has its own random row mask keeping
that fraction.  The batch (bitmaps packed by fx_qmask_pack inside the timed
region, then one search) and the one-by-one form (each request as
engine.search_host runs it alone: a row-list scan under Engine.SPARSE, a
masked scan above) alternate in one process, each bracketed by events on the
stream after one untimed run; medians, minima and maxima over --reps.  Per nq
also the unmasked batch, the batch under one shared mask and a per-query-mask
batch of all-ones masks: what the admission bits cost the filter.

The summary gives, per case, bytes one by one over bytes batched (the rule of
engine.qmask_batch_pays) beside the measured speed-up, and the smallest byte
ratio from which the batch won at every measured point at or above it: the
default of option "qmask_batch_min_ratio".  One floor is enforced: 16 requests
keeping half the rows must run at least 2x faster as one batch (by bytes it
is more than 30x; anything less means the batch ran as scans).

Corpus: the portable generator's N(0, 1) rows, f32; queries N(0, 1); L2,
k = 100 unless told otherwise.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fenix_amd import _lib  # noqa: E402
from fenix_amd.engine import Engine, Shard, qmask_batch_pays  # noqa: E402


def corpus(eng, n, d, seed):
    x = torch.empty((n, d), dtype=torch.float32, device=eng.device)
    step = 1_000_000
    for r0 in range(0, n, step):
        eng.fill(x[r0:r0 + step], seed=seed, row_base=r0)
    return x


def random_bitmap(n, keep, gen):
    """(int32 words [ceil(n / 32)], kept rows) of a random mask, on the device."""
    words = (n + 31) // 32
    bits = torch.rand(words * 32, device=gen.device, generator=gen) < keep
    bits[n:] = False
    w = torch.arange(32, device=gen.device, dtype=torch.int64)
    packed = (bits.view(words, 32).to(torch.int64) << w).sum(dim=1)
    packed = torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed)  # (the word's 32 bits)
    return packed.to(torch.int32), int(bits.sum().item())


def timed(fn):
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    out = fn()
    b.record(st)
    return out, (a, b)


def stats(evs):
    t = [x.elapsed_time(y) for x, y in evs]
    return {"ms": float(np.median(t)), "ms_min": float(min(t)), "ms_max": float(max(t))}


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--d", type=int, default=768)
    p.add_argument("--nq", default="2,16,64,128")
    p.add_argument("--keep", default="0.02,0.1,0.5,0.9")
    p.add_argument("--k", type=int, default=100)
    p.add_argument("--metric", default="l2")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--json", default="")
    a = p.parse_args()
    eng = Engine.get(torch.device("cuda", 0))
    m = _lib.METRICS[a.metric]
    n, d, k = a.rows, a.d, a.k
    shard = Shard(corpus(eng, n, d, seed=0), 0)
    gen = torch.Generator(device=eng.device)
    gen.manual_seed(7)
    ones = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=eng.device)
    points, costs = [], []
    for nq in [int(v) for v in a.nq.split(",")]:
        q = torch.empty((nq, d), dtype=torch.float32, device=eng.device)
        eng.fill(q, seed=1 + nq)
        kind = _lib.qmask_filter_used(n, d, shard.dtype_id, nq, k, m)
        shared, _ = random_bitmap(n, 0.5, gen)
        all_ones = ones.unsqueeze(0).expand(nq, -1).contiguous()
        forms = {"unmasked": lambda: eng.search([shard], q, m, k),
                 "shared_mask": lambda: eng.search([shard], q, m, k, [shared]),
                 "qmask_all_ones": lambda: eng.search([shard], q, m, k, qmasks=[all_ones])}
        evs = {name: [] for name in forms}
        for fn in forms.values():
            fn()
        for _ in range(a.reps):
            for name, fn in forms.items():
                evs[name].append(timed(fn)[1])
        torch.cuda.synchronize()
        cost = {"nq": nq, "slice": kind, **{name: stats(e) for name, e in evs.items()}}
        costs.append(cost)
        print(json.dumps(cost), flush=True)
        for keep in [float(v) for v in a.keep.split(",")]:
            masks, counts = zip(*[random_bitmap(n, keep, gen) for _ in range(nq)])
            qm = torch.stack(masks)

            def batch():
                return eng.search([shard], q, m, k, qmasks=[qm])

            def singly():
                return [eng.search([shard], q[i:i + 1], m, k, [masks[i]], [counts[i]])
                        for i in range(nq)]

            (bd, br), _ = timed(batch)
            outs, _ = timed(singly)
            torch.cuda.synchronize()
            sd, sr = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
            same = bool(torch.equal(br, sr)
                        and torch.equal(bd.view(torch.int32), sd.view(torch.int32)))
            st = eng.scan(shard, q, m, k, qmasks=qm)
            cnt, cap = eng.filter_counts(shard, nq, m, k, st)
            eb, es = [], []
            for _ in range(a.reps):
                eb.append(timed(batch)[1])
                es.append(timed(singly)[1])
            torch.cuda.synchronize()
            sb, ss = stats(eb), stats(es)
            words = _lib.qmask_words(nq)
            bytes_batch = n * (d + 16) + n * 4 * words
            bytes_single = sum((c if c < Engine.SPARSE * n else n) * d * 4 for c in counts)
            rec = {"rows": n, "d": d, "nq": nq, "keep": keep, "k": k, "metric": a.metric,
                   "slice": kind, "batch": sb, "one_by_one": ss,
                   "speedup": ss["ms"] / sb["ms"], "byte_ratio": bytes_single / bytes_batch,
                   "pays_at_default": qmask_batch_pays(counts, n, d, 4, nq),
                   "bit_identical": same,
                   "count_max": int(cnt.max()) if cnt is not None else -1, "cap": cap,
                   "over_cap": int((cnt.astype(np.int64) > cap).sum()) if cnt is not None else -1}
            points.append(rec)
            print(json.dumps(rec), flush=True)
            del masks, qm
    by_ratio = sorted(points, key=lambda r: r["byte_ratio"])
    crossover = None
    for i, r in enumerate(by_ratio):
        if all(s["batch"]["ms_max"] < s["one_by_one"]["ms_min"] for s in by_ratio[i:]):
            crossover = r["byte_ratio"]
            break
    summary = {"crossover_byte_ratio": crossover,
               "all_bit_identical": all(r["bit_identical"] for r in points),
               "option_default": _lib.get_option("qmask_batch_min_ratio") / 100.0,
               "library_sha": _lib.library_sha(), "reps": a.reps}
    print(json.dumps(summary), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"summary": summary, "epilogue_cost": costs, "points": points}, f, indent=1)
    if not summary["all_bit_identical"]:
        raise SystemExit("a per-query-mask batch differs from the requests run one by one")
    for r in points:
        if r["nq"] == 16 and r["keep"] == 0.5 and r["speedup"] < 2.0:
            raise SystemExit(f"16 requests at keep 0.5: the batch is only {r['speedup']:.2f}x "
                             "faster than one by one (floor 2x): it ran as scans")


if __name__ == "__main__":
    main()
