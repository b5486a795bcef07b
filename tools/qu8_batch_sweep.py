"""Batches over quint8 codes: the int8-image path (fx_knn_search_img8_ex)
against per-query exact scans (option "batched" 0), through Engine.search.

    python tools/qu8_batch_sweep.py --json profiles/qu8_batch_sweep.json
    python tools/qu8_batch_sweep.py --rows 10000000 --d 768 --nq 16,256 --reps 7

Per (rows, d, nq): the two paths alternate in one process, each search
bracketed by events on the stream (after one untimed search under the same
options: setting an option drops the binding's planning memo); the medians,
whether rows and distance bits agree, the largest candidate count against
the buffer, and the work nq * rows * d the gate (option "qu8_batch_min_work") compares.  The summary
names the smallest work from which the image path wins at every measured
point at or above it: the option's default.

Corpus: codes 128 + 32 N(0, 1) (clipped), scale 1 / 32, zero point 128;
queries N(0, 1); L2, k = 100 unless told otherwise.
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
from fenix_amd.engine import Engine, Shard  # noqa: E402

SCALE, ZP = 1.0 / 32.0, 128


def codes(eng, n, d, seed):
    """[n, d] uint8 on the device, quantised from the portable generator's
    N(0, 1) rows a million rows at a time."""
    out = torch.empty((n, d), dtype=torch.uint8, device=eng.device)
    step = 1_000_000
    for r0 in range(0, n, step):
        x = torch.empty((min(step, n - r0), d), dtype=torch.float32, device=eng.device)
        eng.fill(x, seed=seed, row_base=r0)
        out[r0:r0 + len(x)] = (x / SCALE + ZP).round_().clamp_(0, 255).to(torch.uint8)
    return out


def timed(fn, **opts):
    """fn() under the options: once untimed, once between two events."""
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with _lib.options(**opts):
        fn()
        a.record(st)
        out = fn()
        b.record(st)
    return out, (a, b)


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="100000,1000000,10000000")
    p.add_argument("--d", default="128,768")
    p.add_argument("--nq", default="2,16,64,256")
    p.add_argument("--k", type=int, default=100)
    p.add_argument("--metric", default="l2")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--json", default="")
    a = p.parse_args()
    eng = Engine.get(torch.device("cuda", 0))
    m = _lib.METRICS[a.metric]
    recs = []
    for n in [int(v) for v in a.rows.split(",")]:
        for d in [int(v) for v in a.d.split(",")]:
            eng.clear_images()
            shard = Shard(codes(eng, n, d, seed=0), 0, SCALE, ZP)
            for nq in [int(v) for v in a.nq.split(",")]:
                q = torch.empty((nq, d), dtype=torch.float32, device=eng.device)
                eng.fill(q, seed=1 + nq)

                def search():
                    return eng.search([shard], q, m, a.k)

                # (the first image search builds the image)
                (idist, irow), _ = timed(search, qu8_batch_min_work=0)
                (edist, erow), _ = timed(search, batched=0)
                torch.cuda.synchronize()
                same = bool(torch.equal(irow, erow)
                            and torch.equal(idist.view(torch.int32), edist.view(torch.int32)))
                with _lib.options(qu8_batch_min_work=0):
                    st = eng.scan(shard, q, m, a.k)
                    counts, cap = eng.filter_counts(shard, nq, m, a.k, st)
                ev_i, ev_e = [], []
                for _ in range(a.reps):
                    ev_i.append(timed(search, qu8_batch_min_work=0)[1])
                    ev_e.append(timed(search, batched=0)[1])
                torch.cuda.synchronize()
                ti = [x.elapsed_time(y) for x, y in ev_i]
                te = [x.elapsed_time(y) for x, y in ev_e]
                rec = {"rows": n, "d": d, "nq": nq, "k": a.k, "metric": a.metric,
                       "work": nq * n * d, "image_ms": float(np.median(ti)),
                       "image_ms_min": float(min(ti)), "image_ms_max": float(max(ti)),
                       "exact_ms": float(np.median(te)), "exact_ms_min": float(min(te)),
                       "exact_ms_max": float(max(te)), "bit_identical": same,
                       "count_max": int(counts.max()) if counts is not None else -1, "cap": cap,
                       "image_held": id(shard.data) in eng._images}
                rec["speedup"] = rec["exact_ms"] / rec["image_ms"]
                recs.append(rec)
                print(json.dumps(rec), flush=True)
            del shard
    # the gate: the smallest work from which the image path wins at every
    # measured point at or above it (beyond the exact path's own spread)
    recs_by_work = sorted(recs, key=lambda r: r["work"])
    gate = None
    for i, r in enumerate(recs_by_work):
        if all(s["image_ms_max"] < s["exact_ms_min"] for s in recs_by_work[i:]):
            gate = r["work"]
            break
    summary = {"gate_work": gate, "all_bit_identical": all(r["bit_identical"] for r in recs),
               "library_sha": _lib.library_sha(), "reps": a.reps,
               "gate_option_default": _lib.get_option("qu8_batch_min_work")}
    print(json.dumps(summary), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"summary": summary, "points": recs}, f, indent=1)
    if not summary["all_bit_identical"]:
        raise SystemExit("the image path differs from the exact scans")


if __name__ == "__main__":
    main()
