"""The coded index's assign over quint8 codes (fx_code_assign_ex, FX_DTYPE_QU8)
against the float32 assign (fx_code_assign) over the same rows dequantised.

    python tools/qu8_code_sweep.py --json profiles/qu8_code_assign.json
    python tools/qu8_code_sweep.py --shapes 1000000x768 --reps 5

Per shape (default 10M x 768 and 6.25M x 1536, 2 x 256 codewords, L2): the
rows are quantiser-range codes (0..127) under one (scale, zero point); the
float32 corpus holds exactly scale * (code - zero_point), so both forms
assign the same values and their outputs must agree bit for bit.  The two
forms alternate in one process, each bracketed by events on the stream after
one untimed run; median, minimum and maximum over --reps (7).

The assign is MFMA-bound and the code build issues the same MFMAs over a
quarter of the bytes, so it should cost the same: the summary says, per
shape, whether the quint8 median is at most the float32 median plus the
float32 runs' own relative range (max - min over median) in this process.
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

SCALE, ZP = 0.04, 56


def corpora(eng, n, d, seed):
    """(uint8 codes [n, d], their float32 values [n, d]) on the device: N(0, 1)
    rows of the portable generator quantised to codes 0..127."""
    codes = torch.empty((n, d), dtype=torch.uint8, device=eng.device)
    vals = torch.empty((n, d), dtype=torch.float32, device=eng.device)
    s = torch.tensor(SCALE, dtype=torch.float32, device=eng.device)
    step = 1_000_000
    for r0 in range(0, n, step):
        v = vals[r0:r0 + step]
        eng.fill(v, seed=seed, row_base=r0)
        c = torch.clamp(torch.round(v / s) + ZP, 0, 127)
        codes[r0:r0 + step] = c.to(torch.uint8)
        v.copy_(s * (c - ZP))
    return codes, vals


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
    p.add_argument("--shapes", default="10000000x768,6250000x1536")
    p.add_argument("--nb", type=int, default=2)
    p.add_argument("--ks", type=int, default=256)
    p.add_argument("--metric", default="l2")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--json", default="")
    a = p.parse_args()
    eng = Engine.get(torch.device("cuda", 0))
    m = _lib.METRICS[a.metric]
    points = []
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        codes, vals = corpora(eng, n, d, seed=0)
        shard = Shard(codes, 0, SCALE, ZP)
        cw = torch.empty((a.nb * a.ks, d), dtype=torch.float32, device=eng.device)
        eng.fill(cw, seed=1)
        cw = (cw * (20.0 * SCALE)).reshape(a.nb, a.ks, d)
        forms = {"f32": lambda: eng.code_assign(vals, cw, m, index=True, dist=True),
                 "quint8": lambda: eng.code_assign(shard, cw, m, index=True, dist=True)}
        out = {name: fn() for name, fn in forms.items()}  # untimed
        torch.cuda.synchronize()
        same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int32) if y.dtype == torch.float32 else y)
                   for x, y in zip(out["f32"], out["quint8"]))
        del out
        evs = {name: [] for name in forms}
        for _ in range(a.reps):
            for name, fn in forms.items():
                evs[name].append(timed(fn)[1])
        torch.cuda.synchronize()
        f, q = stats(evs["f32"]), stats(evs["quint8"])
        spread = (f["ms_max"] - f["ms_min"]) / f["ms"]
        rec = {"rows": n, "d": d, "nb": a.nb, "ks": a.ks, "metric": a.metric, "f32": f,
               "quint8": q, "ratio": q["ms"] / f["ms"], "f32_relative_range": spread,
               "within_f32_range": q["ms"] <= f["ms"] * (1.0 + spread),
               "bit_identical": bool(same)}
        points.append(rec)
        print(json.dumps(rec), flush=True)
        del codes, vals, shard, cw, forms
        torch.cuda.empty_cache()
    summary = {"all_bit_identical": all(r["bit_identical"] for r in points),
               "all_within_f32_range": all(r["within_f32_range"] for r in points),
               "library_sha": _lib.library_sha(), "reps": a.reps}
    print(json.dumps(summary), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"summary": summary, "points": points}, f, indent=1)
    if not summary["all_bit_identical"]:
        raise SystemExit("the quint8 assign differs from the f32 assign over the same rows")


if __name__ == "__main__":
    main()
