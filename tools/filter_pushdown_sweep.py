"""Filtered io.index.call with the filter evaluated on the device
(fx_pred_eval over resident predicate columns) against the same calls with
FENIX_AMD_DEVICE_FILTER=0 (pyarrow evaluates the expression over the whole
table, the mask is packed and uploaded), alternating in one process.

    python tools/filter_pushdown_sweep.py --json profiles/filter_pushdown.json
    python tools/filter_pushdown_sweep.py --rows 10000000 --json profiles/filter_pushdown.json

Per row count (a source file of that many rows x --d f32, written in 1 000-row
batches; 10M x 768 is 30 GB of disk) and per keep fraction, three filters: one
integer compare, a compare and an is_in, and a string equality.  Each call is
timed on the host clock (the host's work is what differs) after one untimed
call that stages the columns; medians, minima and maxima over --reps.  The
kernel alone is timed by events around Engine.pred_eval and reported in time
and in GB/s over the bytes of the columns it reads.

The summary gives the smallest measured row count from which the device path
won (its median below the host path's, the comparison asked of the 1M and 10M
points) at every point at or above it: the default of option
"device_filter_min_rows".  Each point also records whether the device path's
slowest call was below the host path's fastest; on the host clock single calls
of either path stray by several times their median, so that flag is reported
and not what the threshold is taken from.  Row counts given
with --rows replace their earlier points in --json; the others are kept, so a
sweep can be run one row count at a time.
"""

from __future__ import annotations

import argparse
import atexit
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fenix_amd import _lib, engine  # noqa: E402
from fenix_amd.engine import Engine  # noqa: E402
from fenix_amd.io import _resident, index, predicate, table  # noqa: E402

KEEPS = (0.02, 0.1, 0.5, 0.9)
OTHERS = np.array(["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta"], dtype=object)


def write_source(eng, root, name, n, d, batch=1000):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 1000, n).astype(np.int32)
    b = rng.integers(0, 100, n).astype(np.int64)
    strings = {f"s{int(p * 100):02d}": np.where(rng.random(n) < p, "hit", rng.choice(OTHERS, n))
               for p in KEEPS}
    schema = pa.schema([("id", pa.int64()), ("a", pa.int32()), ("b", pa.int64())]
                       + [(s, pa.string()) for s in strings]
                       + [("vector", pa.list_(pa.float32(), d))])
    dev = torch.empty((min(n, 100_000), d), dtype=torch.float32, device=eng.device)

    def batches():
        for s in range(0, n, 100_000):
            m = min(100_000, n - s)
            eng.fill(dev[:m], seed=0, row_base=s)
            arr = pa.FixedSizeListArray.from_arrays(pa.array(dev[:m].cpu().numpy().ravel()),
                                                    list_size=d)
            for c in range(0, m, batch):
                r = slice(s + c, s + min(c + batch, m))
                yield pa.record_batch(
                    [pa.array(np.arange(r.start, r.stop, dtype=np.int64)), pa.array(a[r]),
                     pa.array(b[r])] + [pa.array(v[r], type=pa.string()) for v in strings.values()]
                    + [arr.slice(c, r.stop - r.start)], schema=schema)

    table.make(root, name, pa.RecordBatchReader.from_batches(schema, batches()))


def filters(keep):
    f = pc.field
    return {
        "compare": f("a") < int(round(1000 * keep)),
        "compare_and_is_in": (f("a") < int(round(1000 * keep / 0.95))) & f("b").isin(
            [int(v) for v in range(95)]),
        "string_eq": f(f"s{int(keep * 100):02d}") == "hit",
    }


def stats(t):
    return {"ms": float(np.median(t)), "ms_min": float(min(t)), "ms_max": float(max(t))}


def kernel_alone(eng, root, name, flt, reps):
    """fx_pred_eval alone over the whole source: (stats, bytes of the columns)."""
    path = table.path(root, name)
    key, t = _resident.load_table(path)
    program = predicate.compile(flt, t.schema)
    cols = [_resident.pred_column(key, t, c.name, eng.device) for c in program.columns]
    nbytes = sum(c.values.numel() * c.values.element_size()
                 + (c.valid.numel() * 4 if c.valid is not None else 0) for c in cols)
    eng.pred_eval(program, cols, t.num_rows, 0)
    st = torch.cuda.current_stream()
    evs = []
    for _ in range(reps):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record(st)
        eng.pred_eval(program, cols, t.num_rows, 0)
        y.record(st)
        evs.append((x, y))
    torch.cuda.synchronize()
    s = stats([x.elapsed_time(y) for x, y in evs])
    s["column_bytes"] = nbytes
    s["gb_per_s"] = nbytes / (s["ms"] * 1e-3) / 1e9
    return s


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="10000,100000,1000000,10000000")
    p.add_argument("--d", type=int, default=768)
    p.add_argument("--k", type=int, default=100)
    p.add_argument("--metric", default="l2")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--json", default="")
    a = p.parse_args()
    eng = Engine.get(torch.device("cuda", 0))
    root = tempfile.mkdtemp(prefix="fenix_filter_")
    atexit.register(shutil.rmtree, root, True)
    rows = [int(v) for v in a.rows.split(",")]
    points = []
    if a.json and os.path.exists(a.json):
        with open(a.json) as f:
            points = [r for r in json.load(f)["points"] if r["rows"] not in rows]
    target = np.random.RandomState(0).standard_normal(a.d).astype(np.float32)
    os.environ.pop("FENIX_AMD_DEVICE_FILTER", None)
    with _lib.options(device_filter_min_rows=0):
        for n in rows:
            name = f"sweep/n{n}"
            t0 = time.perf_counter()
            write_source(eng, root, name, n, a.d)
            print(json.dumps({"rows": n, "write_s": round(time.perf_counter() - t0, 1)}),
                  flush=True)
            for keep in KEEPS:
                for fname, flt in filters(keep).items():
                    def call():
                        t0 = time.perf_counter()
                        out = index.call(root, None, name, "vector", target=target,
                                         metric=a.metric, select=["id"], filter=flt, maxval=a.k)
                        return out, (time.perf_counter() - t0) * 1e3

                    def host_call():
                        os.environ["FENIX_AMD_DEVICE_FILTER"] = "0"
                        try:
                            return call()
                        finally:
                            del os.environ["FENIX_AMD_DEVICE_FILTER"]

                    before = index.filter_stats()
                    got, _ = call()      # stages the predicate columns
                    want, _ = host_call()
                    after = index.filter_stats()
                    assert (after["device"], after["host"]) == (before["device"] + 1,
                                                                before["host"] + 1), after
                    td, th = [], []
                    for _ in range(a.reps):
                        td.append(call()[1])
                        th.append(host_call()[1])
                    sd, sh = stats(td), stats(th)
                    rec = {"rows": n, "d": a.d, "k": a.k, "metric": a.metric, "keep": keep,
                           "filter": fname, "expression": str(flt)[:120],
                           "kept_rows": int(index._filter_mask(
                               table.load(root, name).select(["a", "b", f"s{int(keep * 100):02d}"]),
                               flt).sum()),
                           "device": sd, "host": sh, "speedup": sh["ms"] / sd["ms"],
                           "device_wins": sd["ms"] < sh["ms"],
                           "device_wins_every_call": sd["ms_max"] < sh["ms_min"],
                           "same_table": bool(got.equals(want)),
                           "kernel": kernel_alone(eng, root, name, flt, a.reps)}
                    points.append(rec)
                    print(json.dumps(rec), flush=True)
            engine.CACHE.clear()
            engine.RESIDENT.evict_all()
            table.drop(root, name)
    by_rows = sorted({r["rows"] for r in points})
    min_rows = None
    for n in by_rows:
        if all(r["device_wins"] for r in points if r["rows"] >= n):
            min_rows = n
            break
    summary = {"device_filter_min_rows": min_rows,
               "option_default": _lib.get_option("device_filter_min_rows"),
               "device_wins_at_1M_and_10M": all(r["device_wins"] for r in points
                                                if r["rows"] >= 1_000_000),
               "rows_measured": by_rows,
               "points_where_a_single_call_crossed": sum(
                   not r["device_wins_every_call"] for r in points),
               "all_same_table": all(r["same_table"] for r in points),
               "library_sha": _lib.library_sha(), "reps": a.reps}
    print(json.dumps(summary), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"summary": summary, "points": points}, f, indent=1)
    if not summary["all_same_table"]:
        raise SystemExit("a device-filtered call differs from the host-filtered one")


if __name__ == "__main__":
    main()
