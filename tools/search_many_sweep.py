"""The many-target search: (a) building the per-target masks of a probe batch in
one pass over the codes (fx_code_qmask) against one fx_code_mask per target
plus one fx_qmask_pack, and (b) Flight.search_many against the same targets
sent one by one.

    python tools/search_many_sweep.py --json profiles/search_many.json
    python tools/search_many_sweep.py --rows 1000000 --nq 2,16 --reps 5 --skip-flight

(a) Per (nq, shared filter or none): n random composite codes of a ks = 256,
nb = 2 coding (65 536 codes), every target selecting --probes random codes.
Both routes produce the bitmaps, the packed matrix and the counts; they
alternate in one process, each bracketed by events on the stream after an
untimed run; medians, minima and maxima over --reps (at least 20 for a
recorded profile).  The outputs of the two routes are compared bit for bit.
The summary gives the smallest nq from which the one-pass route won at every
measured point at or above it (engine.CODE_QMASK_MIN_NQ names this profile).

(b) --e2e-rows x 128 f32 rows behind an in-process Flight server, k = 10,
--e2e-targets targets: one search_many against that many sequential searches,
without probes and with probes = 64 of 65 536 codes; host wall-clock around
the calls (each returns its table), medians over --e2e-reps after a warm-up.
Every target's rows of search_many are compared with its own search.
"""

from __future__ import annotations

import argparse
import json
import os
import socket
import sys
import tempfile
import time

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fenix_amd  # noqa: E402
from fenix_amd import _lib, engine  # noqa: E402
from fenix_amd.engine import Engine  # noqa: E402

from qmask_sweep import random_bitmap, stats, timed  # noqa: E402


def random_sel(nq, ncodes, probes, gen):
    """int32 [nq, ceil(ncodes / 32)]: every target selects ``probes`` random codes."""
    words = (ncodes + 31) // 32
    bits = torch.zeros((nq, words * 32), dtype=torch.bool, device=gen.device)
    pick = torch.rand((nq, ncodes), device=gen.device, generator=gen).topk(probes, dim=1).indices
    bits.scatter_(1, pick, True)
    w = torch.arange(32, device=gen.device, dtype=torch.int64)
    packed = (bits.view(nq, words, 32).to(torch.int64) << w).sum(dim=2)
    packed = torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed)
    return packed.to(torch.int32)


def mask_building(eng, a) -> tuple:
    n, ncodes = a.rows, a.ks ** 2
    gen = torch.Generator(device=eng.device)
    gen.manual_seed(11)
    codes = torch.randint(0, ncodes, (n,), dtype=torch.int64, device=eng.device, generator=gen)
    shared, _ = random_bitmap(n, 0.5, gen)
    L = _lib.load()
    points = []
    for nq in [int(v) for v in a.nq.split(",")]:
        sel = random_sel(nq, ncodes, a.probes, gen)
        for flt in (None, shared):
            def one_pass():
                return eng.code_qmask(codes, sel, ncodes, flt)

            def per_target():
                outs = [eng.code_mask(codes, sel[q], ncodes, flt) for q in range(nq)]
                bm = torch.stack([o[0] for o in outs])
                cnt = torch.cat([o[1] for o in outs])
                pk = torch.empty((n, _lib.qmask_words(nq)), dtype=torch.int32, device=eng.device)
                with eng.lock:
                    _lib.check(L.fx_qmask_pack(bm.data_ptr(), bm.shape[1], nq, n, pk.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream))
                return bm, pk, cnt

            new, old = one_pass(), per_target()
            torch.cuda.synchronize()
            same = all(torch.equal(x, y) for x, y in zip(new, old))
            del new, old
            en, eo = [], []
            for _ in range(a.reps):
                en.append(timed(one_pass)[1])
                eo.append(timed(per_target)[1])
            torch.cuda.synchronize()
            sn, so = stats(en), stats(eo)
            qw = _lib.qmask_words(nq)
            rec = {"rows": n, "codes": ncodes, "nq": nq, "probes": a.probes,
                   "shared_filter": flt is not None, "one_pass": sn, "per_target": so,
                   "speedup": so["ms"] / sn["ms"], "bit_identical": same,
                   # bytes each route moves, from the shapes
                   "bytes_one_pass": (qw // 4) * (8 * n + (n // 8 if flt is not None else 0))
                   + n * qw * 4 + nq * (n // 8),
                   "bytes_per_target": nq * (8 * n + (n // 8 if flt is not None else 0))
                   + 2 * nq * (n // 8) + n * qw * 4}
            points.append(rec)
            print(json.dumps(rec), flush=True)
    crossover = None
    by_nq = sorted(points, key=lambda r: r["nq"])
    for r in by_nq:
        if all(s["one_pass"]["ms"] < s["per_target"]["ms"] for s in by_nq if s["nq"] >= r["nq"]):
            crossover = r["nq"]
            break
    return points, {"one_pass_wins_from_nq": crossover,
                    "all_bit_identical": all(r["bit_identical"] for r in points),
                    "constant": engine.CODE_QMASK_MIN_NQ}


def wall(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(t)), "ms_min": float(min(t)), "ms_max": float(max(t))}


def end_to_end(eng, a) -> list:
    n, d, k, nq = a.e2e_rows, 128, 10, a.e2e_targets
    x = torch.empty((n, d), dtype=torch.float32, device=eng.device)
    eng.fill(x, seed=3)
    xh = x.cpu().numpy()
    del x
    t = torch.empty((nq, d), dtype=torch.float32, device=eng.device)
    eng.fill(t, seed=4)
    targets = t.cpu().numpy()
    src = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)),
                    "vector": pa.FixedSizeListArray.from_arrays(pa.array(xh.ravel()), d)})
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = []
    with tempfile.TemporaryDirectory() as root:
        server = fenix_amd.Server(root, host="127.0.0.1", port=port)
        try:
            f = fenix_amd.Flight(host="127.0.0.1", port=port)
            f.make_table("sweep/t", src.to_reader(max_chunksize=100_000))
            np.random.seed(5)
            f.make_index(name="sweep/c", source="sweep/t", column="vector",
                         config={"metric": "l2", "codebook_size": a.ks, "num_codebooks": 2,
                                 "batch_size": 2560, "num_epochs": 2})
            for name, kw in (("no_probes", dict()),
                             ("probes", dict(coding="sweep/c", probes=a.probes))):
                kw = dict(metric="l2", select=["id"], maxval=k, **kw)

                def many():
                    return f.search_many(targets, "sweep/t", "vector", **kw)

                def singly():
                    return [f.search(targets[i], "sweep/t", "vector", **kw) for i in range(nq)]

                got, want = many(), singly()
                same = True
                for i, one in enumerate(want):
                    sub = got.filter(pc.field("__TARGET__") == i).drop(["__TARGET__"])
                    # (a search that kept at most k rows answers in table order)
                    same = same and (sub.equals(one) or (
                        one.num_rows <= k and sorted(sub.column("id").to_pylist())
                        == sorted(one.column("id").to_pylist())))
                rec = {"case": name, "rows": n, "d": d, "k": k, "targets": nq,
                       "search_many": wall(many, a.e2e_reps),
                       "sequential": wall(singly, a.e2e_reps), "same_rows": bool(same)}
                rec["speedup"] = rec["sequential"]["ms"] / rec["search_many"]["ms"]
                out.append(rec)
                print(json.dumps(rec), flush=True)
        finally:
            server.shutdown()
            engine.CACHE.clear()
    return out


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--ks", type=int, default=256)
    p.add_argument("--probes", type=int, default=64)
    p.add_argument("--nq", default="2,3,4,8,16,64,256")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--e2e-rows", type=int, default=1_000_000)
    p.add_argument("--e2e-targets", type=int, default=64)
    p.add_argument("--e2e-reps", type=int, default=7)
    p.add_argument("--skip-flight", action="store_true")
    p.add_argument("--json", default="")
    a = p.parse_args()
    eng = Engine.get(torch.device("cuda", 0))
    points, summary = mask_building(eng, a)
    e2e = [] if a.skip_flight else end_to_end(eng, a)
    summary.update(library_sha=_lib.library_sha(), reps=a.reps, e2e_reps=a.e2e_reps)
    print(json.dumps(summary), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"summary": summary, "mask_building": points, "end_to_end": e2e}, f, indent=1)
    if not summary["all_bit_identical"]:
        raise SystemExit("fx_code_qmask differs from the per-target masks")
    if any(not r["same_rows"] for r in e2e):
        raise SystemExit("search_many differs from the targets searched one by one")


if __name__ == "__main__":
    main()
