"""bench.py keeps the driver's output contract (one JSON line with metric,
value, roofline, cpu_baseline ...) on small shapes of each path it reports:
the single-query scan, the batched filter, fp16 rows and quint8 codes.  The
legs beside the headline run under ``--full``; a plain run times the headline
alone and ``--dump-outputs`` writes its result."""

from __future__ import annotations

import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
        "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
        "roofline", "cpu_baseline"}


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_bench(*args: str, env=None) -> dict:
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                         capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("extra", [
    ("--d", "768"),
    ("--nq", "16", "--metric", "cosine"),
    ("--dtype", "f16", "--d", "1536", "--k", "1000", "--metric", "inner_product"),
    ("--dtype", "qu8"),
])
def test_bench_contract(extra):
    rec = run_bench("--full", "--rows", "300000", "--steps", "3", "--warmup", "1",
                    "--no-cpu-baseline", *extra)
    assert KEYS <= set(rec)
    assert rec["n_gpus"] == 1 and rec["steps"] == 3 and rec["value"] > 0
    roof = rec["roofline"]
    assert roof["bound"] in ("hbm", "mfma") and roof["peak"] > 0
    assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"])
    assert rec["config"]["rows_per_gpu"] == 300000


def test_bench_plain_run_is_headline_only_and_dumps_outputs(tmp_path):
    """A plain run carries the headline fields and none of --full's legs;
    --steps sets the number of timed steps; --dump-outputs writes the last
    step's [nq, k] result, the same arrays from run to run (seeded inputs),
    whose first row is the planted one (row 12345 of 300000)."""
    recs, outs = [], []
    for steps, sub in (("3", "a"), ("1", "b")):
        recs.append(run_bench("--rows", "300000", "--steps", steps, "--warmup", "1",
                              "--dump-outputs", str(tmp_path / sub)))
        outs.append({n: np.load(tmp_path / sub / f"{n}.npy") for n in ("distances", "rows")})
        assert sorted(os.listdir(tmp_path / sub)) == ["distances.npy", "rows.npy"]
    for rec, steps in zip(recs, (3, 1)):
        assert KEYS <= set(rec) and rec["steps"] == steps
        assert rec["cpu_baseline"] is None
        assert not {"accelerated_exact", "configs2", "strong", "serve", "filter_image"} & set(rec)
        assert rec["ms_per_step"] > 0
        assert rec["value"] == pytest.approx(300000 * 1e3 / rec["ms_per_step"])
    a, b = outs
    assert a["distances"].dtype == np.float32 and a["distances"].shape == (1, 100)
    assert a["rows"].dtype == np.float64 and a["rows"].shape == (1, 100)
    assert np.array_equal(a["distances"], b["distances"]) and np.array_equal(a["rows"], b["rows"])
    assert np.all(np.diff(a["distances"][0]) >= 0)
    # the planted row lies 1/16 from the query, every other row about sqrt(2 d) = 39 away;
    # 1e-2 covers a float32 norm expansion (eps * 2 d = 2e-4 on the square of 1/16)
    assert a["rows"][0, 0] == 12345 and a["distances"][0, 0] == pytest.approx(1 / 16, abs=1e-2)
    assert len(set(a["rows"][0].tolist())) == 100 and a["rows"].min() >= 0
    assert a["rows"].max() < 300000


def test_bench_serve_devices_needs_full():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rows", "100000",
                          "--steps", "1", "--serve-devices", "0,0"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode != 0
    assert "--full" in out.stderr


def test_bench_cpu_baseline_fields():
    rec = run_bench("--full", "--rows", "200000", "--steps", "2", "--warmup", "1",
                    "--cpu-rows", "20000", "--cpu-seconds", "0.5")
    cpu = rec["cpu_baseline"]
    assert cpu["kind"] in ("port", "reference") and cpu["cores"] >= 1 and cpu["value"] > 0


def test_bench_rccl_path_one_rank():
    """The N > 1 path of bench.py (RCCL process group, all-gather of the per-rank
    top-k, merge, barriers, max-over-ranks all-reduce) launched the way the
    driver launches it, with one rank: the one-GPU box runs every RCCL call
    the 8-GPU scaling run makes."""
    env = dict(os.environ, FENIX_AMD_BENCH_DIST="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "bench.py"),
           "--gpus", "1", "--full", "--rows", "300000", "--steps", "3", "--warmup", "1",
           "--no-cpu-baseline"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["config"]["parallelism"] == "row-shard x1, one process per GPU + RCCL all-gather"
    assert rec["n_gpus"] == 1 and rec["value"] > 0


def test_bench_gpus_n_launches_n_ranks():
    """`bench.py --gpus 2 --full` without a launcher starts 2 ranks itself (here
    with gloo, two ranks sharing the one GPU of the box: RCCL refuses a
    duplicate device) and reports n_gpus 2 over 2 x rows, the strong-scaling
    leg (--rows in total, half per rank) and the single-process serve leg
    (rank 0 alone, two shards through engine._search_all, merged on the one
    device since the ordinal repeats), whose result bench.py checks against
    the ranks' merge.  rank 0 also times the CPU baseline after the timed
    legs while rank 1 waits on the store, so the N > 1 line carries one."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    rec = run_bench("--gpus", "2", "--full", "--dist-backend", "gloo", "--rows", "200000",
                    "--steps", "3", "--warmup", "1", "--cpu-rows", "20000",
                    "--cpu-seconds", "0.5", "--serve-devices", "0,0", env=env)
    assert rec["n_gpus"] == 2
    assert rec["config"]["total_rows"] == 400000
    assert rec["config"]["parallelism"].startswith(
        "row-shard x2, one process per GPU + gloo all-gather; strong leg: 200000 rows over 2")
    strong = rec["strong"]
    assert strong["total_rows"] == 200000 and strong["rows_per_gpu"] == 100000
    assert 0 < strong["frac"] <= 1
    serve = rec["serve"]
    assert "error" not in serve, serve
    assert list(serve["gathers"]) == ["none"]
    assert serve["gathers"]["none"]["equals_rank_path"] is True
    cpu = rec["cpu_baseline"]
    assert cpu is not None and cpu["kind"] == "port" and cpu["value"] > 0 and cpu["cores"] >= 1


def test_bench_serve_devices_one_rank():
    """--serve-devices on a single rank (no process group): one process, three
    row shards on the one GPU, merged there."""
    rec = run_bench("--full", "--rows", "200000", "--steps", "2", "--warmup", "1",
                    "--no-cpu-baseline", "--no-accelerated", "--serve-devices", "0,0,0")
    serve = rec["serve"]
    assert serve["total_rows"] == 600000 and serve["gathers"]["none"]["value"] > 0


def test_bench_gpus_must_match_world_size():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2",
                          "--rows", "100000", "--steps", "1", "--no-cpu-baseline"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode != 0
    assert "WORLD_SIZE=1" in out.stderr
