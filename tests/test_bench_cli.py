"""bench.py's own N > 1 code path, executed on CPU: the driver's launch line (`python -m torch.distributed.run --nnodes=1
--nproc-per-node 2 --master-addr 127.0.0.1 --master-port P bench.py --gpus 2 ...`) with the kernels of the host emulator and gloo
(CADUCEUS_BENCH_TEST_BACKEND=emu, a test hook inside bench.py).  Checks what the 8-GPU run relies on: rank / world handling, one JSON
line from rank 0 only, whole-job token accounting, accumulation micro-steps under no_sync(), the MAX all-reduce of the timing."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(nproc, extra, tmp_path):
    env = dict(os.environ, CADUCEUS_BENCH_TEST_BACKEND="emu", OMP_NUM_THREADS="2", CAD_EMU_THREADS="2")
    tiny = ["--steps", "2", "--warmup", "1", "--seqlen", "256", "--d-model", "32", "--n-layer", "2", "--dtype", "fp32"]
    if nproc == 1:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *tiny, *extra]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), *tiny, *extra]
    out = subprocess.run(cmd, env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines  # rank 0 alone prints, exactly one line
    return json.loads(lines[0])


@pytest.mark.parametrize("nproc,extra,accum,scaling", [
    (2, [], 1, "weak"),                        # configs[3]'s launch shape: one sequence per rank and step
    (2, ["--global-batch", "4"], 2, "strong"),  # the reference's fixed global batch: 2 micro-steps per rank, first under no_sync()
    # configs[3] as the reference runs it on fewer GPUs (hg38.yaml:17: accumulate_grad_batches = 8 / devices): N = 2 -> 4 micro-steps,
    # N = 4 -> 2, global batch 8 either way
    (2, ["--global-batch", "8"], 4, "strong"),
    (4, ["--global-batch", "8"], 2, "strong"),
    # the driver's 8-GPU lines (no 8-GPU node exists for this build: the exact launch line runs here, eight gloo ranks on the emulator):
    # configs[3] = one sequence per rank, global batch 8 (slurm_scripts/run_pretrain_caduceus.sh:5-8,38-42)
    (8, [], 1, "weak"),
    (8, ["--global-batch", "8"], 1, "strong"),
])
def test_bench_two_ranks_over_gloo(tmp_path, nproc, extra, accum, scaling):
    line = _run(nproc, extra, tmp_path)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["n_gpus"] == nproc and line["steps"] == 2 and line["warmup"] == 1
    assert line["scaling"] == scaling and line["higher_is_better"] is True and line["vs_baseline"] is None
    assert line["config"]["parallelism"] == f"dp{nproc}" and line["config"]["accumulate_grad_batches"] == accum
    assert line["config"]["global_batch"] == nproc * accum
    d = line["dist"]
    assert d["world_size"] == nproc and d["backend"] == "gloo" and d["buckets"] >= 1 and d["grad_allreduce_bytes_per_step"] > 0
    assert d["allreduce_exposed_ms_per_step"] is not None and d["allreduce_exposed_ms_per_step"] >= 0.0
    assert d["allreduces_per_step"] == d["buckets"]  # one collective per bucket and optimizer step, however many micro-steps
    # whole-job aggregate: tokens of ALL ranks and micro-steps over the MAX-over-ranks time
    tokens = 256 * nproc * 2 * accum
    assert abs(line["value"] - tokens / (line["ms_per_step"] * 2e-3)) < 1e-6 * line["value"]
    assert "not a measurement" in line["data"]
    assert line["config"]["final_loss"] == line["config"]["final_loss"]  # finite (not NaN)


def test_bench_single_rank_line(tmp_path):
    line = _run(1, [], tmp_path)
    assert line["n_gpus"] == 1 and line["config"]["parallelism"] == "dp1" and line["scaling"] == "weak"
    assert line["dist"]["world_size"] == 1 and line["dist"]["allreduce_exposed_ms_per_step"] is None
    assert line["roofline"] is None and line["cpu_baseline"] is None  # a plain run takes the headline only (evidence: --full)


def test_bench_full_and_dump_outputs(tmp_path):
    """--full runs the evidence beyond the headline in the same process (on the emulator: the extra untimed step; no device timings);
    --dump-outputs writes what the last TIMED step computed, float32 .npy files of at most 64 MB in all."""
    import numpy as np
    out = tmp_path / "dump"
    line = _run(1, ["--full", "--dump-outputs", str(out)], tmp_path)
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    names = sorted(p.name for p in out.iterdir())
    assert names == ["grad_norm.npy", "grads.npy", "logits.npy", "loss.npy", "params.npy"], names
    arrs = {n[:-4]: np.load(out / n) for n in names}
    assert all(a.dtype == np.float32 for a in arrs.values())
    assert sum((out / n).stat().st_size for n in names) <= 64_000_000
    assert arrs["logits"].shape[:2] == (1, 256) and np.isfinite(arrs["logits"]).all()
    assert arrs["params"].size == arrs["grads"].size == line["config"]["params"]
    assert float(arrs["loss"]) == line["config"]["final_loss"]  # the timed step's loss, not the one of --full's extra step
