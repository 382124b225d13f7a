"""A plain `python bench.py --gpus 1 --steps K --warmup W` measures the headline alone; `--dump-outputs DIR` writes the iterate
its last timed step computed, so that two builds can be compared output for output; everything else sits behind `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_dump_outputs_writes_a_fixed_sample_of_a_large_iterate(tmp_path):
    """The sampling branch on a CPU tensor: an iterate above the byte budget is written as the same ascending rows every time,
    float32, within the budget; one below it is written whole."""
    import torch
    import bench
    n, d = 1000, 8
    a = torch.arange((n + 24) * d, dtype=torch.float32).reshape(n + 24, d)        # padding rows below n, as the row partition has
    for run in ("first", "second"):
        bench.dump_outputs(str(tmp_path / run), a, n, budget_bytes=100 * d * 4)
    x, rows = np.load(tmp_path / "first" / "iterate.npy"), np.load(tmp_path / "first" / "iterate_rows.npy")
    assert x.dtype == np.float32 and x.shape == (100, d) and rows.dtype == np.float64 and rows.shape == (100,)
    idx = rows.astype(np.int64)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < n
    np.testing.assert_array_equal(x, a.numpy()[idx])
    np.testing.assert_array_equal(rows, np.load(tmp_path / "second" / "iterate_rows.npy"))
    np.testing.assert_array_equal(x, np.load(tmp_path / "second" / "iterate.npy"))
    bench.dump_outputs(str(tmp_path / "whole"), a, n, budget_bytes=n * d * 4)
    np.testing.assert_array_equal(np.load(tmp_path / "whole" / "iterate.npy"), a.numpy()[:n])
    np.testing.assert_array_equal(np.load(tmp_path / "whole" / "iterate_rows.npy"), np.arange(n))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_iterate(tmp_path):
    """One plain run at a small size: the line carries the headline fields and none of what --full adds, and the dumped iterate is,
    bit for bit, the oracle's after warmup + steps iterations from E_0 on the same seeded graph."""
    import torch
    import oracle
    from cleora_amd import synth
    nodes, pairs, d, steps, warmup = 20_000, 190_000, 64, 2, 1
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--nodes", str(nodes),
                        "--pairs", str(pairs), "--dim", str(d), "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 1 and j["steps"] == steps and j["warmup"] == warmup and j["full"] is False
    assert j["unit"] == "edge*dim/s" and j["higher_is_better"] is True and j["dtype"] == "f32" and j["value"] > 0
    assert j["ms_per_step"] > 0 and j["roofline"]["launches"] == steps
    assert j["value"] == pytest.approx(j["config"]["nnz"] * d / (j["ms_per_step"] * 1e-3), rel=1e-9)
    assert j["cpu_baseline"] is None and j["checks"] == {} and not {"whitened", "end_to_end", "selftest", "partitions"} & set(j)

    g = synth.power_law_graph(nodes, pairs, 2, torch.device("cuda:0"))
    n = g["n"]
    hashes = synth.entity_hashes(n, 0, torch.device("cuda:0")).cpu().numpy().view(np.uint64)
    want, _ = oracle.embed(g["rowptr"].cpu().numpy().astype(np.uint64), g["col"].cpu().numpy().view(np.uint32),
                           g["val_left"].cpu().numpy(), oracle.init(hashes, d, 0), warmup + steps)
    got, rows = np.load(tmp_path / "iterate.npy"), np.load(tmp_path / "iterate_rows.npy")
    assert sorted(os.listdir(tmp_path)) == ["iterate.npy", "iterate_rows.npy"]
    assert got.dtype == np.float32 and rows.dtype == np.float64
    np.testing.assert_array_equal(rows, np.arange(n))
    np.testing.assert_array_equal(got, want)
