"""CPU: bench.py's multi-process launcher and reporting path with the --stub workload (gloo).
`python bench.py --gpus 2` must start the ranks itself (torchrun child, 127.0.0.1) and report
n_gpus == 2 with the whole-job aggregate; a torchrun environment whose WORLD_SIZE disagrees
with --gpus is an error."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], capture_output=True, text=True,
                          timeout=240, env=e, cwd=REPO)


def test_bench_launcher_spawns_ranks():
    r = _run(["--stub", "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "3", "--new-tokens", "5"])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout          # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 6 and d["config"]["parallelism"] == "dp2"
    # 2 ranks x 3 utterances x 5 frames x 9 codebooks per step
    assert abs(d["value"] - 2 * 2 * 3 * 5 * 9 / (d["ms_per_step"] * d["steps"] / 1e3)) / d["value"] < 0.01


def test_bench_single_process_stub():
    r = _run(["--stub", "--steps", "1", "--warmup", "0", "--batch", "2", "--new-tokens", "4"])
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 1


def test_bench_dump_outputs_stub(tmp_path):
    """--dump-outputs writes the last timed step's codes as float32 .npy, the same from run to run; the
    result line of a plain run carries the headline fields and none of the --full measurements."""
    import numpy as np
    got = []
    for d in ("a", "b"):
        r = _run(["--stub", "--steps", "2", "--warmup", "1", "--batch", "2", "--new-tokens", "4",
                  "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line
        assert line["steps"] == 2 and not {"cpu_baseline", "secondary", "roofline", "gemm_roofline"} & set(line)
        assert sorted(os.listdir(tmp_path / d)) == ["codes.npy"]
        got.append(np.load(tmp_path / d / "codes.npy"))
    assert got[0].dtype == np.float32 and got[0].shape == (2, 9, 4)
    assert np.array_equal(got[0][:, 0, 0], [0, 1]) and np.array_equal(got[0], got[1])


def test_bench_dump_sample_is_fixed_and_bounded():
    """An output larger than its budget is dumped as the same seeded, ordered choice of whole blocks."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    n = 10 * bench.DUMP_BLOCK + 17
    t = torch.arange(n, dtype=torch.float64)
    budget = 3 * bench.DUMP_BLOCK * 4 + 100
    a = bench._fixed_sample(torch, t, budget)
    b = bench._fixed_sample(torch, t.clone(), budget)
    assert a.dtype == np.float32 and a.nbytes <= budget and a.size == 3 * bench.DUMP_BLOCK
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0)
    blocks = a.reshape(3, bench.DUMP_BLOCK)
    assert np.all(blocks[:, 0] % bench.DUMP_BLOCK == 0) and np.all(np.diff(blocks, axis=1) == 1)
    small = bench._fixed_sample(torch, t[:100], budget)
    assert np.array_equal(small, np.arange(100, dtype=np.float32))
    assert sum(bench.DUMP_BUDGET.values()) <= 64e6


def test_bench_world_size_mismatch_is_an_error():
    r = _run(["--stub", "--gpus", "4", "--steps", "1"], env={"WORLD_SIZE": "2"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)
