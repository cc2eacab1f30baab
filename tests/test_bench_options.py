"""bench.py's command line without a GPU: argument checks and the --dump-outputs writer (bench.dump_outputs)."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env,
                          cwd=ROOT, timeout=120)


def test_help_lists_full_and_dump_outputs():
    r = _bench(["--help"])
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_steps_below_one_is_refused():
    for args in (["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]):
        r = _bench(args)
        assert r.returncode == 2 and "--steps must be at least 1" in r.stderr, args


def test_dump_outputs_writes_float32_in_full_when_it_fits(tmp_path):
    import bench
    y = torch.randn(4, 3, 8, 8, dtype=torch.bfloat16)
    info = bench.dump_outputs({"normal": y}, str(tmp_path))
    a = np.load(tmp_path / "normal.npy")
    assert a.dtype == np.float32 and a.shape == (4, 3, 8, 8)
    assert np.array_equal(a, y.float().numpy())                  # bf16 -> fp32 is exact
    assert info == {"normal": {"shape": [4, 3, 8, 8], "images": "all"}}


def test_dump_outputs_cuts_to_a_fixed_seeded_subset_within_the_budget(tmp_path):
    import bench
    g = torch.Generator().manual_seed(3)
    normal = torch.rand(10, 3, 16, 16, generator=g)
    depth = torch.rand(10, 1, 16, 16, generator=g)
    per_image = 4 * (3 + 1) * 16 * 16
    budget = 3 * per_image + 2 * 4096                            # room for three images of both outputs
    info = bench.dump_outputs({"normal": normal, "depth": depth}, str(tmp_path / "a"), budget=budget)
    idx = info["normal"]["images"]
    assert idx == info["depth"]["images"] and len(idx) == 3 and idx == sorted(idx) and len(set(idx)) == 3
    total = 0
    for name, t in (("normal", normal), ("depth", depth)):
        path = tmp_path / "a" / f"{name}.npy"
        total += os.path.getsize(path)
        assert np.array_equal(np.load(path), t[idx].numpy())
    assert total <= budget
    # the same call picks the same images
    again = bench.dump_outputs({"normal": normal, "depth": depth}, str(tmp_path / "b"), budget=budget)
    assert again == info
    assert np.array_equal(np.load(tmp_path / "b" / "normal.npy"), np.load(tmp_path / "a" / "normal.npy"))


def test_dump_outputs_of_the_headline_sizes_stay_under_64_mb():
    import bench
    assert bench.DUMP_BYTES <= 64 * 10 ** 6
    b, hw = 32, 384 * 384
    assert 4 * b * 3 * hw + 4096 <= bench.DUMP_BYTES              # the normal head's batch of 32 is written whole
    keep = (bench.DUMP_BYTES - 2 * 4096) // (4 * 4 * hw)          # dual task: normal + depth per image
    assert 1 <= keep < b
