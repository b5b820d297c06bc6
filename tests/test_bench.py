"""bench.py's plain run (the headline only) and --dump-outputs (what the last timed step computed, as .npy files)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg


def test_dump_outputs_whole_within_budget_and_a_fixed_sample_beyond(tmp_path, monkeypatch):
    import bench

    rng = np.random.RandomState(0)
    arrays = {"render": rng.rand(3, 40, 50).astype(np.float32), "xyz": rng.rand(1000, 3).astype(np.float32),
              "loss": np.array([0.25], np.float32)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    for k, a in arrays.items():
        assert np.array_equal(np.load(tmp_path / "whole" / f"{k}.npy"), a)
    budget = 4000
    monkeypatch.setattr(bench, "DUMP_BYTES", budget)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    s1 = {k: np.load(tmp_path / "s1" / f"{k}.npy") for k in arrays}
    s2 = {k: np.load(tmp_path / "s2" / f"{k}.npy") for k in arrays}
    assert sum(a.nbytes for a in s1.values()) <= budget
    assert all(np.array_equal(s1[k], s2[k]) for k in arrays)  # the same sample every run
    assert np.isin(s1["xyz"], arrays["xyz"]).all() and s1["loss"][0] == 0.25 and s1["render"].dtype == np.float32


@pytest.mark.gpu
def test_plain_bench_times_its_steps_and_dumps_the_last_one(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DGM_BENCH_SHARE_GPU")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--workload", "cfg1", "--dump-outputs", str(tmp_path)], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["steps"] == 3 and rec["unit"] == "it/s" and rec["higher_is_better"] is True and rec["dtype"].startswith("f32")
    assert rec["ms_per_step"] > 0 and abs(rec["value"] * rec["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert not {"kernels", "roofline", "steady_state", "cpu_baseline"} & set(rec)  # measured with --full only
    c = pkg("synthetic").CONFIGS["cfg1"]
    files = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64e6
    assert all(a.dtype == np.float32 for a in files.values())
    assert files["render"].shape == (3, c["H"], c["W"]) and files["xyz"].shape == (c["P"], 3)
    assert files["viewspace_points_grad"].shape == (c["P"], 3) and "deform.linear.0.weight" in files
    assert all(np.isfinite(a).all() for a in files.values()) and (files["radii"] > 0).any()
