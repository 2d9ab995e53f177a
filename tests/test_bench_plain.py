"""bench.py without --full: the headline alone, and --dump-outputs.  The helpers on the host; one short run on the GPU."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def _step_result(B, n_agents=2):
    g = torch.Generator().manual_seed(0)
    obs = [torch.rand(B, 5, generator=g) for _ in range(n_agents)]
    rews = [torch.rand(B, generator=g) for _ in range(n_agents)]
    infos = [{"pos_rew": torch.rand(B, generator=g), "not a tensor": 3} for _ in range(n_agents)]
    return obs, rews, torch.arange(B) % 2 == 0, infos


def test_dump_writes_every_returned_array_as_float32(tmp_path):
    import bench

    B = 257
    obs, rews, dones, infos = _step_result(B)
    what = bench.dump_env_outputs(str(tmp_path), ["agent_0", "agent_1"], obs, rews, dones, infos)
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(str(tmp_path / "*.npy")))
    assert names == what["arrays"] == sorted(["done", "obs_agent_0", "obs_agent_1", "reward_agent_0", "reward_agent_1",
                                              "info_agent_0_pos_rew", "info_agent_1_pos_rew"])
    assert what["envs_written"] == B
    for i in (0, 1):
        got = np.load(tmp_path / f"obs_agent_{i}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, obs[i].numpy())
        assert np.array_equal(np.load(tmp_path / f"info_agent_{i}_pos_rew.npy"), infos[i]["pos_rew"].numpy())
    assert np.array_equal(np.load(tmp_path / "done.npy"), dones.float().numpy())


def test_dump_above_the_budget_is_the_same_sample_of_environments_every_time(tmp_path, monkeypatch):
    import bench

    B = 1000
    obs, rews, dones, infos = _step_result(B)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 20000)
    for d in ("a", "b"):
        what = bench.dump_env_outputs(str(tmp_path / d), ["agent_0", "agent_1"], obs, rews, dones, infos)
    assert 0 < what["envs_written"] < B
    idx = np.load(tmp_path / "a" / "env_index.npy")
    assert idx.dtype == np.float64 and len(idx) == what["envs_written"] and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "b" / "env_index.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "obs_agent_1.npy"), obs[1].numpy()[idx.astype(np.int64)])
    payload = sum(np.load(p).nbytes for p in glob.glob(str(tmp_path / "a" / "*.npy")))
    assert payload <= 20000


def test_full_and_dump_outputs_are_options_and_off_by_default(monkeypatch):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    a = bench.parse_args()
    assert not a.full and a.dump_outputs is None and a.steps == 20 and a.warmup == 5
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "somewhere"


@pytest.mark.gpu
def test_plain_bench_line_and_outputs(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W --dump-outputs DIR`: one window of exactly N steps, the six fields of the
    headline, none of the objects that --full adds, and the last step's outputs on disk."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                          "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["metric"].startswith("env-steps/sec") and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 20 and d["warmup"] == 5
    assert d["repeats"]["windows"] == 1 and d["repeats"]["steps_per_window"] == 20
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(d["config"]["global_envs"] * d["config"]["substeps"] / (d["ms_per_step"] * 1e-3), rel=1e-6)
    for moved in ("environment_step", "persistent_rollout", "other_configs", "attached_reference", "cpu_baseline", "cpu_port",
                  "parity", "single_queue"):
        assert moved not in d
    files = glob.glob(str(tmp_path / "*.npy"))
    assert files and sum(os.path.getsize(p) for p in files) <= 64 << 20
    B = d["config"]["num_envs_per_gpu"]
    for p in files:
        x = np.load(p)
        assert x.dtype == np.float32 and x.shape[0] == B and np.isfinite(x).all(), p
    if "headline" in d:  # through the reference's Environment.step: what it returned
        assert "world_step" not in d
        assert {"done", "obs_agent_0", "reward_agent_0"} <= {os.path.basename(p)[:-4] for p in files}
    else:  # the reference is not importable on this machine: World.step alone is the headline, and the line says so
        assert "headline_fallback" in d and [os.path.basename(p) for p in files] == ["state.npy"]
