"""bench.py's plain run, --full and --dump-outputs: what a plain run leaves out, the row sample and the
files of a dump (CPU), and on the GPU that two runs with the same arguments write the same arrays."""
import json
import os

import numpy as np
import pytest
import torch

import bench

NAMES = ("obs", "reward", "terminated", "truncated", "final_obs")


class _Event:
    t = 0.0

    def record(self):
        pass

    def elapsed_time(self, other):
        return 1.0

    def synchronize(self):
        pass


class _CountingWorkload:
    """CPU stand-in for bench.StepWorkload that counts what run() asks of it."""

    def __init__(self, args, rank, local):
        self.N, self.mean_obs, self.collective_device = args.envs, 20.0, None
        self.launches, self.extras_calls = [], 0
        _CountingWorkload.last = self

    def launch(self, k):
        self.launches.append(k)

    def sync(self):
        pass

    def event(self):
        return _Event()

    def outputs(self):
        n = self.N
        return {"obs": torch.full((n, 3), float(len(self.launches))), "reward": torch.arange(n, dtype=torch.float32),
                "terminated": torch.zeros(n, dtype=torch.uint8), "truncated": torch.ones(n, dtype=torch.uint8),
                "final_obs": torch.zeros(n, 3)}

    def extras(self):
        self.extras_calls += 1
        return {"f64": {"dtype": "f64"}, "api_step": {"steps": 1}}

    def close(self):
        pass


def _run(argv, capsys):
    out = bench.run(bench.parse_args(argv), 0, 1, 0, workload_cls=_CountingWorkload)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == json.loads(json.dumps(out))
    return out, _CountingWorkload.last


def test_plain_run_times_only_the_headline(capsys, tmp_path):
    """Without --full: W warm-up steps, the clock warm-up (a count that follows from the arguments), K
    timed steps, each with the next actions; no steady / f64 / API / CPU leg; the line keeps every key
    (the legs null)."""
    assert bench.clock_warmup_steps(0.3, 65536) == 16022 and bench.clock_warmup_steps(0, 65536) == 0
    d, wl = _run(["--steps", "9", "--warmup", "4", "--envs", "100", "--clock-warmup", "1e-6",
                  "--dump-outputs", str(tmp_path)], capsys)
    assert d["clock_warmup_steps"] == bench.clock_warmup_steps(1e-6, 100) == 35
    assert wl.launches == list(range(4 + 35 + 9))
    assert wl.extras_calls == 0
    assert d["steps"] == 9 and d["warmup"] == 4 and d["ms_per_step"] > 0 and d["dtype"] == "f32"
    assert d["f64"] is None and d["api_step"] is None and d["cpu_baseline"] is None
    assert d["roofline"]["steady"] is None and d["roofline"]["kernel_ms"] > 0
    # the dump is taken right after the last timed launch
    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}.npy" for k in NAMES)
    assert np.load(tmp_path / "obs.npy")[0, 0] == len(wl.launches)


def test_full_run_adds_the_other_legs(capsys, tmp_path):
    """--full: the steady launches and extras() run after the dump was taken; each leg's own switch
    still turns it off."""
    d, wl = _run(["--full", "--steps", "5", "--warmup", "2", "--envs", "100", "--clock-warmup", "0",
                  "--steady-steps", "7", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)], capsys)
    assert d["clock_warmup_steps"] == 0 and len(wl.launches) == 2 + 5 + 7 and wl.extras_calls == 1
    assert d["f64"] == {"dtype": "f64"} and d["api_step"] == {"steps": 1} and d["cpu_baseline"] is None
    assert d["roofline"]["steady"]["launches"] == 7
    assert np.load(tmp_path / "obs.npy")[0, 0] == 2 + 5


def test_dump_rows_sample():
    """All rows when they fit; else a sorted sample without repeats, the same every time, that fills the
    budget and no more.  The default workload (65 536 envs x 143 obs) needs the sample."""
    assert bench.dump_rows(1000, 1156) is None
    assert bench.dump_rows(10, 100, budget=1000) is None
    row = 2 * 143 * 4 + 3 * 4
    r = bench.dump_rows(65536, row)
    assert r is not None and len(r) == bench.DUMP_BYTES // row < 65536
    assert np.all(np.diff(r) > 0) and r[0] >= 0 and r[-1] < 65536
    assert np.array_equal(r, bench.dump_rows(65536, row))
    assert len(r) * row + 5 * 128 <= 64 * 10**6


def test_dump_outputs_files(tmp_path):
    """float32 files (float64 kept), flags as 0/1, every array cut to the same rows."""
    n = 50
    outs = {"obs": torch.arange(n * 4, dtype=torch.float32).reshape(n, 4),
            "reward": torch.arange(n, dtype=torch.float64) / 3,
            "terminated": (torch.arange(n) % 2).to(torch.uint8)}
    bench.dump_outputs(outs, str(tmp_path / "all"))
    got = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in outs}
    assert got["obs"].dtype == np.float32 and got["reward"].dtype == np.float64
    assert got["terminated"].dtype == np.float32 and set(np.unique(got["terminated"])) == {0.0, 1.0}
    for k in outs:
        assert np.array_equal(got[k], outs[k].numpy())
    # a budget of 10 rows
    rows = bench.dump_rows(n, 4 * 4 + 8 + 4, budget=10 * 28)
    assert len(rows) == 10
    bench.dump_outputs(outs, str(tmp_path / "cut"), rank=1, budget=10 * 28)
    for k in outs:
        assert np.array_equal(np.load(tmp_path / "cut" / f"{k}.rank1.npy"), outs[k].numpy()[rows])


@pytest.mark.gpu
def test_dump_is_the_last_timed_step_and_repeats(capsys, tmp_path):
    """Two plain runs with the same arguments dump identical arrays, and they are what stepping a fresh
    env W + clock warm-up + K times with the bench's actions gives.  4 099 envs (an odd count, more than
    one block); some episodes of a random rollout end in the last step and most do not, so final_obs has
    rows of both kinds."""
    import gym_usv_amd
    n, W, K = 4099, 3, 37
    C = bench.clock_warmup_steps(1e-5, n)
    assert C == 9
    argv = ["--steps", str(K), "--warmup", str(W), "--envs", str(n), "--seed", "5", "--clock-warmup", "1e-5"]
    dumps = []
    for i in range(2):
        args = bench.parse_args(argv + ["--dump-outputs", str(tmp_path / str(i))])
        d = bench.run(args, 0, 1, 0)
        assert d["steps"] == K and d["clock_warmup_steps"] == C
        assert d["f64"] is None and d["api_step"] is None and d["cpu_baseline"] is None
        dumps.append({k: np.load(tmp_path / str(i) / f"{k}.npy") for k in NAMES})
    capsys.readouterr()
    for k in NAMES:
        assert dumps[0][k].dtype == np.float32 and len(dumps[0][k]) == n
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
    # the same rollout through the public API
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(5 * 7919)
    acts = torch.rand((K, n, 2), device=dev, generator=gen) * torch.tensor([0.8, 2.0], device=dev) \
        + torch.tensor([0.2, -1.0], device=dev)
    env = gym_usv_amd.make_vec("usv-simple", n, device=0, seed=5, copy=False)
    env.reset(seed=5)
    for k in range(W + C + K):
        obs, rew, term, trunc, info = env.step(acts[k % K])
    torch.cuda.synchronize()
    done = info["_final_obs"]
    assert 0 < int(done.sum()) < n
    want = {"obs": obs, "reward": rew, "terminated": term, "truncated": trunc,
            "final_obs": torch.where(done[:, None], info["final_obs"], torch.zeros_like(obs))}
    for k in NAMES:
        assert np.array_equal(dumps[0][k], want[k].float().cpu().numpy()), k
    env.close()
