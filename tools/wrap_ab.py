#!/usr/bin/env python
"""Fused wrappers (DeviceWrappers: one HIP launch per step) against the torch wrappers they replace.

    python tools/wrap_ab.py [--rounds 7] [--steps 1000] [--out profiles/wrap_step_ab.json]

One process, one stream, HIP events; the legs of a comparison alternate every round.  k = 5, D = 143,
scripted inputs resident in HBM (a pool of steps; done rate 1/216 per env and step, the workload's):
  (a) torch    DeviceFrameStack.step(obs, done, final_obs) + the ep_ret / ep_len bookkeeping of
               examples/ppo_torch.py (:158-164), host syncs included -- existing code, the yardstick
  (b) fused    DeviceWrappers.step(obs, rew, done, final_obs)
at 65 536 and 4 096 envs, and
  (c) Sb3VecEnv.step with fused=False and fused=True at 4 096 envs (usv-simple, frame_stack=5; host
      clock around the call, which ends in the adapter's own synchronise).
Per leg: median and min..max over the rounds of the time per step.  (b)'s algorithmic bytes per env
(obs read, ring written 2 - 1/k times, reward, done flag, the two counters read and written) and the HBM
fraction they give at the median are reported too.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-usv_amd"))

K, D = 5, 143
DONE_RATE = 1.0 / 216
PEAK = 8.0e12      # HBM3E peak, B/s (MI355X)


def fused_bytes_per_env_step(k=K, d=D, reward_bytes=4):
    """obs row read; ring written once or twice (the mirror is skipped one step in k); reward, done flag,
    ep_ret (f64) and ep_len (i32) read and written.  Done envs' rows (1 in 216) are not counted."""
    return d * 4 + d * 4 * (2 * k - 1) / k + reward_bytes + 1 + 2 * (8 + 4)


class Inputs:
    def __init__(self, torch, n, pool, dev):
        g = torch.Generator(device=dev).manual_seed(4242)
        self.obs = torch.randn((pool, n, D), device=dev, generator=g)
        self.final = torch.randn((pool, n, D), device=dev, generator=g)
        self.rew = torch.randn((pool, n), device=dev, generator=g)
        self.done = torch.rand((pool, n), device=dev, generator=g) < DONE_RATE
        self.pool = pool


class TorchLeg:
    """(a): the code a user of UsvVectorEnv writes today."""

    def __init__(self, torch, n, inp, dev):
        from gym_usv_amd.sb3 import DeviceFrameStack
        self.torch, self.inp = torch, inp
        self.fs = DeviceFrameStack(n, D, K, dev)
        self.fs.reset(inp.obs[0])
        self.ep_ret = torch.zeros(n, device=dev)
        self.ep_len = torch.zeros(n, device=dev)
        self.finished = []
        self.t = 0

    def step(self):
        torch, i = self.torch, self.t % self.inp.pool
        self.t += 1
        obs, rew, done, final = self.inp.obs[i], self.inp.rew[i], self.inp.done[i], self.inp.final[i]
        out = self.fs.step(obs, done, final)
        self.ep_ret += rew.float()
        self.ep_len += 1
        if bool(done.any()):
            d = done.nonzero().flatten()
            self.finished.append(torch.stack((self.ep_ret[d], self.ep_len[d]), 1))
            self.ep_ret[d] = 0
            self.ep_len[d] = 0
        if len(self.finished) > 256:
            self.finished.clear()
        return out


class FusedLeg:
    """(b)"""

    def __init__(self, torch, n, inp, dev):
        from gym_usv_amd.wrappers import DeviceWrappers
        self.inp = inp
        self.wr = DeviceWrappers(n, D, K, dev, torch.float32)
        self.wr.reset(inp.obs[0])
        self.t = 0

    def step(self):
        i = self.t % self.inp.pool
        self.t += 1
        return self.wr.step(self.inp.obs[i], self.inp.rew[i], self.inp.done[i], self.inp.final[i])


class AdapterLeg:
    """(c)"""

    def __init__(self, torch, n, fused):
        import numpy as np
        from gym_usv_amd.sb3 import Sb3VecEnv
        self.env = Sb3VecEnv("usv-simple", num_envs=n, frame_stack=K, seed=0, fused=fused)
        self.env.reset()
        rng = np.random.default_rng(0)
        self.acts = rng.uniform([0.2, -1], [1, 1], size=(16, n, 2)).astype(np.float32)
        self.t = 0

    def step(self):
        self.t += 1
        return self.env.step(self.acts[self.t % 16])


def run_events(torch, leg, steps):
    """HIP-event and host-clock us per step of `steps` back-to-back steps of a device-side leg."""
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record(s)
    for _ in range(steps):
        leg.step()
    b.record(s)
    b.synchronize()
    t1 = time.perf_counter()
    return a.elapsed_time(b) * 1e3 / steps, (t1 - t0) * 1e6 / steps


def run_host(torch, leg, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        leg.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def summary(xs):
    return {"median_us": round(statistics.median(xs), 3), "min_us": round(min(xs), 3), "max_us": round(max(xs), 3),
            "rounds_us": [round(x, 3) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--adapter-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wrap_step_ab.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wrap_ab.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"what": "interleaved same-process A/B, one stream: (a) DeviceFrameStack.step + ppo_torch.py's ep_ret / "
                   "ep_len bookkeeping (torch ops, host syncs), (b) DeviceWrappers.step (one HIP launch), HIP-event "
                   "time per step; (c) Sb3VecEnv.step fused=False / True, host clock per call",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "n_stack": K, "obs_dim": D,
           "done_rate": DONE_RATE, "peak_bytes_per_s": PEAK, "wrappers": {}, "adapter": {}}
    for n in (65536, 4096):
        inp = Inputs(torch, n, 8 if n > 4096 else 32, dev)
        legs = {"torch": TorchLeg(torch, n, inp, dev), "fused": FusedLeg(torch, n, inp, dev)}
        for leg in legs.values():
            run_events(torch, leg, args.warmup)
        ev = {k: [] for k in legs}
        host = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                e, h = run_events(torch, leg, args.steps)
                ev[k].append(e)
                host[k].append(h)
        entry = {k: dict(summary(ev[k]), host_us=round(statistics.median(host[k]), 3)) for k in legs}
        b = fused_bytes_per_env_step()
        f = entry["fused"]
        f["algorithmic_bytes_per_env"] = round(b, 1)
        f["achieved_bytes_per_s"] = round(b * n / (f["median_us"] * 1e-6), 1)
        f["hbm_roofline_frac"] = round(b * n / (f["median_us"] * 1e-6) / PEAK, 4)
        entry["steps_per_round"] = args.steps
        entry["torch_over_fused_median"] = round(entry["torch"]["median_us"] / f["median_us"], 2)
        entry["fused_max_below_torch_min"] = f["max_us"] < entry["torch"]["min_us"]
        res["wrappers"][str(n)] = entry
        print(json.dumps({f"wrappers_{n}": entry}), flush=True)
        del legs, inp
        torch.cuda.empty_cache()
    n = 4096
    legs = {"unfused": AdapterLeg(torch, n, False), "fused": AdapterLeg(torch, n, True)}
    for leg in legs.values():
        run_host(torch, leg, 50)
    hs = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, leg in legs.items():
            hs[k].append(run_host(torch, leg, args.adapter_steps))
    entry = {k: summary(v) for k, v in hs.items()}
    entry["steps_per_round"] = args.adapter_steps
    entry["fused_median_not_above_unfused_max"] = entry["fused"]["median_us"] <= entry["unfused"]["max_us"]
    entry["fused_over_unfused_median"] = round(entry["fused"]["median_us"] / entry["unfused"]["median_us"], 3)
    res["adapter"][str(n)] = entry
    print(json.dumps({f"adapter_{n}": entry}), flush=True)
    for leg in legs.values():
        leg.env.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
