#!/usr/bin/env python
"""Fused wrappers (DeviceWrappers: one HIP launch per step) against the torch wrappers they replace.

    python tools/wrap_ab.py [--norm] [--rounds 7] [--steps 1000] [--out profiles/wrap_step_ab.json]

One process, one stream, HIP events; the legs of a comparison alternate every round.  k = 5, D = 143,
scripted inputs resident in HBM (a pool of steps; done rate 1/216 per env and step, the workload's):
  (a) torch    DeviceFrameStack.step(obs, done, final_obs) + the ep_ret / ep_len bookkeeping of
               examples/ppo_torch.py (:158-164), host syncs included -- existing code, the yardstick
  (b) fused    DeviceWrappers.step(obs, rew, done, final_obs)
at 65 536 and 4 096 envs, and
  (c) Sb3VecEnv.step with fused=False and fused=True at 4 096 envs (usv-simple, frame_stack=5; host
      clock around the call, which ends in the adapter's own synchronise).
With --norm (its own record, profiles/wrap_norm_ab.json) the legs are instead, at both sizes,
  (n) fused+norm  DeviceWrappers(normalize={}).step: VecFrameStack(VecNormalize(.)) in three launches
  (b) fused       as above, without normalisation: (n) - (b) is what the feature costs
  (t) torch norm  VecNormalize restated in torch ops over DeviceFrameStack, what a user would write
                  instead: obs.double().mean(0), var(0, unbiased=False), the merge, the elementwise ops
and the extra time (n) - (b) is set against the time to read the obs once more at the rate (b) reaches.
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


class FusedNormLeg(FusedLeg):
    """(n)"""

    def __init__(self, torch, n, inp, dev):
        from gym_usv_amd.wrappers import DeviceWrappers
        self.inp = inp
        self.wr = DeviceWrappers(n, D, K, dev, torch.float32, normalize={})
        self.wr.reset(inp.obs[0])
        self.t = 0


class TorchNormLeg:
    """(t): RunningMeanStd + VecNormalize.step_wait in torch ops, then DeviceFrameStack."""

    def __init__(self, torch, n, inp, dev):
        from gym_usv_amd.sb3 import DeviceFrameStack
        self.torch, self.inp, self.n = torch, inp, n
        f8 = dict(dtype=torch.float64, device=dev)
        self.mean, self.var, self.count = torch.zeros(D, **f8), torch.ones(D, **f8), 1e-4
        self.rmean, self.rvar, self.rcount = torch.zeros((), **f8), torch.ones((), **f8), 1e-4
        self.returns = torch.zeros(n, **f8)
        self.fs = DeviceFrameStack(n, D, K, dev)
        self.fs.reset(inp.obs[0])
        self.t = 0

    @staticmethod
    def merge(mean, var, count, x):
        bm, bv, n = x.mean(0), x.var(0, unbiased=False), x.shape[0]
        delta, tot = bm - mean, count + n
        m2 = var * count + bv * n + delta.square() * count * n / tot
        return mean + delta * n / tot, m2 / tot, tot

    def norm_obs(self, x):
        return ((x.double() - self.mean) / (self.var + 1e-8).sqrt()).clamp(-10.0, 10.0).float()

    def step(self):
        i = self.t % self.inp.pool
        self.t += 1
        obs, rew, done, final = self.inp.obs[i], self.inp.rew[i], self.inp.done[i], self.inp.final[i]
        self.mean, self.var, self.count = self.merge(self.mean, self.var, self.count, obs.double())
        self.returns = self.returns * 0.99 + rew.double()
        self.rmean, self.rvar, self.rcount = self.merge(self.rmean, self.rvar, self.rcount, self.returns)
        nrew = (rew.double() / (self.rvar + 1e-8).sqrt()).clamp(-10.0, 10.0).float()
        self.returns = self.returns * (~done)
        out = self.fs.step(self.norm_obs(obs), done, self.norm_obs(final))
        return out, nrew


def norm_main(torch, args, dev):
    """The three legs of --norm; writes args.out."""
    res = {"what": "interleaved same-process A/B, one stream, HIP-event time per step: fused_norm = "
                   "DeviceWrappers(normalize={}).step (partial moments, finalise, normalising step); fused = "
                   "DeviceWrappers.step without normalisation; torch_norm = VecNormalize restated in torch ops + "
                   "DeviceFrameStack.step",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "n_stack": K, "obs_dim": D,
           "done_rate": DONE_RATE, "normalize": {}}
    for n in (65536, 4096):
        inp = Inputs(torch, n, 8 if n > 4096 else 32, dev)
        legs = {"fused_norm": FusedNormLeg(torch, n, inp, dev), "fused": FusedLeg(torch, n, inp, dev),
                "torch_norm": TorchNormLeg(torch, n, inp, dev)}
        for leg in legs.values():
            run_events(torch, leg, args.warmup)
        ev = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                ev[k].append(run_events(torch, leg, args.steps)[0])
        entry = {k: summary(v) for k, v in ev.items()}
        fused, fn = entry["fused"]["median_us"], entry["fused_norm"]["median_us"]
        rate = fused_bytes_per_env_step() * n / (fused * 1e-6)           # B/s the unnormalised step reaches
        reread = D * 4 * n / rate * 1e6                                  # us to read the obs once more at it
        entry["steps_per_round"] = args.steps
        entry["extra_us"] = round(fn - fused, 3)
        entry["extra_us_spread"] = [round(min(ev["fused_norm"]) - max(ev["fused"]), 3),
                                    round(max(ev["fused_norm"]) - min(ev["fused"]), 3)]
        entry["fused_bytes_per_s"] = round(rate, 1)
        entry["obs_reread_us_at_fused_rate"] = round(reread, 3)
        entry["extra_over_reread"] = round((fn - fused) / reread, 2)
        entry["torch_norm_over_fused_norm_median"] = round(entry["torch_norm"]["median_us"] / fn, 2)
        res["normalize"][str(n)] = entry
        print(json.dumps({f"normalize_{n}": entry}), flush=True)
        del legs, inp
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


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
    ap.add_argument("--norm", action="store_true", help="the VecNormalize legs (profiles/wrap_norm_ab.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "wrap_norm_ab.json" if args.norm else "wrap_step_ab.json")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wrap_ab.py needs a GPU")
    dev = torch.device("cuda", 0)
    if args.norm:
        return norm_main(torch, args, dev)
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
