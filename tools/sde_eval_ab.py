#!/usr/bin/env python
"""PPO's update-time gSDE head (DeviceSDE.evaluate: one HIP launch forward, two backward) against the torch head of
examples/ppo_torch.py's update, and one whole update() with and without --eval-kernel.

    python tools/sde_eval_ab.py [--rounds 7] [--out profiles/sde_eval_ab.json]

One process, one stream, HIP events; the legs alternate every round (tools/sde_squash_ab.py's harness).  Inputs
resident in HBM (lat = relu(randn), log_std around -2, A = 2, ratios around 1 on both sides of the clip bounds).

head      one minibatch's policy loss with its backward, per call: mean and log_std are leaves, the latent is
          detached (PPO's learn_features=False), loss = -surrogate.mean(), loss.backward()
  (a) fused   head.evaluate(mean, lat, log_std.exp(), actions, old_log_prob, advantages, clip)
  (b) torch   (lat * lat) @ (log_std.exp() ** 2), Normal(mean, sqrt(var + 1e-6)).log_prob(actions).sum(-1),
              exp, clamp, min, mean
          at (4 096 rows, L = 256), the example's minibatch, and (65 536 rows, L = 256).
update    PPO.update() of --fused --frames --sde-kernel at 4 096 envs x 32 steps, batch 4 096 (320 minibatches:
          gather, both networks, the head, Adam), after one rollout, with and without --eval-kernel; ms per update.

"queued": the same launches issued behind some 10 ms of other work on the stream, so the events time the kernels
back to back and not the host's launch rate.  Where the plain median is well above the queued one
(plain_at_host_call_rate), the plain figure is the host's call rate and says nothing about the kernels.
bytes: what a call must move at least (the latent read once each way, the partials of g_std written and read) over
the queued time, against the 8 TB/s peak.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gym-usv_amd"), os.path.join(ROOT, "examples"), os.path.dirname(os.path.abspath(__file__))]

import sde_squash_ab as S  # noqa: E402

A, L, CLIP = 2, 256, 0.2
SDE_EPS = 1e-6
PEAK_BYTES_PER_S = 8.0e12


class Inputs:
    def __init__(self, torch, n, dev):
        g = torch.Generator(device=dev).manual_seed(4243)
        r = lambda *s: torch.randn(s, device=dev, generator=g)      # noqa: E731
        self.n = n
        self.lat = torch.relu(r(n, L))
        self.mean = (torch.rand((n, A), device=dev, generator=g) * 2 - 0.5).requires_grad_(True)
        self.log_std = (-2.0 + 0.3 * r(L, A)).requires_grad_(True)
        with torch.no_grad():
            std = self.log_std.exp()
            s2 = (self.lat * self.lat) @ (std * std) + SDE_EPS
            self.act = (self.mean + r(n, A) * s2.sqrt()).contiguous()
            logp = torch.distributions.Normal(self.mean, s2.sqrt(), validate_args=False).log_prob(self.act).sum(-1)
            self.old = (logp + 0.25 * r(n)).contiguous()            # ratios e^(+-0.25): both clip bounds are crossed
        self.adv = r(n)

    def clear(self):
        self.mean.grad = self.log_std.grad = None


class FusedHead:
    def __init__(self, torch, inp, dev):
        from gym_usv_amd import DeviceSDE
        self.inp, self.head = inp, DeviceSDE(inp.n, L, A, dev, 12345, (0.0, -1.0), (1.0, 1.0))

    def call(self):
        inp = self.inp
        inp.clear()
        ev = self.head.evaluate(inp.mean, inp.lat, inp.log_std.exp(), inp.act, inp.old, inp.adv, CLIP)
        (-ev.surrogate.mean()).backward()


class TorchHead:
    def __init__(self, torch, inp, dev):
        self.torch, self.inp = torch, inp

    def call(self):
        torch, inp = self.torch, self.inp
        inp.clear()
        var = (inp.lat * inp.lat) @ (inp.log_std.exp() ** 2)
        logp = torch.distributions.Normal(inp.mean, torch.sqrt(var + SDE_EPS), validate_args=False).log_prob(inp.act).sum(-1)
        ratio = (logp - inp.old).exp()
        (-torch.min(ratio * inp.adv, ratio.clamp(1 - CLIP, 1 + CLIP) * inp.adv).mean()).backward()


class Update:
    """One PPO of examples/ppo_torch.py after one rollout; call() is one update()."""

    def __init__(self, envs, n_steps, batch, eval_kernel):
        import gym_usv_amd
        from ppo_torch import PPO
        self.env = gym_usv_amd.make_vec("usv-simple", envs, seed=0, copy=False)
        self.ppo = PPO(self.env, n_steps=n_steps, batch_size=batch, seed=0, fused=True, frames=True, sde_kernel=True,
                       eval_kernel=eval_kernel)
        self.ppo.rollout()

    def call(self):
        self.ppo.update()


def min_bytes(n):
    P = math.ceil(n / math.ceil(n / 1024))
    return {"forward": 4 * n * L, "backward": 4 * n * L + 2 * 4 * P * L * A}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50, help="calls per round and leg at 4 096 rows")
    ap.add_argument("--big-reps", type=int, default=10, help="the same at 65 536 rows")
    ap.add_argument("--queued-reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--update-rounds", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--n-steps", type=int, default=32)
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sde_eval_ab.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sde_eval_ab.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"what": "interleaved same-process A/B, one stream, HIP events. head: us per call of one minibatch's policy "
                   "loss with its backward (fused = DeviceSDE.evaluate, torch = the ops of examples/ppo_torch.py's update "
                   "under autograd; mean and log_std leaves, latent detached); queued = launches issued behind ~10 ms of "
                   "other work (kernel time, not the host's call rate); plain_at_host_call_rate: the plain median is above "
                   "1.3x the queued one.  update: ms per PPO.update() of --fused --frames --sde-kernel (fused = with "
                   "--eval-kernel).  criterion (max_below_torch_min): the fused leg's slowest round is below the torch "
                   "leg's fastest",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "act_dim": A, "latent_dim": L, "clip": CLIP,
           "head": {}, "update": {}}
    big = torch.randn((8192, 8192), device=dev)

    def behind():
        for _ in range(4):
            torch.mm(big, big)
    for n in (4096, 65536):
        inp = Inputs(torch, n, dev)
        legs = {"fused": FusedHead(torch, inp, dev), "torch": TorchHead(torch, inp, dev)}
        entry = S.measure(torch, legs, args, behind, 1, args.big_reps if n >= 65536 else args.reps)
        entry["rows"] = n
        entry["fused"]["scratch_bytes"] = 4 * math.ceil(n / math.ceil(n / 1024)) * L * A
        if n >= 65536:
            b = min_bytes(n)
            t = entry["fused"]["queued"]["median_us"] * 1e-6
            rate = (b["forward"] + b["backward"]) / t
            entry["fused"]["min_bytes"] = b
            entry["fused"]["queued_bytes_per_s"] = round(rate)
            entry["fused"]["queued_share_of_8TBps"] = round(rate / PEAK_BYTES_PER_S, 4)
        res["head"][f"{n}x{L}"] = entry
        print(json.dumps({"head": {f"{n}x{L}": entry}}), flush=True)
        del legs, inp
        torch.cuda.empty_cache()
    del big
    torch.cuda.empty_cache()
    legs = {"fused": Update(args.envs, args.n_steps, args.batch_size, True),
            "torch": Update(args.envs, args.n_steps, args.batch_size, False)}
    for leg in legs.values():
        S.run_events(torch, leg, 1)                        # warm-up: one whole update
    ms = {k: [] for k in legs}
    for _ in range(args.update_rounds):
        for k, leg in legs.items():
            ms[k].append(S.run_events(torch, leg, 1) * 1e-3)
    M = args.envs * args.n_steps
    entry = {k: {"median_ms": round(sorted(v)[len(v) // 2], 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                 "rounds_ms": [round(x, 3) for x in v]} for k, v in ms.items()}
    entry["fused"]["torch_over_this_median"] = round(entry["torch"]["median_ms"] / entry["fused"]["median_ms"], 3)
    entry["fused"]["max_below_torch_min"] = entry["fused"]["max_ms"] < entry["torch"]["min_ms"]
    entry.update(envs=args.envs, n_steps=args.n_steps, batch_size=args.batch_size,
                 minibatches=10 * math.ceil(M / args.batch_size))
    res["update"][f"{args.envs}x{args.n_steps}"] = entry
    print(json.dumps({"update": entry}), flush=True)
    for leg in legs.values():
        leg.env.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
