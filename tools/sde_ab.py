#!/usr/bin/env python
"""Fused gSDE head (DeviceSDE.sample: one HIP launch, no exploration matrix in memory) against the torch
head of examples/ppo_torch.py's rollout_fused that it replaces.

    python tools/sde_ab.py [--rounds 7] [--out profiles/sde_ab.json]

One process, one stream, HIP events; the legs alternate every round.  L = 256, A = 2, inputs resident in
HBM (lat = relu(randn), log_std around -2).  A leg is one sde_sample_freq = 4 cycle of four calls; times
are per call, so the torch leg's sample_weights is amortised over the four steps it serves:
  (a) fused   head.reset_noise() on the first call of the cycle (a host integer), then per call
              log_std.exp() and head.sample(mean, lat, std)
  (b) torch   sample_weights(N) on the first call of the cycle (randn [N, 256, 2] * std), then per call
              the lines of rollout_fused: bmm, the variance matmul, sqrt, Normal.log_prob(a).sum(-1),
              a.contiguous() and the two clamps -- existing code, the yardstick
at 65 536 and 4 096 envs.  "queued": the same launches issued behind some 10 ms of other work on the
stream, so the events time the kernels back to back and not the host's launch rate.  Then one whole
--fused --frames rollout of examples/ppo_torch.py (usv-simple, policy MLP, env step, wrappers, rollout
buffer) with and without --sde-kernel, two PPO objects in this process, interleaved.  Needs a GPU; there
is no fallback.

    python tools/sde_ab.py --libs NAME=PATH [NAME=PATH ...] --out profiles/sde_ab_builds.json

Builds of the library against each other (tools/ab_libs.sh style: each its own ctypes handle): the fused leg
alone at 65 536 envs, plain and pre-queued, interleaved over the rounds.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gym-usv_amd"), os.path.join(ROOT, "examples")]

L, A, FREQ = 256, 2, 4
PEAK = 8.0e12      # HBM3E peak, B/s (MI355X)
SDE_EPS = 1e-6
LOW, HIGH = (0.0, -1.0), (1.0, 1.0)


def fused_bytes_per_env():
    """sample: the latent row and the mean read once; action, clipped action and log-probability written."""
    return 4 * (L + A + 2 * A + 1)


class Inputs:
    def __init__(self, torch, n, dev):
        g = torch.Generator(device=dev).manual_seed(4242)
        self.lat = torch.relu(torch.randn((n, L), device=dev, generator=g))
        self.mean = torch.rand((n, A), device=dev, generator=g) * 2 - 0.5
        self.log_std = -2.0 + 0.3 * torch.randn((L, A), device=dev, generator=g)
        self.lo = torch.tensor(LOW, device=dev)
        self.hi = torch.tensor(HIGH, device=dev)


class FusedLeg:
    def __init__(self, torch, n, inp, dev, lib_path=None):
        from gym_usv_amd import DeviceSDE
        self.inp = inp
        self.head = DeviceSDE(n, L, A, dev, 12345, LOW, HIGH, lib_path=lib_path)

    def rollout(self):
        inp, head = self.inp, self.head
        for t in range(FREQ):
            if t == 0:
                head.reset_noise()
            out = head.sample(inp.mean, inp.lat, inp.log_std.exp())
        return out


class TorchLeg:
    """rollout_fused's gSDE lines (ActorCritic.dist's variance and Normal, sample_weights, the bmm, the clamps)."""

    def __init__(self, torch, n, inp, dev):
        self.torch, self.inp, self.n = torch, inp, n
        self.W = None

    def rollout(self):
        torch, inp = self.torch, self.inp
        for t in range(FREQ):
            if t == 0:
                std = inp.log_std.exp()
                self.W = torch.randn((self.n,) + tuple(std.shape), device=std.device) * std
            var = (inp.lat * inp.lat) @ (inp.log_std.exp() ** 2)
            dist = torch.distributions.Normal(inp.mean, torch.sqrt(var + SDE_EPS), validate_args=False)
            a = dist.mean + torch.bmm(inp.lat.unsqueeze(1), self.W).squeeze(1)
            out = (a.contiguous(), torch.max(torch.min(a, inp.hi), inp.lo), dist.log_prob(a).sum(-1))
        return out


class TorchPart(TorchLeg):
    """One piece of the torch leg on its own, four times per cycle, to say where its time goes:
    "weights" = sample_weights, "bmm" = mean + bmm, "rest" = variance, sqrt, log_prob, sum, clamps, contiguous."""

    def __init__(self, torch, n, inp, dev, part):
        super().__init__(torch, n, inp, dev)
        self.part = part
        std = inp.log_std.exp()
        self.W = torch.randn((n,) + tuple(std.shape), device=dev) * std
        self.a = inp.mean + torch.bmm(inp.lat.unsqueeze(1), self.W).squeeze(1)

    def rollout(self):
        torch, inp = self.torch, self.inp
        for t in range(FREQ):
            if self.part == "weights":
                std = inp.log_std.exp()
                out = torch.randn((self.n,) + tuple(std.shape), device=std.device) * std
            elif self.part == "bmm":
                out = inp.mean + torch.bmm(inp.lat.unsqueeze(1), self.W).squeeze(1)
            else:
                a = self.a
                var = (inp.lat * inp.lat) @ (inp.log_std.exp() ** 2)
                dist = torch.distributions.Normal(inp.mean, torch.sqrt(var + SDE_EPS), validate_args=False)
                out = (a.contiguous(), torch.max(torch.min(a, inp.hi), inp.lo), dist.log_prob(a).sum(-1))
        return out


class RolloutLeg:
    """One rollout of examples/ppo_torch.py's PPO(fused=True, frames=True)."""

    def __init__(self, n, T, sde_kernel):
        import gym_usv_amd
        from ppo_torch import PPO
        self.env = gym_usv_amd.make_vec("usv-simple", n, seed=0, copy=False)
        self.ppo = PPO(self.env, n_steps=T, batch_size=n, seed=0, fused=True, frames=True, sde_kernel=sde_kernel)

    def rollout(self):
        self.ppo.rollout()
        self.ppo.abs_ye = []


def run_events(torch, leg, reps, behind=None):
    """HIP-event us per leg.rollout() of `reps` back-to-back ones; `behind`: see the module docstring."""
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    if behind is not None:
        behind()
    a.record(s)
    for _ in range(reps):
        leg.rollout()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def summary(xs):
    return {"median_us": round(statistics.median(xs), 3), "min_us": round(min(xs), 3), "max_us": round(max(xs), 3),
            "rounds_us": [round(x, 3) for x in xs]}


def versus(this, other, name):
    this[f"{name}_over_this_median"] = round(other["median_us"] / this["median_us"], 2)
    this[f"max_below_{name}_min"] = this["max_us"] < other["min_us"]


def libs_main(torch, args, dev):
    """The fused leg of every build in --libs, same process, interleaved."""
    n = 65536
    res = {"what": "interleaved same-process A/B of builds of the library, one stream, HIP events: DeviceSDE.sample "
                   "over an sde_sample_freq = 4 cycle, us per call; queued = launches issued behind ~10 ms of other work",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "cycles_per_round": args.reps, "envs": n,
           "latent_dim": L, "act_dim": A, "builds": {}}
    big = torch.randn((8192, 8192), device=dev)

    def behind():
        for _ in range(4):
            torch.mm(big, big)
    with torch.no_grad():
        inp = Inputs(torch, n, dev)
        legs = {}
        for spec in args.libs:
            name, path = spec.split("=", 1)
            legs[name] = FusedLeg(torch, n, inp, dev, lib_path=os.path.abspath(path))
            run_events(torch, legs[name], args.warmup)
        ev, queued = {k: [] for k in legs}, {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                ev[k].append(run_events(torch, leg, args.reps) / FREQ)
            for k, leg in legs.items():
                queued[k].append(run_events(torch, leg, 8, behind) / FREQ)
    for k in legs:
        res["builds"][k] = dict(summary(ev[k]), queued=summary(queued[k]))
    print(json.dumps(res["builds"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50, help="four-call cycles per round and leg")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rollout-reps", type=int, default=3, help="whole rollouts per round and leg")
    ap.add_argument("--libs", nargs="+", default=None, metavar="NAME=PATH",
                    help="compare these builds of the library on the fused leg instead")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sde_ab.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sde_ab.py needs a GPU")
    dev = torch.device("cuda", 0)
    if args.libs:
        res = libs_main(torch, args, dev)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", args.out)
        return
    res = {"what": "interleaved same-process A/B, one stream, HIP events, us per call of the gSDE head over an "
                   "sde_sample_freq = 4 cycle: fused = DeviceSDE.sample (reset_noise every 4th call), torch = "
                   "rollout_fused's sample_weights every 4th call + bmm + variance + Normal.log_prob + clamps; "
                   "queued = launches issued behind ~10 ms of other work (kernel time, not the host's call rate); "
                   "rollouts = one whole --fused --frames rollout of examples/ppo_torch.py, us per rollout",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "cycles_per_round": args.reps,
           "latent_dim": L, "act_dim": A, "sde_sample_freq": FREQ, "peak_bytes_per_s": PEAK, "sizes": {}, "rollouts": {}}
    big = torch.randn((8192, 8192), device=dev)

    def behind():
        for _ in range(4):
            torch.mm(big, big)
    with torch.no_grad():
        for n in (65536, 4096):
            inp = Inputs(torch, n, dev)
            legs = {"fused": FusedLeg(torch, n, inp, dev), "torch": TorchLeg(torch, n, inp, dev)}
            for leg in legs.values():
                run_events(torch, leg, args.warmup)
            ev, queued = {k: [] for k in legs}, {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, leg in legs.items():
                    ev[k].append(run_events(torch, leg, args.reps) / FREQ)
                for k, leg in legs.items():
                    queued[k].append(run_events(torch, leg, 8, behind) / FREQ)
            entry = {k: summary(v) for k, v in ev.items()}
            for k, v in queued.items():
                entry[k]["queued"] = summary(v)
            # where the torch leg's time goes: each piece alone, queued, us per execution (sample_weights runs
            # once per four calls in the leg, the other two every call)
            parts = {k: TorchPart(torch, n, inp, dev, k) for k in ("weights", "bmm", "rest")}
            entry["torch"]["parts_queued_us_per_execution"] = {}
            for k, leg in parts.items():
                run_events(torch, leg, 2)
                entry["torch"]["parts_queued_us_per_execution"][k] = summary(
                    [run_events(torch, leg, 4, behind) / FREQ for _ in range(3)])
            del parts
            versus(entry["fused"], entry["torch"], "torch")
            versus(entry["fused"]["queued"], entry["torch"]["queued"], "torch")
            b = fused_bytes_per_env() * n + 4 * L * A
            for e in (entry["fused"], entry["fused"]["queued"]):
                rate = b / (e["median_us"] * 1e-6)
                e["bytes_per_call"] = b
                e["achieved_bytes_per_s"] = round(rate, 1)
                e["hbm_peak_frac"] = round(rate / PEAK, 4)
            entry["torch"]["exploration_matrix_bytes"] = 4 * n * L * A      # allocated by torch, not by fused
            entry["torch"]["bmm_read_bytes_per_call"] = 4 * n * L * (A + 1)
            res["sizes"][str(n)] = entry
            print(json.dumps({str(n): entry}), flush=True)
            del legs, inp
            torch.cuda.empty_cache()
    del big
    torch.cuda.empty_cache()
    for n, T in ((65536, 8), (4096, 32)):
        legs = {"sde_kernel": RolloutLeg(n, T, True), "torch_head": RolloutLeg(n, T, False)}
        for leg in legs.values():
            run_events(torch, leg, 1)
        ev = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                ev[k].append(run_events(torch, leg, args.rollout_reps))
        entry = {k: summary(v) for k, v in ev.items()}
        versus(entry["sde_kernel"], entry["torch_head"], "torch_head")
        entry["n_steps"] = T
        res["rollouts"][f"{n}x{T}"] = entry
        print(json.dumps({f"{n}x{T}": entry}), flush=True)
        for leg in legs.values():
            leg.env.close()
        del legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
