#!/usr/bin/env python
"""Squashed gSDE head (DeviceSDE.squashed: one HIP launch forward, two backward, no exploration matrix in
memory) against a torch-autograd head of the same definition.

    python tools/sde_squash_ab.py [--rounds 7] [--out profiles/sde_squash_ab.json]

One process, one stream, HIP events; the legs alternate every round.  Inputs resident in HBM (lat = relu(randn),
log_std around -3, A = 2).  Two measurements:

update    one SAC actor call with its backward, per call: mean, lat and log_std are leaves,
          loss = (c * actions).sum() + (w * log_prob).sum(), loss.backward()
  (a) fused   head.reset_noise() (a host integer), head.squashed(mean, lat, log_std.exp()), the loss, backward()
  (b) torch   sample_weights by rsample (Normal(0, std).rsample((n,))), bmm(lat[n, 1, L], W[n, L, 2]), the
              variance matmul, tanh, Normal.log_prob minus the tanh correction, the loss, backward()
          at (256 rows, L = 300), the reference configuration's minibatch, and (65 536 rows, L = 256).
collect   the no-grad collection call over an sde_sample_freq = 4 cycle, per call, at 4 096 and 65 536 rows,
          L = 300: fused = reset_noise() every fourth call + squashed under no_grad; torch = sample_weights
          every fourth call + the same lines under no_grad.

"queued": the same launches issued behind some 10 ms of other work on the stream, so the events time the kernels
back to back and not the host's launch rate.  Where the plain median is well above the queued one
(plain_at_host_call_rate), the plain figure is the host's call rate and says nothing about the kernels.  Needs a
GPU; there is no fallback.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gym-usv_amd")]

A, FREQ = 2, 4
SDE_EPS = 1e-6
LOW, HIGH = (0.0, -1.0), (1.0, 1.0)


class Inputs:
    def __init__(self, torch, n, L, dev):
        g = torch.Generator(device=dev).manual_seed(4242)
        self.n, self.L = n, L
        self.lat = torch.relu(torch.randn((n, L), device=dev, generator=g)).requires_grad_(True)
        self.mean = (torch.rand((n, A), device=dev, generator=g) * 2 - 0.5).requires_grad_(True)
        self.log_std = (-3.0 + 0.3 * torch.randn((L, A), device=dev, generator=g)).requires_grad_(True)
        self.c = torch.randn((n, A), device=dev, generator=g)
        self.w = torch.randn((n,), device=dev, generator=g)
        self.lo, self.hi = torch.tensor(LOW, device=dev), torch.tensor(HIGH, device=dev)

    def clear(self):
        self.lat.grad = self.mean.grad = self.log_std.grad = None


def torch_head(torch, inp, W):
    """(actions, env_actions, log_prob) of the squashed head in torch, from the exploration matrices W."""
    std = inp.log_std.exp()
    u = inp.mean + torch.bmm(inp.lat.unsqueeze(1), W).squeeze(1)
    var = (inp.lat * inp.lat) @ (std * std)
    a = torch.tanh(u)
    logp = torch.distributions.Normal(inp.mean, torch.sqrt(var + SDE_EPS), validate_args=False).log_prob(u).sum(-1)
    logp = logp - torch.log(1 - a * a + SDE_EPS).sum(-1)
    return a, inp.lo + (a + 1) * 0.5 * (inp.hi - inp.lo), logp


class FusedUpdate:
    def __init__(self, torch, inp, dev):
        from gym_usv_amd import DeviceSDE
        self.inp, self.head = inp, DeviceSDE(inp.n, inp.L, A, dev, 12345, LOW, HIGH)

    def call(self):
        inp = self.inp
        inp.clear()
        self.head.reset_noise()
        s = self.head.squashed(inp.mean, inp.lat, inp.log_std.exp())
        ((inp.c * s.actions).sum() + (inp.w * s.log_prob).sum()).backward()


class TorchUpdate:
    def __init__(self, torch, inp, dev):
        self.torch, self.inp = torch, inp

    def call(self):
        torch, inp = self.torch, self.inp
        inp.clear()
        W = torch.distributions.Normal(torch.zeros_like(inp.log_std), inp.log_std.exp()).rsample((inp.n,))
        a, _, logp = torch_head(torch, inp, W)
        ((inp.c * a).sum() + (inp.w * logp).sum()).backward()


class FusedCollect:
    def __init__(self, torch, inp, dev):
        from gym_usv_amd import DeviceSDE
        self.torch, self.inp, self.head = torch, inp, DeviceSDE(inp.n, inp.L, A, dev, 12345, LOW, HIGH)

    def call(self):
        inp = self.inp
        with self.torch.no_grad():
            for t in range(FREQ):
                if t == 0:
                    self.head.reset_noise()
                out = self.head.squashed(inp.mean, inp.lat, inp.log_std.exp())
        return out


class TorchCollect:
    def __init__(self, torch, inp, dev):
        self.torch, self.inp = torch, inp

    def call(self):
        torch, inp = self.torch, self.inp
        with torch.no_grad():
            for t in range(FREQ):
                if t == 0:
                    std = inp.log_std.exp()
                    W = torch.randn((inp.n,) + tuple(std.shape), device=std.device) * std
                out = torch_head(torch, inp, W)
        return out


def run_events(torch, leg, reps, behind=None):
    """HIP-event us per leg.call() of `reps` back-to-back ones; `behind`: see the module docstring."""
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    if behind is not None:
        behind()
    a.record(s)
    for _ in range(reps):
        leg.call()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def summary(xs):
    return {"median_us": round(statistics.median(xs), 3), "min_us": round(min(xs), 3), "max_us": round(max(xs), 3),
            "rounds_us": [round(x, 3) for x in xs]}


def measure(torch, legs, args, behind, per_call, reps):
    for leg in legs.values():
        run_events(torch, leg, args.warmup)
    ev, queued = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, leg in legs.items():
            ev[k].append(run_events(torch, leg, reps) / per_call)
        for k, leg in legs.items():
            queued[k].append(run_events(torch, leg, args.queued_reps, behind) / per_call)
    entry = {k: summary(v) for k, v in ev.items()}
    for k, v in queued.items():
        entry[k]["queued"] = summary(v)
        ratio = entry[k]["median_us"] / entry[k]["queued"]["median_us"]
        entry[k]["plain_over_queued_median"] = round(ratio, 2)
        entry[k]["plain_at_host_call_rate"] = ratio > 1.3
    for part in (lambda e: e, lambda e: e["queued"]):
        f, t = part(entry["fused"]), part(entry["torch"])
        f["torch_over_this_median"] = round(t["median_us"] / f["median_us"], 2)
        f["max_below_torch_min"] = f["max_us"] < t["min_us"]
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50, help="calls (update) or four-call cycles (collect) per round and leg")
    ap.add_argument("--big-reps", type=int, default=10, help="the same at 65 536 rows")
    ap.add_argument("--queued-reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sde_squash_ab.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sde_squash_ab.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"what": "interleaved same-process A/B, one stream, HIP events, us per call of the squashed gSDE head: update = "
                   "forward + loss + backward with mean, lat and log_std as leaves (fused = DeviceSDE.squashed, torch = "
                   "rsample + bmm + variance + tanh + log_prob under autograd); collect = the no-grad call over an "
                   "sde_sample_freq = 4 cycle; queued = launches issued behind ~10 ms of other work (kernel time, not the "
                   "host's call rate); plain_at_host_call_rate: the plain median is above 1.3x the queued one",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "act_dim": A, "sde_sample_freq": FREQ,
           "update": {}, "collect": {}}
    big = torch.randn((8192, 8192), device=dev)

    def behind():
        for _ in range(4):
            torch.mm(big, big)
    for kind, shapes, legs_of, per_call in (("update", ((256, 300), (65536, 256)), (FusedUpdate, TorchUpdate), 1),
                                            ("collect", ((4096, 300), (65536, 300)), (FusedCollect, TorchCollect), FREQ)):
        for n, L in shapes:
            inp = Inputs(torch, n, L, dev)
            legs = {"fused": legs_of[0](torch, inp, dev), "torch": legs_of[1](torch, inp, dev)}
            entry = measure(torch, legs, args, behind, per_call, args.big_reps if n >= 65536 else args.reps)
            entry["rows"], entry["latent_dim"] = n, L
            entry["torch"]["exploration_matrix_bytes"] = 4 * n * L * A      # allocated by torch, not by fused
            if kind == "update":
                entry["fused"]["scratch_bytes"] = 4 * math.ceil(n / math.ceil(n / 1024)) * L * A
            res[kind][f"{n}x{L}"] = entry
            print(json.dumps({kind: {f"{n}x{L}": entry}}), flush=True)
            del legs, inp
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
