#!/usr/bin/env python
"""SAC's loss lines and polyak_update (DeviceSACLoss / DevicePolyak: one HIP launch each way) against the torch
lines examples/sac_torch.py runs without --loss-kernel, and one whole SAC.train(8) with and without the flag.

    python tools/sac_loss_ab.py [--rounds 7] [--out profiles/sac_loss_ab.json]

One process, one stream, HIP events; the legs alternate every round (tools/sde_squash_ab.py's harness).  Inputs
resident in HBM, shaped as the example's: q's, rewards, dones and discounts [B, 1], log-probabilities [B].

critic    the TD target and 0.5 (mse(q1, target) + mse(q2, target)) with its backward into q1 and q2
policy    (ent logp - min(q1, q2)).mean() and -(log_ent (logp + target_entropy)).mean() with their backward into
          logp, both q's and log_ent (the torch leg: two backward calls, as the example has them)
          both at B = 256, config_sac's minibatch, and B = 65 536
polyak    the example's critic against its target: 12 tensors, 815 602 floats; torch = mul_ and add_ per tensor
train     SAC.train(8) of --device-replay --sde-kernel at 4 096 envs, batch 256, after 24 collected steps, with and
          without --loss-kernel; ms per call

"queued": the same launches issued behind some 10 ms of other work on the stream, so the events time the kernels
back to back and not the host's launch rate.  Where the plain median is well above the queued one
(plain_at_host_call_rate), the plain figure is the host's call rate.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gym-usv_amd"), os.path.join(ROOT, "examples"), os.path.dirname(os.path.abspath(__file__))]

import sde_squash_ab as S  # noqa: E402

TAU, TE = 0.005, -2.0
PEAK_BYTES_PER_S = 8.0e12


class Inputs:
    def __init__(self, torch, B, dev):
        g = torch.Generator(device=dev).manual_seed(77)
        r = lambda *s: torch.randn(s, device=dev, generator=g)      # noqa: E731
        self.q1, self.q2 = (5 * r(B, 1)).requires_grad_(True), (5 * r(B, 1)).requires_grad_(True)
        self.q1n, self.q2n, self.rew = 5 * r(B, 1), 5 * r(B, 1), 2 * r(B, 1)
        self.done = (torch.rand((B, 1), device=dev, generator=g) < 0.3).float()
        self.disc = torch.full((B, 1), 0.99, device=dev)
        self.logp2 = 2 * r(B) - 1
        self.logp = (2 * r(B) - 1).requires_grad_(True)
        self.log_ent = torch.full((1,), -1.5, device=dev, requires_grad=True)
        self.leaves = (self.q1, self.q2, self.logp, self.log_ent)

    def clear(self):
        for t in self.leaves:
            t.grad = None


class Critic:
    def __init__(self, torch, inp, sl):
        self.torch, self.inp, self.sl = torch, inp, sl

    def call(self):
        torch, x = self.torch, self.inp
        x.clear()
        ent = x.log_ent.detach().exp()
        if self.sl is not None:
            self.sl.critic(x.q1, x.q2, x.q1n, x.q2n, x.rew, x.done, ent_coef=ent, logp_next=x.logp2,
                           discounts=x.disc).loss.backward()
            return
        with torch.no_grad():
            q_next = torch.min(x.q1n, x.q2n) - ent * x.logp2[:, None]
            target = x.rew + (1 - x.done) * x.disc * q_next
        F = torch.nn.functional
        (0.5 * (F.mse_loss(x.q1, target) + F.mse_loss(x.q2, target))).backward()


class Policy:
    def __init__(self, torch, inp, sl):
        self.torch, self.inp, self.sl = torch, inp, sl

    def call(self):
        torch, x = self.torch, self.inp
        x.clear()
        ent = x.log_ent.detach().exp()
        if self.sl is not None:
            p = self.sl.policy(x.logp, x.q1, x.q2, ent, log_ent_coef=x.log_ent, target_entropy=TE)
            (p.actor_loss + p.ent_coef_loss).backward()
            return
        (-(x.log_ent * (x.logp.detach() + TE)).mean()).backward()
        (ent * x.logp[:, None] - torch.min(x.q1, x.q2)).mean().backward()


class Polyak:
    def __init__(self, torch, dev, fused):
        from sac_torch import CONFIG_SAC, Critic as Net
        self.torch = torch
        W = 5 * 143
        self.net, self.tgt = Net(W, 2, CONFIG_SAC["net_arch"]).to(dev), Net(W, 2, CONFIG_SAC["net_arch"]).to(dev)
        self.tensors = len(list(self.net.parameters()))
        self.floats = sum(p.numel() for p in self.net.parameters())
        self.pol = None
        if fused:
            from gym_usv_amd import DevicePolyak
            self.pol = DevicePolyak(list(self.net.parameters()), list(self.tgt.parameters()))

    def call(self):
        if self.pol is not None:
            self.pol.step(TAU)
            return
        with self.torch.no_grad():
            for p, t in zip(self.net.parameters(), self.tgt.parameters()):
                t.mul_(1 - TAU).add_(p, alpha=TAU)


class Train:
    """One SAC of examples/sac_torch.py after `steps` collected steps; call() is one train(gradient_steps)."""

    def __init__(self, envs, steps, loss_kernel):
        import gym_usv_amd
        from sac_torch import SAC
        self.env = gym_usv_amd.make_vec("usv-simple", envs, seed=0, copy=False)
        self.sac = SAC(self.env, seed=0, device_replay=True, sde_kernel=True, loss_kernel=loss_kernel)
        self.sac.collect(12, random_actions=True)
        self.sac.collect(steps - 12, random_actions=False)

    def call(self):
        self.sac.train(self.sac.cfg["gradient_steps"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50, help="calls per round and leg")
    ap.add_argument("--big-reps", type=int, default=20, help="the same at 65 536 rows")
    ap.add_argument("--queued-reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--train-rounds", type=int, default=7)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_loss_ab.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sac_loss_ab.py needs a GPU")
    from gym_usv_amd import DeviceSACLoss
    dev = torch.device("cuda", 0)
    res = {"what": "interleaved same-process A/B, one stream, HIP events, us per call. critic / policy: the loss lines of "
                   "examples/sac_torch.py's gradient step with their backward (fused = DeviceSACLoss, torch = the lines "
                   "the example runs without --loss-kernel). polyak: the example's critic into its target (fused = "
                   "DevicePolyak, torch = mul_ and add_ per tensor). queued = launches issued behind ~10 ms of other work "
                   "(kernel time, not the host's call rate); plain_at_host_call_rate: the plain median is above 1.3x the "
                   "queued one. train: ms per SAC.train(8) of --device-replay --sde-kernel (fused = with --loss-kernel). "
                   "criterion (max_below_torch_min): the fused leg's slowest round is below the torch leg's fastest",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "critic": {}, "policy": {}, "polyak": {},
           "train": {}}
    big = torch.randn((8192, 8192), device=dev)

    def behind():
        for _ in range(4):
            torch.mm(big, big)
    sl = DeviceSACLoss(dev)
    for B in (256, 65536):
        inp = Inputs(torch, B, dev)
        for name, leg in (("critic", Critic), ("policy", Policy)):
            legs = {"fused": leg(torch, inp, sl), "torch": leg(torch, inp, None)}
            entry = S.measure(torch, legs, args, behind, 1, args.big_reps if B >= 65536 else args.reps)
            entry["rows"] = B
            res[name][str(B)] = entry
            print(json.dumps({name: {str(B): entry}}), flush=True)
    legs = {"fused": Polyak(torch, dev, True), "torch": Polyak(torch, dev, False)}
    entry = S.measure(torch, legs, args, behind, 1, args.reps)
    floats = legs["fused"].floats
    entry.update(tensors=legs["fused"].tensors, floats=floats, bytes_moved=12 * floats)   # two reads and a write
    for k in ("fused", "torch"):
        rate = 12 * floats / (entry[k]["queued"]["median_us"] * 1e-6)
        entry[k]["queued_bytes_per_s"] = round(rate)
        entry[k]["queued_share_of_8TBps"] = round(rate / PEAK_BYTES_PER_S, 4)
    res["polyak"] = entry
    print(json.dumps({"polyak": entry}), flush=True)
    del big, legs
    torch.cuda.empty_cache()
    legs = {"fused": Train(args.envs, 24, True), "torch": Train(args.envs, 24, False)}
    for leg in legs.values():
        S.run_events(torch, leg, 1)                        # warm-up: one whole train(8)
    ms = {k: [] for k in legs}
    for _ in range(args.train_rounds):
        for k, leg in legs.items():
            ms[k].append(S.run_events(torch, leg, 1) * 1e-3)
    entry = {k: {"median_ms": round(sorted(v)[len(v) // 2], 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                 "rounds_ms": [round(x, 3) for x in v]} for k, v in ms.items()}
    entry["fused"]["torch_over_this_median"] = round(entry["torch"]["median_ms"] / entry["fused"]["median_ms"], 3)
    entry["fused"]["max_below_torch_min"] = entry["fused"]["max_ms"] < entry["torch"]["min_ms"]
    entry.update(envs=args.envs, batch_size=256, gradient_steps=8)
    res["train"][str(args.envs)] = entry
    print(json.dumps({"train": entry}), flush=True)
    for leg in legs.values():
        leg.env.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
