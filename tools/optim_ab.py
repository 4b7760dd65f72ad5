#!/usr/bin/env python
"""The optimizer step (DeviceAdam: clip_grad_norm_ and Adam.step() as two HIP launches, one without clipping) against
torch's, and one whole PPO update() and SAC.train(8) with and without --adam-kernel.

    python tools/optim_ab.py [--rounds 7] [--out profiles/optim_ab.json]

One process, one stream, HIP events; the legs alternate every round (tools/sde_squash_ab.py's harness).  The
gradients are resident and stay in place: a call is the clip and the step alone.

fused     gym_usv_amd.DeviceAdam
torch     what the examples run without the flag: nn.utils.clip_grad_norm_ + torch.optim.Adam's defaults
torch_fused   clip_grad_norm_(foreach=True) + torch.optim.Adam(fused=True), if this torch build takes it on this
          device; "unavailable" with the error otherwise

ppo       the PPO example's model (13 tensors), max_grad_norm 0.5
critic    the SAC example's critic (12 tensors), no clipping
log_ent   the SAC example's one-element entropy coefficient, no clipping
update    one PPO update() of --fused --frames --sde-kernel --eval-kernel at 4 096 envs x 32 steps; ms per call
train     one SAC.train(8) of --device-replay --sde-kernel --loss-kernel at 4 096 envs; ms per call

"queued": the same launches issued behind some 10 ms of other work on the stream, so the events time the kernels
back to back and not the host's launch rate.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gym-usv_amd"), os.path.join(ROOT, "examples"), os.path.dirname(os.path.abspath(__file__))]

import sde_squash_ab as S  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
ADAM_BYTES_PER_FLOAT = 28                                # p, g, m, v read; p, m, v written


class Step:
    def __init__(self, torch, params, kind, max_norm, lr):
        self.torch, self.params, self.kind, self.max_norm = torch, params, kind, max_norm
        if kind == "fused":
            from gym_usv_amd import DeviceAdam
            self.opt = DeviceAdam(params, lr=lr, max_grad_norm=max_norm)
        else:
            self.opt = torch.optim.Adam(params, lr=lr, **({"fused": True} if kind == "torch_fused" else {}))
        g = torch.Generator(device=params[0].device).manual_seed(5)
        for p in params:
            p.grad = torch.randn(p.shape, device=p.device, generator=g)

    def call(self):
        if self.kind != "fused" and self.max_norm is not None:
            kw = {"foreach": True} if self.kind == "torch_fused" else {}
            self.torch.nn.utils.clip_grad_norm_(self.params, self.max_norm, **kw)
        self.opt.step()


def step_legs(torch, make_params, max_norm, lr):
    legs, missing = {}, None
    for kind in ("fused", "torch", "torch_fused"):
        try:
            leg = Step(torch, make_params(), kind, max_norm, lr)
            leg.call()
            torch.cuda.synchronize()
            legs[kind] = leg
        except Exception as e:                           # this torch build does not take fused=True here: recorded
            if kind != "torch_fused":
                raise
            missing = f"{type(e).__name__}: {e}"[:300]
    return legs, missing


def measure(torch, legs, args, behind, reps, unit="us", scale=1.0):
    for leg in legs.values():
        S.run_events(torch, leg, args.warmup if behind is not None else 1)
    ev, queued = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, leg in legs.items():
            ev[k].append(S.run_events(torch, leg, reps) * scale)
        if behind is not None:
            for k, leg in legs.items():
                queued[k].append(S.run_events(torch, leg, args.queued_reps, behind) * scale)

    def summary(xs):
        return {k.replace("_us", "_" + unit): v for k, v in S.summary(xs).items()}
    entry = {k: summary(v) for k, v in ev.items()}
    for k, v in queued.items():
        if v:
            entry[k]["queued"] = summary(v)
    for other in legs:
        if other == "fused":
            continue
        for part in ((lambda e: e), (lambda e: e.get("queued"))):
            f, t = part(entry["fused"]), part(entry[other])
            if f is None:
                continue
            f[other + "_over_this_median"] = round(t["median_" + unit] / f["median_" + unit], 3)
            f["max_below_" + other + "_min"] = f["max_" + unit] < t["min_" + unit]
    return entry


class PpoUpdate:
    def __init__(self, envs, adam_kernel):
        import gym_usv_amd
        from ppo_torch import PPO
        self.env = gym_usv_amd.make_vec("usv-simple", envs, seed=0, copy=False)
        self.ppo = PPO(self.env, n_steps=32, batch_size=4096, seed=0, fused=True, frames=True, sde_kernel=True,
                       eval_kernel=True, adam_kernel=adam_kernel)
        self.ppo.rollout()

    def call(self):
        self.ppo.update()


class SacTrain:
    def __init__(self, envs, adam_kernel):
        import gym_usv_amd
        from sac_torch import SAC
        self.env = gym_usv_amd.make_vec("usv-simple", envs, seed=0, copy=False)
        self.sac = SAC(self.env, seed=0, device_replay=True, sde_kernel=True, loss_kernel=True, adam_kernel=adam_kernel)
        self.sac.collect(12, random_actions=True)
        self.sac.collect(12, random_actions=False)

    def call(self):
        self.sac.train(self.sac.cfg["gradient_steps"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50, help="calls per round and leg")
    ap.add_argument("--queued-reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_ab.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("optim_ab.py needs a GPU")
    from ppo_torch import CONFIG_PPO, ActorCritic
    from sac_torch import CONFIG_SAC, Critic
    dev = torch.device("cuda", 0)
    res = {"what": "interleaved same-process A/B, one stream, HIP events, us per optimizer step (gradients resident; a call "
                   "is the clip and the step alone). fused = DeviceAdam; torch = clip_grad_norm_ + torch.optim.Adam's "
                   "defaults, what the examples run without --adam-kernel; torch_fused = clip_grad_norm_(foreach=True) + "
                   "Adam(fused=True). queued = launches issued behind ~10 ms of other work (kernel time, not the host's "
                   "call rate). update / train: ms per PPO update() / SAC.train(8) (fused = with --adam-kernel). criterion "
                   "(max_below_<leg>_min): the fused leg's slowest round is below the other leg's fastest",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds}
    big = torch.randn((8192, 8192), device=dev)

    def behind():
        for _ in range(4):
            torch.mm(big, big)
    W = 5 * 143

    def ppo_params():
        torch.manual_seed(0)
        return list(ActorCritic(W, 2, CONFIG_PPO["hidden"], CONFIG_PPO["log_std_init"]).to(dev).parameters())

    def critic_params():
        torch.manual_seed(0)
        return list(Critic(W, 2, CONFIG_SAC["net_arch"]).to(dev).parameters())

    def log_ent_params():
        return [torch.zeros(1, device=dev, requires_grad=True)]
    for name, make, max_norm, lr in (("ppo", ppo_params, CONFIG_PPO["max_grad_norm"], CONFIG_PPO["lr"]),
                                     ("critic", critic_params, None, CONFIG_SAC["lr"]),
                                     ("log_ent", log_ent_params, None, CONFIG_SAC["lr"])):
        legs, missing = step_legs(torch, make, max_norm, lr)
        entry = measure(torch, legs, args, behind, args.reps)
        floats = sum(p.numel() for p in legs["fused"].params)
        entry.update(tensors=len(legs["fused"].params), floats=floats, max_grad_norm=max_norm,
                     launches_per_step=1 if max_norm is None else 2)
        if missing:
            entry["torch_fused"] = {"unavailable": missing}
        # the Adam pass moves 28 B per element; with clipping the norm pass reads 4 more
        moved = (ADAM_BYTES_PER_FLOAT + (0 if max_norm is None else 4)) * floats
        rate = moved / (entry["fused"]["queued"]["median_us"] * 1e-6)
        entry["fused"].update(bytes_moved=moved, queued_bytes_per_s=round(rate),
                              queued_share_of_8TBps=round(rate / PEAK_BYTES_PER_S, 4))
        res[name] = entry
        print(json.dumps({name: entry}), flush=True)
        del legs
    del big
    torch.cuda.empty_cache()
    for name, leg in (("update", PpoUpdate), ("train", SacTrain)):
        legs = {"fused": leg(args.envs, True), "torch": leg(args.envs, False)}
        entry = measure(torch, legs, args, None, 1, unit="ms", scale=1e-3)
        entry["envs"] = args.envs
        res[name] = entry
        print(json.dumps({name: entry}), flush=True)
        for x in legs.values():
            x.env.close()
        del legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
