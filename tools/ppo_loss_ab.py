#!/usr/bin/env python
"""PPO's minibatch loss lines and explained_variance (DevicePPOLoss) against the torch lines examples/ppo_torch.py runs
without --loss-kernel, and one whole PPO.update() with and without the flag.

    python tools/ppo_loss_ab.py [--rounds 7] [--out profiles/ppo_loss_ab.json]

One process, one stream, HIP events; the legs alternate every round (tools/sde_squash_ab.py's harness).  Inputs
resident in HBM, shaped as the example's minibatch: [B] each.

loss      advantage normalisation, ratio, clamp, min, the value loss, -logp.mean(), the weighted sum and the backward
          into log_prob and values, at B = 4 096 (the example's minibatch) and B = 65 536
ev        explained_variance of 131 072 rows (the example's rollout); torch = 1 - (ret - val).var() / ret.var(),
          population variances, as SB3's NumPy line
update    PPO.update() of --fused --frames --sde-kernel --eval-kernel --adam-kernel at 4 096 envs x 32 steps (320
          minibatches), with and without --loss-kernel, after one rollout; ms per call.  The leg without the flag is
          the path the example ran before the flag existed: the baseline.

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

CLIP, VF_COEF, ENT_COEF = 0.2, 0.5, 0.0


class Inputs:
    def __init__(self, torch, B, dev):
        g = torch.Generator(device=dev).manual_seed(78)
        r = lambda: torch.randn(B, device=dev, generator=g)      # noqa: E731
        self.logp, self.values = (2 * r() - 1).requires_grad_(True), (3 * r()).requires_grad_(True)
        self.old = self.logp.detach() - 0.2 * r()
        self.adv, self.ret = r(), 3 * r()

    def clear(self):
        self.logp.grad = self.values.grad = None


class Loss:
    def __init__(self, torch, inp, pl):
        self.torch, self.inp, self.pl = torch, inp, pl

    def call(self):
        torch, x = self.torch, self.inp
        x.clear()
        if self.pl is not None:
            self.pl.loss(x.logp, x.old, x.adv, x.values, x.ret, clip_range=CLIP, vf_coef=VF_COEF,
                         ent_coef=ENT_COEF).loss.backward()
            return
        a_ = (x.adv - x.adv.mean()) / (x.adv.std() + 1e-8)
        ratio = (x.logp - x.old).exp()
        pg = -torch.min(ratio * a_, ratio.clamp(1 - CLIP, 1 + CLIP) * a_).mean()
        vl = ((x.values - x.ret) ** 2).mean()
        ent = -x.logp.mean()
        (pg + VF_COEF * vl - ENT_COEF * ent).backward()


class Explained:
    def __init__(self, torch, inp, pl):
        self.inp, self.pl = inp, pl

    def call(self):
        v, y = self.inp.values.detach(), self.inp.ret
        if self.pl is not None:
            return self.pl.explained_variance(v, y)
        return 1 - (y - v).var(unbiased=False) / y.var(unbiased=False)


class Update:
    """One PPO of examples/ppo_torch.py after a rollout; call() is one update() on that rollout."""

    def __init__(self, envs, loss_kernel):
        import gym_usv_amd
        from ppo_torch import PPO
        self.env = gym_usv_amd.make_vec("usv-simple", envs, seed=0, copy=False)
        self.ppo = PPO(self.env, seed=0, fused=True, frames=True, sde_kernel=True, eval_kernel=True, adam_kernel=True,
                       loss_kernel=loss_kernel)
        self.ppo.rollout()

    def call(self):
        self.ppo.update()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50, help="calls per round and leg")
    ap.add_argument("--big-reps", type=int, default=20, help="the same at 65 536 rows and more")
    ap.add_argument("--queued-reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--update-rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_loss_ab.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ppo_loss_ab.py needs a GPU")
    from gym_usv_amd import DevicePPOLoss
    dev = torch.device("cuda", 0)
    res = {"what": "interleaved same-process A/B, one stream, HIP events, us per call. loss: the loss lines of "
                   "examples/ppo_torch.py's minibatch with their backward (fused = DevicePPOLoss.loss, torch = the lines "
                   "the example runs without --loss-kernel). ev: explained_variance of a rollout (fused = "
                   "DevicePPOLoss.explained_variance, torch = two var() calls). queued = launches issued behind ~10 ms of "
                   "other work (kernel time, not the host's call rate); plain_at_host_call_rate: the plain median is above "
                   "1.3x the queued one. update: ms per PPO.update() of --fused --frames --sde-kernel --eval-kernel "
                   "--adam-kernel, 320 minibatches of 4 096 (fused = with --loss-kernel; torch = without, the path before "
                   "the flag existed). criterion (max_below_torch_min): the fused leg's slowest round is below the torch "
                   "leg's fastest",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "loss": {}, "ev": {}, "update": {}}
    big = torch.randn((8192, 8192), device=dev)

    def behind():
        for _ in range(4):
            torch.mm(big, big)
    pl = DevicePPOLoss(dev)
    for B in (4096, 65536):
        inp = Inputs(torch, B, dev)
        legs = {"fused": Loss(torch, inp, pl), "torch": Loss(torch, inp, None)}
        entry = S.measure(torch, legs, args, behind, 1, args.big_reps if B >= 65536 else args.reps)
        entry["rows"] = B
        res["loss"][str(B)] = entry
        print(json.dumps({"loss": {str(B): entry}}), flush=True)
    inp = Inputs(torch, 131072, dev)
    legs = {"fused": Explained(torch, inp, pl), "torch": Explained(torch, inp, None)}
    entry = S.measure(torch, legs, args, behind, 1, args.big_reps)
    entry["rows"] = 131072
    res["ev"]["131072"] = entry
    print(json.dumps({"ev": entry}), flush=True)
    del big, legs
    torch.cuda.empty_cache()
    legs = {"fused": Update(args.envs, True), "torch": Update(args.envs, False)}
    for leg in legs.values():
        S.run_events(torch, leg, 1)                        # warm-up: one whole update()
    ms = {k: [] for k in legs}
    for _ in range(args.update_rounds):
        for k, leg in legs.items():
            ms[k].append(S.run_events(torch, leg, 1) * 1e-3)
    entry = {k: {"median_ms": round(sorted(v)[len(v) // 2], 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                 "rounds_ms": [round(x, 3) for x in v]} for k, v in ms.items()}
    entry["fused"]["torch_over_this_median"] = round(entry["torch"]["median_ms"] / entry["fused"]["median_ms"], 3)
    entry["fused"]["max_below_torch_min"] = entry["fused"]["max_ms"] < entry["torch"]["min_ms"]
    entry.update(envs=args.envs, n_steps=32, batch_size=4096, minibatches=320)
    res["update"][str(args.envs)] = entry
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
