#!/usr/bin/env python
"""The CAPS regulariser (DeviceCAPS: one HIP launch for the perturbed observations, one for both terms with their
gradients, one backward) against the torch lines examples/sac_torch.py runs with --caps alone, and one whole
SAC.train(8) with --caps --caps-kernel against --caps.

    python tools/caps_ab.py [--rounds 7] [--out profiles/caps_ab.json]

One process, one stream, HIP events; the legs alternate every round (tools/sde_squash_ab.py's harness).  Inputs
resident in HBM, shaped as the example's: observations [B, 715], means [B, 2].

near      obs + eps z: DeviceCAPS.near against obs + eps * torch.randn_like(obs), at B = 256 and B = 65 536; the
          large size with its achieved bytes per second (one read and one write of the array) against the 8 TB/s peak
loss      lambda_t L_T + lambda_s L_S from three [B, 2] means with its backward into all three, at B = 256 and
          B = 65 536: DeviceCAPS.loss against tanh, vector_norm and mean
train     SAC.train(8) of --device-replay --sde-kernel --loss-kernel --caps at 4 096 envs, batch 256, after 24
          collected steps, with and without --caps-kernel; ms per call

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

LT, LS, EPS, W, A = 10.0, 5.0, 0.1, 715, 2
PEAK_BYTES_PER_S = 8.0e12


class Near:
    def __init__(self, torch, obs, caps):
        self.torch, self.obs, self.caps = torch, obs, caps

    def call(self):
        if self.caps is not None:
            self.caps.reset_noise()
            self.caps.near(self.obs)
            return
        self.obs + EPS * self.torch.randn_like(self.obs)


class Loss:
    def __init__(self, torch, B, dev, caps):
        g = torch.Generator(device=dev).manual_seed(78)
        self.torch, self.caps = torch, caps
        self.m = (2 * torch.rand((B, A), device=dev, generator=g) - 1).requires_grad_(True)
        self.mn = (self.m.detach() + 0.3 * torch.randn((B, A), device=dev, generator=g)).requires_grad_(True)
        self.mr = (self.m.detach() + 0.05 * torch.randn((B, A), device=dev, generator=g)).requires_grad_(True)

    def call(self):
        torch = self.torch
        for t in (self.m, self.mn, self.mr):
            t.grad = None
        if self.caps is not None:
            self.caps.loss(self.m, self.mn, self.mr).loss.backward()
            return
        a = torch.tanh(self.m)
        temporal = torch.linalg.vector_norm(a - torch.tanh(self.mn), dim=-1).mean()
        spatial = torch.linalg.vector_norm(a - torch.tanh(self.mr), dim=-1).mean()
        (LT * temporal + LS * spatial).backward()


class Train:
    """One SAC of examples/sac_torch.py after `steps` collected steps; call() is one train(gradient_steps)."""

    def __init__(self, envs, steps, caps_kernel):
        import gym_usv_amd
        from sac_torch import SAC
        self.env = gym_usv_amd.make_vec("usv-simple", envs, seed=0, copy=False)
        self.sac = SAC(self.env, seed=0, device_replay=True, sde_kernel=True, loss_kernel=True, caps=True,
                       caps_kernel=caps_kernel)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caps_ab.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("caps_ab.py needs a GPU")
    from gym_usv_amd import DeviceCAPS
    dev = torch.device("cuda", 0)
    res = {"what": "interleaved same-process A/B, one stream, HIP events, us per call. near: obs + eps z over [B, 715] (fused = "
                   "DeviceCAPS.near with a new epoch per call, torch = obs + eps * randn_like(obs)). loss: the CAPS loss "
                   "from three [B, 2] means with its backward (fused = DeviceCAPS.loss, torch = tanh, vector_norm, mean). "
                   "queued = launches issued behind ~10 ms of other work (kernel time, not the host's call rate); "
                   "plain_at_host_call_rate: the plain median is above 1.3x the queued one. train: ms per SAC.train(8) of "
                   "--device-replay --sde-kernel --loss-kernel --caps (fused = with --caps-kernel). criterion "
                   "(max_below_torch_min): the fused leg's slowest round is below the torch leg's fastest",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "near": {}, "loss": {}, "train": {}}
    big = torch.randn((8192, 8192), device=dev)

    def behind():
        for _ in range(4):
            torch.mm(big, big)
    caps = DeviceCAPS(dev, 5, LT, LS, EPS, squash=True)
    for B in (256, 65536):
        reps = args.big_reps if B >= 65536 else args.reps
        obs = torch.randn((B, W), device=dev)
        legs = {"fused": Near(torch, obs, caps), "torch": Near(torch, obs, None)}
        entry = S.measure(torch, legs, args, behind, 1, reps)
        entry.update(rows=B, width=W, bytes_moved=8 * B * W)          # one read and one write
        for k in ("fused", "torch"):
            rate = 8 * B * W / (entry[k]["queued"]["median_us"] * 1e-6)
            entry[k]["queued_bytes_per_s"] = round(rate)
            entry[k]["queued_share_of_8TBps"] = round(rate / PEAK_BYTES_PER_S, 4)
        res["near"][str(B)] = entry
        print(json.dumps({"near": {str(B): entry}}), flush=True)
        del obs, legs
        legs = {"fused": Loss(torch, B, dev, caps), "torch": Loss(torch, B, dev, None)}
        entry = S.measure(torch, legs, args, behind, 1, reps)
        entry.update(rows=B, act_dim=A)
        res["loss"][str(B)] = entry
        print(json.dumps({"loss": {str(B): entry}}), flush=True)
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
