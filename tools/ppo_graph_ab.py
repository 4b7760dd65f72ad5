#!/usr/bin/env python
"""The PPO update recorded as a HIP graph (examples/ppo_torch.py --graph: gym_usv_amd.capture_step over
DeviceRollout.sampler, DeviceSDE.evaluate, DevicePPOLoss and the capturable DeviceAdam) against the same update
launched one Python call at a time, and the sampler's gather against the gather that reads an index tensor.

    python tools/ppo_graph_ab.py [--rounds 5] [--out profiles/ppo_graph_ab.json]

One process, one stream, HIP events; the legs alternate every round (tools/sde_squash_ab.py's harness, as
tools/graph_ab.py uses it).

update   one PPO.update() of --fused --frames --sde-kernel --eval-kernel --adam-kernel --loss-kernel at 4 096 envs x 32
         steps (320 minibatches of 4 096), ms per call: "parent" without --perm-kernel (randperm + gather, the flag set
         of the commit before the sampler), "eager" with --perm-kernel, "graph" with --perm-kernel --graph
step     one minibatch step alone, us per call: "eager" (sampler.next, forward, loss, backward, optimizer, one Python
         call at a time), "graph" (one replay), and each "queued": issued behind some 10 ms of other work on the stream,
         so the events time the kernels back to back.  The eager step's queued figure is the floor a replay is compared
         with.
gather   sampler.next(out) against gather(perm[k B:(k + 1) B], out) over a resident randperm, with the same outputs, us
         per call, plain and queued, at 65 536 samples of 524 288 and at 4 096 of 131 072, frame and full storage
         (W = 715, A = 2).

The criterion (max_below_*_min) is the project's standing one: a leg is faster only if its slowest round is below the
other leg's fastest.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gym-usv_amd"), os.path.join(ROOT, "examples"), os.path.dirname(os.path.abspath(__file__))]

import sde_squash_ab as S  # noqa: E402

FLAGS = dict(fused=True, frames=True, sde_kernel=True, eval_kernel=True, adam_kernel=True, loss_kernel=True)


class Update:
    """One trainer behind one rollout; ``call`` is one PPO.update() on it (the graph leg records its step in the
    first)."""

    def __init__(self, envs, n_steps, batch, perm, graph):
        import gym_usv_amd
        from ppo_torch import PPO
        self.env = gym_usv_amd.make_vec("usv-simple", envs, seed=0, copy=False)
        self.ppo = PPO(self.env, n_steps=n_steps, batch_size=batch, seed=0, perm_kernel=perm, graph=graph, **FLAGS)
        self.ppo.rollout()
        self.call()

    def call(self):
        self.ppo.update()


class Step:
    """One minibatch step of ``update``'s trainer: its eager calls, or a replay."""

    def __init__(self, update):
        self.ppo = update.ppo

    def call(self):
        if self.ppo.graph:
            self.ppo.captured.replay()
        else:
            self.ppo.sampled_step(None)


class Gather:
    """``perm``: sampler.next(out); otherwise gather(perm[k B:(k + 1) B], out) over the slices of one resident
    ``randperm``, as the update without the sampler reads them: both legs visit the whole rollout, so neither reads
    rows that the call before left in the cache."""

    def __init__(self, torch, ro, B, perm):
        from gym_usv_amd.rollout import RolloutSamples
        d = ro.device
        self.out = RolloutSamples(*(torch.zeros(s, device=d) for s in ((B, ro.w), (B, ro.a), (B,), (B,), (B,), (B,))))
        self.smp = ro.sampler(B, 1) if perm else None
        self.ro, self.B, self.k, self.perm = ro, B, 0, torch.randperm(ro.n * ro.n_steps, device=d)

    def call(self):
        if self.smp is not None:
            self.smp.next(out=self.out)
        else:
            self.ro.gather(self.perm[self.k * self.B:(self.k + 1) * self.B], out=self.out)
            self.k = (self.k + 1) % (self.perm.numel() // self.B)


def measure(torch, legs, args, behind, reps, unit, scale, base):
    """Rounds of every leg in turn; each leg but ``base`` is compared with it."""
    for leg in legs.values():
        S.run_events(torch, leg, args.warmup)
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
    for k, e in entry.items():
        for b in base:
            if k == b:
                continue
            e[f"{b}_over_this_median"] = round(entry[b]["median_" + unit] / e["median_" + unit], 3)
            e[f"max_below_{b}_min"] = e["max_" + unit] < entry[b]["min_" + unit]
            if "queued" in e:
                q, bq = e["queued"], entry[b]["queued"]
                q[f"{b}_over_this_median"] = round(bq["median_" + unit] / q["median_" + unit], 3)
                q[f"max_below_{b}_min"] = q["max_" + unit] < bq["min_" + unit]
                e[f"this_median_over_{b}_queued_median"] = round(e["median_" + unit] / bq["median_" + unit], 3)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="calls per round and leg (step, gather)")
    ap.add_argument("--queued-reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--n-steps", type=int, default=32)
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_graph_ab.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ppo_graph_ab.py needs a GPU")
    from gym_usv_amd.rollout import DeviceRollout
    dev = torch.device("cuda", 0)
    res = {"what": "interleaved same-process A/B, one stream, HIP events. update: ms per PPO.update() of --fused --frames "
                   "--sde-kernel --eval-kernel --adam-kernel --loss-kernel; parent = without --perm-kernel, eager = with it, "
                   "graph = with --perm-kernel --graph. step: us per minibatch step; queued = issued behind ~10 ms of other "
                   "work (kernel time, not the host's call rate): the eager step's queued figure is the floor a replay is "
                   "compared with. gather: us per call of sampler.next(out) (perm) and gather(perm[k B:(k + 1) B], out) over a "
                   "resident randperm (gather). criterion "
                   "(max_below_X_min): this leg's slowest round is below leg X's fastest",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds, "envs": args.envs,
           "n_steps": args.n_steps, "batch_size": args.batch_size}
    big = torch.randn((8192, 8192), device=dev)

    def behind():
        for _ in range(4):
            torch.mm(big, big)
    shape = (args.envs, args.n_steps, args.batch_size)
    legs = {"parent": Update(*shape, False, False), "eager": Update(*shape, True, False), "graph": Update(*shape, True, True)}
    res["update"] = measure(torch, legs, args, None, 1, "ms", 1e-3, ("parent", "eager"))
    res["update"]["minibatches"] = legs["graph"].ppo.cfg["n_epochs"] * legs["graph"].ppo.sampler.batches_per_epoch
    print(json.dumps({"update": res["update"]}), flush=True)
    steps = {k: Step(legs[k]) for k in ("eager", "graph")}
    res["step"] = measure(torch, steps, args, behind, args.reps, "us", 1.0, ("eager",))
    print(json.dumps({"step": res["step"]}), flush=True)
    for x in legs.values():
        x.env.close()
    del legs, steps
    torch.cuda.empty_cache()
    res["gather"] = {}
    for n, T, B in ((16384, 32, 65536), (4096, 32, 4096)):
        for frames in (True, False):
            ro = DeviceRollout(n, T, 715, 2, dev, n_stack=5 if frames else None)
            ro.start.copy_(torch.rand(ro.start.shape, device=dev) < 0.02)      # live masks with something to clear
            for t in (ro.frames if frames else ro.obs, ro.act, ro.val, ro.logp, ro.adv, ro.ret):
                t.normal_()
            pair = {"gather": Gather(torch, ro, B, False), "perm": Gather(torch, ro, B, True)}
            key = f"{B}_of_{n * T}_{'frames' if frames else 'full'}"
            res["gather"][key] = measure(torch, pair, args, behind, args.reps, "us", 1.0, ("gather",))
            assert ro.bad_indices() == 0
            print(json.dumps({key: res["gather"][key]}), flush=True)
            del pair, ro
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
