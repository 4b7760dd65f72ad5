#!/usr/bin/env python
"""The SAC update recorded as a HIP graph (examples/sac_torch.py --graph: gym_usv_amd.capture_step over the capturable
DeviceAdam, DeviceSDE and DeviceCAPS) against the same update launched one Python call at a time.

    python tools/graph_ab.py [--rounds 5] [--out profiles/graph_ab.json]

One process, one stream, HIP events; the legs alternate every round (tools/sde_squash_ab.py's harness, as
tools/optim_ab.py uses it).

train        one SAC.train(8) of --device-replay --sde-kernel --loss-kernel --adam-kernel at 4 096 envs, ms per call:
             "eager" without --graph, "graph" with it (eight randint + gather launches and eight replays)
train_caps   the same with --caps --caps-kernel
step         one gradient step alone on a resident minibatch, us per call, in three forms: "eager" (the launches
             issued one Python call at a time, at the host's call rate), "graph" (one replay), and each "queued": issued
             behind some 10 ms of other work on the stream, so the events time the kernels back to back.  The eager
             step's queued figure is the floor a replay is compared with: what the same kernels cost once launching
             them is free.

The criterion (max_below_eager_min) is the project's standing one: the graph leg is faster only if its slowest round
is below the eager leg's fastest.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gym-usv_amd"), os.path.join(ROOT, "examples"), os.path.dirname(os.path.abspath(__file__))]

import sde_squash_ab as S  # noqa: E402

FLAGS = dict(device_replay=True, sde_kernel=True, loss_kernel=True, adam_kernel=True)


class SacTrain:
    """One trainer with a filled buffer; ``call`` is one SAC.train(8)."""

    def __init__(self, envs, graph, caps):
        import gym_usv_amd
        from sac_torch import SAC
        self.env = gym_usv_amd.make_vec("usv-simple", envs, seed=0, copy=False)
        self.sac = SAC(self.env, seed=0, graph=graph, caps=caps, caps_kernel=caps, **FLAGS)
        self.sac.collect(12, random_actions=True)
        self.sac.collect(12, random_actions=False)
        self.call()                                          # the graph leg records its step here

    def call(self):
        self.sac.train(self.sac.cfg["gradient_steps"])


class GradStep:
    """One gradient step of ``train``'s trainer on a resident minibatch: the eager trainer's launches, or a replay."""

    def __init__(self, train):
        self.sac = train.sac
        self.mb = self.sac.static_mb if self.sac.graph else self.sac.minibatch()

    def call(self):
        if self.sac.graph:
            self.sac.captured.replay()
        else:
            self.sac.gradient_step(self.mb)


def measure(torch, legs, args, behind, reps, unit, scale):
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
    g, e = entry["graph"], entry["eager"]
    g["eager_over_this_median"] = round(e["median_" + unit] / g["median_" + unit], 3)
    g["max_below_eager_min"] = g["max_" + unit] < e["min_" + unit]
    if "queued" in e:                                       # the floor: the eager launches with launching free
        g["this_median_over_eager_queued_median"] = round(g["median_" + unit] / e["queued"]["median_" + unit], 3)
        g["queued"]["max_below_eager_queued_min"] = g["queued"]["max_" + unit] < e["queued"]["min_" + unit]
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="calls per round and leg")
    ap.add_argument("--queued-reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_ab.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("graph_ab.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"what": "interleaved same-process A/B, one stream, HIP events. train / train_caps: ms per SAC.train(8) of "
                   "--device-replay --sde-kernel --loss-kernel --adam-kernel (train_caps: and --caps --caps-kernel), eager = "
                   "without --graph, graph = with it. step: us per gradient step on a resident minibatch; queued = issued "
                   "behind ~10 ms of other work (kernel time, not the host's call rate): the eager step's queued figure is "
                   "the floor a replay is compared with. criterion (max_below_eager_min): the graph leg's slowest round is "
                   "below the eager leg's fastest",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds, "envs": args.envs}
    big = torch.randn((8192, 8192), device=dev)

    def behind():
        for _ in range(4):
            torch.mm(big, big)
    for name, caps in (("train", False), ("train_caps", True)):
        legs = {"eager": SacTrain(args.envs, False, caps), "graph": SacTrain(args.envs, True, caps)}
        res[name] = measure(torch, legs, args, None, 1, "ms", 1e-3)
        print(json.dumps({name: res[name]}), flush=True)
        if caps:
            steps = {k: GradStep(v) for k, v in legs.items()}
            res["step"] = measure(torch, steps, args, behind, args.reps, "us", 1.0)
            res["step"]["flags"] = "as train_caps"
            print(json.dumps({"step": res["step"]}), flush=True)
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
