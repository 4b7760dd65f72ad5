#!/usr/bin/env python
"""Device rollout buffer (DeviceRollout: HIP kernels, no host sync) against the torch rollout buffer of
examples/ppo_torch.py that it replaces.

    python tools/rollout_ab.py [--rounds 7] [--out profiles/rollout_ab.json]

One process, one stream, HIP events; the legs alternate every round.  k = 5, D = 143 (W = 715), scripted
inputs resident in HBM (a pool of steps; done rate 1/216 per env and step, half of them truncations), the
stacked observation read from a ring-shaped buffer at the window offset of the step, and the same stand-in
value function (one Linear) in every leg.  A leg is one whole rollout: T steps, then the advantages.
  (a) torch        what examples/ppo_torch.py does per step and per rollout without --fused: the b_* stores,
                   the clone of the stacked obs, the truncation bookkeeping with its host syncs
                   (bool(trunc.any()), done.nonzero(), bool(tr.any())), the value of the compacted terminal
                   rows, and advantages() -- existing code, the yardstick
  (b) fused        DeviceRollout.put_obs / put_step per step, one value pass over term_obs, gae
  (s) store only   put_obs alone: its bytes per second against the HBM peak
at 4 096 envs x T = 32 and 65 536 envs x T = 8.  Per leg: median and min..max over the rounds of the time
per rollout.  Needs a GPU; there is no fallback.

    python tools/rollout_ab.py --frames [--out profiles/rollout_frames_ab.json]

The frame leg: frame-deduplicated storage (DeviceRollout(n_stack=5)) against full storage of the same
build, same process, stream and rounds, at the same two sizes:
  store_full / store_frames   put_obs alone; "queued": the same launches issued behind some 10 ms of other
                              work on the stream, so the events time the kernels back to back and not the
                              host's launch rate (which bounds both legs alike at 4 096 envs)
  fused_full / fused_frames   the whole rollout, as (b)
  gather_frames / gather_full / gather_torch
                              one minibatch of B samples (B = 4 096 from 4 096 x 32, B = 65 536 from
                              65 536 x 8; consecutive slices of one device permutation): DeviceRollout.gather
                              on frame storage, on full storage, and the six indexed reads of
                              examples/ppo_torch.py's update() on the full buffer; bytes per second count
                              every field read once and written once, and the index.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-usv_amd"))

K, D, A = 5, 143, 2
W = K * D
DONE_RATE = 1.0 / 216
PEAK = 8.0e12      # HBM3E peak, B/s (MI355X)
GAMMA, LAM = 0.99, 0.95


def store_bytes_per_env(w=W, a=A):
    """put_obs: the obs row, the action, the value and the log-probability, each read once and written once."""
    return 2 * 4 * (w + a + 2)


class Inputs:
    def __init__(self, torch, n, pool, dev):
        from gym_usv_amd import _lib
        g = torch.Generator(device=dev).manual_seed(4242)
        stride = _lib.load().usv_wrap_ring_stride(D, K)
        self.ring = torch.randn((n, stride), device=dev, generator=g)
        self.final = torch.randn((n, W), device=dev, generator=g)
        self.act = torch.randn((pool, n, A), device=dev, generator=g)
        self.val = torch.randn((pool, n), device=dev, generator=g)
        self.logp = torch.randn((pool, n), device=dev, generator=g)
        self.rew = torch.randn((pool, n), device=dev, generator=g)
        done = torch.rand((pool, n), device=dev, generator=g) < DONE_RATE
        self.trunc = done & (torch.rand((pool, n), device=dev, generator=g) < 0.5)
        self.term = done & ~self.trunc
        self.done = done
        self.pool = pool
        self.vf = torch.nn.Linear(W, 1).to(dev)

    def window(self, t):
        off = ((t + 1) % K) * D
        return self.ring[:, off:off + W]

    def value(self, x):
        return self.vf(x).squeeze(-1)


class TorchLeg:
    """(a): PPO.rollout's buffer lines and PPO.advantages of examples/ppo_torch.py."""

    def __init__(self, torch, n, T, inp, dev):
        self.torch, self.inp, self.n, self.T = torch, inp, n, T
        z = lambda *s: torch.zeros(s, device=dev)   # noqa: E731
        self.b_obs, self.b_act = z(T, n, W), z(T, n, A)
        self.b_logp, self.b_val, self.b_rew, self.b_done = z(T, n), z(T, n), z(T, n), z(T, n)
        self.obs = inp.window(0).clone()
        self.i = 0

    def rollout(self):
        torch, inp = self.torch, self.inp
        with torch.no_grad():
            for t in range(self.T):
                i = self.i % inp.pool
                self.i += 1
                self.b_obs[t] = self.obs
                self.b_act[t] = inp.act[i]
                self.b_logp[t] = inp.logp[i]
                self.b_val[t] = inp.val[i]
                rew, term, trunc, done = inp.rew[i], inp.term[i], inp.trunc[i], inp.done[i]
                r = rew.float().clone()
                if bool(trunc.any()):
                    idx = done.nonzero().flatten()
                    term_rows = inp.final[idx]                     # DeviceFrameStack.step's compacted rows
                    tr = (trunc & ~term)[idx]
                    if bool(tr.any()):
                        r[idx[tr]] += GAMMA * inp.value(term_rows[tr])
                self.b_rew[t] = r
                self.b_done[t] = done.float()
                self.obs = inp.window(t + 1).clone()
            last_v = inp.value(self.obs)
        adv = torch.zeros_like(self.b_rew)
        gae = torch.zeros(self.n, device=adv.device)
        for t in reversed(range(self.T)):
            nv = last_v if t == self.T - 1 else self.b_val[t + 1]
            nonterm = 1.0 - self.b_done[t]
            delta = self.b_rew[t] + GAMMA * nv * nonterm - self.b_val[t]
            gae = delta + GAMMA * LAM * nonterm * gae
            adv[t] = gae
        return adv, adv + self.b_val


class FusedLeg:
    """(b)."""

    def __init__(self, torch, n, T, inp, dev, n_stack=None):
        from gym_usv_amd.rollout import DeviceRollout
        self.torch, self.inp, self.T = torch, inp, T
        self.ro = DeviceRollout(n, T, W, A, dev, n_stack=n_stack)
        self.i = 0

    def rollout(self):
        inp, ro = self.inp, self.ro
        with self.torch.no_grad():
            for t in range(self.T):
                i = self.i % inp.pool
                self.i += 1
                ro.put_obs(t, inp.window(t), inp.act[i], inp.val[i], inp.logp[i])
                ro.put_step(t, inp.rew[i], inp.term[i], inp.trunc[i], inp.final)
            return ro.gae(inp.value(inp.window(self.T)), inp.value(ro.term_obs), GAMMA, LAM)


class StoreLeg(FusedLeg):
    """(s): put_obs alone."""

    def rollout(self):
        inp, ro = self.inp, self.ro
        for t in range(self.T):
            ro.put_obs(t, inp.window(t), inp.act[0], inp.val[0], inp.logp[0])


def gather_bytes_per_sample(w=W, a=A):
    """gather: the obs row, the action and the four scalars read once and written once, and the index."""
    return 2 * 4 * (w + a + 4) + 8


class GatherLeg:
    """One minibatch per call: consecutive slices of a device permutation of the rollout `ro`, which a
    FusedLeg has filled.  how = "kernel": ro.gather; "torch": update()'s six indexed reads."""

    def __init__(self, torch, ro, B, how):
        self.torch, self.ro, self.B, self.how = torch, ro, B, how
        self.M = ro.n_steps * ro.n
        self.perm = torch.randperm(self.M, device=ro.device, generator=torch.Generator(device=ro.device).manual_seed(7))
        self.at = 0
        if how == "torch":
            M = self.M
            self.flat = (ro.obs.reshape(M, -1), ro.act.reshape(M, -1), ro.val.reshape(M), ro.logp.reshape(M),
                         ro.adv.reshape(M), ro.ret.reshape(M))

    def rollout(self):
        if self.at + self.B > self.M:
            self.at = 0
        i = self.perm[self.at:self.at + self.B]
        self.at += self.B
        if self.how == "torch":
            return [x[i] for x in self.flat]
        return self.ro.gather(i)


def frames_main(torch, args, dev):
    res = {"what": "interleaved same-process A/B, one stream, HIP events: frame-deduplicated storage "
                   "(DeviceRollout(n_stack=5)) against full storage of the same build; store_* = put_obs alone and "
                   "fused_* = a whole rollout (T steps + advantages), us per rollout; gather_* = one minibatch of B "
                   "samples, us per minibatch (frames / full: DeviceRollout.gather, torch: six indexed reads)",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "rollouts_per_round": args.reps,
           "gathers_per_round": 10 * args.reps, "n_stack": K, "obs_dim": D, "act_dim": A, "done_rate": DONE_RATE,
           "peak_bytes_per_s": PEAK, "sizes": {}}
    for n, T, B in ((4096, 32, 4096), (65536, 8, 65536)):
        inp = Inputs(torch, n, 64 if n <= 4096 else 16, dev)
        legs = {"store_full": StoreLeg(torch, n, T, inp, dev),
                "store_frames": StoreLeg(torch, n, T, inp, dev, n_stack=K),
                "fused_full": FusedLeg(torch, n, T, inp, dev),
                "fused_frames": FusedLeg(torch, n, T, inp, dev, n_stack=K)}
        for k in ("fused_full", "fused_frames"):
            legs[k].rollout()                                             # the buffers the gathers read
        legs["gather_frames"] = GatherLeg(torch, legs["fused_frames"].ro, B, "kernel")
        legs["gather_full"] = GatherLeg(torch, legs["fused_full"].ro, B, "kernel")
        legs["gather_torch"] = GatherLeg(torch, legs["fused_full"].ro, B, "torch")
        reps = {k: args.reps * (10 if k.startswith("gather") else 1) for k in legs}
        for k, leg in legs.items():
            run_events(torch, leg, args.warmup)
        big = torch.randn((8192, 8192), device=dev)

        def behind():
            for _ in range(4):
                torch.mm(big, big)
        ev = {k: [] for k in legs}
        queued = {"store_full": [], "store_frames": []}
        order = ["store_full", "store_frames", "fused_full", "fused_frames", "gather_frames", "gather_full",
                 "gather_torch"]                                          # the gathers after the rollouts that refill
        for _ in range(args.rounds):
            for k in order:
                ev[k].append(run_events(torch, legs[k], reps[k]))
            for k in queued:
                queued[k].append(run_events(torch, legs[k], 4, behind))
        entry = {k: summary(v) for k, v in ev.items()}
        for k, v in queued.items():                                       # the kernels alone, launches pre-queued
            entry[k]["queued"] = summary(v)
        f, g = entry["store_frames"]["queued"], entry["store_full"]["queued"]
        f["full_over_this_median"] = round(g["median_us"] / f["median_us"], 2)
        f["max_below_full_min"] = f["max_us"] < g["min_us"]
        entry["n_steps"], entry["batch"] = T, B
        moved = {"store_full": store_bytes_per_env() * n * T,
                 "store_frames": 2 * 4 * ((A + 2) * T + W + D * (T - 1)) * n}
        for k in ("gather_frames", "gather_full", "gather_torch"):
            moved[k] = gather_bytes_per_sample() * B
        for k, b in moved.items():
            rate = b / (entry[k]["median_us"] * 1e-6)
            entry[k]["bytes"] = b
            entry[k]["achieved_bytes_per_s"] = round(rate, 1)
            entry[k]["hbm_peak_frac"] = round(rate / PEAK, 4)
        for k in ("store", "fused"):
            f, g = entry[k + "_frames"], entry[k + "_full"]
            f["full_over_this_median"] = round(g["median_us"] / f["median_us"], 2)
            f["max_below_full_min"] = f["max_us"] < g["min_us"]
        for k in ("gather_frames", "gather_full"):
            entry[k]["torch_over_this_median"] = round(entry["gather_torch"]["median_us"] / entry[k]["median_us"], 2)
        ro_f, ro_o = legs["fused_frames"].ro, legs["fused_full"].ro
        entry["obs_storage_bytes"] = {"frames": ro_f.frames.numel() * 4, "full": ro_o.obs.numel() * 4}
        res["sizes"][f"{n}x{T}"] = entry
        print(json.dumps({f"{n}x{T}": entry}), flush=True)
        del legs, inp, ro_f, ro_o, big
        torch.cuda.empty_cache()
    return res


def run_events(torch, leg, reps, behind=None):
    """HIP-event us per rollout of `reps` back-to-back rollouts.  `behind`: a callable that first puts
    some 10 ms of other work on the stream, so that the launches queue up behind it and the events see
    the kernels back to back, without the host's launch rate."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="rollouts per round and leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", action="store_true", help="the frame-storage and gather legs instead")
    ap.add_argument("--out", default=None,
                    help="default: profiles/rollout_ab.json, profiles/rollout_frames_ab.json with --frames")
    args = ap.parse_args()
    name = "rollout_frames_ab.json" if args.frames else "rollout_ab.json"
    args.out = args.out or os.path.join(ROOT, "profiles", name)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rollout_ab.py needs a GPU")
    dev = torch.device("cuda", 0)
    if args.frames:
        write(args.out, frames_main(torch, args, dev))
        return
    res = {"what": "interleaved same-process A/B, one stream, HIP-event time per rollout (T steps + advantages): "
                   "torch = examples/ppo_torch.py's buffer stores, truncation bookkeeping with host syncs and "
                   "advantages(); fused = DeviceRollout; store = put_obs alone",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "rollouts_per_round": args.reps,
           "n_stack": K, "obs_dim": D, "act_dim": A, "done_rate": DONE_RATE, "peak_bytes_per_s": PEAK, "sizes": {}}
    for n, T in ((4096, 32), (65536, 8)):
        inp = Inputs(torch, n, 64 if n <= 4096 else 16, dev)
        legs = {"torch": TorchLeg(torch, n, T, inp, dev), "fused": FusedLeg(torch, n, T, inp, dev),
                "store": StoreLeg(torch, n, T, inp, dev)}
        for leg in legs.values():
            run_events(torch, leg, args.warmup)
        ev = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                ev[k].append(run_events(torch, leg, args.reps))
        entry = {k: summary(v) for k, v in ev.items()}
        entry["n_steps"] = T
        b = store_bytes_per_env() * n * T
        rate = b / (entry["store"]["median_us"] * 1e-6)
        entry["store"]["bytes_per_rollout"] = b
        entry["store"]["achieved_bytes_per_s"] = round(rate, 1)
        entry["store"]["hbm_peak_frac"] = round(rate / PEAK, 4)
        entry["fused"]["torch_over_this_median"] = round(entry["torch"]["median_us"] / entry["fused"]["median_us"], 2)
        entry["fused"]["max_below_torch_min"] = entry["fused"]["max_us"] < entry["torch"]["min_us"]
        res["sizes"][f"{n}x{T}"] = entry
        print(json.dumps({f"{n}x{T}": entry}), flush=True)
        del legs, inp
        torch.cuda.empty_cache()
    write(args.out, res)


def write(out, res):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
