#!/usr/bin/env python
"""Device replay buffer (DeviceReplay: frame-deduplicated ring, one-launch sampling) against a torch
full-storage replay of the same build.

    python tools/replay_ab.py [--rounds 7] [--out profiles/replay_ab.json]

One process, one stream, HIP events; the legs alternate every round.  k = 5, D = 143 (W = 715), scripted
inputs resident in HBM (a pool of steps; done rate 1/216 per env and step, half of them truncations), the
stacked observation read from a ring-shaped buffer at the window offset of the step.
  store_device / store_torch    one env step into the buffer: DeviceReplay.put_obs + put_step (two launches)
                                against two [R, N, W] tensors written by row copies (obs, the where() of
                                final_stack and the next window, action, reward, done, timeout)
  gather_device / gather_torch  one minibatch of B pre-drawn indices: DeviceReplay.gather (one launch)
                                against five indexed reads and the dones product
at 65 536 envs x R = 16 (B = 65 536) and 4 096 envs x R = 96 (about config_sac's 400 000 transitions;
B = 256, config_sac's, and B = 4 096).  Per leg: median and min..max over the rounds, plain and "queued":
the same calls issued behind some 10 ms of other work on the stream, so the events time the kernels back
to back and not the host's call rate.  Bytes per second count what each leg has to move at least (every
field read once and written once) against the 8 TB/s peak.  Needs a GPU; there is no fallback.
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


def store_bytes_per_env(device):
    """One step: the obs floats kept (2 D, or 2 k D), the action, the reward, term and trunc in, done / timeout
    (and age) out."""
    floats = (2 * D if device else 2 * W) + A + 1
    return 2 * 4 * floats + 2 + (3 if device else 2 * 4)


def gather_bytes_per_sample(device):
    """One sample: the index, the obs floats read ((k + 1) D, or 2 k D), the 2 k D written, the action and the
    two scalars read and written."""
    return 8 + 4 * ((K + 1) * D if device else 2 * W) + 4 * 2 * W + 2 * 4 * (A + 2)


class Inputs:
    def __init__(self, torch, n, pool, dev):
        from gym_usv_amd import _lib
        g = torch.Generator(device=dev).manual_seed(4242)
        stride = _lib.load().usv_wrap_ring_stride(D, K)
        self.ring = torch.randn((n, stride), device=dev, generator=g)
        self.final = torch.randn((n, W), device=dev, generator=g)
        self.act = torch.randn((pool, n, A), device=dev, generator=g)
        self.rew = torch.randn((pool, n), device=dev, generator=g)
        done = torch.rand((pool, n), device=dev, generator=g) < DONE_RATE
        self.trunc = done & (torch.rand((pool, n), device=dev, generator=g) < 0.5)
        self.term = done & ~self.trunc
        self.pool = pool

    def window(self, t):
        off = ((t + 1) % K) * D
        return self.ring[:, off:off + W]


class DeviceStore:
    def __init__(self, torch, n, R, inp, dev):
        from gym_usv_amd import DeviceReplay
        self.inp, self.rb, self.t = inp, DeviceReplay(n, R * n, W, A, dev, n_stack=K), 0

    def call(self):
        inp, t = self.inp, self.t
        i = t % inp.pool
        self.rb.put_obs(inp.window(t), inp.act[i])
        self.rb.put_step(inp.rew[i], inp.term[i], inp.trunc[i], inp.window(t + 1), inp.final)
        self.t = t + 1


class TorchStore:
    def __init__(self, torch, n, R, inp, dev):
        self.torch, self.inp, self.R, self.t = torch, inp, R, 0
        z = lambda *s: torch.zeros(s, device=dev)       # noqa: E731
        self.obs, self.next_obs, self.act = z(R, n, W), z(R, n, W), z(R, n, A)
        self.rew, self.done, self.timeout = z(R, n), z(R, n), z(R, n)

    def call(self):
        torch, inp, t = self.torch, self.inp, self.t
        i, p = t % inp.pool, t % self.R
        self.obs[p] = inp.window(t)
        self.act[p] = inp.act[i]
        term, trunc = inp.term[i], inp.trunc[i]
        done = term | trunc
        self.next_obs[p] = torch.where(done[:, None], inp.final, inp.window(t + 1))
        self.rew[p] = inp.rew[i]
        self.done[p] = done.float()
        self.timeout[p] = (trunc & ~term).float()
        self.t = t + 1

    def nbytes(self):
        return sum(x.numel() * x.element_size() for x in (self.obs, self.next_obs, self.act, self.rew, self.done,
                                                          self.timeout))


class Gather:
    """One minibatch per call: consecutive slices of pre-drawn uniform indices."""

    def __init__(self, torch, store, B, n, R, dev):
        self.store, self.B, self.at = store, B, 0
        self.idx = torch.randint(0, R * n, (64 * B,), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
        if isinstance(store, TorchStore):
            s = store
            self.flat = (s.obs.reshape(-1, W), s.act.reshape(-1, A), s.next_obs.reshape(-1, W), s.done.reshape(-1),
                         s.timeout.reshape(-1), s.rew.reshape(-1))

    def call(self):
        if self.at + self.B > self.idx.numel():
            self.at = 0
        i = self.idx[self.at:self.at + self.B]
        self.at += self.B
        if isinstance(self.store, TorchStore):
            o, a, nx, dn, to, rw = self.flat
            return o[i], a[i], nx[i], (dn[i] * (1 - to[i])).reshape(-1, 1), rw[i].reshape(-1, 1)
        return self.store.rb.gather(i)


def run_events(torch, leg, reps, behind=None):
    """HIP-event us per call of `reps` back-to-back calls.  `behind`: a callable that first puts some 10 ms
    of other work on the stream, so that the launches queue up behind it."""
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


def versus(dev_entry, torch_entry):
    for d, t in ((dev_entry, torch_entry), (dev_entry["queued"], torch_entry["queued"])):
        d["torch_over_this_median"] = round(t["median_us"] / d["median_us"], 2)
        d["max_below_torch_min"] = d["max_us"] < t["min_us"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=40, help="calls per round and leg")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_ab.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("replay_ab.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"what": "interleaved same-process A/B, one stream, HIP events: DeviceReplay against a torch full-storage "
                   "replay (two [R, N, W] tensors); store_* = one env step into the buffer, us per step; gather_*_B = "
                   "one minibatch of B samples, us per minibatch; queued = the same calls issued behind ~10 ms of "
                   "other work on the stream",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_round": args.reps, "n_stack": K,
           "obs_dim": D, "act_dim": A, "done_rate": DONE_RATE, "peak_bytes_per_s": PEAK, "sizes": {}}
    for n, R, batches in ((65536, 16, (65536,)), (4096, 96, (256, 4096))):
        inp = Inputs(torch, n, 16 if n > 4096 else 64, dev)
        stores = {"store_device": DeviceStore(torch, n, R, inp, dev), "store_torch": TorchStore(torch, n, R, inp, dev)}
        for leg in stores.values():                                       # fill both rings
            for _ in range(R + 1):
                leg.call()
        legs = dict(stores)
        for B in batches:
            legs[f"gather_device_{B}"] = Gather(torch, stores["store_device"], B, n, R, dev)
            legs[f"gather_torch_{B}"] = Gather(torch, stores["store_torch"], B, n, R, dev)
        for leg in legs.values():
            run_events(torch, leg, args.warmup)
        big = torch.randn((8192, 8192), device=dev)

        def behind():
            for _ in range(4):
                torch.mm(big, big)
        ev, queued = {k: [] for k in legs}, {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                ev[k].append(run_events(torch, leg, args.reps))
            for k, leg in legs.items():
                queued[k].append(run_events(torch, leg, min(args.reps, 16), behind))
        entry = {k: summary(v) for k, v in ev.items()}
        for k, v in queued.items():
            entry[k]["queued"] = summary(v)
        for k in legs:
            device = "_device" in k
            b = store_bytes_per_env(device) * n if k.startswith("store") else gather_bytes_per_sample(device) * int(k.rsplit("_", 1)[1])
            entry[k]["bytes"] = b
            for e in (entry[k], entry[k]["queued"]):
                rate = b / (e["median_us"] * 1e-6)
                e["achieved_bytes_per_s"] = round(rate, 1)
                e["hbm_peak_frac"] = round(rate / PEAK, 4)
        versus(entry["store_device"], entry["store_torch"])
        for B in batches:
            versus(entry[f"gather_device_{B}"], entry[f"gather_torch_{B}"])
        entry["rows"], entry["batches"] = R, list(batches)
        entry["allocated_bytes"] = {"device": stores["store_device"].rb.nbytes(), "torch": stores["store_torch"].nbytes()}
        res["sizes"][f"{n}x{R}"] = entry
        print(json.dumps({f"{n}x{R}": entry}), flush=True)
        del legs, stores, inp, big
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
