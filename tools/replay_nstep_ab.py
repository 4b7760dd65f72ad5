#!/usr/bin/env python
"""N-step sampling of the device replay buffer (DeviceReplay.gather_nstep, one launch) against the torch
full-storage gather_nstep of examples/sac_torch.py and against the one-step DeviceReplay.gather of the same
build at the same batch.

    python tools/replay_nstep_ab.py [--rounds 7] [--out profiles/replay_nstep_ab.json] [--libs NAME=PATH ...]

One process, one stream, HIP events; the legs alternate every round (tools/replay_ab.py's method, inputs and
helpers).  k = 5, D = 143 (W = 715), done rate 1/216 per env and step, half of them truncations; both rings
hold the same R + 1 scripted steps.
  gather_device_B         DeviceReplay.gather of B pre-drawn indices: the yardstick of the same build
  nstep_device_N_B        DeviceReplay.gather_nstep with n_steps = N in (1, 3, 5): one launch
  nstep_torch_N_B         TorchReplay.gather_nstep: three indexed reads per step of the run and six more
at 4 096 envs x R = 96 (B = 256 and 4 096) and 65 536 envs x R = 16 (B = 65 536).  Per leg: median and
min..max over the rounds, plain and "queued" (the calls issued behind some 10 ms of other work on the stream,
so the events time the kernels back to back and not the host's call rate).  Bytes per second count what a
leg has to move at least against the 8 TB/s peak: gather (k + 1) D floats read and 2 k D written per sample,
gather_nstep 2 k D read and 2 k D written plus N (done, timeout, age, reward) scans.  --libs NAME=PATH adds
legs nstep_NAME_N_B for further builds of the library on the same ring (e.g. -DUSV_RP_NSTEP_SHARE=1), checked
bitwise against the product before timing.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "gym-usv_amd"), os.path.join(ROOT, "examples"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import replay_ab as AB  # noqa: E402

K, D, A, W, PEAK = AB.K, AB.D, AB.A, AB.W, AB.PEAK
N_STEPS = (1, 3, 5)
GAMMA = 0.99


def nstep_bytes_per_sample(device, n_steps):
    """The index, 2 k D floats read and 2 k D written, the action read and written, the three scalars
    written, and per step of the run the reward and the done / timeout (/ age) bytes (floats in torch)."""
    return 8 + 4 * 2 * W + 4 * 2 * W + 2 * 4 * A + 3 * 4 + n_steps * (4 + (3 if device else 8))


class Leg:
    def __init__(self, fn, idx, B):
        self.fn, self.idx, self.B, self.at = fn, idx, B, 0

    def call(self):
        if self.at + self.B > self.idx.numel():
            self.at = 0
        i = self.idx[self.at:self.at + self.B]
        self.at += self.B
        return self.fn(i)


def view_of(torch, rb, n_steps, lib_path=None):
    """A second DeviceReplay over the buffers of `rb`, with its own n_steps (no call changes the table) and,
    with `lib_path`, another build of the library."""
    from gym_usv_amd import DeviceReplay
    v = DeviceReplay(rb.n, rb.rows * rb.n, rb.w, rb.a, rb.device, n_stack=rb.n_stack, n_steps=n_steps, gamma=GAMMA,
                     lib_path=lib_path)
    for name in ("frames", "next_frame", "act", "rew", "done", "timeout", "age", "age_now"):
        setattr(v, name, getattr(rb, name))
    v._puts, v._count = rb._puts, rb._count
    v._bind()
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=40, help="calls per round and leg")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_nstep_ab.json"))
    ap.add_argument("--libs", nargs="*", default=[], metavar="NAME=PATH",
                    help="further builds of the library: their gather_nstep on the same ring, legs nstep_NAME_N_B")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("replay_nstep_ab.py needs a GPU")
    from gym_usv_amd.replay import discount_table
    from sac_torch import TorchReplay
    dev = torch.device("cuda", 0)
    libs = dict(x.split("=", 1) for x in args.libs)
    res = {"what": "interleaved same-process A/B, one stream, HIP events, us per minibatch of B samples: "
                   "DeviceReplay.gather_nstep (n_steps N) against the torch full-storage gather_nstep and against "
                   "DeviceReplay.gather of the same build; queued = the same calls issued behind ~10 ms of other work "
                   "on the stream",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_round": args.reps, "n_stack": K,
           "obs_dim": D, "act_dim": A, "gamma": GAMMA, "done_rate": AB.DONE_RATE, "peak_bytes_per_s": PEAK, "sizes": {}}
    for n, R, batches in ((4096, 96, (256, 4096)), (65536, 16, (65536,))):
        inp = AB.Inputs(torch, n, 16 if n > 4096 else 64, dev)
        store = AB.DeviceStore(torch, n, R, inp, dev)
        shadow = TorchReplay(n, R * n, W, A, dev)
        for t in range(R + 1):                                             # the same steps into both rings
            i = t % inp.pool
            shadow.put_obs(inp.window(t), inp.act[i])
            shadow.put_step(inp.rew[i], inp.term[i], inp.trunc[i], inp.window(t + 1), inp.final)
            store.call()
        views = {ns: view_of(torch, store.rb, ns) for ns in N_STEPS}
        others = {(name, ns): view_of(torch, store.rb, ns, os.path.abspath(path)) for name, path in libs.items()
                  for ns in N_STEPS}
        tables = {ns: discount_table(GAMMA, ns) for ns in N_STEPS}
        legs, nbytes = {}, {}
        for B in batches:
            idx = torch.randint(0, R * n, (64 * B,), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
            legs[f"gather_device_{B}"] = Leg(store.rb.gather, idx, B)
            nbytes[f"gather_device_{B}"] = AB.gather_bytes_per_sample(True) * B
            for ns in N_STEPS:
                legs[f"nstep_device_{ns}_{B}"] = Leg(views[ns].gather_nstep, idx, B)
                legs[f"nstep_torch_{ns}_{B}"] = Leg(lambda i, ns=ns: shadow.gather_nstep(i, ns, tables[ns]), idx, B)
                nbytes[f"nstep_device_{ns}_{B}"] = nstep_bytes_per_sample(True, ns) * B
                nbytes[f"nstep_torch_{ns}_{B}"] = nstep_bytes_per_sample(False, ns) * B
                for name in libs:
                    legs[f"nstep_{name}_{ns}_{B}"] = Leg(others[name, ns].gather_nstep, idx, B)
                    nbytes[f"nstep_{name}_{ns}_{B}"] = nbytes[f"nstep_device_{ns}_{B}"]
            # builds of the library agree bitwise before they are timed (the torch ring does not: the pool's
            # windows do not evolve by the frame-stack rule, as in replay_ab.py; the tests compare the two)
            i = idx[:B]
            for ns in N_STEPS:
                for lib in libs:
                    for x, y in zip(views[ns].gather_nstep(i), others[lib, ns].gather_nstep(i)):
                        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (lib, ns, B)
        for leg in legs.values():
            AB.run_events(torch, leg, args.warmup)
        big = torch.randn((8192, 8192), device=dev)

        def behind():
            for _ in range(4):
                torch.mm(big, big)
        ev, queued = {k: [] for k in legs}, {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                ev[k].append(AB.run_events(torch, leg, args.reps))
            for k, leg in legs.items():
                queued[k].append(AB.run_events(torch, leg, min(args.reps, 16), behind))
        entry = {k: AB.summary(v) for k, v in ev.items()}
        for k, v in queued.items():
            entry[k]["queued"] = AB.summary(v)
        for k in legs:
            entry[k]["bytes"] = nbytes[k]
            for e in (entry[k], entry[k]["queued"]):
                rate = nbytes[k] / (e["median_us"] * 1e-6)
                e["achieved_bytes_per_s"] = round(rate, 1)
                e["hbm_peak_frac"] = round(rate / PEAK, 4)
        for B in batches:
            one = entry[f"gather_device_{B}"]
            for ns in N_STEPS:
                d, t = entry[f"nstep_device_{ns}_{B}"], entry[f"nstep_torch_{ns}_{B}"]
                AB.versus(d, t)
                for e, o in ((d, one), (d["queued"], one["queued"])):
                    e["over_gather_median"] = round(e["median_us"] / o["median_us"], 3)
                for name in libs:
                    v = entry[f"nstep_{name}_{ns}_{B}"]
                    for e, o in ((v, d), (v["queued"], d["queued"])):
                        e["over_product_median"] = round(e["median_us"] / o["median_us"], 3)
        entry["rows"], entry["batches"], entry["n_steps"] = R, list(batches), list(N_STEPS)
        res["sizes"][f"{n}x{R}"] = entry
        print(json.dumps({f"{n}x{R}": entry}), flush=True)
        del legs, views, others, store, shadow, inp, big
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
