#!/usr/bin/env python
"""Scan-free step (ignore_obstacles) against the default scanning step of the same build.

    python tools/ignore_obstacles_ab.py [--rounds 7] [--steps 2000] [--out profiles/ignore_obstacles_ab.json]

Per configuration two handles of the same library, seed and env count (one scanning, one ignoring) are
stepped in alternation on the same device, in one process: each round times `--steps` back-to-back
usv_step launches of one, then of the other, with one HIP event pair around the block (bench.py's launch
path: the C-ABI call with its arguments bound once, actions resident in HBM).  Reported per configuration
and handle: the median and min..max over the rounds of the event time per step, the host's enqueue time
per step (the loop without a synchronise: a step shorter than it is bound by the launch path, not by the
kernel), and for the ignoring step its algorithmic bytes per env and the fraction of the 8 TB/s HBM
roofline they give at the median time (DESIGN.md "ignore_obstacles").  Needs a GPU; there is no fallback.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-usv_amd"))

CONFIGS = [("usv-simple", "f32", 65536), ("usv-simple", "f32", 524288),
           ("usv-asmc-simple", "f32", 65536), ("usv-simple", "f64", 65536)]
PEAK = 8.0e12      # HBM3E peak, B/s (MI355X)


def noscan_bytes_per_env_step(env_id, precision):
    """Bytes one scan-free env-step must move, counted as bench.py's algorithmic_bytes_per_env_step
    counts the scanning step, without the obstacle rows and the obstacle count: action in; obs, reward
    and two flags out; 16 real state fields and elapsed read; 9 real fields, elapsed and the scan flag
    written; usv-asmc-simple's 16 ASMC values read and written."""
    w = 4 if precision == "f32" else 8
    asmc = 2 * 16 * w if env_id == "usv-asmc-simple" else 0
    return 8 + 143 * 4 + w + 2 + (16 * w + 4) + (9 * w + 2 * 4) + asmc


class Leg:
    def __init__(self, env_id, precision, n, ignore, pool, seed=0, lib_path=None):
        import torch
        import gym_usv_amd
        self.torch = torch
        env = self.env = gym_usv_amd.make_vec(env_id, n, device=0, seed=seed, precision=precision,
                                              ignore_obstacles=ignore, lib_path=lib_path)
        env.reset(seed=seed)
        dev = env.device
        gen = torch.Generator(device=dev).manual_seed(7919)
        lo, span = torch.tensor([0.2, -1.0], device=dev), torch.tensor([0.8, 2.0], device=dev)
        self.acts = torch.rand((pool, n, 2), device=dev, generator=gen) * span + lo
        self.obs = torch.empty((n, 143), device=dev)
        self.fobs = torch.empty((n, 143), device=dev)
        self.rew = torch.empty(n, device=dev, dtype=torch.float32 if precision == "f32" else torch.float64)
        self.term = torch.empty(n, device=dev, dtype=torch.uint8)
        self.trunc = torch.empty(n, device=dev, dtype=torch.uint8)
        self.stream = torch.cuda.current_stream(dev)
        vp = ctypes.c_void_p
        outs = (vp(self.obs.data_ptr()), vp(self.rew.data_ptr()), vp(self.term.data_ptr()),
                vp(self.trunc.data_ptr()), vp(self.fobs.data_ptr()), vp(self.stream.cuda_stream))
        self.bound = [(env._h, vp(self.acts[i].data_ptr())) + outs for i in range(pool)]
        self.fn = env.lib.usv_step
        self.k = 0

    def run(self, steps):
        """(event us per step, host enqueue us per step) of `steps` back-to-back launches."""
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        pool = len(self.bound)
        t0 = time.perf_counter()
        a.record(self.stream)
        for _ in range(steps):
            if self.fn(*self.bound[self.k % pool]) != 0:
                raise RuntimeError(self.env.lib.usv_last_error().decode())
            self.k += 1
        b.record(self.stream)
        t1 = time.perf_counter()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / steps, (t1 - t0) * 1e6 / steps


def summary(xs):
    return {"median_us": round(statistics.median(xs), 3), "min_us": round(min(xs), 3), "max_us": round(max(xs), 3),
            "rounds_us": [round(x, 3) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ignore_obstacles_ab.json"))
    ap.add_argument("--configs", default="", help="comma-separated indices into CONFIGS (default: all)")
    ap.add_argument("--split-lib", default=None,
                    help="a library built with -DUSV_NOSCAN_F64_SPLIT: also compare usv-asmc-simple f64's scan-free "
                         "step with the ASMC chain inside the step (this build) and in its own launch (that one)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ignore_obstacles_ab.py needs a GPU")
    pick = [int(i) for i in args.configs.split(",")] if args.configs else range(len(CONFIGS))
    res = {"what": "interleaved same-process A/B of the scan-free step (ignore_obstacles) against the default "
                   "scanning step of the same build: HIP-event time per usv_step over back-to-back launches, "
                   "handles alternating every round",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "steps_per_round": args.steps,
           "peak_bytes_per_s": PEAK, "configs": {}}
    for ci in pick:
        env_id, precision, n = CONFIGS[ci]
        steps = args.steps if n <= 65536 else max(200, args.steps // 8)
        pool = 16 if n <= 65536 else 4
        legs = {"scan": Leg(env_id, precision, n, False, pool), "ignore": Leg(env_id, precision, n, True, pool)}
        for leg in legs.values():
            leg.run(args.warmup)
        ev = {k: [] for k in legs}
        host = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                e, h = leg.run(steps)
                ev[k].append(e)
                host[k].append(h)
        b = noscan_bytes_per_env_step(env_id, precision)
        ig, sc = summary(ev["ignore"]), summary(ev["scan"])
        ig["host_enqueue_us"] = round(statistics.median(host["ignore"]), 3)
        sc["host_enqueue_us"] = round(statistics.median(host["scan"]), 3)
        ig["algorithmic_bytes_per_env"] = b
        ig["achieved_bytes_per_s"] = round(b * n / (ig["median_us"] * 1e-6), 1)
        ig["hbm_roofline_frac"] = round(b * n / (ig["median_us"] * 1e-6) / PEAK, 4)
        entry = {"steps_per_round": steps, "scan": sc, "ignore": ig,
                 "ignore_median_below_scan_min": ig["median_us"] < sc["min_us"]}
        res["configs"][f"{env_id}_{precision}_{n}"] = entry
        print(json.dumps({f"{env_id}_{precision}_{n}": entry}), flush=True)
        for leg in legs.values():
            leg.env.close()
        del legs
        torch.cuda.empty_cache()
    if args.split_lib:
        n = 65536
        legs = {"chain_inside": Leg("usv-asmc-simple", "f64", n, True, 16),
                "chain_split": Leg("usv-asmc-simple", "f64", n, True, 16, lib_path=os.path.abspath(args.split_lib))}
        for leg in legs.values():
            leg.run(args.warmup)
        ev = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                ev[k].append(leg.run(args.steps)[0])
        torch.cuda.synchronize()
        same = all(bool(torch.equal(getattr(legs["chain_inside"], t), getattr(legs["chain_split"], t)))
                   for t in ("obs", "rew", "trunc"))
        entry = {k: summary(v) for k, v in ev.items()}
        entry["outputs_bitwise_equal_after_all_steps"] = same
        res["usv-asmc-simple_f64_65536_chain_placement"] = entry
        print(json.dumps({"usv-asmc-simple_f64_65536_chain_placement": entry}), flush=True)
        for leg in legs.values():
            leg.env.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
