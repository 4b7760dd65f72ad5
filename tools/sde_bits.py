#!/usr/bin/env python
"""SHA-256 of every output of the gSDE heads on fixed inputs: do two builds of the library compute the same bits?

    USV_LIB_PATH=<parent's libusvhip.so> python tools/sde_bits.py --label parent --out profiles/sde_refactor_bits.json
    python tools/sde_bits.py --label new --out profiles/sde_refactor_bits.json

The first run writes its digests to --out; a later run compares its own with them entry for entry, adds its label
to "builds" and records "equal" (exit status 1, and its digests kept under its label, where they differ).  Through
DeviceSDE: sample, weights, squashed and evaluate forward and backward, evaluate with and without the PPO arguments
and with an attached and a detached latent.  Inputs: the host tests' (tests/sde_squash_ref.py, sde_eval_ref.py),
hashed too, over their SHAPES plus (2, 4096, 2), sixteen passes, and (2050, 4, 1), R = 3 with a ragged last partial.
Needs a GPU; there is no fallback.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gym-usv_amd"), os.path.join(ROOT, "tests")]


def digests(torch, dev, n, L, A):
    import sde_eval_ref as E
    import sde_squash_ref as Q
    from gym_usv_amd import DeviceSDE
    out = {}

    def put(name, *tensors):
        for i, t in enumerate(tensors):
            if t is not None:
                out[f"{name}[{i}]"] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    def leaves(*arrays, grad=(True, True, True)):
        ts = [torch.from_numpy(x).to(dev) for x in arrays]
        return [t.requires_grad_(g) for t, g in zip(ts, grad)] + ts[3:]

    head = DeviceSDE(n, L, A, dev, Q.SEED, Q.LOW[:A], Q.HIGH[:A], env_id_offset=Q.GID0)
    head.epoch, sq, ev = Q.EPOCH, Q.inputs(n, L, A), E.inputs(n, L, A)
    put("inputs", *(torch.from_numpy(x) for x in (*sq, *ev)))
    with torch.no_grad():
        mean, lat, std, _, _ = leaves(*sq, grad=(False,) * 3)
        put("sample", *head.sample(mean, lat, std))
        put("weights", head.weights(std))
        put("squashed.no_grad", *head.squashed(mean, lat, std))
    mean, lat, std, ga, gl = leaves(*sq)
    s = head.squashed(mean, lat, std)
    put("squashed", *s)
    ((s.actions * ga).sum() + (s.log_prob * gl).sum()).backward()
    put("squashed.grad", mean.grad, lat.grad, std.grad)
    for ppo in (True, False):
        for attached in (True, False):
            mean, lat, std, act, old, adv, gl, gs = leaves(*ev, grad=(True, attached, True))
            e = head.evaluate(mean, lat, std, act, *((old, adv, E.CLIP) if ppo else ()))
            name = f"evaluate.{'ppo' if ppo else 'plain'}.{'attached' if attached else 'detached'}"
            put(name, *e)
            ((e.log_prob * gl).sum() + ((e.surrogate * gs).sum() if ppo else 0.0)).backward()
            put(name + ".grad", mean.grad, lat.grad, std.grad)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True, help="this build's name in --out, e.g. parent or new")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sde_refactor_bits.json"))
    args = ap.parse_args()
    import torch
    import sde_squash_ref as Q
    if not torch.cuda.is_available():
        raise SystemExit("sde_bits.py needs a GPU")
    what = "SHA-256 of the bytes of every DeviceSDE output per shape (n, L, A); equal: every build in builds gave these"
    res = json.load(open(args.out)) if os.path.exists(args.out) else {"what": what, "builds": [], "equal": True}
    shapes = (*Q.SHAPES, (2, 4096, 2), (2050, 4, 1))
    mine = {f"{n}x{L}x{A}": digests(torch, torch.device("cuda", 0), n, L, A) for n, L, A in shapes}
    res["builds"].append(args.label)
    if res.setdefault("digests", mine) != mine:
        res["equal"], res[args.label] = False, mine
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out, "builds", res["builds"], "equal", res["equal"])
    sys.exit(0 if res["equal"] else 1)


if __name__ == "__main__":
    main()
