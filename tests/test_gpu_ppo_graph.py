"""examples/ppo_torch.py with ``--perm-kernel`` and ``--graph`` on the GPU: 64 envs x 8 steps, minibatches of 128,
2 epochs, 2 updates (M = 512: four minibatches an epoch, sixteen gradient steps)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FLAGS = dict(fused=True, frames=True, sde_kernel=True, eval_kernel=True, adam_kernel=True, loss_kernel=True,
             perm_kernel=True)
CFG = dict(envs=64, updates=2, n_steps=8, batch_size=128, seed=3, n_epochs=2, log=lambda s: None)
LOGGED = ("policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "explained_variance", "std_mean")


def ppo_torch():
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "examples")) if p not in sys.path]
    import ppo_torch
    return ppo_torch


def run(graph, **over):
    keep = {}
    hist = ppo_torch().train(graph=graph, keep=keep, **dict(FLAGS, **over), **CFG)
    ppo = keep["ppo"]
    return hist, [p.detach().clone() for p in ppo.model.parameters()], ppo


def bitwise(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_ppo_example_with_graph():
    mod = ppo_torch()
    for bad in (dict(FLAGS, adam_kernel=False), dict(FLAGS, perm_kernel=False), dict(FLAGS, eval_kernel=False),
                dict(FLAGS, loss_kernel=False), dict(FLAGS, check_loss=True), dict(FLAGS, check_eval=True)):
        with pytest.raises(ValueError):
            mod.train(graph=True, **bad, **CFG)
    h1, p1, ppo = run(True)
    h2, p2, _ = run(True)
    assert len(h1) == 2 and h1[-1]["env_steps"] == 2 * 8 * 64
    assert ppo.opt.step_count == 16                          # the warm-up's four steps were undone
    assert (ppo.sampler.epoch, ppo.sampler.batch) == (4, 0)
    assert bitwise(p1, p2)                                   # two runs of one seed
    for rec in h1:
        for k in LOGGED:
            assert np.isfinite(rec[k]), (k, rec)
    h3, p3, eager = run(False)
    assert eager.opt.step_count == 16 and (eager.sampler.epoch, eager.sampler.batch) == (4, 0)
    diff = max(float((a - b).abs().max()) for a, b in zip(p1, p3))
    print(f"PPO example, 64 envs x 8 steps, sixteen gradient steps: largest |parameter difference| with and without "
          f"--graph = {diff!r}")
    assert np.isfinite(diff)


@pytest.mark.parametrize("frames", (False, True))
def test_perm_kernel_without_graph_visits_every_sample(frames):
    """--perm-kernel alone, with the torch head, loss and optimizer: the sampler under the plain update loop."""
    keep = {}
    hist = ppo_torch().train(fused=True, frames=frames, perm_kernel=True, keep=keep, **CFG)
    ppo = keep["ppo"]
    assert len(hist) == 2 and (ppo.sampler.epoch, ppo.sampler.batch) == (4, 0) and ppo.ro.bad_indices() == 0
    for rec in hist:
        for k in LOGGED[:3]:
            assert np.isfinite(rec[k]), (k, rec)
