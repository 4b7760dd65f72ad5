"""Cold paths of the block-queue step ("Cold paths").

The same-step reset and the terminal-obs path of step_q_body re-read their arguments where they begin,
and the reset takes its env's episode counter (the Philox counter of its draws) from a copy staged in
LDS before the barrier instead of loading it.  A counter staged from the wrong env, lane half or block
changes the reset's random stream, so every comparison here is bitwise: per step obs, reward,
terminated, truncated and the final_obs rows of done envs, at the end the whole state blob.

References: the wave kernel (kind 1, "16,7,1"), whose reset still loads its own counter, and the split
queue (kind 4, "128,7,4").  Under test: the forced 128-env fused block ("128,7,5"; "128,7,6" for
usv-asmc-simple) and the default variant, at these env counts the 16-env small-block kernel.
Shapes: 129 (a full block plus a block of one env with no env B), 255 (an odd, partial block), 384.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = (129, 255, 384)
ENV_IDS = ("usv-simple", "usv-asmc-simple")
REFS = ("16,7,1", "128,7,4")
LIMIT_STAGGER = 6
# elapsed steps at the start of the staggered case, by env index mod 8 (pairs are envs 2p, 2p + 1): with
# a 6-step limit the pairs reset on different steps, env A first, env B first, or both on one step;
# the block index shifts the pattern, so a wave's last pair resets in some blocks and not in others
STAGGER = np.array([0, 3, 2, 2, 5, 1, 4, 4])


def fused_variant(env_id):
    return "128,7,6" if env_id == "usv-asmc-simple" else "128,7,5"


def make(env_id, n, **kw):
    import gym_usv_amd
    return gym_usv_amd.make_vec(env_id, n, device=0, **kw)


def _actions(n, T, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    lo = torch.tensor([0.2, -1.0], device="cuda")
    return [torch.rand(n, 2, device="cuda", generator=gen) * torch.tensor([0.8, 2.0], device="cuda") + lo
            for _ in range(T)]


@functools.lru_cache(maxsize=None)
def rollout(env_id, n, variant, case, api=False):
    """One rollout of `case`; returns (per-step outputs on the host, state blob, episode counters before
    the first step, episode counters at the end).  Cached: a reference runs once for all its tests.
    api=False steps through usv_step (no done mask, no info rows: the plain instantiations), api=True
    through the public step() with info rows (the DONE / INFO instantiations)."""
    T, limit = {"all": (7, 3), "stagger": (9, LIMIT_STAGGER), "explicit": (8, 4), "api": (9, 4)}[case]
    env = make(env_id, n, seed=17, max_episode_steps=limit, kernel_variant=variant, copy=False, info=api)
    env.reset(seed=17)
    if case == "stagger":
        i = np.arange(n)
        env.set_field("episode", 1000 + 37 * i)            # distinct per env
        env.set_field("elapsed", (STAGGER[i % 8] + i // 16) % LIMIT_STAGGER)
    ep0 = env.get_field("episode").copy()
    acts = _actions(n, T, 5)
    obs = torch.zeros(n, env.obs_dim, device="cuda")
    fobs = torch.zeros_like(obs)
    rew = torch.zeros(n, device="cuda")
    term = torch.zeros(n, dtype=torch.uint8, device="cuda")
    trunc = torch.zeros_like(term)
    outs = []
    for t, a in enumerate(acts):
        if case == "explicit" and t == 3:
            o, _ = env.reset(seed=91)                      # fresh counters for the next launch to stage
            outs.append((o.cpu().clone(),))
        if api:
            o, r, te, tr, info = env.step(a)
            dn = info["_final_obs"]
            assert torch.equal(dn, te | tr)
            fo = info["final_obs"]
            extra = tuple(info[k].cpu().clone() for k in ("position", "velocity", "ye", "angle_to_target"))
            te, tr = te.to(torch.uint8), tr.to(torch.uint8)
        else:
            assert env.step_raw(a, obs, rew, term, trunc, fobs) == 0
            o, r, te, tr, fo, extra = obs, rew, term, trunc, fobs, ()
            dn = (te | tr).bool()
        outs.append((o.cpu().clone(), r.cpu().clone(), te.cpu().clone(), tr.cpu().clone(),
                     fo[dn].cpu().clone()) + extra)
    torch.cuda.synchronize()
    blob = env.state_blob()
    ep1 = env.get_field("episode").copy()
    env.close()
    return outs, blob, ep0, ep1


def assert_same(env_id, n, case, api=False):
    for v in (fused_variant(env_id), None):
        got, blob, _, _ = rollout(env_id, n, v, case, api)
        for ref_v in REFS:
            ref, rblob, _, _ = rollout(env_id, n, ref_v, case, api)
            assert len(ref) == len(got)
            for t, (x, y) in enumerate(zip(ref, got)):
                for j, (p, q) in enumerate(zip(x, y)):
                    # bitwise (NaN-safe: a float compare would hide or invent differences)
                    assert p.shape == q.shape and np.array_equal(p.numpy().view(np.uint8), q.numpy().view(np.uint8)), \
                        f"{env_id} n={n} {case}: variant {v} differs from {ref_v} at entry {t}, output {j}"
            bad = np.flatnonzero(blob != rblob)
            assert bad.size == 0, f"{env_id} n={n} {case}: variant {v} vs {ref_v}: state differs in {bad.size} bytes"


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("env_id", ENV_IDS)
def test_all_envs_reset_twice(env_id, n):
    """3-step limit, 7 steps: every pair has both envs done on steps 3 and 6, each wave's last pair
    included, and every env's episode counter rose by exactly 2: one per reset, none missed or run
    twice.  (An env that starts an episode within the termination distance of an obstacle terminates on
    that episode's first step, in every variant alike, and is then reset three times in the 7 steps:
    its counter must have risen by exactly 3.  So the count is checked against the done flags.)"""
    assert_same(env_id, n, "all")
    for v in (fused_variant(env_id), None) + REFS:
        outs, _, ep0, ep1 = rollout(env_id, n, v, "all")
        dones = np.stack([((te | tr) != 0).numpy() for _, _, te, tr, _ in outs])      # [T, n]
        trunc = np.stack([(tr != 0).numpy() for _, _, _, tr, _ in outs])
        rose = ep1 - ep0
        assert np.array_equal(rose, dones.sum(0)), f"variant {v}: a reset did not bump its counter once"
        assert rose.min() >= 2, f"variant {v}: episode counters rose by {np.unique(rose)}"
        timed = trunc.sum(0) == dones.sum(0)               # envs whose every reset was the time limit's
        assert timed.sum() >= n // 2 and np.array_equal(rose[timed], np.full(timed.sum(), 2))
        assert dones[2].sum() >= n // 2 and dones[5].sum() >= n // 2


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("env_id", ENV_IDS)
def test_staggered_resets_with_distinct_counters(env_id, n):
    """Distinct episode counters and staggered elapsed steps: resets of env A only, env B only and of
    both, on different steps in different blocks."""
    assert_same(env_id, n, "stagger")
    _, _, ep0, ep1 = rollout(env_id, n, REFS[0], "stagger")
    assert (ep1 - ep0).min() >= 1                      # 9 steps of a 6-step limit: every env was reset


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("env_id", ENV_IDS)
def test_explicit_reset_mid_rollout(env_id, n):
    """An explicit reset(seed=...) between two launches: the next launch stages the fresh counters."""
    assert_same(env_id, n, "explicit")


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("env_id", ENV_IDS)
def test_public_step_with_done_mask_and_info(env_id, n):
    """The public step(): done mask and info rows on (the DONE / INFO instantiations)."""
    assert_same(env_id, n, "api", api=True)
