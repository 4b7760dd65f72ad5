"""The CAPS regulariser (usv_caps_perturb / usv_caps_loss) restated from its definition, not from the C++ header.

``loss``: NumPy float32 in the stated order.  Per row with A elements, k ascending: a = pi(mean), b = pi(mean_next),
c = pi(mean_near) (pi = tanh when squashing, the identity otherwise), dt = a - b, ds = a - c, nT = sqrt(sum dt dt),
nS = sqrt(sum ds ds), the sums ascending from +0.0 with the multiply and the add rounded separately; temporal =
S(nT) / B and spatial = S(nS) / B with sac_loss_ref's sum S; loss = (lambda_t temporal) + (lambda_s spatial).  The
unit gradients: wT = 0 where nT == 0 and (lambda_t / B) / nT elsewhere, wS likewise, eT = wT dt, eS = wS ds,
g_mean = (eT + eS) da, g_next = (-eT) db, g_near = (-eS) dc with da = 1 - a a when squashing and no factor otherwise.
With squash=False programs are compared with it bit for bit (NumPy's tanh is not the programs').

``torch_loss``: torch-CPU float64 autograd of the definition's lines (``torch.linalg.vector_norm`` over the action
axis, ``.mean()``).  Errors against it: the loss's over the loss, each gradient's over (lambda_t + lambda_s) / B.

``normals``: the perturbation's z in float64: element j of row r is normal j % 4 of sde_ref's block j // 4 with
counter (r lo, r hi, epoch, j // 4).
"""
import numpy as np

import sac_loss_ref as S
import sde_ref as R

f32 = np.float32
CEILING = 1e-4                                            # on every normalised error: a condition
FLOOR = 0.05                                              # the least distance of a row in action space (squash cases)
ROWS = (1, 63, 256, 1024, 1025, 2049)
ACTS = (1, 2, 3, 8)


def pi(m, squash):
    m = np.asarray(m, f32)
    if not squash:
        return m, None
    a = np.tanh(m).astype(f32)
    return a, f32(1.0) - a * a


def distance(d):
    """sqrt of the ascending float32 sum of squares over the last axis."""
    acc = np.zeros(d.shape[0], f32)
    for k in range(d.shape[1]):
        acc = acc + d[:, k] * d[:, k]
    return np.sqrt(acc)


def loss(mean, mean_next, mean_near, lambda_t, lambda_s, squash):
    """dict of float32 loss, temporal, spatial and g_mean, g_next, g_near [B, A]."""
    B = f32(len(mean))
    lt, ls = f32(lambda_t), f32(lambda_s)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        (a, da), (b, db), (c, dc) = pi(mean, squash), pi(mean_next, squash), pi(mean_near, squash)
        dt, ds = a - b, a - c
        nT, nS = distance(dt), distance(ds)
        temporal, spatial = f32(S.fsum(nT) / B), f32(S.fsum(nS) / B)
        wT = np.where(nT == 0, f32(0.0), (lt / B) / np.where(nT == 0, f32(1.0), nT)).astype(f32)
        wS = np.where(nS == 0, f32(0.0), (ls / B) / np.where(nS == 0, f32(1.0), nS)).astype(f32)
        eT, eS = wT[:, None] * dt, wS[:, None] * ds
        g_mean, g_next, g_near = eT + eS, -eT, -eS
        if squash:
            g_mean, g_next, g_near = g_mean * da, g_next * db, g_near * dc
    return {"loss": f32((lt * temporal) + (ls * spatial)), "temporal": temporal, "spatial": spatial,
            "g_mean": g_mean.astype(f32), "g_next": g_next.astype(f32), "g_near": g_near.astype(f32)}


def scaled(g, up):
    return S.scaled(g, up)


def torch_loss(mean, mean_next, mean_near, lambda_t, lambda_s, squash):
    """The definition in torch-CPU float64 with autograd: the same dict in float64."""
    import torch
    t = lambda v: torch.tensor(np.asarray(v, np.float64), dtype=torch.float64, requires_grad=True)   # noqa: E731
    m, mn, mr = t(mean), t(mean_next), t(mean_near)
    act = torch.tanh if squash else (lambda x: x)
    a = act(m)
    temporal = torch.linalg.vector_norm(a - act(mn), dim=-1).mean()
    spatial = torch.linalg.vector_norm(a - act(mr), dim=-1).mean()
    total = float(f32(lambda_t)) * temporal + float(f32(lambda_s)) * spatial
    total.backward()
    return {"loss": float(total.detach()), "temporal": float(temporal.detach()), "spatial": float(spatial.detach()),
            "g_mean": m.grad.numpy(), "g_next": mn.grad.numpy(), "g_near": mr.grad.numpy()}


def errors(got, ref, lambda_t, lambda_s):
    """{quantity: largest normalised error}: loss, temporal, spatial over themselves, the gradients over
    (lambda_t + lambda_s) / B."""
    B = len(ref["g_mean"])
    out = {k: abs(float(got[k]) - ref[k]) / abs(ref[k]) for k in ("loss", "temporal", "spatial")}
    scale = (float(lambda_t) + float(lambda_s)) / B
    for k in ("g_mean", "g_next", "g_near"):
        out[k] = float(np.abs(np.asarray(got[k], np.float64).reshape(ref[k].shape) - ref[k]).max()) / scale
    return out


def inputs(B, A, seed=0, equal_rows=True, nan_row=False):
    """(mean, mean_next, mean_near) float32 [B, A] within the clipped mean's +-2.  With equal_rows, every fifth row
    of mean_next equals mean bit for bit (zero temporal distance) and row 2 of mean_near does (zero spatial distance);
    nan_row puts one NaN into mean_near's middle row."""
    rng = np.random.default_rng(7000 * B + 10 * A + seed)
    mean = rng.uniform(-2.0, 2.0, (B, A)).astype(f32)
    mean_next = (mean + 0.3 * rng.standard_normal((B, A))).astype(f32)
    mean_near = (mean + 0.05 * rng.standard_normal((B, A))).astype(f32)
    if equal_rows:
        mean_next[::5] = mean[::5]
        if B > 2:
            mean_near[2] = mean[2]
    if nan_row:
        mean_near[B // 2, A - 1] = np.nan
    return mean, mean_next, mean_near


def floored_inputs(B, A, seed=0, squash=True):
    """Inputs whose every row has both distances in action space at least FLOOR: with smaller ones the direction
    dt / nT amplifies the rounding of tanh (an error of u in a and b is an error of about u / nT in the gradient).
    The first action of mean_next and of mean_near is moved away from mean's, towards zero where tanh is steepest,
    until |a_0 - b_0| >= FLOOR in float64; the other actions are free."""
    mean, mean_next, mean_near = inputs(B, A, seed, equal_rows=False)
    act = np.tanh if squash else (lambda x: x)
    a0 = act(mean[:, 0].astype(np.float64))
    for other in (mean_next, mean_near):
        target = a0 - np.sign(a0 + (a0 == 0)) * (FLOOR + 0.01)       # in (-1, 1): |a0| < 1
        moved = (np.arctanh(target) if squash else target).astype(f32)
        close = np.abs(a0 - act(other[:, 0].astype(np.float64))) < FLOOR + 0.005
        other[close, 0] = moved[close]
    for other in (mean_next, mean_near):
        d = np.linalg.norm(act(mean.astype(np.float64)) - act(other.astype(np.float64)), axis=1)
        assert (d >= FLOOR).all(), d.min()
    return mean, mean_next, mean_near


def blocks_of(W):
    return (W + 3) // 4


def normals(seed, epoch, rows, W, row0=0):
    """(z [rows, W] float64, r [rows, W] float64: the Box-Muller radius of each element's pair) of rows
    row0 .. row0 + rows - 1."""
    nb = blocks_of(W)
    z, r = R.normals(seed, row0, epoch, rows, 4 * nb, 1)
    return z.reshape(rows, 4 * nb)[:, :W], r.reshape(rows, 4 * nb)[:, :W]
