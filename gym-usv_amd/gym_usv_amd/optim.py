"""The optimizer step without its eager-torch glue: ``clip_grad_norm_`` and ``Adam.step()`` over a whole parameter
list as one HIP launch without clipping and two with it.

``DeviceAdam`` is ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` followed by ``torch.optim.Adam(params, lr,
betas, eps).step()`` (torch 2.x; ``amsgrad=False``, ``weight_decay=0``, ``maximize=False``) behind ``usv_adam_step``
(include/usv_hip.h)::

    opt = DeviceAdam(model.parameters(), lr=3e-4, max_grad_norm=0.5)
    opt.zero_grad()                # set_to_none, as torch's default
    loss.backward()
    norm = opt.step()              # 0-dim device tensor: the norm before clipping; None without max_grad_norm
    opt.lr = 1e-4                  # read at every step (schedules); opt.step_count is a host int

The norm's sum of squares is taken in a fixed order that depends on the tensors' sizes alone
(gym-usv_amd/csrc/usv_optim_math.hpp; tests/optim_ref.py restates it), so a run's parameters are bitwise
reproducible, whatever the grid or the stream.  All on the current stream, without a host sync.

``DeviceAdam(..., capturable=True)`` is the form a HIP graph can replay (``torch.optim.Adam``'s ``capturable``): the
step number and ``lr`` live in a small block of device memory, a one-thread launch at the head of every ``step()``
moves the number on and derives the bias corrections from it on the device (``usv_adam_step_dev``), and no kernel
argument depends on the step.  ``gym_usv_amd.capture_step`` records such a step once and replays it.

Two deviations from torch.  ``.grad`` is not written back: the clipped gradient exists in the kernel's registers
only (SB3 discards it at the next ``zero_grad``).  A parameter whose ``.grad`` is None at ``step()`` is a
``ValueError``: torch skips such a parameter and keeps a step count per parameter, this class keeps one count for
the list.
"""
from __future__ import annotations

import math

import torch

from . import _lib


def refuse_capture(who, remedy):
    """``RuntimeError`` where the current stream is recording a graph: ``who`` passes a host counter to its kernels
    as an argument, which a graph would freeze."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{who} while the stream is capturing a graph: {remedy}")


def _check_hyper(lr, betas, eps, max_grad_norm):
    """The hyper-parameter rules, which need no device; returns them as floats (``max_grad_norm`` None: -1.0)."""
    lr, eps, b1, b2 = float(lr), float(eps), float(betas[0]), float(betas[1])
    if not (math.isfinite(lr) and lr >= 0.0):
        raise ValueError(f"lr must be finite and >= 0, not {lr}")
    if not (math.isfinite(eps) and eps >= 0.0):
        raise ValueError(f"eps must be finite and >= 0, not {eps}")
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"betas must be in [0, 1), not {(b1, b2)}")
    if max_grad_norm is None:
        return lr, (b1, b2), eps, -1.0
    mg = float(max_grad_norm)
    if not mg >= 0.0:
        raise ValueError(f"max_grad_norm must be >= 0 or None, not {mg}")
    return lr, (b1, b2), eps, mg


class DeviceAdam:
    """Adam with an optional global-norm gradient clip over ``params`` (float32, contiguous, on one ROCm device;
    anything else is a ``ValueError``; there is no CPU fallback).  ``lr``, ``betas``, ``eps`` and ``max_grad_norm`` are
    attributes read at every ``step``.  The moments live in two flat buffers (``exp_avg``, ``exp_avg_sq``: each
    parameter's segment padded to four floats).

    ``capturable=True``: ``step()`` is legal inside ``torch.cuda.graph`` and a replay is a step that counts.  The step
    number and ``lr`` live in a 32-byte device block (``usv_adam_step_dev``, include/usv_hip.h); ``step()`` issues one
    launch more than the default form, the one thread that advances the block.  ``opt.lr = x`` writes the block with
    an ordinary stream-ordered write (a ``RuntimeError`` while capturing: the write would be recorded, not made);
    reading ``opt.step_count`` copies the block's number to the host, **a host sync**: keep it out of the training
    loop.  The betas, ``eps`` and ``max_grad_norm`` are baked into a captured graph.  So are the addresses of the
    gradients, hence the rule torch's whole-network capture uses: put ``zero_grad(set_to_none=True)`` *inside* the
    captured region, so that the captured backward allocates the gradients from the graph's private pool, at
    addresses that every replay finds again.  The bias corrections are derived on the device, whose ``pow`` is not
    the host's: they are within one float32 ulp of the default form's, and where they are equal so is every result.

    In the default form ``step()`` under capture is a ``RuntimeError``: it would freeze the step number."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, lib_path=None,
                 capturable=False):
        params = list(params)
        if not params:
            raise ValueError("params must be a non-empty list of tensors")
        for p in params:
            if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("every parameter must be a contiguous float32 tensor")
            if p.device != params[0].device:
                raise ValueError("every parameter must be on one device")
        if params[0].device.type != "cuda":
            raise ValueError("DeviceAdam runs on a ROCm GPU only (no CPU fallback)")
        lr, self.betas, self.eps, mg = _check_hyper(lr, betas, eps, max_grad_norm)
        self.max_grad_norm = None if max_grad_norm is None else mg
        self.device = params[0].device
        self.lib = _lib.load(lib_path)
        self.params, self.capturable = params, bool(capturable)
        self._clock = None
        if self.capturable:                                  # lr (f64), step (i64), step_size and bc2_sqrt (f32), pad
            words = (int(self.lib.usv_adam_clock_bytes()) + 7) // 8
            self._clock = torch.zeros(words, dtype=torch.int64, device=self.device)
        self.lr, self.step_count = lr, 0
        n = len(params)
        self._n = n
        self._table = (_lib.UsvAdamTensor * n)(*(_lib.UsvAdamTensor(p.data_ptr(), None, p.numel()) for p in params))
        self._state_floats = int(self.lib.usv_adam_state_floats(self._table, n))
        self._scratch_floats = int(self.lib.usv_adam_scratch_floats(self._table, n))
        z = lambda k: torch.zeros(max(4, k), dtype=torch.float32, device=self.device)     # noqa: E731
        self.exp_avg, self.exp_avg_sq = z(self._state_floats), z(self._state_floats)
        self._scratch = z(self._scratch_floats)              # its ticket word: zero once, the kernels keep it so
        self._offsets, at = [], 0
        for p in params:
            self._offsets.append(at)
            at += (p.numel() + 3) // 4 * 4

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        if self._clock is not None:                          # the default form's is checked by the step that reads it
            value = _check_hyper(value, (0.0, 0.0), 0.0, None)[0]
            refuse_capture("DeviceAdam.lr was set", "set it between replays, outside the captured region")
            self._clock[0:1].view(torch.float64).fill_(value)
        self._lr = value

    @property
    def step_count(self):
        """The number of steps taken.  With ``capturable=True`` it is read from the device block: a host sync."""
        return self._steps if self._clock is None else int(self._clock[1].item())

    @step_count.setter
    def step_count(self, value):
        value = int(value)
        if value < 0:
            raise ValueError("step_count must be >= 0")
        if self._clock is not None:
            refuse_capture("DeviceAdam.step_count was set", "set it outside the captured region")
            self._clock[1:2].fill_(value)
        self._steps = value

    def clock(self):
        """``capturable=True``: ``(step, lr, step_size, bc2_sqrt)`` of the last step as the device block holds them (the
        two scalars as float32 values); a host sync, for tests and checkpoints."""
        if self._clock is None:
            raise RuntimeError("clock() is for capturable=True: the default form keeps no device block")
        host = self._clock.cpu()
        f = host.view(torch.float32)
        return int(host[1]), float(host.view(torch.float64)[0]), f[4].item(), f[5].item()

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none or p.grad is None:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.zero_()

    def step(self):
        """Two launches (one without ``max_grad_norm``) per 96 tensors on the current stream, and with ``capturable=True``
        one more for the whole list.  Returns the norm of all gradients before clipping as a 0-dim device tensor, or
        None without ``max_grad_norm``."""
        tab, keep = self._table, None
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None:
                raise ValueError(f"parameter {i} has no .grad: DeviceAdam steps every parameter of its list")
            if g.dtype is not torch.float32:
                raise ValueError(f"the .grad of parameter {i} is not float32")
            if not g.is_contiguous():
                g = g.contiguous()
                keep = (keep or []) + [g]                    # alive until the launches are queued
            tab[i].param, tab[i].grad = p.data_ptr(), g.data_ptr()
        mg = self.max_grad_norm
        if self._clock is None:
            refuse_capture("DeviceAdam.step() of a default (capturable=False) optimizer was called",
                           "its step number is a kernel argument that a graph would freeze; make it with capturable=True")
        norm = None if mg is None else torch.empty((), dtype=torch.float32, device=self.device)
        tail = (self.betas[0], self.betas[1], self.eps, -1.0 if mg is None else mg, self._scratch.data_ptr(),
                self._scratch_floats, None if norm is None else norm.data_ptr(), _lib.stream_ptr(self.device))
        head = (tab, self._n, self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self._state_floats)
        if self._clock is None:
            _lib.check(self.lib.usv_adam_step(*head, self._steps + 1, self._lr, *tail), self.lib)
            self._steps += 1
        else:
            _lib.check(self.lib.usv_adam_step_dev(*head, self._clock.data_ptr(), self._clock.numel() * 8, *tail),
                       self.lib)
        return norm

    def _segment(self, buf, i):
        p = self.params[i]
        return buf[self._offsets[i]:self._offsets[i] + p.numel()].view(p.shape)

    def state_dict(self):
        """``torch.optim.Adam``'s layout: ``state[i] = {step, exp_avg, exp_avg_sq}`` (copies out of the flat buffers; empty
        before the first step, as torch's) and one param group.  ``max_grad_norm`` is not part of it."""
        proto = torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps)
        group = dict(proto.param_groups[0], params=list(range(self._n)))
        state, steps = {}, self.step_count
        if steps > 0:
            for i in range(self._n):
                state[i] = {"step": torch.tensor(float(steps)),
                            "exp_avg": self._segment(self.exp_avg, i).clone(),
                            "exp_avg_sq": self._segment(self.exp_avg_sq, i).clone()}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        """From ``state_dict()`` or a ``torch.optim.Adam``'s over the same parameters (one param group; ``amsgrad``,
        ``weight_decay`` and ``maximize`` off; one step count for all parameters)."""
        groups, state = sd["param_groups"], sd["state"]
        if len(groups) != 1 or len(groups[0]["params"]) != self._n:
            raise ValueError(f"the state dict must have one param group of {self._n} parameters")
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize") or g.get("weight_decay"):
            raise ValueError("DeviceAdam has no amsgrad, maximize or weight_decay")
        lr, betas, eps, _ = _check_hyper(g["lr"], g["betas"], g["eps"], None)
        ids = list(g["params"])
        steps = {int(state[k]["step"]) for k in ids if k in state}
        if len(steps) > 1 or (state and any(k not in state for k in ids)):
            raise ValueError("DeviceAdam keeps one step count: every parameter's state must have the same step")
        for i, k in enumerate(ids):
            if k in state:
                for name, buf in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
                    if tuple(state[k][name].shape) != tuple(self.params[i].shape):
                        raise ValueError(f"{name} of parameter {i} has another shape than the parameter")
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        for i, k in enumerate(ids):
            if k in state:
                self._segment(self.exp_avg, i).copy_(state[k]["exp_avg"])
                self._segment(self.exp_avg_sq, i).copy_(state[k]["exp_avg_sq"])
        self.betas, self.eps = betas, eps
        self.lr, self.step_count = lr, steps.pop() if steps else 0          # capturable: both write the device block
