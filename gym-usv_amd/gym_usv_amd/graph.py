"""Record one gradient step as a HIP graph and replay it: the kernels of the trainer classes are no longer the cost
of an update, launching them one Python call at a time is.

    opt = DeviceAdam(params, lr=3e-4, max_grad_norm=0.5, capturable=True)
    head = DeviceSDE(B, 256, 2, device, seed, low, high, capturable=True)

    def step():                                  # reads static input tensors, returns what is to be logged
        head.reset_noise()
        opt.zero_grad()                          # set_to_none: the captured backward allocates from the graph's pool
        loss = compute_loss(static_obs)
        loss.backward()
        opt.step()
        return loss

    captured = capture_step(step)                # step() has now run warmup + 1 times
    for batch in batches:
        static_obs.copy_(batch)
        loss = captured.replay()                 # the same tensor every time, holding this replay's value

What a graph freezes is every kernel argument and every address.  So the objects inside ``fn`` must keep their
counters in device memory (``capturable=True`` for ``DeviceAdam``, ``DeviceSDE`` and ``DeviceCAPS``; in their default
form they raise ``RuntimeError`` under capture), ``DevicePolyak.prepare()`` must have uploaded its table (the warm-up
calls see to that), inputs must be static tensors that the caller copies into, and nothing in ``fn`` may synchronise,
copy to the host or branch on a device value.  Scratch buffers that grow with the batch grow in the warm-up calls:
warm up with the batch size that is captured.
"""
from __future__ import annotations

import torch


class CapturedStep:
    """``graph``: the ``torch.cuda.CUDAGraph``.  ``out``: what the captured call returned, static tensors that every
    replay overwrites.  ``replay()`` launches the graph on the current stream and returns ``out``."""

    def __init__(self, graph, out):
        self.graph, self.out = graph, out

    def replay(self):
        self.graph.replay()
        return self.out


def capture_step(fn, warmup=3):
    """Runs ``fn()`` ``warmup`` times on a side stream (allocations, scratch growth and table uploads happen there),
    captures one more call into a graph and replays it once, so that the captured call has taken effect like the
    others: ``fn`` has then run ``warmup + 1`` times, and ``out`` holds the last call's results.  The capture is on
    one stream, so the graph is a chain of kernels without parallel branches.  Returns a ``CapturedStep``."""
    if warmup < 1:
        raise ValueError("warmup must be >= 1: the first call allocates and uploads, which cannot be captured")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    graph.replay()
    return CapturedStep(graph, out)
