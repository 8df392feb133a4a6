"""Jumping knowledge's 'max' (PyG's ``JumpingKnowledge('max')`` as models/models.py:810, 840, 869, 897 use it): the
autograd seam over ``sngnn_jk_max_forward`` / ``sngnn_jk_max_backward`` (csrc/jk.hip) and the plain op sequence the A/B
switch and every input outside the kernel's case run.

    jk_max   out = torch.stack(xs, -1).max(-1)[0]          (the first maximal layer wins a tie; a NaN wins and sticks)

The reference's line stacks the L layers into an [N, C, L] copy, reduces it and keeps an int64 index per element; its
backward scatters into a zeroed [N, C, L] tensor and hands every layer a stride-L view.  The kernel reads each layer's
rows once, writes the maximum and one byte per element (the layer it came from - all the backward saves), and the
backward writes each layer's dense gradient once."""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib

# A/B switch of the fused jump (csrc/jk.hip; tests flip it, SNGNN_JK_FUSE=0 starts a process with it off): off, jk_max
# runs torch.stack(...).max(...)
FUSE_JK = os.environ.get("SNGNN_JK_FUSE", "1") != "0"

MAX_LAYERS = 8          # SNGNN_JK_MAX_LAYERS

last_path = None        # "fused" | "plain": what the last jk_max ran


def _pointers(ts):
    """The host array of device pointers the entries read during the call (None: a NULL entry)."""
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


class _JKMax(torch.autograd.Function):
    """``max_l xs[l]`` as one launch; ``which`` (uint8, the winning layer per element) is all the backward saves, and
    it is not written where no layer requires a gradient."""

    @staticmethod
    def forward(ctx, *xs):
        xs = [x.contiguous() for x in xs]
        n, c = xs[0].shape
        out = torch.empty_like(xs[0])
        which = torch.empty((n, c), dtype=torch.uint8, device=out.device) if any(ctx.needs_input_grad) else None
        _lib.call("sngnn_jk_max_forward", out.device, _pointers(xs), len(xs), n, c, out, which)
        if which is not None:
            ctx.save_for_backward(which)
        return out

    @staticmethod
    def backward(ctx, g):
        which, = ctx.saved_tensors
        g = g.contiguous()
        n, c = g.shape
        grads = [torch.empty_like(g) if need else None for need in ctx.needs_input_grad]
        _lib.call("sngnn_jk_max_backward", g.device, g, which, len(grads), n, c, _pointers(grads))
        return tuple(grads)


def jk_fusable(xs) -> bool:
    """1 .. 8 fp32 GPU [N, C] tensors of one shape on one device (C >= 1)."""
    x0 = xs[0]
    return (1 <= len(xs) <= MAX_LAYERS and x0.dim() == 2 and x0.size(1) >= 1
            and all(x.dtype == torch.float32 and x.is_cuda and x.device == x0.device for x in xs))


def jk_max_plain(xs) -> torch.Tensor:
    """The reference's op sequence."""
    return torch.stack(list(xs), dim=-1).max(dim=-1)[0]


def jk_max(xs) -> torch.Tensor:
    """Differentiable (in every layer) elementwise maximum over the layers ``xs`` (a sequence of [N, C] tensors of one
    shape on the GPU), with ``torch.stack(xs, -1).max(-1)``'s semantics exactly.  One layer returns ``xs[0]``.  Up to
    ``MAX_LAYERS`` fp32 layers run the kernel (non-contiguous ones are made contiguous); more layers, half rows and
    ``FUSE_JK`` off run :func:`jk_max_plain`.  An empty list, CPU tensors and layers of different shapes are refused."""
    global last_path
    xs = list(xs)
    if not xs or not all(torch.is_tensor(x) for x in xs):
        raise ValueError("jk_max needs a non-empty sequence of tensors")
    if not all(x.is_cuda for x in xs):
        raise ValueError("the layers must live on the GPU (there is no CPU path)")
    if any(x.shape != xs[0].shape for x in xs):
        raise ValueError(f"the layers must have one shape, got {[tuple(x.shape) for x in xs]}")
    if len(xs) == 1:
        return xs[0]
    if FUSE_JK and jk_fusable(xs):
        last_path = "fused"
        return _JKMax.apply(*xs)
    last_path = "plain"
    return jk_max_plain(xs)
