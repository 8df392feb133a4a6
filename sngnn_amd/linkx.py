"""LINKX's join of the two embeddings (models/models.py:1135-1143): the autograd seam over ``sngnn_linkx_join_*``
(csrc/linkx.hip) and the plain op sequence the A/B switch and every input outside the kernels' case run.  Re-exported
by ``sngnn_amd.ops`` (``ops.linkx_join``, ``ops.linkx_join_plain``).

    a = log_softmax(zA), x = log_softmax(zX)      (lsm=False: a = zA, x = zX)
    y = relu(W [a | x] + b + a + x)

``zA`` and ``zX`` are the last linears' outputs of ``mlpA`` and ``mlpX``: the reference's ``MLP.forward`` ends in
``log_softmax``, so the join works on log-probabilities, and the kernel takes the row's maximum and sum in the tile it
multiplies."""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import _lib

# A/B switch of the fused join (csrc/linkx.hip; tests flip it, SNGNN_LINKX_FUSE=0 starts a process with it off): off,
# linkx_join runs the reference's op sequence in torch - log_softmax, cat, the linear map, add, relu.  On by default: the
# fused arm won every run of tools/bench_linkx.py against it (profiles/linkx.txt)
FUSE_LINKX = os.environ.get("SNGNN_LINKX_FUSE", "1") != "0"

MAX_WIDTH = 128          # SNGNN_LINKX_MAX_H: W resident in LDS
TILE_ROWS = (32, 64)     # rows of a tile of the kernels: 32 at H <= 64, 64 above (join_threads / 8)

last_path = None         # "fused" | "plain": what the last linkx_join ran


def _check(zA, zX, weight, bias):
    for t, what in ((zA, "zA"), (zX, "zX"), (weight, "weight"), (bias, "bias")):
        if not torch.is_tensor(t):
            raise ValueError(f"{what} must be a tensor")
        if not t.is_cuda:
            raise ValueError(f"{what} must live on the GPU (there is no CPU path)")
        if t.device != zA.device or t.dtype != zA.dtype:
            raise ValueError(f"{what} must have zA's device and dtype ({zA.device}, {zA.dtype}), got {t.device}, {t.dtype}")
    if zA.dim() != 2 or zA.size(1) < 1 or zX.shape != zA.shape:
        raise ValueError(f"zA and zX must have one shape [N, H] with H >= 1, got {tuple(zA.shape)} and {tuple(zX.shape)}")
    h = zA.size(1)
    if weight.shape != (h, 2 * h):
        raise ValueError(f"weight must be [{h}, {2 * h}] (Linear(2H, H).weight), got {tuple(weight.shape)}")
    if bias.shape != (h,):
        raise ValueError(f"bias must be [{h}], got {tuple(bias.shape)}")


class _LinkxJoin(torch.autograd.Function):
    """``sngnn_linkx_join_forward`` / ``_backward``.  Saved: ``ax = [a | x]`` (with the output and the weight); the
    weight and bias gradients are one ``sngnn_linear_wgrad(g, ax)`` with F = 2H."""

    @staticmethod
    def forward(ctx, zA, zX, weight, bias, lsm):
        zA, zX = zA.contiguous(), zX.contiguous()
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        n, h = zA.shape
        ax = torch.empty((n, 2 * h), dtype=torch.float32, device=zA.device)
        y = torch.empty_like(zA)
        _lib.call("sngnn_linkx_join_forward", zA.device, zA, zX, w, b, n, h, int(lsm), ax, y)
        ctx.lsm = bool(lsm)
        ctx.save_for_backward(ax, y, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        ax, y, w = ctx.saved_tensors
        n, h = y.shape
        gy = gy.contiguous()
        if gy.dtype != torch.float32 or gy.shape != y.shape:
            raise ValueError(f"grad_y must be a float32 {tuple(y.shape)} tensor, got {gy.dtype} {tuple(gy.shape)}")
        g, gzA, gzX = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
        _lib.call("sngnn_linkx_join_backward", y.device, gy, y, ax, w, n, h, int(ctx.lsm), g, gzA, gzX)
        gw = gb = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            gw = torch.empty((h, 2 * h), dtype=torch.float32, device=y.device)
            gb = torch.empty(h, dtype=torch.float32, device=y.device)
            ws = _lib.workspace("wgrad", _lib.load().sngnn_linear_wgrad_workspace_bytes(n, h, 2 * h), y.device)
            _lib.call("sngnn_linear_wgrad", y.device, g, ax, n, h, 2 * h, gw, gb, ws)          # g^T [a | x], sum g
        return gzA, gzX, gw, gb, None


def _log_softmax(z):
    """``log_softmax(z, dim=1)`` with the row's sum of exponentials added and logged in float64, as the kernel does.  The
    MLPs' outputs may be log-probabilities already (``embed_logits`` chains, the tests' rows): their sum is 1 + a little,
    and torch's fp32 sum rounds the little - all of the largest element's result - away."""
    zs = z - z.detach().amax(dim=1, keepdim=True)          # (the result does not depend on the shift: no gradient)
    return zs - zs.exp().sum(dim=1, keepdim=True, dtype=torch.float64).log().to(z.dtype)


class _PlainLinear(torch.autograd.Function):
    """``F.linear`` with ``ops.linear``'s weight gradient (``sngnn_linear_wgrad``: the [C, F] result reduces over all N
    rows); restated here because this module is a leaf under ``ops`` and does not import it."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g, x = g.contiguous(), x.contiguous()
        (n, f), c = x.shape, g.size(1)
        gw = torch.empty((c, f), dtype=torch.float32, device=g.device)
        gb = torch.empty(c, dtype=torch.float32, device=g.device)
        ws = _lib.workspace("wgrad", _lib.load().sngnn_linear_wgrad_workspace_bytes(n, c, f), g.device)
        _lib.call("sngnn_linear_wgrad", g.device, g, x, n, c, f, gw, gb, ws)
        return (g.mm(weight) if ctx.needs_input_grad[0] else None), gw, gb


def linkx_join_plain(zA: torch.Tensor, zX: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, lsm: bool = True,
                     inner_activation: bool = False, inner_dropout: bool = False) -> torch.Tensor:
    """The reference's op sequence (models.py:476, 1137-1143) on the GPU: ``log_softmax`` of either embedding, ``cat``,
    the linear map with ``ops.linear``'s weight gradient, ``F.dropout(x)`` with its default ``training=True`` as the reference has it, ``relu``, add and
    ``relu``.  Any width and floating type."""
    _check(zA, zX, weight, bias)
    a = _log_softmax(zA) if lsm else zA
    x = _log_softmax(zX) if lsm else zX
    cat = torch.cat((a, x), dim=-1)
    h = _PlainLinear.apply(cat, weight, bias) if cat.dtype == torch.float32 else F.linear(cat, weight, bias)
    if inner_dropout:
        h = F.dropout(h)
    if inner_activation:
        h = F.relu(h)
    return F.relu(h + a + x)


def join_fusable(zA, inner_activation: bool = False, inner_dropout: bool = False) -> bool:
    return (FUSE_LINKX and not inner_activation and not inner_dropout and torch.is_tensor(zA)
            and zA.dtype == torch.float32 and zA.dim() == 2 and 1 <= zA.size(1) <= MAX_WIDTH)


def linkx_join(zA: torch.Tensor, zX: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, lsm: bool = True, *,
               inner_activation: bool = False, inner_dropout: bool = False) -> torch.Tensor:
    """Differentiable (in all four tensors) ``relu(W [a | x] + b + a + x)`` with ``a, x = log_softmax(zA),
    log_softmax(zX)`` (``lsm=False``: the embeddings themselves).  ``zA``, ``zX`` [N, H]; ``weight`` [H, 2H] and
    ``bias`` [H] of ``Linear(2H, H)``.  GPU tensors; fused (two kernels and the library's weight gradient, no host
    synchronisation) for fp32 rows with ``H <= MAX_WIDTH``; ``FUSE_LINKX`` off, a wider join, another floating type,
    ``inner_activation`` or ``inner_dropout`` run :func:`linkx_join_plain`.  ``linkx.last_path`` says which."""
    global last_path
    if join_fusable(zA, inner_activation, inner_dropout):
        _check(zA, zX, weight, bias)
        last_path = "fused"
        return _LinkxJoin.apply(zA, zX, weight, bias, bool(lsm))
    last_path = "plain"
    return linkx_join_plain(zA, zX, weight, bias, lsm, inner_activation, inner_dropout)
