"""The fused training-mode batch norm between two conv layers (csrc/batchnorm.hip): the autograd seam over
``sngnn_bn_train_forward`` / ``sngnn_bn_train_backward`` (bias -> relu -> norm -> dropout) and ``sngnn_bn_post_forward`` /
``sngnn_bn_post_backward`` (norm -> relu -> dropout).  Re-exported by ``sngnn_amd.ops`` (``ops.batch_norm_act``,
``ops.batch_norm_post_act``)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib


def bn_train_workspace(c: int, device) -> torch.Tensor:
    """The scratch of ``sngnn_bn_train_forward`` / ``_backward`` at width ``c`` (grow-only, per device)."""
    return _lib.workspace("bn_train", _lib.load().sngnn_bn_train_workspace_bytes(int(c)), device)


class _BatchNormAct(torch.autograd.Function):
    """bias + relu + training-mode batch norm + dropout in three launches each way (``sngnn_bn_train_forward`` /
    ``_backward``).  Saved: x, the per-channel vectors, the caller's ``keep`` or the seed - nothing else of size
    [N, C]: the backward recomputes relu, xhat and the mask from x.  ``stats`` = (running_mean, running_var, eps,
    momentum), the running tensors None for a norm that tracks none.  ``act``: the ``HiddenEpilogue`` of the
    producer whose stores already applied bias + relu to ``x`` - ``grad_x`` carries relu' already, and the producer
    is told so (``premasked``)."""

    @staticmethod
    def forward(ctx, x, bias, gamma, beta, stats, p, keep, seed, act):
        n, c = x.shape
        running_mean, running_var, eps, momentum = stats
        out = torch.empty_like(x)
        mean = torch.empty(c, dtype=torch.float32, device=x.device)
        invstd = torch.empty_like(mean)
        scale = 1.0 / (1.0 - p) if p > 0.0 else 1.0
        _lib.call("sngnn_bn_train_forward", x.device, x, bias, n, c, gamma, beta, float(eps), float(momentum), running_mean,
                  running_var, keep, scale, seed, float(p), out, mean, invstd, bn_train_workspace(c, x.device))
        ctx.p, ctx.scale, ctx.act = float(p), scale, act
        # (the seed is saved as the tensor it is: advancing it in place before this node's backward trips autograd's
        # version check instead of drawing another mask silently)
        ctx.save_for_backward(x, bias, gamma, mean, invstd, keep, seed)
        return out

    @staticmethod
    def backward(ctx, g):
        x, bias, gamma, mean, invstd, keep, seed = ctx.saved_tensors
        n, c = x.shape
        g = g.contiguous()
        grad_x = torch.empty_like(x)
        grad_gamma, grad_beta = torch.empty_like(mean), torch.empty_like(mean)
        grad_bias = torch.empty_like(mean) if bias is not None else None
        _lib.call("sngnn_bn_train_backward", x.device, g, x, bias, n, c, gamma, mean, invstd, keep, ctx.scale, seed, ctx.p,
                  grad_x, grad_gamma, grad_beta, grad_bias, bn_train_workspace(c, x.device))
        if ctx.act is not None:
            ctx.act.premasked = grad_x.data_ptr()          # (which tensor: _take_premasked checks it)
        return grad_x, grad_bias, grad_gamma, grad_beta, None, None, None, None, None


def _bn_inputs(x, bn, bias, p, keep, seed):
    """The checks both orders share; returns ``(x, bias, gamma, beta, stats, p, keep, seed)`` as the kernels take them
    (and counts the batch in ``bn.num_batches_tracked``)."""
    if not isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
        raise ValueError("bn must be a BatchNorm1d module")
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError("x must be a [N, C] tensor")
    if x.dtype != torch.float32:
        raise ValueError("x must be float32 (the fused batch norm is fp32 only)")
    if not x.is_cuda:
        raise ValueError("x must live on the GPU (there is no CPU path)")
    if not 1 <= x.size(1) <= _lib.MAX_CHANNELS:
        raise ValueError(f"x: C must be in [1, {_lib.MAX_CHANNELS}]")
    x = x.contiguous()
    n, c = x.shape
    if n < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    if bn.num_features != c or not bn.affine or bn.weight is None or bn.bias is None:
        raise ValueError(f"bn must be an affine BatchNorm1d over x's {c} channels")
    if bn.momentum is None:
        raise ValueError("bn.momentum must be a number (the cumulative average has no fused form)")
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"p must be in [0, 1), got {p}")
    if keep is not None and seed is not None:
        raise ValueError("keep and seed exclude each other")

    def vec(t, what):
        if t.dtype != torch.float32 or t.numel() != c or t.device != x.device:
            raise ValueError(f"{what} must be a float32 tensor of {c} elements on x's device")
        return t if t.is_contiguous() else t.contiguous()

    gamma, beta = vec(bn.weight, "bn.weight"), vec(bn.bias, "bn.bias")
    if bias is not None:
        bias = vec(bias, "bias")
    if p == 0.0:
        keep = seed = None
    elif keep is not None:
        if keep.dtype != torch.uint8 or keep.shape != x.shape or keep.device != x.device:
            raise ValueError("keep must be a uint8 tensor of x's shape on x's device")
        keep = keep.contiguous()
    elif seed is not None:
        if seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != x.device:
            raise ValueError("seed must be an int64 tensor of one element on x's device")
    else:
        raise ValueError("p > 0 needs a keep mask or a seed")
    running_mean = running_var = None
    if bn.track_running_stats and bn.running_mean is not None:
        running_mean, running_var = vec(bn.running_mean, "bn.running_mean"), vec(bn.running_var, "bn.running_var")
        if running_mean is not bn.running_mean or running_var is not bn.running_var:
            raise ValueError("bn's running statistics must be contiguous (they are updated in place)")
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
    return x, bias, gamma, beta, (running_mean, running_var, bn.eps, bn.momentum), p, keep, seed


def batch_norm_act(x: torch.Tensor, bn: torch.nn.BatchNorm1d, bias: Optional[torch.Tensor] = None, p: float = 0.0,
                   keep: Optional[torch.Tensor] = None, seed: Optional[torch.Tensor] = None,
                   act=None) -> torch.Tensor:
    """What the wrappers run between two conv layers in training with ``bn=True`` (models.py:204-209): ``x + bias``,
    relu, ``bn`` on the batch's statistics (biased variance; the running statistics and ``num_batches_tracked``
    updated on the device as torch does) and a dropout of rate ``p`` - ``keep``: the caller's uint8 [N, C]
    Bernoulli(1 - p) mask, or ``seed``: an int64 [1] device counter the kernel draws the mask from (the aggregation
    epilogue's draw: ``HiddenEpilogue``), never both; ``p == 0``: no mask.  The relu is idempotent: rows that already
    are ``relu(conv + bias)`` go in with ``bias=None`` (``act``: that producer's ``HiddenEpilogue``, which then
    receives its gradient pre-masked).  Contiguous fp32 GPU tensors, an affine ``bn`` of x's width with a numeric
    momentum, at least two rows; everything else raises (there is no CPU path)."""
    x, bias, gamma, beta, stats, p, keep, seed = _bn_inputs(x, bn, bias, p, keep, seed)
    return _BatchNormAct.apply(x, bias, gamma, beta, stats, p, keep, seed, act)


class _BatchNormPostAct(torch.autograd.Function):
    """Training-mode batch norm + relu + dropout, in that order, in three launches each way
    (``sngnn_bn_post_forward`` / ``_backward``).  Saved: x, the per-channel vectors, the caller's ``keep`` or the seed -
    nothing else of size [N, C]: the backward recomputes xhat, the relu mask and the keep mask from x."""

    @staticmethod
    def forward(ctx, x, gamma, beta, stats, p, keep, seed):
        n, c = x.shape
        running_mean, running_var, eps, momentum = stats
        out = torch.empty_like(x)
        mean = torch.empty(c, dtype=torch.float32, device=x.device)
        invstd = torch.empty_like(mean)
        scale = 1.0 / (1.0 - p) if p > 0.0 else 1.0
        _lib.call("sngnn_bn_post_forward", x.device, x, n, c, gamma, beta, float(eps), float(momentum), running_mean,
                  running_var, keep, scale, seed, float(p), out, mean, invstd, bn_train_workspace(c, x.device))
        ctx.p, ctx.scale = float(p), scale
        ctx.save_for_backward(x, gamma, beta, mean, invstd, keep, seed)
        return out

    @staticmethod
    def backward(ctx, g):
        x, gamma, beta, mean, invstd, keep, seed = ctx.saved_tensors
        n, c = x.shape
        g = g.contiguous()
        grad_x = torch.empty_like(x)
        grad_gamma, grad_beta = torch.empty_like(mean), torch.empty_like(mean)
        _lib.call("sngnn_bn_post_backward", x.device, g, x, n, c, gamma, beta, mean, invstd, keep, ctx.scale, seed, ctx.p,
                  grad_x, grad_gamma, grad_beta, bn_train_workspace(c, x.device))
        return grad_x, grad_gamma, grad_beta, None, None, None, None


def batch_norm_post_act(x: torch.Tensor, bn: torch.nn.BatchNorm1d, p: float = 0.0, seed: Optional[torch.Tensor] = None,
                        keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What GCNII runs behind every layer in training (models.py:1295-1298): ``bn`` on the batch's statistics, relu,
    then a dropout of rate ``p`` - the other order of :func:`batch_norm_act`, with the same running-statistics and
    ``num_batches_tracked`` updates, the same ``keep`` / ``seed`` and the same demands on ``x`` and ``bn``."""
    x, _, gamma, beta, stats, p, keep, seed = _bn_inputs(x, bn, None, p, keep, seed)
    return _BatchNormPostAct.apply(x, gamma, beta, stats, p, keep, seed)
