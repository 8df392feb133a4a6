"""The argument checks the operator modules share (``ops``, ``prop``, ``gat``): a leaf module, so none of them needs
another for a check."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib

# storage types of the half path (sngnn_agg_forward_half / sngnn_agg_backward_half, sngnn_attn_*_half,
# sngnn_signed_*_half): the fp32 operator on h.float(), only the stored rows rounded once to the type
HALF_DTYPES = {torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}


def check_rows(t: torch.Tensor, n: int, what: str, half: bool = False, max_channels: int = _lib.MAX_CHANNELS) -> torch.Tensor:
    """``max_channels``: the widest row the operator takes where that is not the library's limit itself (the ACM
    filterbank's [N, 3C] table: 2C <= MAX_CHANNELS)."""
    if t.dtype != torch.float32 and not (half and t.dtype in HALF_DTYPES):
        if half:
            raise ValueError(f"{what} must be float32, float16 or bfloat16, got {t.dtype}")
        raise ValueError(f"{what} must be float32 (the reference path is fp32 only)")
    if not t.is_cuda:
        raise ValueError(f"{what} must live on the GPU (there is no CPU path)")
    if t.dim() != 2 or t.size(0) != n:
        raise ValueError(f"{what} must have shape [{n}, C], got {tuple(t.shape)}")
    if not 1 <= t.size(1) <= max_channels:
        raise ValueError(f"{what}: C must be in [1, {max_channels}]")
    return t.contiguous()


def check_grad_dtype(grad_out: torch.Tensor, rows: torch.Tensor, what: str) -> None:
    """``grad_out`` of a half call has the rows' dtype; of an fp32 call, float32."""
    if grad_out.dtype != rows.dtype:
        raise ValueError(f"grad_out must have {what}'s dtype {rows.dtype}, got {grad_out.dtype}")


def check_flat(t: torch.Tensor, like: Optional[torch.Tensor], what: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise ValueError(f"{what} must be a float32 tensor (the fused GGCN transition is fp32 only)")
    if not t.is_cuda:
        raise ValueError(f"{what} must live on the GPU (there is no CPU path)")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous, got shape {tuple(t.shape)} with strides {t.stride()}")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{what} must have prop's shape {tuple(like.shape)} and device, got {tuple(t.shape)} on {t.device}")
    return t


def check_whole_graph_with_loops(graph, rows: torch.Tensor, what: str, op: str, edges: str, partition) -> None:
    """What operator ``op`` (named in the messages; ``edges``: whose edge list it needs) asks before ``check_rows``:
    no half rows ``what``, the whole, loop-replaced graph, no node-range ``partition`` (dist.current_partition())."""
    if rows.dtype in HALF_DTYPES:
        raise ValueError(f"{what} is {rows.dtype}: {op} has no half-width path (cast the rows to torch.float32)")
    if partition is not None or graph.num_nodes != graph.num_total_nodes:
        raise ValueError(f"{op} runs on one GPU: node-range partitions are not implemented for it")
    if not graph.add_loops or graph.remove_loops != _lib.LOOPS_REPLACE:
        raise ValueError(f"{op} needs {edges} edge list: a graph built with add_loops=True, remove_loops=LOOPS_REPLACE")
