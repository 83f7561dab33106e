"""Pooled sequence embeddings straight from the backbone's last layer: the final add + norm and
the pooling over the sequence run as one pass over the pre-norm stream (ops.pool_head, csrc/pool.hip).  The normed (S, B, L, D)
activation, its fp32 residual copy and the strand concatenation of `model.caduceus(ids)` are never written; the pooled sums are fp32.

Frames.  A non-RCPS model gives (B, D).  An RCPS model gives (B, D, 2) in the frame of downstream.DNAEmbeddingModelCaduceus pooled over
the sequence: [..., 0] is the forward strand, [..., 1] the reverse-complement strand "back in the forward frame" -- which is strand 1 of
the t-frame as it lies (no channel flip) with its positions running the other way.  So on strand 1 "first" and "last" exchange roles
and a window centre c becomes L - 1 - c; mean and max do not care.
"""
from __future__ import annotations

import contextlib
from typing import Optional

import torch

from .modeling_caduceus import Caduceus
from .ops import PoolUnsupported

POOLINGS = ("mean", "max", "first", "last", "window")


def backbone_of(model):
    """The CaduceusMixerModel of a Caduceus, CaduceusForMaskedLM or CaduceusForSequenceClassification."""
    caduceus = model if isinstance(model, Caduceus) else getattr(model, "caduceus", None)
    if not isinstance(caduceus, Caduceus):
        raise TypeError("pooled_embeddings takes a Caduceus, CaduceusForMaskedLM or CaduceusForSequenceClassification model, got "
                        f"{type(model).__name__}")
    return caduceus.backbone


def window_half(window_tokens: int) -> int:
    """vep.window_mean's offsets -w // 2 .. w // 2 as the head's -half .. half; they are symmetric only for an even w."""
    w = int(window_tokens)
    if w < 0 or w % 2:
        raise PoolUnsupported(f"pooled_embeddings: window_tokens must be even and >= 0 (offsets -w // 2 .. w // 2 are not symmetric "
                              f"about the centre for an odd w), got {window_tokens}")
    return w // 2


def tframe_pooling(pooling: str, S: int, B: int, L: int, device, centre: Optional[torch.Tensor] = None,
                   window_tokens: Optional[int] = None):
    """(mode, centre (S, B) int64 | None, half) of forward_tframe_pooled for a pooling named in the forward frame.  Built on the device from
    device tensors: nothing is read back."""
    if pooling not in POOLINGS:
        raise NotImplementedError(f"Pooling strategy `{pooling}` not implemented.")
    if pooling in ("mean", "max"):
        if centre is not None or window_tokens is not None:
            raise ValueError(f"pooled_embeddings: centre and window_tokens belong to pooling 'window', not {pooling!r}")
        return pooling, None, 0
    if pooling == "window":
        if centre is None or window_tokens is None:
            raise ValueError("pooled_embeddings: pooling 'window' takes centre (B,) and window_tokens")
        if centre.dtype != torch.int64 or tuple(centre.shape) != (B,):
            raise TypeError(f"pooled_embeddings: centre is ({B},) int64")
        c, half = centre.to(device), window_half(window_tokens)
    else:  # one-row gathers
        if centre is not None or window_tokens is not None:
            raise ValueError(f"pooled_embeddings: centre and window_tokens belong to pooling 'window', not {pooling!r}")
        c, half = torch.full((B,), 0 if pooling == "first" else L - 1, dtype=torch.int64, device=device), 0
    # strand 1 stores its positions the other way round
    return "window", (c.unsqueeze(0) if S == 1 else torch.stack([c, (L - 1) - c], 0)), half


def pooled_embeddings(model, input_ids: torch.Tensor, pooling: str = "mean", *, centre: Optional[torch.Tensor] = None,
                      window_tokens: Optional[int] = None, grad: bool = False) -> torch.Tensor:
    """Sequence embeddings of input_ids (B, L): the model's last hidden states pooled over the sequence, fp32.
    pooling: "mean", "max", "first", "last", or "window" -- the mean over positions centre[b] + [-w // 2, w // 2] with w = window_tokens,
    clamped to [0, L - 1] so that an edge token repeats (vep.window_mean); centre is (B,) int64, any value.
    Returns (B, D), or (B, D, 2) for an RCPS model (see the module docstring for the frame).  Runs under the model's precision scope and
    torch.no_grad(); reads nothing back from the device.  grad=True follows the ambient grad mode instead: the embeddings then
    back-propagate into the model through the pool head's backward (ops.pool_head_grad)."""
    backbone = backbone_of(model)
    if input_ids.dim() != 2:
        raise ValueError(f"pooled_embeddings: input_ids is (B, L), got {tuple(input_ids.shape)}")
    B, L = input_ids.shape
    S = 2 if backbone.rcps else 1
    with contextlib.nullcontext() if grad else torch.no_grad(), model._precision_scope():
        mode, cen, half = tframe_pooling(pooling, S, B, L, input_ids.device, centre, window_tokens)
        out = backbone.forward_tframe_pooled(input_ids, None, mode, cen, half, grad=grad)  # (S, B, D)
    return out[0] if S == 1 else out.permute(1, 2, 0)
