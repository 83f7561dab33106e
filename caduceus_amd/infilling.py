"""Masked infilling by iterative unmasking (MaskGIT-style): the way a bi-directional or RCPS model produces sequence.

A bi-directional stack has no left-to-right factorisation (`generate` refuses it), but it can fill the positions of a sequence that
hold the mask token: predict all of them, commit the ones the model is surest of, mask the rest again, repeat.  `infill` does that in
`steps` rounds; a round is one full-sequence forward (backbone.forward_tframe) and one launch of the unmask head (ops.lm_head_unmask,
cad_lm_head_unmask: the logit row, the sampler and the log-probability of the drawn id per open position, nothing per vocabulary
entry), followed by the commit rule in a handful of torch ops on (B, L) device tensors.  Nothing is read back from the device inside
the loop: data-dependent checks are made only on arguments the host already holds.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import Tensor

from . import ops
from .generation import _logit_mask
from .scoring import _device, _head, _ids

ORDERS = ("confidence", "left_to_right")
SCHEDULES = ("cosine", "linear")


def open_fraction(schedule: str, r: int, steps: int) -> float:
    """f(r): the share of a row's initially open positions that may stay open after round r = 0 .. steps - 1 (fp64 on the host).
    cosine: cos(pi / 2 (r + 1) / steps); linear: 1 - (r + 1) / steps; the last round is exactly 0, so it commits everything."""
    if r >= steps - 1:
        return 0.0
    if schedule == "cosine":
        return math.cos(math.pi / 2.0 * (r + 1) / steps)
    return 1.0 - (r + 1) / steps


def commit(ids_out: Tensor, conf: Tensor, cur: Tensor, n_open: Tensor, keep_open: Tensor, mask_token_id: int, order: str):
    """The commit rule of one round on device tensors.  cur (B, L): the ids the round started from; ids_out, conf: what the unmask head
    gave for them; n_open (B): the open positions of each row in cur; keep_open (B) <= n_open: how many may stay open.
    Commits n_open - keep_open open positions per row -- "confidence": those with the largest conf, ties to the lower position;
    "left_to_right": the leftmost -- and leaves the others at mask_token_id.  Returns (ids (B, L), committed (B, L) bool).
    A stable sort per row and a comparison with the per-row count: no nonzero(), no boolean indexing, nothing read back."""
    B, Lq = cur.shape
    is_open = cur == mask_token_id
    low = torch.full_like(conf, float("-inf"))
    key = torch.where(is_open, conf if order == "confidence" else torch.zeros_like(conf), low)  # closed positions sort behind every open one
    by_key = torch.sort(key, dim=1, descending=True, stable=True).indices
    place = torch.empty_like(by_key).scatter_(1, by_key, torch.arange(Lq, device=cur.device).expand(B, Lq))
    committed = is_open & (place < (n_open - keep_open).unsqueeze(1))
    return torch.where(committed, ids_out, cur), committed


def infill(model, input_ids: Tensor, *, mask_token_id: int, allowed_token_ids, steps: int = 8, order: str = "confidence",
           schedule: str = "cosine", top_k: int = 1, top_p: float = 0.0, temperature: float = 1.0, seed: Optional[int] = None,
           row_offset: int = 0, return_logprobs: bool = False):
    """ids (B, L) with every position of input_ids (B, L) that held mask_token_id filled by an id of allowed_token_ids; the other
    positions, and the caller's tensor, stay as they are.  Any CaduceusForMaskedLM: RCPS, bi-directional or causal.

    steps rounds; round r runs one forward of the current ids and draws an id at every open position by `generate`'s sampler rules
    (top_k == 1: the argmax, ties to the lowest id; top_k == 0 keeps all; top_p in (0, 1): nucleus; temperature > 0), the uniform of
    position l of row b keyed by (seed, row_offset + b, (r << 32) + l): the same (seed, row, round, position) gives the same draw
    whatever the batch, and a position drawn again in a later round gets a fresh uniform.  seed None with top_k != 1 draws one seed
    from torch's default generator (host side, once per call).
    With n0[b] positions of row b open at the start, at most floor(n0[b] f(r)) stay open after round r -- schedule "cosine":
    f(r) = cos(pi / 2 (r + 1) / steps), "linear": 1 - (r + 1) / steps, the last round 0 --; order "confidence" commits the open
    positions whose drawn id the model gives the largest log-probability (ties to the lower position), "left_to_right" the leftmost.
    return_logprobs: also (B, L) fp32, the model's log-probability, over allowed_token_ids, of each filled id in the round that
    committed it (temperature, top_k and top_p not applied: the number masked_logprobs would give there); 0.0 where nothing was masked.
    allowed_token_ids is required and must not hold mask_token_id: a position could draw the mask and never close."""
    if int(steps) != steps or steps < 1:
        raise ValueError(f"steps must be a positive integer, got {steps}")
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
    if schedule not in SCHEDULES:
        raise ValueError(f"schedule must be one of {SCHEDULES}, got {schedule!r}")
    ops.check_sampling(top_k, top_p, temperature)
    steps = int(steps)
    w, comp = _head(model)
    V = w.shape[0]
    if not 0 <= int(mask_token_id) < V:
        raise ValueError(f"mask_token_id must lie in [0, {V}), got {mask_token_id}")
    if allowed_token_ids is None:
        raise ValueError("infill needs allowed_token_ids (e.g. the four bases): without it a position could draw any special token")
    allowed = tuple(sorted({int(i) for i in allowed_token_ids}))
    if int(mask_token_id) in allowed:
        raise ValueError(f"allowed_token_ids must not hold mask_token_id {mask_token_id}: a position could draw the mask and never close")
    mask = _logit_mask(allowed, V, "cpu")
    dev = _device(model)
    # (a pinned staging copy: the transfer is queued on the stream like everything behind it)
    mask = mask.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else mask.to(dev)
    cur = _ids("input_ids", input_ids, V, dev)
    B, Lq = cur.shape
    if Lq >= 1 << 32:
        raise ValueError("infill: the round number sits above bit 32 of the uniform's position, L must stay below 2^32")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if top_k != 1 else 0
    backbone = model.caduceus.backbone
    with model._precision_scope(), torch.no_grad():
        n0 = (cur == mask_token_id).sum(dim=1)
        n_open = n0
        logp = torch.zeros((B, Lq), dtype=torch.float32, device=dev)
        for r in range(steps):
            hidden_t = backbone.forward_tframe(cur)  # (S, B, L, D)
            ids_out, conf = ops.lm_head_unmask(hidden_t, w, comp, cur, mask_token_id=int(mask_token_id), top_k=int(top_k), top_p=float(top_p),
                                               temperature=float(temperature), seed=int(seed), row_offset=int(row_offset), position=r << 32,
                                               logit_mask=mask)
            keep_open = torch.minimum(n_open, torch.floor(n0.double() * open_fraction(schedule, r, steps)).long())
            cur, committed = commit(ids_out, conf, cur, n_open, keep_open, int(mask_token_id), order)
            logp = torch.where(committed, conf, logp)
            n_open = keep_open
    return (cur, logp) if return_logprobs else cur
