"""Per-token log-likelihood scoring: how likely is this sequence, or this base, under the model?

  sequence_logprobs   causal stacks: teacher-forced log p(ids[t + 1] | ids[..t]); their sum is the sequence log-likelihood, exp of the
                      negative mean the perplexity.  Optionally in chunks through the inference cache, for bounded activation memory.
  masked_logprobs     any CaduceusForMaskedLM (RCPS, bi-directional or causal): log-probabilities of every id at masked positions.
  variant_llr         zero-shot variant score log p(alt) - log p(ref) at the variant position, the reference sequence masked there.

All three end in ops.lm_head_score (cad_lm_head_score): the log-probabilities come straight from the final hidden state, on the scored
rows only; no (B, L, V) logits tensor exists.  `allowed_token_ids` (e.g. the four bases: the padded vocabulary is mostly specials)
restricts the normalisation the way `generate` restricts sampling, with the same mask (generation._logit_mask).  Everything runs under
the model's precision scope and no_grad, and nothing is read back from the device: data-dependent checks are made only on arguments
the host already holds (lists, CPU tensors).
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import ops
from .generation import InferenceParams, _logit_mask
from .vep import find_variant_idx


def _head(model):
    """(weight (V, D), complement map | None) of the LM head, or ScoreUnsupported."""
    head = model.lm_head
    w = head.weight
    if getattr(head, "bias", None) is not None or getattr(getattr(head, "lm_head", None), "bias", None) is not None:
        raise ops.ScoreUnsupported("scoring: cad_lm_head_score covers a bias-free LM head only; score this head from model(ids).logits")
    V, D = w.shape
    if not ops.lm_head_score_supported(D, V, torch.float32):
        raise ops.ScoreUnsupported(f"scoring: cad_lm_head_score does not serve vocab_size {V} (vocab_size <= 16); score this head from "
                                   "model(ids).logits")
    return w, (head.complement_map if model.config.rcps else None)


def _device(model):
    return model.caduceus.backbone.embeddings.word_embeddings.weight.device


def _ids(name, ids, V, dev) -> Tensor:
    """(B, L) int64 on the model's device; ids the host holds are range-checked first."""
    ids = torch.as_tensor(ids)
    if ids.dim() != 2 or ids.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"{name} must be a (B, L) integer tensor")
    if ids.device.type == "cpu" and ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= V):
        raise ValueError(f"{name} must lie in [0, {V}) (the padded vocabulary)")
    return ids.to(dev).long()


def _ignore_index(model, ignore_index):
    if ignore_index is None:
        ignore_index = getattr(model.config, "pad_token_id", None)
    return -100 if ignore_index is None else int(ignore_index)


def sequence_logprobs(model, input_ids: Tensor, *, allowed_token_ids=None, ignore_index: Optional[int] = None,
                      chunk_len: Optional[int] = None) -> Tensor:
    """(B, L - 1) fp32: entry t is log p(input_ids[:, t + 1] | input_ids[:, :t + 1]) under a causal CaduceusForMaskedLM, normalised
    over allowed_token_ids (default: the whole padded vocabulary).  A next token equal to ignore_index (default: config.pad_token_id)
    scores 0.0, so a row's sum is the log-likelihood of its real tokens; a next token outside allowed_token_ids scores -inf.
    chunk_len: None runs one full-sequence forward; an integer runs the sequence through an inference cache in chunks of that many
    positions (activation memory bounded by the chunk; the states carry the context), scoring each chunk as it leaves the stack.
    A bi-directional or RCPS stack has no left-to-right factorisation and raises NotImplementedError: use masked_logprobs."""
    backbone = model.caduceus.backbone
    try:
        backbone._require_stepwise()
    except NotImplementedError:
        raise NotImplementedError("sequence_logprobs needs a causal stack (bidirectional=False, rcps=False): a bi-directional or RCPS "
                                  "model sees the token it would be asked to predict; use masked_logprobs for such a model") from None
    w, _ = _head(model)
    V = w.shape[0]
    dev = _device(model)
    ids = _ids("input_ids", input_ids, V, dev)
    B, L = ids.shape
    if L < 2:
        raise ValueError("sequence_logprobs needs at least two positions")
    if chunk_len is not None and (int(chunk_len) != chunk_len or chunk_len < 1):
        raise ValueError(f"chunk_len must be a positive integer or None, got {chunk_len}")
    mask = _logit_mask(allowed_token_ids, V, dev)
    ign = _ignore_index(model, ignore_index)
    with model._precision_scope(), torch.no_grad():
        if chunk_len is None:
            hidden_t = backbone.forward_tframe(ids)  # (1, B, L, D)
            # every row is scored against its successor; the last position has none and is dropped
            targets = torch.cat([ids[:, 1:], ids[:, :1]], dim=1)
            return ops.lm_head_score(hidden_t, w, None, targets=targets, logit_mask=mask, ignore_index=ign)[:, :-1]
        out = torch.empty((B, L - 1), dtype=torch.float32, device=dev)
        params = InferenceParams(max_seqlen=L, max_batch_size=B)
        for c0 in range(0, L - 1, int(chunk_len)):
            c1 = min(c0 + int(chunk_len), L - 1)
            hidden_t = backbone.forward_tframe_cached(ids[:, c0:c1], None, params)  # (1, B, c1 - c0, D)
            params.seqlen_offset = c1
            out[:, c0:c1] = ops.lm_head_score(hidden_t, w, None, targets=ids[:, c0 + 1:c1 + 1], logit_mask=mask, ignore_index=ign)
        return out


def masked_logprobs(model, input_ids: Tensor, positions, *, mask_token_id: int, allowed_token_ids=None) -> Tensor:
    """(B, P, V) fp32: log softmax over allowed_token_ids (-inf at the other ids) at positions (B, P) of input_ids (B, L), each of those
    positions replaced by mask_token_id in a COPY of the ids (the caller's tensor is left as it is).  One forward of any
    CaduceusForMaskedLM; only the B P gathered rows of the final hidden state reach the head."""
    w, comp = _head(model)
    V = w.shape[0]
    dev = _device(model)
    ids = _ids("input_ids", input_ids, V, dev)
    B, L = ids.shape
    if not 0 <= int(mask_token_id) < V:
        raise ValueError(f"mask_token_id must lie in [0, {V}), got {mask_token_id}")
    pos = torch.as_tensor(positions)
    if pos.dim() != 2 or pos.shape[0] != B or pos.shape[1] < 1 or pos.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"positions must be a ({B}, P) integer tensor")
    if pos.device.type == "cpu" and (int(pos.min()) < 0 or int(pos.max()) >= L):
        raise ValueError(f"positions must lie in [0, {L})")
    pos = pos.to(dev).long()
    mask = _logit_mask(allowed_token_ids, V, dev)
    with model._precision_scope(), torch.no_grad():
        masked = ids.clone()
        masked.scatter_(1, pos, int(mask_token_id))
        rows = pos + torch.arange(B, device=dev).unsqueeze(1) * L  # (before the forward: behind it only the result is allocated)
        hidden_t = model.caduceus.backbone.forward_tframe(masked)  # (S, B, L, D)
        return ops.lm_head_score(hidden_t, w, comp, row_index=rows, logit_mask=mask, want_all=True)


def variant_llr(model, ref_ids: Tensor, alt_ids: Tensor, *, mask_token_id: int, allowed_token_ids=None) -> Tensor:
    """(B,) fp32 zero-shot variant score log p(alt base) - log p(ref base): ONE forward of ref_ids (B, L) with the variant position
    (vep.find_variant_idx) masked.  ref and alt must differ at exactly one position per row: host-held ids are checked and raise
    ValueError; ids already on the device are not read back, and a row that breaks the rule scores NaN."""
    w, _ = _head(model)
    V = w.shape[0]
    dev = _device(model)
    ref_h, alt_h = torch.as_tensor(ref_ids), torch.as_tensor(alt_ids)
    if ref_h.shape != alt_h.shape:
        raise ValueError(f"ref_ids {tuple(ref_h.shape)} and alt_ids {tuple(alt_h.shape)} differ in shape")
    if ref_h.device.type == "cpu" and alt_h.device.type == "cpu" and ref_h.dim() == 2:
        ndiff = (ref_h != alt_h).sum(dim=1)
        if bool((ndiff != 1).any()):
            raise ValueError("variant_llr: ref_ids and alt_ids must differ at exactly one position per row; rows "
                             f"{(ndiff != 1).nonzero().flatten().tolist()} differ at {ndiff[ndiff != 1].tolist()}")
    ref, alt = _ids("ref_ids", ref_h, V, dev), _ids("alt_ids", alt_h, V, dev)
    single = (ref != alt).sum(dim=1) == 1
    pos = find_variant_idx(ref, alt).clamp_min(0).unsqueeze(1)  # (B, 1)
    lp = masked_logprobs(model, ref, pos, mask_token_id=mask_token_id, allowed_token_ids=allowed_token_ids)[:, 0]  # (B, V)
    llr = lp.gather(1, alt.gather(1, pos)) - lp.gather(1, ref.gather(1, pos))
    return torch.where(single, llr[:, 0], torch.full_like(llr[:, 0], float("nan")))
