"""Nucleotide attributions: which bases drive this prediction?

  attribute(model, input_ids, target, allowed_token_ids=..., method=...)
    "gradient"      (B, L, A) fp32: d score / d onehot at the allowed ids (columns in ascending id order) -- input-gradient saliency
    "grad_x_input"  (B, L) fp32: that gradient at the base the position holds
    "integrated"    (B, L) fp32: integrated gradients from the uniform mixture of the allowed bases to the sequence

The score is differentiated with respect to the t-frame embedding output only: the layers run under mixer.input_grad_only(), whose
backward computes no weight gradient, and the gradient dh (S, B, L, D) goes straight into ops.embed_attrib (cad_embed_attrib):
  d score / d onehot[b,l,v] = <dh0[b,l], E[v]> + <dh1[b,l], E[comp v]>
is the LM head's logit row with dh as the hidden state and the embedding table as the weight.  Neither a (B, L, V) tensor nor a
reference-frame (B, L, 2 D) gradient is written.  With centre=True the mean over the allowed ids is subtracted at every position: the
one-hot input lives on the simplex, where only differences between bases mean something.  Rows are independent, so ONE backward of
score.sum() yields every row's gradient.  Nothing is read back from the device, no parameter's requires_grad or .grad and no module's
training flag is touched.
"""
from __future__ import annotations

from typing import Callable, Optional, Union

import torch
from torch import Tensor

from . import engine, mixer, ops
from .embedding import backbone_of
from .generation import _logit_mask
from .mamba import act_dtype_of, as_requested
from .modeling_caduceus import CaduceusForMaskedLM, CaduceusForSequenceClassification
from .scoring import _ids

METHODS = ("gradient", "grad_x_input", "integrated")


class MaskedTarget:
    """The masked-LM score of one position per row: log p(token_ids[b]) at positions[b] with that position replaced by mask_token_id
    in a copy of the ids, the log-softmax running over allowed_token_ids; with ref_token_ids, log p(ref_token_ids[b]) is subtracted --
    scoring.variant_llr's quantity."""

    def __init__(self, positions, token_ids, ref_token_ids=None, *, mask_token_id: int):
        self.positions, self.token_ids, self.ref_token_ids, self.mask_token_id = positions, token_ids, ref_token_ids, int(mask_token_id)


def _per_row(name, t, B, hi, dev) -> Tensor:
    """(B,) int64 on the device; values the host holds are range-checked first."""
    t = torch.as_tensor(t)
    if t.dim() != 1 or t.shape[0] != B or t.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"{name} must be a ({B},) integer tensor")
    if t.device.type == "cpu" and (int(t.min()) < 0 or int(t.max()) >= hi):
        raise ValueError(f"{name} must lie in [0, {hi})")
    return t.to(dev).long()


def _embedding(model, backbone, masked_lm_head: bool):
    """(embedding table (V, D), complement map | None), or AttribUnsupported."""
    we = backbone.embeddings.word_embeddings
    E = we.weight
    V, D = E.shape
    if not ops.embed_attrib_supported(D, V, torch.float32):
        raise ops.AttribUnsupported(f"attribution: cad_embed_attrib does not serve vocab_size {V} (vocab_size <= 16)")
    if masked_lm_head:
        head = model.lm_head
        if getattr(head, "bias", None) is not None or getattr(getattr(head, "lm_head", None), "bias", None) is not None:
            raise ops.AttribUnsupported("attribution: a MaskedTarget covers a bias-free LM head only; give the score as a callable target")
    return E, (we.complement_map if backbone.rcps else None)


def attribute(model, input_ids: Tensor, target: Union[int, Tensor, MaskedTarget, Callable[[Tensor], Tensor]], *, allowed_token_ids,
              method: str = "grad_x_input", centre: bool = True, steps: int = 16) -> Tensor:
    """Attributions of a score to the bases of input_ids (B, L); allowed_token_ids names the bases (e.g. A, C, G, T).
    target:
      int or (B,) int64          CaduceusForSequenceClassification: that class logit, through the model's own pooling, pool head
                                 (fused_pool_train: ops.pool_head_grad) and conjoin settings.  With post-hoc conjoining input_ids is
                                 (B, L, 2) and the result carries that trailing axis.
      MaskedTarget               CaduceusForMaskedLM: log p(token) (minus log p(ref token)) at one masked position per row.  The masked
                                 copy is what is attributed: the masked position itself holds no base and gets grad_x_input 0.0.
      callable                   any of Caduceus, the masked LM or the classifier: takes the final hidden state in the reference layout
                                 (B, L, D | 2 D), returns (B,) scores.
    method: see the module docstring.  A position whose id is not allowed (N, pad, mask) gets 0.0 from "grad_x_input" and "integrated".
    "integrated": the baseline is the uniform mixture of the allowed bases (mean_A E[a] on strand 0, mean_A E[comp a] on strand 1, so an
    RCPS model needs allowed_token_ids closed under the complement map); the path x0 + alpha_k (x - x0) is walked at the midpoints
    alpha_k = (k + 1/2) / steps, the gradients are averaged in fp32, and <avg dh, E[id] - x0> is the centred grad_x_input of the
    averaged gradient: centre=False raises."""
    backbone = backbone_of(model)
    if method not in METHODS:
        raise ValueError(f"attribute: method is one of {METHODS}, got {method!r}")
    if method == "integrated":
        if not centre:
            raise ValueError('attribute: "integrated" measures from the mixture of the allowed bases, which is the centred quantity; '
                             "centre=False has no meaning for it")
        if int(steps) != steps or steps < 1:
            raise ValueError(f"attribute: steps must be a positive integer, got {steps}")
    kind = "masked" if isinstance(target, MaskedTarget) else "callable" if callable(target) else "class"
    if kind == "masked" and not isinstance(model, CaduceusForMaskedLM):
        raise TypeError(f"attribute: a MaskedTarget needs a CaduceusForMaskedLM, got {type(model).__name__}")
    if kind == "class":
        if isinstance(target, bool) or not isinstance(target, (int, Tensor)):
            raise TypeError("attribute: target is a class index (int or (B,) int64), a MaskedTarget, or a callable on the final hidden "
                            f"state, got {type(target).__name__}")
        if not isinstance(model, CaduceusForSequenceClassification):
            raise TypeError(f"attribute: a class-index target needs a CaduceusForSequenceClassification, got {type(model).__name__}")
    E, comp = _embedding(model, backbone, kind == "masked")
    V = E.shape[0]
    dev = E.device
    allowed = sorted({int(i) for i in allowed_token_ids})
    if not allowed or allowed[0] < 0 or allowed[-1] >= V:
        raise ValueError(f"attribute: allowed_token_ids must name ids in [0, {V}) (the padded vocabulary), got {allowed}")
    if method == "integrated" and backbone.rcps:
        cmap = {int(k): int(v) for k, v in model.config.complement_map.items()}
        if {cmap[a] for a in allowed} != set(allowed):
            raise ValueError(f"attribute: integrated gradients of an RCPS model need allowed_token_ids closed under the complement map, "
                             f"got {allowed}")
    conjoin = kind == "class" and model.conjoins()
    ids = torch.as_tensor(input_ids)
    if conjoin:
        if ids.dim() != 3 or ids.shape[-1] != 2:
            raise ValueError("attribute: with post-hoc conjoining input_ids is (B, L, 2): the forward and the reverse-complement input")
        ids = torch.cat([ids[..., 0], ids[..., 1]], dim=0)  # one pass over (2 B, L), as in the model's forward
    ids = _ids("input_ids", ids, V, dev)
    B, Lq = ids.shape
    nB = B // 2 if conjoin else B
    allowed_t = torch.tensor(allowed, dtype=torch.int64, device=dev)

    if kind == "class":
        nl = model.num_labels
        cls = (torch.full((nB,), int(target), dtype=torch.int64) if isinstance(target, int) else target)
        cls = _per_row("target", cls, nB, nl, dev).unsqueeze(1)

        def score(h):
            return model.logits_from_hidden0(h).float().gather(1, cls)[:, 0]
    elif kind == "masked":
        if not 0 <= target.mask_token_id < V:
            raise ValueError(f"attribute: mask_token_id must lie in [0, {V}), got {target.mask_token_id}")
        pos = _per_row("MaskedTarget.positions", target.positions, B, Lq, dev)
        tok = _per_row("MaskedTarget.token_ids", target.token_ids, B, V, dev).unsqueeze(1)
        ref = None if target.ref_token_ids is None else _per_row("MaskedTarget.ref_token_ids", target.ref_token_ids, B, V, dev).unsqueeze(1)
        ids = ids.clone()
        ids.scatter_(1, pos.unsqueeze(1), target.mask_token_id)  # (a copy: the caller's tensor is left as it is)
        mask = _logit_mask(allowed, V, dev)
        rows = torch.arange(B, device=dev)

        def score(h):
            hidden_t = backbone.forward_tframe(None, None, None, hidden0=h)       # (S, B, L, D)
            picked = hidden_t[:, rows, pos].unsqueeze(2)                          # (S, B, 1, D): the head sees the scored rows only
            logits, _ = model.logits_tframe(picked, None, -100)                   # the differentiable ops.lm_head
            logp = torch.log_softmax(logits[:, 0].float() + mask, dim=-1)
            s = logp.gather(1, tok)
            return (s if ref is None else s - logp.gather(1, ref))[:, 0]
    else:
        def score(h):
            hidden_t = backbone.forward_tframe(None, None, None, hidden0=h)
            s = target(as_requested(engine.from_tframe(hidden_t), h))
            if not isinstance(s, Tensor) or tuple(s.shape) != (B,):
                raise ValueError(f"attribute: a callable target returns ({B},) scores, one per row, got "
                                 f"{tuple(s.shape) if isinstance(s, Tensor) else type(s).__name__}")
            return s.float()

    def grad_of(h):
        h = h.detach().requires_grad_(True)
        return torch.autograd.grad(score(h).sum(), inputs=[h])[0]

    with model._precision_scope(), torch.enable_grad(), mixer.input_grad_only():
        act = act_dtype_of(E)
        x = backbone.embeddings.forward_tframe(ids, torch.float32 if E.dtype == torch.float32 else act).detach()
        if method == "integrated":
            with torch.no_grad():
                Ef = E.detach().float()
                base = [Ef[allowed_t].mean(0)] + ([Ef[comp[allowed_t]].mean(0)] if comp is not None else [])
                x0 = torch.stack(base).view(len(base), 1, 1, -1)
                diff = x.float() - x0
                dh = torch.zeros(x.shape, dtype=torch.float32, device=dev)
            for k in range(int(steps)):
                with torch.no_grad():
                    point = (x0 + ((k + 0.5) / steps) * diff).to(x.dtype)
                g = grad_of(point)
                with torch.no_grad():
                    dh += g
            with torch.no_grad():
                dh /= steps
        else:
            dh = grad_of(x)
        with torch.no_grad():
            out = ops.embed_attrib(dh, E, comp, ids, allowed_t, centre=centre, want_grad=method == "gradient",
                                   want_gxi=method != "gradient")
    return torch.stack([out[:nB], out[nB:]], dim=-1) if conjoin else out
