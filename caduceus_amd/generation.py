"""Step-wise decoding of a causal Caduceus stack (CaduceusConfig(bidirectional=False, rcps=False)): the inference cache of
mamba_ssm 1.2.0 (`InferenceParams`, mamba_ssm/utils/generation.py) and a minimal greedy loop over the HIP step kernels
(ops.mamba_step).  A bi-directional or RCPS stack has no step-wise form and raises NotImplementedError.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import torch
from torch import Tensor


@dataclass
class InferenceParams:
    """Inference parameters that are passed to the main model in order to efficiently calculate and store the context during
    inference (upstream's fields).  key_value_memory_dict: {layer_idx: (conv_state, ssm_state)}, filled on first use."""
    max_seqlen: int
    max_batch_size: int
    seqlen_offset: int = 0
    batch_size_offset: int = 0
    key_value_memory_dict: dict = field(default_factory=dict)
    lengths_per_sample: Optional[Tensor] = None

    def reset(self, max_seqlen, max_batch_size):
        self.max_seqlen = max_seqlen
        self.max_batch_size = max_batch_size
        self.seqlen_offset = 0
        if self.lengths_per_sample is not None:
            self.lengths_per_sample.zero_()


def decode_step(model, token_ids: Tensor, inference_params: InferenceParams) -> Tensor:
    """Logits (B, V) fp32 of the LAST position of token_ids (B, L) for a causal CaduceusForMaskedLM, through the cache; advances
    inference_params.seqlen_offset by L.  L == 1 behind a prefill is one constant-time step; seqlen_offset == 0 is the prefill itself,
    and L > 1 behind a prefill its next chunk."""
    with model._precision_scope(), torch.no_grad():
        hidden_t = model.caduceus.backbone.forward_tframe_cached(token_ids, None, inference_params)  # (1, B, L, D)
        logits, _ = model.logits_tframe(hidden_t[:, :, -1:].contiguous(), None, -100)
    inference_params.seqlen_offset += token_ids.shape[1]
    return logits[:, 0]


def generate(model, input_ids: Tensor, max_new_tokens: int, return_logits: bool = False):
    """Greedy continuation: ids (B, L0 + max_new_tokens) -- one prefill of input_ids (B, L0), then one decode_step per new token.
    return_logits: also the list of the max_new_tokens logits (B, V) each new token was the argmax of."""
    B, L0 = input_ids.shape
    params = InferenceParams(max_seqlen=L0 + max_new_tokens, max_batch_size=B)
    ids, all_logits = [input_ids], []
    cur = input_ids
    for _ in range(max_new_tokens):
        logits = decode_step(model, cur, params)
        cur = logits.argmax(dim=-1, keepdim=True).to(input_ids.dtype)
        ids.append(cur)
        all_logits.append(logits)
    out = torch.cat(ids, dim=1)
    return (out, all_logits) if return_logits else out
