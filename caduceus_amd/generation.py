"""Step-wise decoding of a causal Caduceus stack (CaduceusConfig(bidirectional=False, rcps=False)): the inference cache of
mamba_ssm 1.2.0 (`InferenceParams`, mamba_ssm/utils/generation.py), a minimal greedy loop over the HIP step kernels
(ops.mamba_step), and sampled generation (top_k / top_p / temperature, mamba_ssm's `sample`) with one library call per token
(`DecodeStack`, ops.decode_token).  A bi-directional or RCPS stack has no step-wise form and raises NotImplementedError.
"""
from __future__ import annotations

import contextlib
import ctypes as C
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


class DecodeUnsupported(ValueError):
    """The stack is causal but outside what cad_decode_token serves (see DecodeStack)."""


def _logit_mask(allowed_token_ids, V: int, device) -> Optional[Tensor]:
    """(V) fp32, 0 at the allowed ids and -inf elsewhere; None for no restriction."""
    if allowed_token_ids is None:
        return None
    allowed = sorted({int(i) for i in allowed_token_ids})
    if not allowed:
        raise ValueError("allowed_token_ids is empty: no token could be generated")
    if allowed[0] < 0 or allowed[-1] >= V:
        raise ValueError(f"allowed_token_ids must lie in [0, {V}) (the padded vocabulary), got {allowed}")
    mask = torch.full((V,), float("-inf"), dtype=torch.float32)
    mask[allowed] = 0.0
    return mask.to(device)


class DecodeStack:
    """A causal CaduceusForMaskedLM prepared for one library call per generated token (cad_decode_token: the whole stack, the LM head and
    the sampler as 3 n_layer + 1 launches on the current stream, nothing allocated, nothing read back).

    Built once per model and batch size: it collects the pointers of every parameter (and holds the tensors), builds the per-layer
    records, owns the scratch and the id / logits / uniform buffers, and binds to the cache tensors of its `InferenceParams`, which
    the kernels go on updating in place.  The parameters must be the fp32 master tensors; `dtype` is the compute dtype (default:
    the one a forward would take here: bf16 under bf16 autocast, fp16 inside fp16_kernels(), else fp32).
    A weight swap needs a new DecodeStack: the recorded pointers are re-checked at every prefill, and a replaced or reallocated
    parameter raises (in-place updates of the same storage are seen, as they are by any kernel).

    Served: bidirectional=False, rcps=False; a bias-free (tied or untied) head with vocab_size <= 64; d_model and d_inner <= 2048,
    d_state <= 64, d_conv <= 4.  A bi-directional / RCPS stack raises NotImplementedError (NO_STEPWISE_FORM), anything else outside
    the list DecodeUnsupported (a ValueError).

        stack = DecodeStack(model, max_batch_size=B)
        logits = stack.prefill(prompt, top_k=4, seed=7)      # (B, V); the first new token is in stack.next_ids
        for _ in range(n - 1):
            ids, logits = stack.step(top_k=4, seed=7)        # feeds its own last ids back without leaving the device
    `next_ids`, and what `step` returns, are views of the stack's buffers: the next call overwrites them."""

    MAX_MASKS = 8

    def __init__(self, model, max_batch_size: int, dtype: Optional[torch.dtype] = None, max_seqlen: int = 1 << 30):
        from . import _lib as L
        from . import ops
        from .mamba import act_dtype_of, norm_params
        backbone = model.caduceus.backbone
        backbone._require_stepwise()
        emb = backbone.embeddings.word_embeddings.weight
        with model._precision_scope():
            act = act_dtype_of(emb) if dtype is None else dtype
        head = model.lm_head
        if getattr(head, "bias", None) is not None:
            raise DecodeUnsupported("DecodeStack: the fused token covers a bias-free LM head only; use generate(..., fused=False)")
        V, D = head.weight.shape
        mixers = [layer.mixer.mamba_fwd for layer in backbone.layers]
        m0 = mixers[0]
        E, N, R, K = m0.d_inner, m0.d_state, m0.dt_rank, m0.d_conv
        if tuple(emb.shape) != (V, D) or not ops.decode_supported(D, E, N, R, K, V, act):
            raise DecodeUnsupported(f"DecodeStack: cad_decode_token does not serve d_model {D}, d_inner {E}, d_state {N}, dt_rank {R}, "
                                    f"d_conv {K}, vocab_size {V} in {act} (vocab_size <= 64, widths <= 2048, d_state <= 64, d_conv <= 4); "
                                    "use generate(..., fused=False)")
        self.model, self.act, self.max_batch_size = model, act, int(max_batch_size)
        self.V, self.D = V, D
        dev = emb.device
        self.inference_params = InferenceParams(max_seqlen=max_seqlen, max_batch_size=self.max_batch_size)
        self.inference_params.key_value_memory_dict = backbone.allocate_inference_cache(self.max_batch_size, max_seqlen, dtype=act)
        self._params = self._collect()
        if any(p is not None and (p.dtype != torch.float32 or not p.is_contiguous()) for _, p in self._params):
            raise DecodeUnsupported("DecodeStack: parameters must be contiguous float32 master tensors (compute in bf16 through autocast)")
        self._ptrs = [None if p is None else p.data_ptr() for _, p in self._params]
        named = dict(self._params)
        recs = (L.DecodeLayer * len(mixers))()
        for i, layer in enumerate(backbone.layers):
            conv, ssm = self.inference_params.key_value_memory_dict[i]
            g = lambda name: L.ptr(named[f"{i}.{name}"])
            _, _, eps, is_rms = norm_params(layer.norm)
            recs[i] = L.DecodeLayer(L.ptr(conv), L.ptr(ssm), g("W_in"), g("b_in"), g("conv_w"), g("conv_b"), g("W_x"), g("W_dt"), g("dt_bias"),
                                    g("A_log"), g("Dskip"), g("W_out"), g("b_out"), g("norm_w"), g("norm_b"), float(eps), int(is_rms))
        _, _, eps_f, rms_f = norm_params(backbone.norm_f)
        self._ids = torch.zeros(self.max_batch_size, dtype=torch.int64, device=dev)
        self._logits = torch.zeros(self.max_batch_size * V, dtype=torch.float32, device=dev)
        self._u = torch.zeros(self.max_batch_size, dtype=torch.float32, device=dev)
        self._scratch = ops.decode_scratch(self.max_batch_size, D, E, dev)
        self._recs = recs
        self._masks = {}  # allowed_token_ids -> logit mask on the device, the MAX_MASKS most recently built
        self._args = L.DecodeArgs(recs, L.ptr(named["emb"]), L.ptr(named["normf_w"]), L.ptr(named["normf_b"]), L.ptr(named["head_w"]),
                                  L.ptr(self._ids), L.ptr(self._logits), L.ptr(self._ids), L.ptr(self._u), L.ptr(self._scratch),
                                  ops.sampler_args(), 0, len(mixers), D, E, N, R, K, V, L.dtype_code(act), float(eps_f), int(rms_f))
        self.batch_size = 0

    def _collect(self):
        """[(name, tensor | None)] of everything the argument record points to, in a fixed order."""
        from .mamba import norm_params
        backbone = self.model.caduceus.backbone
        out = [("emb", backbone.embeddings.word_embeddings.weight), ("head_w", self.model.lm_head.weight)]
        w, b, _, _ = norm_params(backbone.norm_f)
        out += [("normf_w", w), ("normf_b", b)]
        for i, layer in enumerate(backbone.layers):
            m = layer.mixer.mamba_fwd
            w, b, _, _ = norm_params(layer.norm)
            for name, p in (("W_in", m.in_proj.weight), ("b_in", m.in_proj.bias), ("conv_w", m.conv1d.weight), ("conv_b", m.conv1d.bias),
                            ("W_x", m.x_proj.weight), ("W_dt", m.dt_proj.weight), ("dt_bias", m.dt_proj.bias), ("A_log", m.A_log),
                            ("Dskip", m.D), ("W_out", m.out_proj.weight), ("b_out", m.out_proj.bias), ("norm_w", w), ("norm_b", b)):
                out.append((f"{i}.{name}", p))
        return [(n, None if p is None else p.detach()) for n, p in out]

    def _check_pointers(self):
        now = self._collect()
        for (name, p), old in zip(now, self._ptrs):
            if (None if p is None else p.data_ptr()) != old:
                raise RuntimeError(f"DecodeStack: parameter {name} was replaced since this stack was built; a weight swap needs a new "
                                   "DecodeStack")

    def _scope(self):
        from .mamba import fp16_kernels
        stack = contextlib.ExitStack()
        stack.enter_context(torch.no_grad())
        stack.enter_context(torch.autocast(self._ids.device.type, dtype=self.act if self.act != torch.float32 else torch.bfloat16,
                                           enabled=self.act != torch.float32))
        stack.enter_context(fp16_kernels(self.act == torch.float16))
        return stack

    def _sampler(self, top_k, top_p, temperature, seed, row_offset, allowed_token_ids, position):
        from . import ops
        key = None if allowed_token_ids is None else tuple(allowed_token_ids)
        if key not in self._masks:
            while len(self._masks) >= self.MAX_MASKS:  # a caller that varies the set per call does not grow the stack without bound
                del self._masks[next(iter(self._masks))]
            self._masks[key] = _logit_mask(allowed_token_ids, self.V, self._ids.device)
        return ops.sampler_args(top_k, top_p, temperature, seed, row_offset, position, self._masks[key])

    @property
    def next_ids(self) -> Tensor:
        """(B) int64: the ids the last prefill / step sampled (a view: the next call overwrites it)."""
        return self._ids[:self.batch_size]

    @property
    def uniforms(self) -> Tensor:
        """(B) fp32: the uniforms the last prefill / step consumed (a view)."""
        return self._u[:self.batch_size]

    def prefill(self, input_ids: Tensor, top_k: int = 1, top_p: float = 0.0, temperature: float = 1.0, seed: int = 0, row_offset: int = 0,
                allowed_token_ids=None) -> Tensor:
        """Resets the cache, runs the prompt input_ids (B, L0) through the full-sequence kernels (forward_tframe_cached) and returns the
        logits (B, V) of its last position; the first new token, sampled from them with the given arguments, is left in `next_ids`."""
        from . import _lib as L
        B, L0 = input_ids.shape
        if B > self.max_batch_size:
            raise ValueError(f"this DecodeStack holds {self.max_batch_size} rows, the batch has {B}")
        self._check_pointers()
        ip = self.inference_params
        ip.seqlen_offset = 0
        with self._scope():
            hidden_t = self.model.caduceus.backbone.forward_tframe_cached(input_ids, None, ip)
            logits, _ = self.model.logits_tframe(hidden_t[:, :, -1:].contiguous(), None, -100)
        ip.seqlen_offset = L0
        self.batch_size = B
        self._args.B = B
        out = self._logits[:B * self.V].view(B, self.V)
        out.copy_(logits[:, 0])
        s = self._sampler(top_k, top_p, temperature, seed, row_offset, allowed_token_ids, L0)
        stream = L.stream_and_check(self._scratch)
        L.check(L.get_lib().cad_sample_tokens(L.ptr(self._logits), B, self.V, C.byref(s), L.ptr(self._ids), L.ptr(self._u), stream),
                "cad_sample_tokens")
        return out

    def step(self, ids: Optional[Tensor] = None, top_k: int = 1, top_p: float = 0.0, temperature: float = 1.0, seed: int = 0,
             row_offset: int = 0, allowed_token_ids=None):
        """One token: consumes ids (B) -- default: its own last `next_ids`, which never leave the device --, advances the cache and returns
        (next_ids (B) int64, logits (B, V) fp32), the next token sampled from those logits.  The uniform of row b is keyed by
        (seed, row_offset + b, position of the sampled token in the sequence).
        ids given here are the caller's to keep in [0, vocab_size): the kernel clamps an id outside that range to the nearest valid
        one rather than read outside the embedding table, where decode_step's embedding lookup would raise."""
        from . import _lib as L
        from . import ops
        if self.batch_size == 0:
            raise RuntimeError("DecodeStack.step before prefill")
        B = self.batch_size
        if ids is not None:
            self._ids[:B].copy_(ids.reshape(B))
        ip = self.inference_params
        self._args.sampler = self._sampler(top_k, top_p, temperature, seed, row_offset, allowed_token_ids, ip.seqlen_offset + 1)
        ops.decode_token(self._args, L.stream_and_check(self._scratch))
        ip.seqlen_offset += 1
        return self._ids[:B], self._logits[:B * self.V].view(B, self.V)


def _generate_sampled(model, input_ids, max_new_tokens, return_logits, sampling, eos_token_id, fused):
    from . import ops
    B, L0 = input_ids.shape
    dev = input_ids.device
    stack = None
    if fused is not False:
        try:
            stack = DecodeStack(model, B)
        except DecodeUnsupported:
            if fused:
                raise
    out = torch.empty((B, L0 + max_new_tokens), dtype=input_ids.dtype, device=dev)
    out[:, :L0] = input_ids
    all_logits = []
    done = torch.zeros(B, dtype=torch.bool, device=dev) if eos_token_id is not None else None
    eos = None if eos_token_id is None else torch.full((B,), int(eos_token_id), dtype=torch.int64, device=dev)
    if stack is None:  # today's loop, the sampler as its own launch (a vocabulary beyond 64 ids: the same rules in torch ops)
        params = InferenceParams(max_seqlen=L0 + max_new_tokens, max_batch_size=B)
        mask = _logit_mask(sampling["allowed_token_ids"], model.config.vocab_size, dev)
        kw = {k: sampling[k] for k in ("top_k", "top_p", "temperature", "seed")}
    cur = input_ids
    for t in range(max_new_tokens):
        if stack is None:
            logits = decode_step(model, cur, params)
            nxt = ops.sample_tokens(logits, position=L0 + t, logit_mask=mask, **kw)
        elif t == 0:
            logits = stack.prefill(input_ids, **sampling)
            nxt = stack.next_ids
        else:
            nxt, logits = stack.step(cur, **sampling)
        cur = None  # (the stack feeds its own ids back)
        if done is not None:  # rows that have emitted eos keep emitting it: a mask on the device, nothing is read back
            done |= nxt == eos
            nxt = cur = torch.where(done, eos, nxt)
        out[:, L0 + t] = nxt
        if stack is None:
            cur = nxt.to(input_ids.dtype).unsqueeze(1)
        if return_logits:
            all_logits.append(logits.clone())
    return (out, all_logits) if return_logits else out


def generate(model, input_ids: Tensor, max_new_tokens: int, return_logits: bool = False, *, top_k: int = 1, top_p: float = 0.0,
             temperature: float = 1.0, seed: Optional[int] = None, allowed_token_ids=None, eos_token_id: Optional[int] = None,
             fused: Optional[bool] = None):
    """Continuation: ids (B, L0 + max_new_tokens) -- one prefill of input_ids (B, L0), then one decode step per new token.
    return_logits: also the list of the max_new_tokens logits (B, V) each new token was drawn from.

    With the first four arguments only: the greedy loop over decode_step (argmax on the logits).  Any of the keyword arguments selects
    sampled generation by mamba_ssm's rules (ops.sample_tokens): `allowed_token_ids` restricts the ids that can appear (e.g. the four
    bases; the padded vocabulary is mostly specials), top_k == 1 is the argmax (ties to the lowest id), top_k == 0 keeps all, top_p in
    (0, 1) is nucleus sampling, temperature > 0 divides the kept logits.  seed: keys the uniforms, u = f(seed, row, position), so a
    (seed, row, position) gives the same token whatever the batch; None with top_k != 1 draws one seed from torch's default generator
    (host side, once per call).  eos_token_id: a row that has emitted it keeps emitting it; the loop always runs max_new_tokens steps
    and never reads a tensor back.  fused: True runs the token through DecodeStack (one library call per token) and raises where that
    is unsupported; None does so where supported, else the decode_step loop with the sampler as its own launch; False forces that loop."""
    from . import ops
    sampled = (top_k != 1 or top_p != 0.0 or temperature != 1.0 or seed is not None or allowed_token_ids is not None
               or eos_token_id is not None)
    if sampled or fused is not None:
        ops.check_sampling(top_k, top_p, temperature)
        V = model.config.vocab_size
        if allowed_token_ids is not None:
            allowed_token_ids = tuple(sorted({int(i) for i in allowed_token_ids}))
            _logit_mask(allowed_token_ids, V, "cpu")
        if eos_token_id is not None and not 0 <= int(eos_token_id) < V:
            raise ValueError(f"eos_token_id must lie in [0, {V}), got {eos_token_id}")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if top_k != 1 else 0
        sampling = dict(top_k=int(top_k), top_p=float(top_p), temperature=float(temperature), seed=int(seed),
                        allowed_token_ids=allowed_token_ids)
        return _generate_sampled(model, input_ids, max_new_tokens, return_logits, sampling, eos_token_id, fused)
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
