"""The mixer-level boundary the reference sits on, re-implemented over the HIP engine:
`Mamba`, `Block`, `RMSNorm`, `rms_norm_fn`, `layer_norm_fn` with the constructor / forward signatures of
mamba-ssm 1.2.0 (imported by the reference at /root/reference/caduceus/modeling_caduceus.py:11-27 and
modeling_rcps.py:12-18; SURVEY.md section 8b "lower (mixer) boundary").  Parameter names, shapes and
initialisation follow upstream so that state dicts are interchangeable.
"""
from __future__ import annotations

import contextlib
import math
import threading
from typing import Optional

import torch
from torch import nn

from . import engine, ops


def requested_dtype(x: torch.Tensor) -> torch.dtype:
    """The dtype the caller asked for: the autocast dtype when autocast is on (the reference trains under AMP,
    configs/experiment/hg38/hg38.yaml:20), else the dtype of x."""
    dt = x.dtype
    dev = x.device.type
    try:
        if torch.is_autocast_enabled(dev):
            dt = torch.get_autocast_dtype(dev)
    except (TypeError, RuntimeError):
        pass
    return dt


_fp16 = threading.local()


def fp16_kernels_enabled() -> bool:
    """True inside `fp16_kernels()` (this thread)."""
    return bool(getattr(_fp16, "on", False))


@contextlib.contextmanager
def fp16_kernels(enabled: bool = True):
    """Opt-in fp16 compute path (thread-local): while active, a float16 request -- fp16 autocast, or fp16 inputs without
    autocast -- runs the float16 instantiations of the kernels (fp16 activations in HBM, fp32 arithmetic and accumulation inside
    the kernels, fp32 parameters: the contract of the bf16 path) instead of the fp32 kernels.  `enabled=False` switches it off
    for a nested region.  CaduceusConfig(fp16_kernels=True) enters it in the models' forward."""
    prev = getattr(_fp16, "on", False)
    _fp16.on = bool(enabled)
    try:
        yield
    finally:
        _fp16.on = prev


def act_dtype_of(x: torch.Tensor) -> torch.dtype:
    """Compute dtype of the kernels for input x.  fp32 and bf16 are implemented, and fp16 behind the opt-in `fp16_kernels()`.
    Without the opt-in a float16 request (the reference's own AMP precision, and vep_embeddings.py:352) is COMPUTED BY THE FP32
    KERNELS -- at least as accurate as fp16 arithmetic -- and the module outputs are rounded to float16 (as_requested); inside
    `fp16_kernels()` it is computed by the fp16 kernels and this returns torch.float16."""
    dt = requested_dtype(x)
    if dt == torch.float16:
        return torch.float16 if fp16_kernels_enabled() else torch.float32
    if dt not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"caduceus_amd computes in float32 or bfloat16 (requested {dt}); on MI355X use bf16")
    return dt


def as_requested(t: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Output t of a module called with input x: float16 when float16 was requested (see act_dtype_of), else unchanged."""
    return t.to(torch.float16) if requested_dtype(x) == torch.float16 else t


# The reference passes `inference_params` through its bi-directional and RCPS wrappers and lets both directions share one cache
# (modeling_caduceus.py:122-132, modeling_rcps.py:201-206); that is not a decode step of anything, so it is not restated here.
NO_STEPWISE_FORM = ("step-wise decoding needs a causal stack (bidirectional=False, rcps=False): a right-to-left direction has no "
                    "step-wise form, every new token would change the state at every earlier position")


class Mamba(nn.Module):
    """Parameter container + single-direction forward with the signature of mamba_ssm.modules.mamba_simple.Mamba."""

    def __init__(self, d_model, d_state=16, d_conv=4, expand=2, dt_rank="auto", dt_min=0.001, dt_max=0.1,
                 dt_init="random", dt_scale=1.0, dt_init_floor=1e-4, conv_bias=True, bias=False, use_fast_path=True,
                 layer_idx=None, device=None, dtype=None):
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        self.d_model, self.d_state, self.d_conv, self.expand = d_model, d_state, d_conv, expand
        self.d_inner = int(expand * d_model)
        self.dt_rank = math.ceil(d_model / 16) if dt_rank == "auto" else dt_rank
        self.use_fast_path = use_fast_path
        self.layer_idx = layer_idx
        if d_conv > 4:
            raise NotImplementedError("d_conv <= 4 (same limit as upstream causal_conv1d)")
        self.in_proj = nn.Linear(d_model, self.d_inner * 2, bias=bias, **factory_kwargs)
        self.conv1d = nn.Conv1d(self.d_inner, self.d_inner, bias=conv_bias, kernel_size=d_conv, groups=self.d_inner,
                                padding=d_conv - 1, **factory_kwargs)
        self.x_proj = nn.Linear(self.d_inner, self.dt_rank + d_state * 2, bias=False, **factory_kwargs)
        self.dt_proj = nn.Linear(self.dt_rank, self.d_inner, bias=True, **factory_kwargs)
        # dt_proj init preserves variance at initialisation; bias = softplus^-1(dt), dt ~ logU[dt_min, dt_max]
        dt_init_std = self.dt_rank ** -0.5 * dt_scale
        if dt_init == "constant":
            nn.init.constant_(self.dt_proj.weight, dt_init_std)
        elif dt_init == "random":
            nn.init.uniform_(self.dt_proj.weight, -dt_init_std, dt_init_std)
        else:
            raise NotImplementedError
        dt = torch.exp(torch.rand(self.d_inner, **factory_kwargs) * (math.log(dt_max) - math.log(dt_min))
                       + math.log(dt_min)).clamp(min=dt_init_floor)
        inv_dt = dt + torch.log(-torch.expm1(-dt))
        with torch.no_grad():
            self.dt_proj.bias.copy_(inv_dt)
        self.dt_proj.bias._no_reinit = True
        A = torch.arange(1, d_state + 1, dtype=torch.float32, device=device).repeat(self.d_inner, 1).contiguous()
        self.A_log = nn.Parameter(torch.log(A))
        self.A_log._no_weight_decay = True
        self.D = nn.Parameter(torch.ones(self.d_inner, device=device))
        self.D._no_weight_decay = True
        self.out_proj = nn.Linear(self.d_inner, d_model, bias=bias, **factory_kwargs)

    def forward(self, hidden_states, inference_params=None):
        """hidden_states: (B, L, D) -> (B, L, D), left-to-right.  With `inference_params` (generation.InferenceParams) the layer's
        (conv_state, ssm_state) are looked up by layer_idx in its key_value_memory_dict (allocated on first use) and left up to date:
        seqlen_offset == 0 is a prefill, seqlen_offset > 0 with L == 1 one `step`, with L > 1 the next chunk of a prefill."""
        if inference_params is None:
            act = act_dtype_of(hidden_states)
            out = engine.bimamba_tframe(hidden_states.to(act).unsqueeze(0), self, None, None, strand_swap=False)
            return as_requested(out[0], hidden_states)
        B, L, _ = hidden_states.shape
        act = act_dtype_of(hidden_states)
        conv_state, ssm_state = self._get_states_from_cache(inference_params, B, act)
        if inference_params.seqlen_offset > 0 and L == 1:
            return self.step(hidden_states, conv_state, ssm_state)[0]
        dev = hidden_states.device.type
        with torch.no_grad(), torch.autocast(dev, enabled=False):  # (the compute dtype is decided: see engine.bimamba_tframe)
            out = engine.mamba_prefill(hidden_states.to(act), self, conv_state, ssm_state, cont=inference_params.seqlen_offset > 0)
        return as_requested(out, hidden_states)

    def step(self, hidden_states, conv_state, ssm_state):
        """mamba_ssm `Mamba.step`: one token hidden_states (B, 1, D) -> (out (B, 1, D), conv_state, ssm_state), the two states updated
        in place in their first B rows.  Runs the step kernels (ops.mamba_step) on the fp32 master parameters."""
        B, L, _ = hidden_states.shape
        if L != 1:
            raise ValueError("Only support decoding with 1 token at a time for now")
        act = act_dtype_of(hidden_states)
        if conv_state.dtype != act:
            raise TypeError(f"conv_state is {conv_state.dtype} but this call computes in {act}: allocate the cache with dtype={act}")
        need = (B, self.d_inner, self.d_state, self.dt_rank)
        scratch = getattr(self, "_step_scratch", None)
        if scratch is None or scratch[0] != need or scratch[1].device != hidden_states.device:
            scratch = (need, ops.mamba_step_scratch(*need, hidden_states.device))
            self._step_scratch = scratch  # (a plain attribute: not a buffer, never saved)
        f = lambda p: None if p is None else p.float()
        with torch.no_grad():
            out = ops.mamba_step(hidden_states[:, 0].to(act).contiguous(), conv_state, ssm_state, f(self.in_proj.weight),
                                 f(self.in_proj.bias), f(self.conv1d.weight), f(self.conv1d.bias), f(self.x_proj.weight),
                                 f(self.dt_proj.weight), f(self.dt_proj.bias), f(self.A_log), f(self.D), f(self.out_proj.weight),
                                 f(self.out_proj.bias), scratch[1], act)
        return as_requested(out.unsqueeze(1), hidden_states), conv_state, ssm_state

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        """(conv_state (B, E, d_conv) in `dtype`, ssm_state (B, E, N) fp32), zeroed.  dtype: the compute dtype of the calls that will
        use the cache (default: the parameters' dtype; under bf16 autocast pass torch.bfloat16)."""
        device = self.out_proj.weight.device
        conv_dtype = self.conv1d.weight.dtype if dtype is None else dtype
        conv_state = torch.zeros(batch_size, self.d_inner, self.d_conv, device=device, dtype=conv_dtype)
        ssm_state = torch.zeros(batch_size, self.d_inner, self.d_state, device=device, dtype=torch.float32)
        return conv_state, ssm_state

    def _get_states_from_cache(self, inference_params, batch_size, act):
        if self.layer_idx is None:
            raise ValueError("a Mamba that is used with inference_params needs a layer_idx")
        kv = inference_params.key_value_memory_dict
        if self.layer_idx not in kv:  # allocated on first use, as upstream does -- in the compute dtype of this call
            kv[self.layer_idx] = self.allocate_inference_cache(max(batch_size, inference_params.max_batch_size),
                                                               inference_params.max_seqlen, dtype=act)
        conv_state, ssm_state = kv[self.layer_idx]
        if conv_state.shape[0] < batch_size:
            raise ValueError(f"the inference cache holds {conv_state.shape[0]} rows, the batch has {batch_size}")
        return conv_state, ssm_state


class RMSNorm(nn.Module):
    """mamba_ssm.ops.triton.layernorm.RMSNorm: weight only, `bias` registered as None."""

    def __init__(self, hidden_size, eps=1e-5, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(hidden_size, device=device, dtype=dtype))
        self.register_parameter("bias", None)

    def forward(self, x, residual=None, prenorm=False, residual_in_fp32=False):
        return rms_norm_fn(x, self.weight, self.bias, residual=residual, eps=self.eps, prenorm=prenorm,
                           residual_in_fp32=residual_in_fp32)


def _norm_fn(x, weight, bias, residual, prenorm, eps, is_rms):
    act = act_dtype_of(x)
    shape = x.shape
    xs = x.reshape(1, -1, shape[-1])
    rs = None if residual is None else residual.reshape(1, -1, shape[-1]).float()
    if xs.dtype not in (torch.float32, act):
        xs = xs.to(act)
    y, res = ops.add_norm(xs, rs, weight, bias, eps, is_rms, False, act)
    y = as_requested(y.reshape(shape), x)
    return y if not prenorm else (y, res.reshape(shape))


def rms_norm_fn(x, weight, bias, residual=None, prenorm=False, residual_in_fp32=False, eps=1e-6):
    """Fused add + RMSNorm (single strand).  The residual stream is always kept in fp32 by this engine."""
    return _norm_fn(x, weight, bias, residual, prenorm, eps, True)


def layer_norm_fn(x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False, is_rms_norm=False):
    return _norm_fn(x, weight, bias, residual, prenorm, eps, is_rms_norm)


def norm_params(norm: nn.Module):
    """(weight, bias, eps, is_rms) of an RMSNorm / nn.LayerNorm module."""
    if isinstance(norm, RMSNorm):
        return norm.weight, norm.bias, norm.eps, True
    if isinstance(norm, nn.LayerNorm):
        return norm.weight, norm.bias, norm.eps, False
    raise TypeError("Only LayerNorm and RMSNorm are supported")


class Block(nn.Module):
    """mamba_ssm.modules.mamba_simple.Block (Caduceus-Ph layers): Add -> Norm -> Mixer, returning (hidden, residual)."""

    def __init__(self, dim, mixer_cls, norm_cls=nn.LayerNorm, fused_add_norm=False, residual_in_fp32=False):
        super().__init__()
        self.residual_in_fp32 = residual_in_fp32
        self.fused_add_norm = fused_add_norm
        self.mixer = mixer_cls(dim)
        self.norm = norm_cls(dim)

    def forward_tframe(self, hidden: torch.Tensor, residual: Optional[torch.Tensor], act: torch.dtype):
        w, b, eps, is_rms = norm_params(self.norm)
        hn, residual = ops.add_norm(hidden, residual, w, b, eps, is_rms, False, act, want_fp8=True)  # (feeds the mixer's in_proj)
        return self.mixer.forward_tframe(hn, strand_swap=False), residual

    def forward(self, hidden_states, residual=None, inference_params=None):
        act = act_dtype_of(hidden_states)
        h = hidden_states.unsqueeze(0)
        if h.dtype not in (torch.float32, act):
            h = h.to(act)
        r = None if residual is None else residual.unsqueeze(0).float()
        if inference_params is not None:  # the cached path: add + norm as always, then the mixer with its cache
            getattr(self.mixer, "_require_stepwise", lambda: None)()  # (a bi-directional mixer raises before any launch)
            w, b, eps, is_rms = norm_params(self.norm)
            with torch.no_grad():
                hn, res = ops.add_norm(h, r, w, b, eps, is_rms, False, act)
            return as_requested(self.mixer(hn[0], inference_params=inference_params), hidden_states), res[0]
        out, res = self.forward_tframe(h, r, act)
        return as_requested(out[0], hidden_states), res[0]

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        return self.mixer.allocate_inference_cache(batch_size, max_seqlen, dtype=dtype, **kwargs)
