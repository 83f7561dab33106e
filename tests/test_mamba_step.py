"""Step-wise decoding of one left-to-right Mamba: the step kernels (cad_mamba_step), the prefill that fills the cache and the chunked
prefill that continues from it, held to an fp64 restatement of the recurrence (written here; it shares no code with the package).

The rule: what comes out of the cache path (outputs; the two states after every step) may be at most 1.5 times as far from fp64 as the
SAME quantity from the full-sequence path in one piece (bf16 / fp16; 1.5 is the project's factor,
test_engine_b16.py::test_bf16_engine_error_is_the_library_branch_s).  In fp32 both errors are rounding noise and a ratio means nothing:
both are capped by the project's fp32 parity bound, 6e-4 relative (test_model_parity.py::test_model_matches_reference_fp32).  The
one-piece yardstick of a state after t tokens is the state a single prefill of those t tokens leaves (the full-sequence kernels).
Widths: d_model 64 (E 128, R 4) and d_model 40 (E 80, R 3: E no multiple of 64, R no multiple of 4; the full-sequence forward accepts
it on both backends)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from caduceus_amd import _lib, engine, ops
from caduceus_amd.generation import InferenceParams
from caduceus_amd.mamba import Mamba, fp16_kernels
from conftest import ROOT

FACTOR = 1.5
FP32_BOUND = 6e-4
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (d_model, d_conv, bias and conv_bias)
WIDTHS = [(64, 4, False), (64, 2, True), (40, 4, True), (40, 2, False)]


def _mamba(d_model, d_conv, bias, dev, seed=0):
    torch.manual_seed(seed)
    m = Mamba(d_model, d_conv=d_conv, bias=bias, conv_bias=bias, layer_idx=0)
    with torch.no_grad():
        if bias:
            m.in_proj.bias.normal_(std=0.1)
            m.out_proj.bias.normal_(std=0.1)
            m.conv1d.bias.normal_(std=0.1)
        m.A_log.add_(0.3 * torch.randn_like(m.A_log))
        m.D.add_(0.2 * torch.randn_like(m.D))
    return m.to(dev).eval()


def _ref64(m, x):
    """fp64 restatement of mamba-ssm `Mamba.step`, token by token, from empty states.  x: (B, L, D).  Returns outputs (B, L, D) and,
    after every token, conv_state (B, E, K) and ssm_state (B, E, N)."""
    d = lambda p: None if p is None else p.detach().double().cpu()
    W_in, b_in, W_x, W_dt, dt_b = d(m.in_proj.weight), d(m.in_proj.bias), d(m.x_proj.weight), d(m.dt_proj.weight), d(m.dt_proj.bias)
    cw, cb, W_out, b_out = d(m.conv1d.weight).squeeze(1), d(m.conv1d.bias), d(m.out_proj.weight), d(m.out_proj.bias)
    A, Dp = -torch.exp(d(m.A_log)), d(m.D)
    x = x.detach().double().cpu()
    B, L, _ = x.shape
    E, N, R, K = m.d_inner, m.d_state, m.dt_rank, m.d_conv
    conv = torch.zeros(B, E, K, dtype=torch.float64)
    ssm = torch.zeros(B, E, N, dtype=torch.float64)
    outs, convs, ssms = [], [], []
    for t in range(L):
        xz = x[:, t] @ W_in.t()
        if b_in is not None:
            xz = xz + b_in
        xs, z = xz[:, :E], xz[:, E:]
        conv = torch.cat([conv[:, :, 1:], xs.unsqueeze(2)], dim=2)
        pre = (conv * cw).sum(-1)
        if cb is not None:
            pre = pre + cb
        xc = F.silu(pre)
        dbc = xc @ W_x.t()
        dt = F.softplus(dbc[:, :R] @ W_dt.t() + dt_b)
        Bm, Cm = dbc[:, R:R + N], dbc[:, R + N:]
        ssm = torch.exp(dt.unsqueeze(2) * A) * ssm + dt.unsqueeze(2) * Bm.unsqueeze(1) * xc.unsqueeze(2)
        y = ((ssm * Cm.unsqueeze(1)).sum(-1) + Dp * xc) * F.silu(z)
        out = y @ W_out.t()
        if b_out is not None:
            out = out + b_out
        outs.append(out)
        convs.append(conv)
        ssms.append(ssm)
    return torch.stack(outs, 1), convs, ssms


def _err(got, ref):
    return float((got.detach().double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300))


def _hold(name, err_cache, err_one_piece, dtype):
    """The rule of this file (module docstring); prints the figures before it asserts."""
    print(f"{name}: cache path {err_cache:.3e}  one piece {err_one_piece:.3e}  [{dtype}]")
    if dtype == torch.float32:
        assert err_cache <= FP32_BOUND and err_one_piece <= FP32_BOUND, (name, err_cache, err_one_piece)
    else:
        assert err_cache <= FACTOR * err_one_piece, (name, err_cache, err_one_piece)


def _scope(dtype):
    return fp16_kernels(dtype == torch.float16)


def _params(B, max_batch=4):
    return InferenceParams(max_seqlen=64, max_batch_size=max_batch)


def _prefill_states(m, x):
    """(conv_state, ssm_state) rows [0, B) after ONE prefill of x (B, L, D) through the full-sequence kernels."""
    ip = _params(x.shape[0])
    m(x, inference_params=ip)
    conv, ssm = ip.key_value_memory_dict[0]
    return conv[:x.shape[0]], ssm[:x.shape[0]]


@pytest.mark.parametrize("L0,B", [(2, 1), (7, 3)])
@pytest.mark.parametrize("d_model,d_conv,bias", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_prefill_then_steps_against_fp64(backend, dtype, d_model, d_conv, bias, L0, B):
    """L0 + 9 tokens in one piece, and as a prefill of L0 (2 < d_conv: the left pad) followed by 9 steps: outputs and, after every
    step, both states against fp64 by the rule; the state tensors are updated in place."""
    _, dev = backend
    T = 9
    m = _mamba(d_model, d_conv, bias, dev)
    torch.manual_seed(1)
    x = torch.randn(B, L0 + T, d_model, device=dev).to(dtype)
    with torch.no_grad(), _scope(dtype):
        ref_out, ref_conv, ref_ssm = _ref64(m, x)
        one = m(x)
        ip = _params(B)
        outs = [m(x[:, :L0], inference_params=ip)]
        ip.seqlen_offset += L0
        conv, ssm = ip.key_value_memory_dict[0]
        assert conv.shape == (4, m.d_inner, d_conv) and ssm.shape == (4, m.d_inner, m.d_state)
        assert conv.dtype == dtype and ssm.dtype == torch.float32
        ptrs = (conv.data_ptr(), ssm.data_ptr())
        for t in range(L0, L0 + T):
            outs.append(m(x[:, t:t + 1], inference_params=ip))
            ip.seqlen_offset += 1
            assert ip.key_value_memory_dict[0][0] is conv and ip.key_value_memory_dict[0][1] is ssm
            assert (conv.data_ptr(), ssm.data_ptr()) == ptrs
            assert torch.isfinite(ssm).all() and torch.isfinite(conv.float()).all()
            conv1, ssm1 = _prefill_states(m, x[:, :t + 1])
            _hold(f"ssm_state after token {t}", _err(ssm[:B], ref_ssm[t]), _err(ssm1, ref_ssm[t]), dtype)
            _hold(f"conv_state after token {t}", _err(conv[:B], ref_conv[t]), _err(conv1, ref_conv[t]), dtype)
        got = torch.cat(outs, dim=1)
    assert got.shape == one.shape and got.dtype == one.dtype
    _hold("stepped outputs", _err(got[:, L0:], ref_out[:, L0:]), _err(one[:, L0:], ref_out[:, L0:]), dtype)
    _hold("all outputs", _err(got, ref_out), _err(one, ref_out), dtype)


@pytest.mark.parametrize("L0", [2, 7])
@pytest.mark.parametrize("d_model,d_conv,bias", [(64, 4, True), (40, 2, False)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_prefill_states_are_the_scan_carry_and_the_last_columns_of_x(backend, dtype, d_model, d_conv, bias, L0):
    """After a prefill ssm_state is the hT of ops.selective_scan_stateful on the same operands, bit for bit (the same kernel), and
    conv_state the last d_conv columns of x, zero-padded on the left when L0 < d_conv."""
    _, dev = backend
    B = 3
    m = _mamba(d_model, d_conv, bias, dev)
    torch.manual_seed(2)
    x = torch.randn(B, L0, d_model, device=dev).to(dtype)
    E, N, R = m.d_inner, m.d_state, m.dt_rank
    with torch.no_grad(), _scope(dtype):
        conv, ssm = _prefill_states(m, x)
        xz = engine._in_proj(m, x.reshape(B * L0, d_model), B, L0, dtype)
        xc, delta, A, Bm, Cm, Dp, dt_bias = engine._scan_inputs(xz, m, B, 0, 1, dtype)
        _, hT = ops.selective_scan_stateful(xc, delta, A, Bm, Cm, Dp, xz[E:], dt_bias, None, B, 0, 1)
    assert torch.equal(ssm, hT.permute(1, 0, 2))
    xs = xz[:E].permute(1, 0, 2)  # (B, E, L0)
    want = torch.zeros(B, E, d_conv, dtype=dtype, device=dev)
    n = min(L0, d_conv)
    want[:, :, d_conv - n:] = xs[:, :, L0 - n:]
    assert torch.equal(conv, want)


@pytest.mark.parametrize("d_model,d_conv,bias", [(64, 4, False), (40, 2, True)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_chunked_prefill_against_fp64(backend, dtype, d_model, d_conv, bias):
    """Chunks of 5 + 1 + 6 through the cache (the middle one is a step) against one 12-token forward, by the rule; the states left
    behind against those of one 12-token prefill."""
    _, dev = backend
    B = 3
    m = _mamba(d_model, d_conv, bias, dev)
    torch.manual_seed(3)
    x = torch.randn(B, 12, d_model, device=dev).to(dtype)
    with torch.no_grad(), _scope(dtype):
        ref_out, ref_conv, ref_ssm = _ref64(m, x)
        one = m(x)
        ip = _params(B)
        outs = []
        for a, b in ((0, 5), (5, 6), (6, 12)):
            outs.append(m(x[:, a:b], inference_params=ip))
            ip.seqlen_offset += b - a
        conv, ssm = ip.key_value_memory_dict[0]
        conv1, ssm1 = _prefill_states(m, x)
    _hold("chunked outputs", _err(torch.cat(outs, 1), ref_out), _err(one, ref_out), dtype)
    _hold("last chunk's outputs", _err(outs[2], ref_out[:, 6:]), _err(one[:, 6:], ref_out[:, 6:]), dtype)
    _hold("ssm_state", _err(ssm[:B], ref_ssm[-1]), _err(ssm1, ref_ssm[-1]), dtype)
    _hold("conv_state", _err(conv[:B], ref_conv[-1]), _err(conv1, ref_conv[-1]), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_edge_values(backend, dtype):
    """dt_bias on both branches of softplus' threshold (delta + bias > 20 and far below), A_log with exp(dt A) within 1e-6 of 1 and
    below 1e-30, an all-zero token among the steps: the states stay finite and outputs and states keep the rule."""
    _, dev = backend
    B, L0, T, d_model = 3, 3, 6, 64
    m = _mamba(d_model, 4, True, dev)
    E = m.d_inner
    with torch.no_grad():
        m.dt_proj.bias[0:E:4] = 24.0    # softplus(x) = x
        m.dt_proj.bias[1:E:4] = -12.0   # softplus(x) ~ exp(x)
        m.dt_proj.bias[2:E:4] = 19.5    # next to the threshold, either side with delta
        m.A_log[:, 0] = -20.0           # A = -2e-9: exp(dt A) = 1 - O(1e-7) even at dt = 24
        m.A_log[:, 1] = 5.0             # A = -148: exp(dt A) < 1e-30 where dt > 0.5
    torch.manual_seed(4)
    x = torch.randn(B, L0 + T, d_model, device=dev).to(dtype)
    x[:, L0 + 2] = 0
    with torch.no_grad(), _scope(dtype):
        ref_out, ref_conv, ref_ssm = _ref64(m, x)
        dt_last = F.softplus(m.dt_proj.bias.double().cpu())
        decay = torch.exp(-dt_last.unsqueeze(1) * torch.exp(m.A_log.double().cpu()))
        assert float((1 - decay[:, 0]).abs().max()) < 1e-6 and float(decay[0:E:4, 1].max()) < 1e-30  # the regimes are the named ones
        one = m(x)
        ip = _params(B)
        outs = [m(x[:, :L0], inference_params=ip)]
        ip.seqlen_offset += L0
        for t in range(L0, L0 + T):
            outs.append(m(x[:, t:t + 1], inference_params=ip))
            ip.seqlen_offset += 1
        conv, ssm = ip.key_value_memory_dict[0]
        assert torch.isfinite(ssm).all() and torch.isfinite(conv.float()).all()
        conv1, ssm1 = _prefill_states(m, x)
    got = torch.cat(outs, 1)
    assert torch.isfinite(got.float()).all()
    _hold("stepped outputs", _err(got[:, L0:], ref_out[:, L0:]), _err(one[:, L0:], ref_out[:, L0:]), dtype)
    _hold("ssm_state", _err(ssm[:B], ref_ssm[-1]), _err(ssm1, ref_ssm[-1]), dtype)
    _hold("conv_state", _err(conv[:B], ref_conv[-1]), _err(conv1, ref_conv[-1]), dtype)


@pytest.mark.parametrize("d_model,d_conv,bias", [(64, 4, True), (40, 2, False)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_rows_are_independent_and_spare_cache_rows_untouched(backend, dtype, d_model, d_conv, bias):
    """Stepping rows {0, 1, 2} together equals stepping each alone, bit for bit (outputs and states); row 3 of a 4-row cache keeps
    the values it had."""
    _, dev = backend
    m = _mamba(d_model, d_conv, bias, dev)
    torch.manual_seed(5)
    x = torch.randn(3, 4, d_model, device=dev).to(dtype)
    with torch.no_grad(), _scope(dtype):
        conv, ssm = m.allocate_inference_cache(4, 64, dtype=dtype)
        conv.copy_(torch.randn(conv.shape, device=dev).to(dtype))
        ssm.copy_(torch.randn(ssm.shape, device=dev))
        conv0, ssm0 = conv.clone(), ssm.clone()
        together = []
        for t in range(4):
            out, c, s = m.step(x[:, t:t + 1], conv, ssm)
            assert c is conv and s is ssm
            together.append(out)
        together = torch.cat(together, 1)
        assert torch.equal(conv[3], conv0[3]) and torch.equal(ssm[3], ssm0[3])
        for r in range(3):
            c1, s1 = conv0[r:r + 1].clone(), ssm0[r:r + 1].clone()
            alone = torch.cat([m.step(x[r:r + 1, t:t + 1], c1, s1)[0] for t in range(4)], 1)
            assert torch.equal(alone, together[r:r + 1]), r
            assert torch.equal(c1[0], conv[r]) and torch.equal(s1[0], ssm[r]), r


def test_unsupported_shapes_are_refused(backend):
    """d_conv 5: cad_mamba_step_supported is false and the call returns CAD_ERR_UNSUPPORTED (the states are not touched)."""
    _, dev = backend
    lib = _lib.get_lib()
    D, E, N, R = 64, 128, 16, 4
    assert lib.cad_mamba_step_supported(D, E, N, R, 4, _lib.CAD_F32) == 1
    assert lib.cad_mamba_step_supported(D, E, N, R, 5, _lib.CAD_F32) == 0
    assert lib.cad_mamba_step_supported(D, E, N, R, 0, _lib.CAD_F32) == 0
    assert lib.cad_mamba_step_supported(D, E, N, R, 4, 7) == 0
    assert lib.cad_mamba_step_scratch_floats(3, E, N, R) >= 3 * E
    z = lambda *s: torch.zeros(*s, device=dev)
    conv, ssm = torch.ones(2, E, 5, device=dev), torch.ones(2, E, N, device=dev)
    t = dict(h=z(2, D), out=z(2, D), conv_state=conv, ssm_state=ssm, W_in=z(2 * E, D), conv_w=z(E, 5), W_x=z(R + 2 * N, E), W_dt=z(E, R),
             dt_bias=z(E), A_log=z(E, N), Dskip=z(E), W_out=z(D, E), scratch=z(int(lib.cad_mamba_step_scratch_floats(2, E, N, R))))
    a = _lib.MambaStepArgs(B=2, D=D, E=E, N=N, R=R, K=5, dtype=_lib.CAD_F32, **{k: _lib.ptr(v) for k, v in t.items()})
    assert lib.cad_mamba_step(ctypes.byref(a), _lib.stream_and_check(*t.values())) == 2  # CAD_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.mamba_step(t["h"], conv, ssm, t["W_in"], None, t["conv_w"], None, t["W_x"], t["W_dt"], t["dt_bias"], t["A_log"], t["Dskip"],
                       t["W_out"], None, t["scratch"])
    assert bool((conv == 1).all()) and bool((ssm == 1).all())


def _header_step_struct():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "caduceus_hip.h")).read(), flags=re.S)
    body = re.search(r"struct cad_mamba_step_args \{(.*?)\};", txt, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = decl.split(",")
            fields.append(names[0].split()[-1].lstrip("*"))
            fields += [n.strip().lstrip("*") for n in names[1:]]
    return fields


def test_step_args_mirror_the_header(tmp_path):
    """MambaStepArgs: the header's field order, and the size a C compiler gives the struct."""
    assert [f[0] for f in _lib.MambaStepArgs._fields_] == _header_step_struct()
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "caduceus_hip.h"\nint main(){printf("%zu\\n", sizeof(cad_mamba_step_args));return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)]).decode()) == ctypes.sizeof(_lib.MambaStepArgs)
