"""The decode path -- the three step kernels (csrc/step_kernels.h, csrc/step.hip), the decode token's launch 1 with the add+norm in front
and its tail (csrc/decode.hip, csrc/cad_rownorm.h) -- held to float64 element by element, at the edges of the kernels' geometry.

In the manner of test_norm_head_fp64.py (hold, gam, U, UO, FLOOR, UF, OVER, an_reference and LOG_ULPS are imported from there) and of
test_conv_embed_fp64.py (EXP2_ULPS, RCP_ULPS and sigmoid_bounds, the conv + SiLU bound's sigma part, are imported from there): the
references are written here in torch.float64, start from the operands AS STORED and share no code with the package; every tolerance
is derived below from how the kernel rounds and nothing in it is fitted to a result.  Notation as there: u = 2^-24,
g(n) = n u / (1 - n u), uo = 0 / 2^-8 / 2^-11 for a value rounded to T = fp32 / bf16 / fp16, floor = half the spacing of T's subnormals,
UF = 2^-126 per fp32 operation that may underflow.  rT(v, e) = e + uo (|v| + e) + floor is one rounding to T of a value v known to e.

THE RULE: the intermediate scratch contents (xc | z | y, and res0 | res1 | out of the decode token) are part of what is checked.  Each
launch is held against fp64 from what the device actually handed it, so a tolerance is one launch's own rounding, never compounded.

Launch 1 (st_in_conv_rows), from h as stored:
  xz     S = W_in h.  64 lane partials (fused multiply-adds), a 6-step butterfly, in ANY association:
         e = g(D + 8) sum |W h| + D UF;  stored rounded to T: rT(S, e);  with b_in the kernel adds the bias ROUNDED TO T (a stated rounding
         point: the reference rounds it itself, so it is exact there) in fp32 and rounds again: v = S + rT(b), e' = e + u (|v| + e),
         then rT(v, e').  z in the scratch and the new conv_state column are held to this.
  window conv_state columns 0 .. K-2 equal the old columns 1 .. K-1 bit for bit; rows >= B of both states are untouched.
  xc     from the device's new conv_state: pre = b + sum_k w_k win_k, a chain of K fused multiply-adds from b:
         e_P = g(K) (|b| + sum |w win|) + K UF;  sigma by sigmoid_bounds;  e_o = (|P| + e_P)(s + e_s)(1 + u) - |P s| + UF;  rT(o, e_o).
Launch 2 (step_ssm_kernel), from the device's xc and z and the test's copy of the old ssm_state:
  dbc    = W_x xc rounded to T in LDS, not observable: e_dbc = rT(dbc, g(E + 8) sum |W_x xc| + E UF) is carried forward.
  delta  a chain of R fused multiply-adds: e0 = sum |W_dt| e_dbc + g(R) sum |W_dt| (|dbc| + e_dbc) + R UF, rounded: e_delta = rT(delta, e0).
  x      = delta + dt_bias, one fp32 add: e_x = e_delta + u (|x| + e_delta).
  dt     = softplus(x).  softplus is 1-Lipschitz: e_x passes through.  The kernel returns x^ itself where x^ > 20, which is off by
         log1p(exp(-x^)) <= exp(-20): added wherever x + e_x > 20 (either branch may be taken next to the threshold).  Otherwise
         e = exp2(fl(x^ fl(log2 e))): relative rho_e = expm1(g(2) (|x| + e_x) + 2 u EXP2_ULPS); the result is
         log(w) (e rcp(w - 1)), w = fl(1 + e), which is log1p(e^) up to the roundings of w, w - 1, the constant ln 2, three products and
         the log / rcp instructions (log(w) / (w - 1) moves by less than the relative change of w): rho_r = g(6) + 2 u (LOG_ULPS +
         RCP_ULPS); and |log1p(e^) - log1p(e)| <= sigma(x) rho_e (1 + rho_e).  (The d == 0 branch returns e for log1p(e): e / 2 < u.)
         e_dt = e_x + sigma(x + e_x) rho_e (1 + rho_e) + (dt + e_x) rho_r + 4 UF + [x + e_x > 20] log1p(exp(-(x - e_x))).
  decay  P = exp(-a), a = dt |A|, |A| = exp(A_log) computed as exp2: relative rho_A = expm1(g(2) |A_log| + 2 u EXP2_ULPS).  The
         argument dt A log2 e (two products and the rounded constant, g(3)) is off, in natural units, by
         d = |A| e_dt + a (rho_A + g(3)) + (dt + e_dt) UF;  e_P = P expm1(d + 2 u EXP2_ULPS) + UF  (UF: a result flushed to zero).
  state  h = P s0 + dt B xc (B the T-rounded dbc value, known to e_dbc): upper magnitudes multiplied through, the true ones
         subtracted, four roundings (three products and the add, fused or not):
         e_h = (P + e_P)|s0| - P |s0| + (dt + e_dt)(|B| + e_B)|xc| - dt |B xc| + g(4) (both upper magnitudes) + 2 UF.  fp32 output,
         held for EVERY n in [0, N).
  y      part = sum_n C_n h_n (N terms over 16 lanes and a 4-step butterfly, any association):
         e_part = sum (|C| e_h + e_C (|h| + e_h)) + g(N + 8) sum (|C| + e_C)(|h| + e_h) + N UF;
         y1 = part + D xc: e_y1 = e_part + g(2) (sum (|C| + e_C)(|h| + e_h) + |D xc|) + UF;
         gate = z sigma(z), z exact as read (sigmoid_bounds with e_P = 0): e_g = |z| e_s + u |z| (s + e_s) + UF -- at z = -100 the
         kernel's sigma is exactly 0 and the gate -0, which the absolute UF terms carry; at z = +100 sigma is 1 and the gate z;
         y = y1 gate: e_y = (|y1| + e_y1)(|gate| + e_g)(1 + u) - |y1 gate| + UF; stored as rT(y, e_y).
Launch 3 (step_out_kernel), from the device's y: the dot bound of launch 1 with E for D, one or two roundings to T.

Decode token (generation.DecodeStack, one step on a cache the test fills with drawn values, so that every window column and state lane
is non-zero and the full-sequence kernels' own shape limits do not restrict the geometry):
  residual  layer 0: equals emb[id] bit for bit; later layers: t = out + res, one fp32 add: u |t| (an_reference's res_out).
  xz        fp64 add+norm by an_reference (y, tol_y; the row statistics in cad_add_norm_fwd's order, which cad_row_norm_lds of csrc/cad_rownorm.h restates),
            through the W_in dot: e = sum |W| tol_y + g(D + 8) sum |W| (|y| + tol_y) + D UF, then the roundings of launch 1.
  xc, ssm_state, y, out   as above, from the device's conv_state / xc, z / y.
  logits    final add+norm of the device's out + res (an_reference), through the head dot with the same carry; fp32 output.
  ids       equal ops.sample_tokens on the device's own logits with the same seed, row_offset and position.
  A two-layer stack overwrites layer 0's scratch: layer 0 (and the tail behind it) is checked on a one-layer stack over the same
  layer-0 weights, whose out is then the input of the two-layer stack's layer 1; layer 0's states of the two stacks are equal bits.

The ulp constants of v_exp_f32, v_rcp_f32, v_log_f32 and v_rsq_f32 are the project's (assumptions about the hardware).
Non-finite values follow hold's rule; a row of h scaled until its xz overflows fp16 leaves every other row's bits unchanged.

Worst err / tol per output over all cases of a family (pytest -s prints them; test_zz_report_worst_ratios lists them), emulator |
MI355X, as fp32 / bf16 / fp16 (ssm_state, logits and the residual are fp32 outputs: one figure; the wide cases run in fp32 / bf16):
  family          z                        conv_state               xc                       ssm_state     y                        out
  step      emu   .030 / .977 / .920       .031 / .967 / .964       .425 / .995 / .995       .826          .011 / .519 / .493       .055 / .960 / .910
            hip   .030 / .977 / .920       .031 / .967 / .964       .443 / .995 / .995       .826          .010 / .519 / .493       .059 / .960 / .910
  step-edge emu   .011 / .837 / .739       .012 / .823 / .793       .240 / .985 / .945       .887          .001 / .279 / .370       .016 / .691 / .800
            hip   .011 / .837 / .739       .012 / .823 / .793       .314 / .985 / .945       .887          .001 / .279 / .370       .020 / .691 / .800
  step-wide emu   .000 / .849              .000 / .812              .396 / .994              .442          .000 / .232              .000 / .782
            hip   .000 / .849              .000 / .812              .396 / .994              .442          .000 / .232              .000 / .782
  overflow  emu = hip (fp16)  z .824, conv_state .761, xc .951, ssm_state .387, y .204, out .787; the overflowing row: classes equal
  decode    emu   .016 / .380 / .377       .022 / .351 / .385       .532 / .993 / .995       .450          .002 / .349 / .372       .010 / .944 / .942
            hip   .011 / .380 / .377       .013 / .351 / .385       .463 / .993 / .995       .450          .004 / .349 / .372       .013 / .944 / .942
  decode residual 1.000 (one fp32 add: an error of exactly half an ulp occurs) and logits .366 on both.
The 16-bit figures sit just under 1 because the last rounding to T dominates there and an error of nearly half an ulp of T occurs among
thousands of elements; a 16-bit result is the same on both backends wherever the fp32 values in front of it round alike.
No bound was exceeded on either backend and no kernel was changed.  The 65536-byte LDS request at width 2048 is accepted on both.
"""
import copy
import ctypes as C
import math

import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops
from caduceus_amd.generation import DecodeStack
from caduceus_amd.mamba import norm_params
from test_conv_embed_fp64 import EXP2_ULPS, RCP_ULPS, sigmoid_bounds
from test_decode_stack import _model
from test_norm_head_fp64 import FLOOR, LOG_ULPS, OVER, TAG, U, UF, UO, WORST, an_reference, gam, hold  # noqa: F401

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
TYPES = [pytest.param(F32, id="f32"), pytest.param(BF, id="bf16"), pytest.param(HF, id="f16")]
TYPES2 = TYPES[:2]
PARAMS = ("W_in", "b_in", "conv_w", "conv_b", "W_x", "W_dt", "dt_bias", "A_log", "Dskip", "W_out", "b_out")


# =========================================================================================================================================
# references
# =========================================================================================================================================
def rT(v, e, dt):
    """One rounding to T of a value v known to e."""
    return e + UO[dt] * (v.abs() + e) + FLOOR[dt]


def proj_bound(v, e_v, W, b, dt):
    """round_T(W v (+ round_T(b))) for rows v (B, n) fp64 known to e_v (None: exact): (ref, tol)."""
    Wd = W.double()
    n = Wd.shape[1]
    S = v @ Wd.t()
    if e_v is None:
        e = gam(n + 8) * (v.abs() @ Wd.abs().t()) + n * UF
    else:
        e = e_v @ Wd.abs().t() + gam(n + 8) * ((v.abs() + e_v) @ Wd.abs().t()) + n * UF
    e = rT(S, e, dt)
    if b is not None:
        S = S + b.to(dt).double()
        e = rT(S, e + U * (S.abs() + e), dt)
    return S, e


def conv_silu_bound(win, w, b, dt):
    """xc from the window win (B, E, K) fp64 as stored.  A non-finite pre-activation keeps its class: (+inf) sigma = +inf, (-inf) 0 = NaN."""
    Wd = w.double()
    K = Wd.shape[1]
    Bv = torch.zeros(Wd.shape[0], dtype=torch.float64) if b is None else b.double()
    P = Bv + (win * Wd).sum(-1)
    fin = torch.isfinite(P)
    Pf = torch.where(fin, P, torch.zeros_like(P))
    e_P = torch.where(fin, gam(K) * (Bv.abs() + (win.abs() * Wd.abs()).sum(-1)) + K * UF, torch.zeros_like(P))
    s, _, e_s, _ = sigmoid_bounds(Pf, e_P)
    o = Pf * s
    e_o = (Pf.abs() + e_P) * (s + e_s) * (1 + U) - o.abs() + UF
    return torch.where(fin, o, P * torch.sigmoid(P)), torch.where(fin, rT(o, e_o, dt), torch.zeros_like(P))


def ssm_bound(xc, z, s0, p, dt):
    """Launch 2 from xc, z (B, E) and the old state s0 (B, E, N): {"ssm": (ref, tol), "y": (ref, tol), "hi": |share of states n >= 16 in y|}."""
    X, Z, S0 = xc.double(), z.double(), s0.double()
    Wx, Wd = p["W_x"].double(), p["W_dt"].double()
    E, R = Wd.shape
    N = p["A_log"].shape[1]
    dbc = X @ Wx.t()
    e = gam(E + 8) * (X.abs() @ Wx.abs().t()) + E * UF
    e_dbc = rT(dbc, e, dt)
    up_dbc = dbc.abs() + e_dbc
    delta = dbc[:, :R] @ Wd.t()
    e0 = e_dbc[:, :R] @ Wd.abs().t() + gam(R) * (up_dbc[:, :R] @ Wd.abs().t()) + R * UF
    e_delta = rT(delta, e0, dt)
    x = delta + p["dt_bias"].double()
    e_x = e_delta + U * (x.abs() + e_delta)
    sp = x.clamp_min(0) + torch.log1p(torch.exp(-x.abs()))
    rho_e = torch.expm1(gam(2) * (x.abs() + e_x) + 2 * U * EXP2_ULPS)
    rho_r = gam(6) + 2 * U * (LOG_ULPS + RCP_ULPS)
    e_dt = e_x + torch.sigmoid(x + e_x) * rho_e * (1 + rho_e) + (sp + e_x) * rho_r + 4 * UF + \
        torch.where(x + e_x > 20, torch.log1p(torch.exp(-(x - e_x))), torch.zeros_like(x))
    Al = p["A_log"].double()
    Aabs = torch.exp(Al)
    rho_A = torch.expm1(gam(2) * Al.abs() + 2 * U * EXP2_ULPS)
    a = sp[:, :, None] * Aabs
    P = torch.exp(-a)
    d = Aabs * e_dt[:, :, None] + a * (rho_A + gam(3)) + (sp + e_dt)[:, :, None] * UF
    e_P = P * torch.expm1((d + 2 * U * EXP2_ULPS).clamp_max(50.0)) + UF
    Bm, Cm, eB, eC = dbc[:, None, R:R + N], dbc[:, None, R + N:], e_dbc[:, None, R:R + N], e_dbc[:, None, R + N:]
    inp = sp[:, :, None] * Bm * X[:, :, None]
    up1 = (P + e_P) * S0.abs()
    up2 = (sp + e_dt)[:, :, None] * (Bm.abs() + eB) * X.abs()[:, :, None]
    h = P * S0 + inp
    e_h = (up1 - P * S0.abs()) + (up2 - inp.abs()) + gam(4) * (up1 + up2) + 2 * UF
    up_h = h.abs() + e_h
    up_part = ((Cm.abs() + eC) * up_h).sum(-1)
    e_part = (Cm.abs() * e_h + eC * up_h).sum(-1) + gam(N + 8) * up_part + N * UF
    Dx = p["Dskip"].double() * X
    y1 = (Cm * h).sum(-1) + Dx
    e_y1 = e_part + gam(2) * (up_part + Dx.abs()) + UF
    s, _, e_s, _ = sigmoid_bounds(Z, torch.zeros_like(Z))
    gate = Z * s
    e_g = Z.abs() * e_s + U * Z.abs() * (s + e_s) + UF
    y = y1 * gate
    e_y = (y1.abs() + e_y1) * (gate.abs() + e_g) * (1 + U) - y.abs() + UF
    hi = ((Cm * h)[..., 16:].sum(-1) * gate).abs()
    return {"ssm": (h, e_h + FLOOR[F32]), "y": (y, rT(y, e_y, dt)), "hi": hi}


def check_behind_xz(bk, tag, dt, p, xz, e_xz, conv0, ssm0, O, bad_rows=()):
    """Everything behind the in-projection, from the device's own intermediates O (out, conv, ssm, xc, z, y; CPU).  conv0 / ssm0: the
    states before the call (all cache rows).  bad_rows: rows whose xz is non-finite (held up to xc only).  Returns ssm_bound's result."""
    B, E = O["z"].shape
    K = conv0.shape[2]
    hold(bk, f"{tag}.z", O["z"], xz[:, E:], e_xz[:, E:], dt)
    assert torch.equal(O["conv"][:B, :, :K - 1], conv0[:B, :, 1:]), "the window's old columns are not the old ones shifted by one"
    assert torch.equal(O["conv"][B:], conv0[B:]) and torch.equal(O["ssm"][B:], ssm0[B:]), "cache rows >= B were written"
    hold(bk, f"{tag}.conv_state", O["conv"][:B, :, K - 1], xz[:, :E], e_xz[:, :E], dt)
    hold(bk, f"{tag}.xc", O["xc"], *conv_silu_bound(O["conv"][:B].double(), p["conv_w"].reshape(E, K), p["conv_b"], dt), dt)
    g = torch.tensor([r for r in range(B) if r not in bad_rows])
    r2 = ssm_bound(O["xc"][g], O["z"][g], ssm0[:B][g], p, dt)
    hold(bk, f"{tag}.ssm_state", O["ssm"][:B][g], *r2["ssm"], F32)
    hold(bk, f"{tag}.y", O["y"][g], *r2["y"], dt)
    hold(bk, f"{tag}.out", O["out"][g], *proj_bound(O["y"][g].double(), None, p["W_out"], p["b_out"], dt), dt)
    return r2


# =========================================================================================================================================
# 1. cad_mamba_step
# =========================================================================================================================================
def draw(B, D, E, N, R, K, dtype, seed, b_in=True, conv_b=True, b_out=True):
    """Operands of one step, every size independent.  The cache has one row more than the batch.  A = -(0.05 .. 1) (slow decay) and
    the old state of lanes n >= 16 is four times larger, so that those lanes carry a visible share of y."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    p = dict(W_in=rn(2 * E, D) / math.sqrt(D), b_in=0.3 * rn(2 * E) if b_in else None, conv_w=0.5 * rn(E, K),
             conv_b=0.2 * rn(E) if conv_b else None, W_x=2 * rn(R + 2 * N, E) / math.sqrt(E), W_dt=rn(E, R) / math.sqrt(R),
             dt_bias=-1 + 0.5 * rn(E), A_log=torch.log(0.05 + 0.95 * torch.rand(E, N, generator=g)), Dskip=1 + 0.2 * rn(E),
             W_out=rn(D, E) / math.sqrt(E), b_out=0.3 * rn(D) if b_out else None)
    ssm = rn(B + 1, E, N)
    ssm[:, :, 16:] *= 4
    return dict(p=p, h=rn(B, D).to(dtype), conv=rn(B + 1, E, K).to(dtype), ssm=ssm, dtype=dtype)


def run(dev, c, rows=None):
    """ops.mamba_step on copies of the case's operands (rows: a list of batch rows run as a batch of their own); everything it wrote, on
    the CPU.  The scratch is the test's, with sentinels behind the 3 B E floats the call may use."""
    d = lambda t: None if t is None else t.clone().to(dev)
    h, conv, ssm = c["h"], c["conv"], c["ssm"]
    if rows is not None:
        h, conv, ssm = h[rows], torch.cat([conv[rows], conv[-1:]]), torch.cat([ssm[rows], ssm[-1:]])
    B, E = h.shape[0], c["p"]["W_dt"].shape[0]
    conv, ssm = d(conv), d(ssm)
    scratch = torch.full((3 * B * E + 8,), -512.0, dtype=F32, device=dev)
    out = ops.mamba_step(d(h), conv, ssm, *[d(c["p"][k]) for k in PARAMS], scratch)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    s = scratch.cpu()
    assert bool((s[3 * B * E:] == -512.0).all()), "the scratch was written beyond 3 B E floats"
    xc, z, y = (s[i * B * E:(i + 1) * B * E].view(B, E) for i in range(3))
    return dict(out=out.cpu(), conv=conv.cpu(), ssm=ssm.cpu(), xc=xc, z=z, y=y)


def check_step(bk, c, O, tag="step", bad_rows=()):
    dt = c["dtype"]
    xz, e_xz = proj_bound(c["h"].double(), None, c["p"]["W_in"], c["p"]["b_in"], dt)
    return check_behind_xz(bk, tag, dt, c["p"], xz, e_xz, c["conv"], c["ssm"], O, bad_rows)


def step_case(backend, *a, tag="step", **kw):
    name, dev = backend
    c = draw(*a, **kw)
    O = run(dev, c)
    return c, O, check_step(name, c, O, tag)


def same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("B", [1, 8, 9, 16, 17])
@pytest.mark.parametrize("dtype", TYPES)
def test_batch_groups(backend, B, dtype):
    """ST_BT = 8 rows per workgroup of launches 1 and 3: one row, a full group, a group of one row behind one and behind two full ones."""
    step_case(backend, B, 64, 128, 16, 4, 4, dtype, 100 + B)


@pytest.mark.parametrize("E", [17, 70, 72])
@pytest.mark.parametrize("dtype", TYPES)
def test_ragged_channel_groups(backend, E, dtype):
    """E no multiple of ST_WAVES = 4 (launch 1: idle waves in the last workgroup) or of ST_CH = 16 (launch 2: dead 16-lane groups)."""
    step_case(backend, 3, 40, E, 16, 3, 4, dtype, 200 + E)


@pytest.mark.parametrize("N", [1, 15, 17, 32, 33, 64])
@pytest.mark.parametrize("dtype", TYPES)
def test_state_lanes(backend, N, dtype):
    """Lane q of a channel's 16 owns states q, q + 16, ..: one to four trips, ragged and full.  Every state is held; with N > 16 the
    share of the states n >= 16 in y must exceed y's tolerance in most elements (asserted in fp64: their loss would be seen in y too)."""
    c, O, r2 = step_case(backend, 3, 40, 80, N, 3, 4, dtype, 300 + N)
    if N > 16:
        seen = float((r2["hi"] > r2["y"][1]).double().mean())
        print(f"states n >= 16 exceed y's tolerance in {seen:.2f} of the elements")
        assert seen >= 0.5, seen


@pytest.mark.parametrize("biases", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", TYPES)
def test_conv_widths(backend, K, biases, dtype):
    step_case(backend, 3, 40, 72, 16, 3, K, dtype, 400 + K, b_in=biases, conv_b=biases, b_out=biases)


@pytest.mark.parametrize("D,R", [(37, 1), (63, 3), (65, 65), (130, 3), (257, 1)])
@pytest.mark.parametrize("dtype", TYPES)
def test_dot_trips(backend, D, R, dtype):
    """The 64-lane strided dot over D: under one trip, one short of it, one past it, three and five trips; M = R + 2 N rows of W_x over
    the 4 waves of launch 2 with M % 4 != 0 (R 1, 3, 65 at N 5: M = 11, 13, 75)."""
    assert (R + 10) % 4 != 0
    step_case(backend, 3, D, 70, 5, R, 4, dtype, 500 + D, b_in=D % 2 == 0)


@pytest.mark.parametrize("B,D,E", [(8, 2048, 2048), (9, 1024, 2048)], ids=["B8-D2048-E2048", "B9-D1024-E2048"])
@pytest.mark.parametrize("dtype", TYPES2)
def test_width_limit(backend, B, D, E, dtype):
    """ST_WIDTH_MAX: 8 rows of 2048 fp32 values are exactly the 65536 bytes of LDS a plain launch may ask for (launches 1 and 3)."""
    assert min(B, 8) * max(D, E) * 4 == 65536
    step_case(backend, B, D, E, 16, 8, 4, dtype, 600 + B, tag="step-wide")


def _refusal(dev, B, D, E, N, R, K):
    z = lambda *s: torch.ones(*s, device=dev)
    t = dict(h=z(B, D), out=z(B, D), conv_state=z(B, E, K), ssm_state=z(B, E, N), W_in=z(2 * E, D), conv_w=z(E, max(K, 1)),
             W_x=z(R + 2 * N, E), W_dt=z(E, R), dt_bias=z(E), A_log=z(E, N), Dskip=z(E), W_out=z(D, E), scratch=z(3 * B * E))
    if K == 0:  # (an empty tensor has no address: the window pointer must still be given)
        t["conv_state"] = z(B, E, 1)
    a = L.MambaStepArgs(B=B, D=D, E=E, N=N, R=R, K=K, dtype=L.CAD_F32, **{k: L.ptr(v) for k, v in t.items()})
    rc = L.get_lib().cad_mamba_step(C.byref(a), L.stream_and_check(*t.values()))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((t["conv_state"] == 1).all()) and bool((t["ssm_state"] == 1).all()) and bool((t["out"] == 1).all())
    return rc


@pytest.mark.parametrize("what,shape", [("D", (2, 2049, 8, 4, 2, 4)), ("E", (2, 8, 2049, 4, 2, 4)), ("N", (2, 8, 8, 65, 2, 4)),
                                        ("R", (2, 8, 8, 4, 2049, 4)), ("K5", (2, 8, 8, 4, 2, 5)), ("K0", (2, 8, 8, 4, 2, 0)),
                                        ("B", (65536, 4, 4, 1, 1, 1))], ids=["D2049", "E2049", "N65", "R2049", "K5", "K0", "B65536"])
def test_refusals(backend, what, shape):
    """One past every limit: the error code, before any launch -- both states and out keep their values.  The neighbouring served shape
    is accepted by the support function."""
    _, dev = backend
    B, D, E, N, R, K = shape
    lib = L.get_lib()
    if what == "B":
        assert lib.cad_mamba_step_supported(D, E, N, R, K, L.CAD_F32) == 1
        assert _refusal(dev, *shape) == 1  # CAD_ERR_BAD_ARG
    else:
        assert lib.cad_mamba_step_supported(D, E, N, R, K, L.CAD_F32) == 0
        assert lib.cad_mamba_step_supported(min(D, 2048), min(E, 2048), min(N, 64), min(R, 2048), min(max(K, 1), 4), L.CAD_F32) == 1
        assert _refusal(dev, *shape) == 2  # CAD_ERR_UNSUPPORTED


@pytest.mark.parametrize("dtype", TYPES)
def test_rows_alone_and_twice(backend, dtype):
    """B = 17 (three workgroups of launches 1 / 3, the last with one row): row r equals row r run alone -- out, both states and the three
    scratch rows, bit for bit -- and the same call twice gives equal bits."""
    name, dev = backend
    c = draw(17, 64, 128, 33, 4, 3, dtype, 700)
    O = run(dev, c)
    check_step(name, c, O)
    same_bits(O, run(dev, c), "the same call twice")
    for r in (0, 7, 8, 15, 16):
        one = run(dev, c, rows=[r])
        for k in ("out", "xc", "z", "y"):
            assert torch.equal(one[k][0], O[k][r]), (k, r)
        assert torch.equal(one["conv"][0], O["conv"][r]) and torch.equal(one["ssm"][0], O["ssm"][r]), r


@pytest.mark.parametrize("dtype", TYPES)
def test_edge_values(backend, dtype):
    """Per element: dt_bias either side of softplus' threshold 20 (24; 19.5 and 20 - 2^-10 with delta on both sides; -12; -100:
    exp underflows), exp(dt A) within 1e-6 of 1 and below 1e-30, an all-zero token, gates z = +-100 (silu(z) = z / -0)."""
    name, dev = backend
    B, D, E, N = 4, 64, 128, 16
    c = draw(B, D, E, N, 4, 4, dtype, 800)
    p = c["p"]
    p["dt_bias"][0::8], p["dt_bias"][1::8], p["dt_bias"][2::8] = 24.0, -12.0, 19.5
    p["dt_bias"][3::8], p["dt_bias"][4::8] = 20.0 - 2.0 ** -10, -100.0
    p["A_log"][:, 0], p["A_log"][:, 1] = -20.0, 5.0
    p["W_in"][E + 5:2 * E:16], p["b_in"][E + 5:2 * E:16] = 0.0, 100.0
    p["W_in"][E + 6:2 * E:16], p["b_in"][E + 6:2 * E:16] = 0.0, -100.0
    c["h"][2] = 0
    O = run(dev, c)
    r2 = check_step(name, c, O, tag="step-edge")
    zd = O["z"].double()
    assert bool((zd[:, 5::16] == 100).all()) and bool((zd[:, 6::16] == -100).all())
    yd = O["y"][:, 6::16]
    assert bool((yd == 0).all()), "silu(-100) is -0 in fp32"
    dtv = torch.nn.functional.softplus(p["dt_bias"].double())  # (delta ~ 0.3: the regimes are the named ones)
    decay = torch.exp(-dtv[:, None] * torch.exp(p["A_log"].double()))
    assert float((1 - decay[:, 0]).abs().max()) < 1e-6 and float(decay[0::8, 1].max()) < 1e-30
    assert bool(torch.isfinite(O["ssm"]).all()) and bool(torch.isfinite(O["out"].float()).all())
    return r2


def test_fp16_overflowing_row(backend):
    """fp16, row 1 of h scaled by 2^15: part of its xz passes 65520.  z and the new window column are +-inf exactly where the fp64 value
    says (hold's rule), xc keeps the class (+inf -> +inf, -inf -> NaN); the row's y, state and out are NaN as in fp64 (every dbc value
    sums a NaN).  Every other row has the bits of the run without the scaling."""
    name, dev = backend
    c = draw(3, 64, 128, 16, 4, 4, HF, 900)
    base = run(dev, c)
    c2 = dict(c, h=c["h"].clone())
    c2["h"][1] = (c["h"][1].float() * 2.0 ** 15).clamp(-6e4, 6e4).to(HF)
    O = run(dev, c2)
    xz, _ = proj_bound(c2["h"].double(), None, c["p"]["W_in"], c["p"]["b_in"], HF)
    n_over = int((xz[1].abs() >= OVER[HF]).sum())
    assert 8 < n_over < xz[1].numel() - 8, n_over  # the case has both classes
    check_step(name, c2, O, tag="step-overflow", bad_rows=(1,))
    for r in (0, 2):
        for k in O:
            assert torch.equal(O[k][r], base[k][r]), (k, r)
    assert torch.equal(O["conv"][3], base["conv"][3]) and torch.equal(O["ssm"][3], base["ssm"][3])
    xc = O["xc"][1].double()
    assert bool(torch.isnan(xc).any())
    dbc = xc @ c["p"]["W_x"].double().t()
    assert bool(torch.isnan(dbc).all())  # the fp64 reference of everything behind it is NaN
    nan = lambda t: torch.full(t.shape, float("nan"), dtype=torch.float64)
    for k, dt in (("y", HF), ("ssm", F32), ("out", HF)):
        hold(name, f"step-overflow.{k}-row", O[k][1], nan(O[k][1]), torch.zeros(O[k][1].shape, dtype=torch.float64), dt)


# =========================================================================================================================================
# 2. cad_decode_token through DecodeStack
# =========================================================================================================================================
SAMPLING = dict(top_k=0, top_p=0.9, temperature=0.8, seed=1234, row_offset=3)
OFFSET = 7


def _mixer_params(m):
    c = lambda t: None if t is None else t.detach().cpu()
    return dict(W_in=c(m.in_proj.weight), b_in=c(m.in_proj.bias), conv_w=c(m.conv1d.weight).reshape(m.d_inner, -1), conv_b=c(m.conv1d.bias),
                W_x=c(m.x_proj.weight), W_dt=c(m.dt_proj.weight), dt_bias=c(m.dt_proj.bias), A_log=c(m.A_log), Dskip=c(m.D),
                W_out=c(m.out_proj.weight), b_out=c(m.out_proj.bias))


def _norm(mod):
    w, b, eps, is_rms = norm_params(mod)
    return w.detach().cpu(), None if b is None else b.detach().cpu(), float(eps), bool(is_rms)


def _step_stack(model, dtype, B, states, ids):
    """One DecodeStack.step on a cache filled with `states` [(conv, ssm)] per layer; returns everything the token wrote, on the CPU,
    in the layout cad_decode_scratch_floats documents: xc | z | y | res0 | res1 | out."""
    dev = ids.device
    stack = DecodeStack(model, B, dtype=dtype)
    ip = stack.inference_params
    for i, (c0, s0) in enumerate(states):
        conv, ssm = ip.key_value_memory_dict[i]
        assert conv.shape == c0.shape and ssm.shape == s0.shape and conv.dtype == dtype and ssm.dtype == F32
        conv.copy_(c0.to(dev)), ssm.copy_(s0.to(dev))
    stack.batch_size, stack._args.B, ip.seqlen_offset = B, B, OFFSET
    nxt, logits = stack.step(ids, **SAMPLING)
    want = ops.sample_tokens(logits.clone(), position=OFFSET + 1, **SAMPLING)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert ip.seqlen_offset == OFFSET + 1
    assert torch.equal(nxt.cpu(), want.cpu()), "the token is not the sampler's on the token's own logits"
    D, E = stack.D, model.caduceus.backbone.layers[0].mixer.mamba_fwd.d_inner
    s = stack._scratch.cpu()
    BE, BD = B * E, B * D
    assert s.numel() == 3 * BE + 3 * BD
    O = {k: s[i * BE:(i + 1) * BE].view(B, E) for i, k in enumerate(("xc", "z", "y"))}
    O["res"] = [s[3 * BE + i * BD:3 * BE + (i + 1) * BD].view(B, D) for i in range(2)]
    O["out"] = s[3 * BE + 2 * BD:].view(dtype)[:BD].view(B, D)
    O["logits"] = logits.cpu().clone()
    O["states"] = [tuple(t.cpu().clone() for t in ip.key_value_memory_dict[i]) for i in range(len(states))]
    return O


def _check_layer(bk, tag, dt, layer, x_in, res_in, O, li, state0):
    """Layer li of the token that left O: x_in (B, D) its hidden input as stored (emb rows in fp32, or the layer below's out in T)."""
    B, D = x_in.shape
    w, b, eps, is_rms = _norm(layer.norm)
    ref = an_reference(x_in.view(1, B, D), None if res_in is None else res_in.view(1, B, D), w, b, eps, is_rms, False, dt)
    res_out = O["res"][li & 1]
    if res_in is None:
        assert torch.equal(res_out, x_in), "layer 0's residual is not emb[id]"
    else:
        hold(bk, f"{tag}.residual", res_out, *ref["res_out"], F32)
    p = _mixer_params(layer.mixer.mamba_fwd)
    xz, e_xz = proj_bound(ref["y"][0][0], ref["y"][1][0], p["W_in"], p["b_in"], dt)
    conv1, ssm1 = O["states"][li]
    check_behind_xz(bk, tag, dt, p, xz, e_xz, state0[0], state0[1], dict(O, conv=conv1, ssm=ssm1))


def _check_tail(bk, tag, dt, model, O, n_layer):
    B, D = O["out"].shape
    w, b, eps, is_rms = _norm(model.caduceus.backbone.norm_f)
    hn, tol = an_reference(O["out"].view(1, B, D), O["res"][(n_layer - 1) & 1].view(1, B, D), w, b, eps, is_rms, False, dt)["y"]
    Wh = model.lm_head.weight.detach().double().cpu()
    e = tol[0] @ Wh.abs().t() + gam(D + 8) * ((hn[0].abs() + tol[0]) @ Wh.abs().t()) + D * UF
    hold(bk, f"{tag}.logits", O["logits"], hn[0] @ Wh.t(), e, F32)


# d_model (38: W = 1, one trip of the row walk; 70: W = 1, two trips; 260: W = 4, two trips; 1024), RMSNorm / LayerNorm with bias,
# vocab_size (24, 64: the tail's VMAX = 64 instantiation), B, d_state, d_conv, n_layer: every edge at least once per dtype
STACKS = [(38, True, 16, 1, 16, 4, 1), (38, False, 24, 5, 33, 3, 2), (70, True, 64, 4, 16, 1, 2), (70, False, 16, 9, 33, 4, 1),
          (260, True, 24, 8, 33, 3, 1), (260, False, 64, 9, 16, 4, 2), (1024, True, 16, 5, 16, 4, 1), (1024, False, 24, 1, 33, 3, 1)]


@pytest.mark.parametrize("d_model,rms,V,B,N,K,n_layer", STACKS,
                         ids=[f"D{c[0]}-{'rms' if c[1] else 'ln'}-V{c[2]}-B{c[3]}-N{c[4]}-K{c[5]}-L{c[6]}" for c in STACKS])
@pytest.mark.parametrize("dtype", TYPES)
def test_decode_token(backend, dtype, d_model, rms, V, B, N, K, n_layer):
    name, dev = backend
    over = {} if V == 16 else {"vocab_size": V}
    _, model = _model(dev, d_model, N, K, rms, seed=d_model + V, head_std=0.5, n_layer=n_layer, **over)
    layers = model.caduceus.backbone.layers
    assert len(layers) == n_layer and model.lm_head.weight.shape == (V, d_model)
    E = layers[0].mixer.mamba_fwd.d_inner
    g = torch.Generator().manual_seed(B + N)
    states = [(torch.randn(B, E, K, generator=g).to(dtype), torch.randn(B, E, N, generator=g)) for _ in range(n_layer)]
    ids = torch.randint(0, V, (B,), generator=g)
    emb = model.caduceus.backbone.embeddings.word_embeddings.weight.detach().cpu()[ids]
    with torch.no_grad():
        one = model
        if n_layer == 2:  # layer 0 on a one-layer stack over the same weights (see the header)
            one = copy.deepcopy(model)
            one.caduceus.backbone.layers = torch.nn.ModuleList(list(one.caduceus.backbone.layers)[:1])
        O1 = _step_stack(one, dtype, B, states[:1], ids.to(dev))
        _check_layer(name, "decode", dtype, layers[0], emb, None, O1, 0, states[0])
        _check_tail(name, "decode", dtype, one, O1, 1)
        if n_layer == 2:
            O2 = _step_stack(model, dtype, B, states, ids.to(dev))
            assert torch.equal(O2["res"][0], emb)
            assert torch.equal(O2["states"][0][0], O1["states"][0][0]) and torch.equal(O2["states"][0][1], O1["states"][0][1])
            _check_layer(name, "decode", dtype, layers[1], O1["out"], O1["res"][0], O2, 1, states[1])
            _check_tail(name, "decode", dtype, model, O2, 2)


def test_zz_report_worst_ratios(backend):
    """Prints the worst err / tol per output and type recorded by the tests above (run with -s to see it)."""
    name, dev = backend
    mine = {k: v for k, v in WORST.items() if k[0] == name and k[1].split(".")[0].startswith(("step", "decode"))}
    for (bk, key) in sorted(mine):
        print(f"[fp64 summary] {bk} {key}: {mine[(bk, key)]:.3f}")
    assert all(v <= 1.0 for v in mine.values())
