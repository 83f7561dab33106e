"""Fused add+norm (csrc/addnorm.hip) and the LM head (csrc/lmhead.hip) held to float64, element by element, at the row counts where their
grid-stride / multi-tile walks start, at every width class, on misaligned operands and at edge values.

References are written here in torch.float64 and start from the inputs AS STORED (after their rounding to bf16 / fp16).  Every output
element must satisfy |out - ref| <= tol with a tol DERIVED below from how the kernel rounds; nothing in it is fitted to a result.
Notation: u = 2^-24 (fp32 unit roundoff), g(n) = n u / (1 - n u) (n fp32 roundings in a row, any order, fused or not -- so the bounds do
not depend on how -ffp-contract fuses multiply-adds), uo = 0 / 2^-8 / 2^-11 for an fp32 / bf16 / fp16 OUTPUT (an fp32 output's last rounding
is already one of the counted fp32 operations), floor = half the spacing of the output format's subnormals, UF = 2^-126 per fp32 product or
exp that may underflow (covers gradual underflow and flush-to-zero).

Approximate instructions (the third part of every bound, carried explicitly as constants below):
  RSQ_ULPS = 1   cad_rsqrt is v_rsq_f32 on the device (the emulator computes 1 / sqrtf, both correctly rounded operations).  The
                 micro-architecture notes list the instruction's cost only, no accuracy, so 1 ulp (= 2 u relative) is assumed.
  EXP_ULPS = 2, LOG_ULPS = 2   expf / logf of the LM head: the device's and the host's libm document <= 1 ulp for both; 2 is "a few".

add+norm, per row, t = x + residual (|t^ - t| <= r = u |t| if a residual is added, else 0):
  mean  (LayerNorm)  |m^ - m| <= e_m = g(D + 4) mean|t|            (D adds and the roundings of t, 1/D and the product)
  d = t - m          |d^ - d| <= e_d = e_m + r + u (|d| + e_m)
  Q = sum d^2        sum (d + c + rho)^2 = Q + D c^2 + 2 sum (d + c) rho + sum rho^2  for a constant shift c = m - m^ (sum d = 0): the error
                     of the mean enters the TWO-PASS variance only in second order, dQ = D e_m^2 + sum (2 (|d| + e_m) rho + rho^2); a
                     one-pass variance  mean(t^2) - m^2  misses this bound by orders of magnitude once |m| >> spread (the mean-1e3 case).
  arg = Q / D + eps  e_arg = (dQ + g(D + 2) (Q + dQ)) / D (1 + g(3)) + g(3) arg   (eps is the fp32 value the kernel receives)
  rstd               relative d_r = ((1 - e_arg / arg)^-1/2 - 1 + 1)(1 + 2 u RSQ_ULPS) - 1
  y = d rstd w + b   e = (|d| + e_d) rstd (1 + d_r) |w| (1 + g(2)) - |d rstd w|  +  u (that + |b|);   tol = e + uo (|y| + e) + floor
  residual stream    tol = r
  backward           g = dy w (u |g|);  xh as above (e_xh);  sgx = mean(g xh), sg = mean(g): perturbed inputs + g(D + 4) mean|terms|;
                     dx = rstd (g - sg - xh sgx) + dres_out, each step "upper bound of the magnitudes - true magnitude" plus its own
                     roundings;  dweight / dbias: sum |dy| e_xh + g(n + 2) sum |dy| (|xh| + e_xh) + n UF with n = rows x strands terms, valid
                     for any association order (walk, LDS fold of the four waves, slot fold).
LM head:
  logits             tol = e_z = g(S D + 2) sum |h w| + S D UF   (S D products: the two strands' sums are added; fp32 output)
  row loss           lse(z) - z[label], from the kernel's own logits: lse is 1-Lipschitz in max|e_z| = E; exp terms carry
                     rho_e = 2 u EXP_ULPS + u (spread + 1) relative (spread = max |z - max z| + 2 E: rounding of the argument), their
                     sum g(V) more; logf 2 u LOG_ULPS |log se|; two more roundings u |lse| + u |row|.
  loss               (sum e_row + g(n + 3) sum (row + e_row)) / n + 2 u |loss|  over the n counted rows; n = 0 gives 0 / 0 = NaN, as
                     F.cross_entropy does.  Labels outside [0, V) other than ignore_index are SKIPPED by the kernel (F.cross_entropy would
                     raise): the expected value is the reference with those rows masked out like ignored ones.
  G = d loss / d z   (p - onehot) coef + dlogits, exactly 0 in rows that do not count (as F.cross_entropy: no 0 * inf);
                     p relative exp(2 E + 2 rho_e + g(V + 2)) - 1, plus UF;  g(4) for the subtraction, coef = dloss / n and the product.
  dhidden            e_G |W| + g(V + 2) (|G| + e_G) |W|, then uo / floor of the hidden type
  dW                 e_G^T |h| + g(rows S + 2) (|G| + e_G)^T |h| + rows S UF  (rows x strands terms, any order: tiles, waves, slots)
  The general kernel's backward (D = 40, or hidden not 16-byte aligned) is the torch path of ops._LmHead.backward: for 16-bit hidden it
  rounds G and W to that type and each strand's two products once more (uo terms added where `torch_path`).
Non-finite references: the kernel must be non-finite in the same class (NaN / +inf / -inf) at the same element; a finite value whose
distance to the output format's overflow threshold is below its tolerance may come out either way.

Misalignment: operands as views one element into a larger buffer take the scalar add+norm kernels (the launchers' `vec` flag) and the
general LM-head forward / torch backward.  The scalar add+norm kernel's result does not depend on the address: at D % 4 != 0 the
misaligned result equals the aligned one bit for bit (same kernel, same association order).  At D % 4 == 0 the aligned call takes the
VECTOR kernel, whose lanes own other channels (4 consecutive ones per 256), so its wave sums associate differently: that identity does
not hold there, and the misaligned result is held to the bounds only.
"""
import ctypes as C
import math

import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
U = 2.0 ** -24
UO = {F32: 0.0, BF: 2.0 ** -8, HF: 2.0 ** -11}
FLOOR = {F32: 2.0 ** -150, BF: 2.0 ** -134, HF: 2.0 ** -25}
# overflow threshold: values of at least this magnitude round to inf (max + half an ulp)
OVER = {F32: (2 - 2.0 ** -24) * 2.0 ** 127, BF: (2 - 2.0 ** -8) * 2.0 ** 127, HF: 65520.0}
UF = 2.0 ** -126
RSQ_ULPS, EXP_ULPS, LOG_ULPS = 1, 2, 2
TAG = {F32: "f32", BF: "bf16", HF: "f16"}
WORST = {}  # (backend, output[dtype]) -> worst err / tol, printed by the last test
# the type pairs cad_add_norm_fwd accepts (the AN_FWD dispatch of csrc/addnorm.hip)
AN_TYPES = [pytest.param(F32, F32, id="f32-f32"), pytest.param(F32, BF, id="f32-bf16"), pytest.param(BF, BF, id="bf16-bf16"),
            pytest.param(F32, HF, id="f32-f16"), pytest.param(HF, HF, id="f16-f16")]
LM_TYPES = [pytest.param(F32, id="f32"), pytest.param(BF, id="bf16"), pytest.param(HF, id="f16")]
COMP = torch.tensor([0, 1, 2, 3, 4, 5, 6, 10, 9, 8, 7, 11, 12, 13, 14, 15])  # an involution: 7 <-> 10, 8 <-> 9
COMP12 = torch.tensor([0, 1, 2, 11, 4, 5, 6, 8, 7, 9, 10, 3])               # 3 <-> 11, 7 <-> 8


def gam(n):
    return n * U / (1.0 - n * U)


def hold(backend, name, out, ref, tol, dtype):
    """Every element: |out - ref| <= tol, non-finite classes equal (see the header); records the worst err / tol."""
    o, ref, tol = out.detach().double().cpu().reshape(-1), ref.reshape(-1), tol.reshape(-1)
    assert o.shape == ref.shape == tol.shape, (name, o.shape, ref.shape, tol.shape)
    assert not bool(torch.isnan(tol).any()) and bool((tol >= 0).all()), name
    ref_nan = torch.isnan(ref)
    must_inf = ~ref_nan & (ref.abs() - tol >= OVER[dtype])
    may_inf = ~ref_nan & (ref.abs() + tol >= OVER[dtype])
    same_inf = torch.isinf(o) & (torch.sign(o) == torch.sign(ref))
    err = (o - ref).abs()
    near = torch.isfinite(o) & (err <= tol)
    ok = torch.where(ref_nan, torch.isnan(o), torch.where(must_inf, same_inf, near | (may_inf & same_inf)))
    fin = torch.isfinite(o) & torch.isfinite(ref)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    worst = float(ratio[fin].max()) if bool(fin.any()) else 0.0
    key = (backend, f"{name}[{TAG[dtype]}]")
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"[fp64] {backend} {name}[{TAG[dtype]}]: worst err / tol = {worst:.3f} over {o.numel()} elements")
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        raise AssertionError(f"{name}[{TAG[dtype]}]: {int((~ok).sum())} of {o.numel()} elements outside the bound; first at {i}: "
                             f"out {float(o[i])!r} ref {float(ref[i])!r} tol {float(tol[i])!r}; worst err / tol {worst:.3f}")


# =========================================================================================================================================
# add+norm
# =========================================================================================================================================
def an_reference(x, res, w, b, eps, is_rms, swap, ydt, dy=None, dro=None):
    """fp64 values and tolerances of every add+norm output.  x (S, R, D) as stored; res / dro fp32 or None; dy (S, R, D) as stored in the
    OUTPUT frame.  Returns {name: (ref, tol)} in the frames the kernel writes (y, res_out: output frame; dx, dres_in: input frame)."""
    S, R, D = x.shape
    xdt = x.dtype
    eps32 = float(torch.tensor(eps, dtype=F32))
    fr = (lambda t: t.flip(0).flip(-1)) if swap else (lambda t: t)  # input frame <-> output frame (an involution)
    t = x.double()
    r = torch.zeros_like(t)
    if res is not None:
        t = t + res.double()
        r = U * t.abs()
    r_t = r
    win = (w.double().flip(0) if swap else w.double())  # the weight that multiplies INPUT channel c
    bin_ = None if b is None else (b.double().flip(0) if swap else b.double())
    if is_rms:
        e_m, d = 0.0, t
    else:
        m = t.mean(-1, keepdim=True)
        e_m = gam(D + 4) * t.abs().mean(-1, keepdim=True)
        d = t - m
        r = r + U * (d.abs() + e_m)
    e_d = e_m + r
    Q = (d * d).sum(-1, keepdim=True)
    dQ = D * e_m ** 2 + (2 * (d.abs() + e_m) * r + r * r).sum(-1, keepdim=True)
    arg = Q / D + eps32
    e_arg = (dQ + gam(D + 2) * (Q + dQ)) / D * (1 + gam(3)) + gam(3) * arg
    rel = e_arg / arg
    assert float(rel.max()) < 0.5, "the statistics bound is void"
    rstd = arg ** -0.5
    d_r = (1 - rel) ** -0.5 * (1 + 2 * U * RSQ_ULPS) - 1
    xh = d * rstd
    xh_up = (d.abs() + e_d) * rstd * (1 + d_r)
    core = xh * win
    core_up = xh_up * win.abs() * (1 + gam(2))
    y = core if bin_ is None else core + bin_
    e = core_up - core.abs()
    if bin_ is not None:
        e = e + U * (core_up + bin_.abs())
    out = {"y": (fr(y), fr(e + UO[ydt] * (y.abs() + e) + FLOOR[ydt])), "res_out": (fr(t), fr(r_t))}
    if dy is None:
        return out
    del core, core_up, y, e
    dyin = fr(dy.double())
    gr = dyin * win
    g_up = gr.abs() * (1 + U)
    e_xh = xh_up * (1 + gam(2)) - xh.abs()
    x_up = xh.abs() + e_xh
    sgx = (gr * xh).mean(-1, keepdim=True)
    a_up = (g_up * x_up).sum(-1, keepdim=True) / D
    e_sgx = (a_up - (gr.abs() * xh.abs()).sum(-1, keepdim=True) / D) + gam(D + 4) * a_up
    if is_rms:
        sg, e_sg = 0.0 * sgx, 0.0 * sgx
    else:
        sg = gr.mean(-1, keepdim=True)
        b_up = g_up.sum(-1, keepdim=True) / D
        e_sg = (b_up - gr.abs().sum(-1, keepdim=True) / D) + gam(D + 4) * b_up
    prod_up = x_up * (sgx.abs() + e_sgx)
    inner = gr - sg - xh * sgx
    e_in = U * gr.abs() + e_sg + (prod_up - xh.abs() * sgx.abs()) + gam(3) * (g_up + sg.abs() + e_sg + prod_up)
    p_up = rstd * (1 + d_r) * (inner.abs() + e_in)
    dx = rstd * inner
    e_dx = p_up - dx.abs()
    if dro is not None:
        droin = fr(dro.double())
        dx = dx + droin
        e_dx = e_dx + gam(2) * (p_up + droin.abs())
    else:
        e_dx = e_dx + gam(2) * p_up
    out["dx"] = (dx, e_dx + UO[xdt] * (dx.abs() + e_dx) + FLOOR[xdt])
    out["dres_in"] = (dx, e_dx + FLOOR[F32])
    n = S * R
    flipc = (lambda v: v.flip(0)) if swap else (lambda v: v)
    out["dweight"] = (flipc((dyin * xh).sum((0, 1))),
                      flipc((dyin.abs() * e_xh).sum((0, 1)) + gam(n + 2) * (dyin.abs() * x_up).sum((0, 1)) + n * UF))
    out["dbias"] = (flipc(dyin.sum((0, 1))), flipc(gam(n + 1) * dyin.abs().sum((0, 1)) + FLOOR[F32]))
    return out


def an_inputs(S, R, D, xdt, ydt, has_res, has_bias, seed, backward=True):
    """Gaussian rows.  dy correlates with the normed row and has a mean, so that the dweight / dbias sums are coherent (|sum| is a sizeable
    part of sum |terms|, which the bound scales with), and one row in 256 is 2^12 times larger than the others, so that single rows
    matter to the sums."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, R, D, generator=g).to(xdt)
    res = torch.randn(S, R, D, generator=g) if has_res else None
    w = 1 + 0.2 * torch.randn(D, generator=g)
    b = 0.1 * torch.randn(D, generator=g) if has_bias else None
    if not backward:
        return x, res, w, b, None, None
    scale = torch.where(torch.rand(S, R, 1, generator=g) < 1 / 256, 1.0, 2.0 ** -12)
    base = x.float() + (res if res is not None else 0)
    dy = (scale * (0.5 * base + 0.25 + torch.randn(S, R, D, generator=g))).to(ydt)
    dro = torch.randn(S, R, D, generator=g) * scale
    return x, res, w, b, dy, dro


def an_check(backend, x, res, w, b, eps, is_rms, swap, ydt, dy, dro, tag="addnorm"):
    """Through ops.add_norm and autograd (the production path), every output against an_reference."""
    name, dev = backend
    S, R, D = x.shape

    def leaf(t):
        return None if t is None else t.detach().clone().to(dev).requires_grad_(True)
    xd, rd, wd, bd = leaf(x), leaf(res), leaf(w), leaf(b)
    y, s = ops.add_norm(xd.reshape(S, 1, R, D), None if rd is None else rd.reshape(S, 1, R, D), wd, bd, eps, is_rms, swap, ydt)
    ref = an_reference(x, res, w, b, eps, is_rms, swap, ydt, dy, dro)
    hold(name, f"{tag}.y", y, *ref["y"], ydt)
    hold(name, f"{tag}.res_out", s, *ref["res_out"], F32)
    if dy is None:
        return
    torch.autograd.backward([y, s], [dy.to(dev).reshape(y.shape), dro.to(dev).reshape(s.shape)])
    hold(name, f"{tag}.dx", xd.grad, *ref["dx"], x.dtype)
    if rd is not None:
        hold(name, f"{tag}.dres_in", rd.grad, *ref["dres_in"], F32)
    hold(name, f"{tag}.dweight", wd.grad, *ref["dweight"], F32)
    if bd is not None:
        hold(name, f"{tag}.dbias", bd.grad, *ref["dbias"], F32)


def _an_bwd_rows_per_wave(S, R, D):
    """From the exported workgroup count: workgroups = ceil(rows / (4 rows_per_wave))."""
    a = L.AddNormBwdArgs(None, None, None, None, None, None, None, None, None, None, R, S, D, 1, 0, 0, 0)
    nb = L.get_lib().cad_add_norm_bwd_slots(C.byref(a))
    rpw = [k for k in range(8, 65) if (S * R + 4 * k - 1) // (4 * k) == nb]
    return rpw, nb


# ---- small-row width sweep: every width class and every edge of one -------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 4, 63, 64, 65, 252, 255, 256, 260, 512, 516, 1020, 1023, 1024])
@pytest.mark.parametrize("xdt,ydt", AN_TYPES)
def test_add_norm_width_sweep(backend, D, xdt, ydt):
    """R = 9 rows per strand: 18 rows in one workgroup, the backward's waves walk 8, 8 and 2 rows.  D % 4 != 0: scalar kernels; else the
    KMAX = 1 / 2 / 4 vector kernels (<= 256, <= 512, <= 1024) with full and ragged last 256-channel steps."""
    for k, (is_rms, has_res, has_bias, swap) in enumerate([(True, True, False, True), (False, False, True, False),
                                                           (False, True, True, True), (True, False, True, False)]):
        x, res, w, b, dy, dro = an_inputs(2, 9, D, xdt, ydt, has_res, has_bias, 100 * D + k)
        an_check(backend, x, res, w, b, 1e-5, is_rms, swap, ydt, dy, dro)


# ---- forward walk: more than 8192 workgroups x 4 rows ---------------------------------------------------------------------------------
FWD_WALK = [  # D, is_rms, residual, bias, swap, (x type, y type)
    (30, True, True, False, True, (F32, F32)), (30, False, False, True, False, (BF, BF)),
    (30, False, True, True, True, (F32, HF)), (30, True, False, True, False, (HF, HF)),
    (64, True, True, False, True, (BF, BF)), (64, False, False, True, False, (F32, BF)),
    (64, False, True, True, True, (HF, HF)), (64, True, False, True, False, (F32, F32)),
    (260, False, True, True, True, (BF, BF)), (260, True, False, False, False, (F32, HF)),
    (260, True, True, True, True, (F32, F32)), (260, False, False, False, False, (HF, HF)),
    (1020, False, True, True, True, (BF, BF)), (1020, True, False, False, False, (F32, F32)),
    (1020, True, True, True, True, (F32, BF)), (1020, False, False, False, False, (F32, HF)),
]


@pytest.mark.parametrize("D,is_rms,has_res,has_bias,swap,types", FWD_WALK,
                         ids=[f"D{c[0]}-{'rms' if c[1] else 'ln'}-res{int(c[2])}-b{int(c[3])}-swap{int(c[4])}-{TAG[c[5][0]]}-{TAG[c[5][1]]}"
                              for c in FWD_WALK])
def test_add_norm_forward_walk(backend, D, is_rms, has_res, has_bias, swap, types):
    """2 x 16387 = 32774 rows: the forward's 8192 workgroups of 4 waves cover 32768 rows per trip, so six waves take a second row and the
    last workgroup-iteration is ragged (32774 % 4 = 2).  The backward runs at D <= 64 (8 rows per wave, ragged last workgroup)."""
    xdt, ydt = types
    S, R = 2, 16387
    assert S * R > 8192 * 4 and (S * R) % 4 != 0
    x, res, w, b, dy, dro = an_inputs(S, R, D, xdt, ydt, has_res, has_bias, 7 * D + int(is_rms), backward=D <= 64)
    an_check(backend, x, res, w, b, 1e-5, is_rms, swap, ydt, dy, dro, tag="addnorm-walk")


# ---- backward walk: 8, an intermediate number and 64 rows per wave ------------------------------------------------------------------------
BWD_WALK = [  # S, R, D, is_rms, bias, swap, types, rows per wave
    (2, 16387, 260, False, True, True, (BF, BF), 8), (1, 32771, 516, True, False, False, (F32, F32), 8),
    (2, 40001, 64, False, True, True, (BF, BF), 19), (1, 80003, 30, True, True, False, (F32, HF), 19),
    (1, 50003, 260, True, False, False, (F32, F32), 12),
    (1, 262144 + 37, 4, False, True, False, (F32, BF), 64), (2, 131072 + 19, 3, False, True, True, (HF, HF), 64),
]


@pytest.mark.parametrize("S,R,D,is_rms,has_bias,swap,types,rpw", BWD_WALK,
                         ids=[f"S{c[0]}-R{c[1]}-D{c[2]}-{'rms' if c[3] else 'ln'}-rpw{c[7]}" for c in BWD_WALK])
def test_add_norm_backward_walk(backend, S, R, D, is_rms, has_bias, swap, types, rpw):
    """Row counts at which a backward wave walks 8 (the minimum), 12 / 19 and 64 (the maximum) rows, the last workgroup ragged: LayerNorm
    with bias among them, the KMAX = 2 / 4 vector kernels at 8 and 12 rows, a small D where 64 rows per wave need >= 262144 rows."""
    xdt, ydt = types
    got, nb = _an_bwd_rows_per_wave(S, R, D)
    assert got == [rpw], (got, nb)
    assert (S * R) % (4 * rpw) != 0
    x, res, w, b, dy, dro = an_inputs(S, R, D, xdt, ydt, True, has_bias, 13 * D + rpw)
    an_check(backend, x, res, w, b, 1e-5, is_rms, swap, ydt, dy, dro, tag="addnorm-walk")


# ---- edge values ----------------------------------------------------------------------------------------------------------------------------
def _edge_case(kind, S, R, D, xdt, ydt, g):
    """(x, res, w, b, dy, dro, eps).  16-bit x cannot hold a large mean with a small spread: the fp32 residual carries it."""
    x = torch.randn(S, R, D, generator=g)
    res = torch.randn(S, R, D, generator=g)
    w = 1 + 0.2 * torch.randn(D, generator=g)
    b = 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(S, R, D, generator=g)
    dro = torch.randn(S, R, D, generator=g)
    if kind == "zeros":
        x, res = 0 * x, 0 * res
        x[0, 0], res[0, 0] = torch.randn(D, generator=g), torch.randn(D, generator=g)  # one ordinary row among them
    elif kind == "tiny":
        x, res = 1e-4 * x, 1e-4 * res
    elif kind == "large":
        x, res = (1e4 * x).clamp(-6e4, 6e4), 1e4 * res
    elif kind == "constant":
        x = torch.randn(S, R, 1, generator=g).expand(S, R, D).contiguous()
        res = torch.randn(S, R, 1, generator=g).expand(S, R, D).contiguous()
    elif kind == "mean1e3":
        x, res = 0.1 * x, 1e3 + 0.1 * res
    elif kind == "outlier":
        x, res = torch.ones(S, R, D), torch.zeros(S, R, D)
        x[..., D // 3] = 1e4
    elif kind == "weight-zeros-negative":
        w = torch.randn(D, generator=g)
        w[::3] = 0.0
    elif kind == "dy-zero-rows":
        dy[:, ::2] = 0.0
        dro[:, 1::4] = 0.0
    elif kind == "overflow":
        w = 3e4 * (1 + 0.2 * torch.randn(D, generator=g))  # |xhat| reaches ~3: |y| passes 65520 in part of the elements
    else:
        raise KeyError(kind)
    return x.to(xdt), res, w, b, dy.to(ydt), dro


EDGES = ["zeros", "tiny", "large", "constant", "mean1e3", "outlier", "weight-zeros-negative", "dy-zero-rows"]


@pytest.mark.parametrize("kind", EDGES)
@pytest.mark.parametrize("D", [64, 30])
@pytest.mark.parametrize("xdt,ydt", AN_TYPES)
def test_add_norm_edge_values(backend, kind, D, xdt, ydt):
    """One vector D and one scalar D; RMSNorm and LayerNorm, with the residual (both norms) and without (alternating)."""
    g = torch.Generator().manual_seed(EDGES.index(kind) * 1000 + D)
    for k, is_rms in enumerate([True, False]):
        x, res, w, b, dy, dro, = _edge_case(kind, 2, 6, D, xdt, ydt, g)
        an_check(backend, x, res, w, b if not is_rms else None, 1e-5, is_rms, bool(k), ydt, dy, dro, tag="addnorm-edge")
        if kind in ("zeros", "constant", "outlier", "tiny"):
            an_check(backend, x, None, w, b, 1e-5, is_rms, not bool(k), ydt, dy, dro, tag="addnorm-edge")


@pytest.mark.parametrize("D", [64, 30])
@pytest.mark.parametrize("xdt", [F32, HF])
@pytest.mark.parametrize("is_rms", [True, False])
def test_add_norm_fp16_overflow(backend, D, xdt, is_rms):
    """fp16 outputs beyond the format's range: +-inf exactly where the fp64 value rounds to it (>= 65520 in magnitude), finite and within
    the bound elsewhere; the backward is unaffected."""
    g = torch.Generator().manual_seed(4242 + D)
    x, res, w, b, dy, dro = _edge_case("overflow", 2, 6, D, xdt, HF, g)
    ref_y = an_reference(x, res, w, b, 1e-5, is_rms, False, HF)["y"][0]
    n_over = int((ref_y.abs() >= OVER[HF]).sum())
    assert 0 < n_over < ref_y.numel() // 2, n_over  # the case has both classes
    an_check(backend, x, res, w, b, 1e-5, is_rms, False, HF, dy, dro, tag="addnorm-edge")


# ---- misaligned operands, sentinels around the outputs ----------------------------------------------------------------------------------
SENT = -512.0  # exact in every type


class Arena:
    """Tensors as views `off` elements into sentinel-filled buffers (8 elements of sentinel on both sides)."""

    def __init__(self, dev, off):
        self.dev, self.off, self.bufs = dev, off, []

    def put(self, t=None, shape=None, dtype=None):
        if t is None and shape is None:
            return None
        shape, dtype = (t.shape, t.dtype) if t is not None else (shape, dtype)
        n = math.prod(shape)
        buf = torch.full((n + 16,), SENT, dtype=dtype, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        view = buf[8 + self.off: 8 + self.off + n].view(shape)
        assert (view.data_ptr() % 16 != 0) == bool(self.off)
        if t is not None:
            view.copy_(t.to(self.dev))
        self.bufs.append((buf, 8 + self.off, n))
        return view

    def intact(self):
        for buf, lo, n in self.bufs:
            c = buf.cpu()
            assert bool((c[:lo] == SENT).all()) and bool((c[lo + n:] == SENT).all()), "bytes outside a view were written"


def an_direct(dev, off, x, res, w, b, eps, is_rms, swap, ydt, dy, dro):
    """cad_add_norm_fwd + cad_add_norm_bwd_slotted on operands and outputs placed by an Arena; returns the outputs (views)."""
    S, R, D = x.shape
    A = Arena(dev, off)
    lib = L.get_lib()
    xd, rd, wd, bd = A.put(x), A.put(res), A.put(w), A.put(b)
    y, s = A.put(shape=x.shape, dtype=ydt), A.put(shape=x.shape, dtype=F32)
    rstd, mean = A.put(shape=(S * R,), dtype=F32), (None if is_rms else A.put(shape=(S * R,), dtype=F32))
    stream = L.stream_and_check(xd, rd, wd, bd, y, s, rstd, mean)
    a = L.AddNormArgs(L.ptr(xd), L.ptr(rd), L.ptr(wd), L.ptr(bd), L.ptr(y), L.ptr(s), L.ptr(rstd), L.ptr(mean), R, S, D, float(eps),
                      int(is_rms), int(swap), L.dtype_code(x.dtype), L.dtype_code(ydt), None, None)
    L.check(lib.cad_add_norm_fwd(C.byref(a), stream), "cad_add_norm_fwd")
    dyd, drod = A.put(dy), A.put(dro)
    dx, dri = A.put(shape=x.shape, dtype=x.dtype), (None if res is None else A.put(shape=x.shape, dtype=F32))
    dw, db = torch.zeros(D, dtype=F32, device=dev), (None if b is None else torch.zeros(D, dtype=F32, device=dev))
    ab = L.AddNormBwdArgs(L.ptr(dyd), L.ptr(drod), L.ptr(s), L.ptr(rstd), L.ptr(mean), L.ptr(wd), L.ptr(dx), L.ptr(dri), L.ptr(dw),
                          L.ptr(db), R, S, D, int(is_rms), int(swap), L.dtype_code(x.dtype), L.dtype_code(ydt))
    n = lib.cad_add_norm_bwd_slots(C.byref(ab))
    ws, bs = ops.wgrad_slots(n, D, dev), (None if db is None else ops.wgrad_slots(n, D, dev))
    L.check(lib.cad_add_norm_bwd_slotted(C.byref(ab), L.ptr(ws), L.ptr(bs), stream), "cad_add_norm_bwd_slotted")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    A.intact()
    return {"y": y, "res_out": s, "dx": dx, "dres_in": dri, "dweight": dw, "dbias": db}


@pytest.mark.parametrize("D", [30, 63, 64, 260, 1020])
@pytest.mark.parametrize("xdt,ydt", AN_TYPES)
def test_add_norm_misaligned(backend, D, xdt, ydt):
    """Every operand and output one element into its buffer: the launchers' `vec` flag sends D % 4 == 0 to the scalar kernels too.  Same
    bounds; sentinels around every view intact; at D % 4 != 0 bit-identical to the aligned call (see the header for D % 4 == 0)."""
    name, dev = backend
    for k, (is_rms, has_res, has_bias, swap) in enumerate([(True, True, False, True), (False, True, True, False), (False, False, True, True)]):
        x, res, w, b, dy, dro = an_inputs(2, 9, D, xdt, ydt, has_res, has_bias, 31 * D + k)
        ref = an_reference(x, res, w, b, 1e-5, is_rms, swap, ydt, dy, dro)
        outs = {}
        for off in (1, 0):
            outs[off] = an_direct(dev, off, x, res, w, b, 1e-5, is_rms, swap, ydt, dy, dro)
            for key, t in outs[off].items():
                if t is not None:
                    dt = ydt if key == "y" else (xdt if key == "dx" else F32)
                    hold(name, f"addnorm-{'misaligned' if off else 'direct'}.{key}", t, *ref[key], dt)
        if D % 4 != 0:
            for key, t in outs[1].items():
                if t is not None:
                    assert torch.equal(t.float().cpu(), outs[0][key].float().cpu()), f"{key}: the scalar kernel's result depends on the address"


# =========================================================================================================================================
# LM head
# =========================================================================================================================================
def lm_reference(h, W, comp, labels, ign, dlogits, dloss, torch_path):
    """fp64 values and tolerances.  h (S, R, D) as stored, W (V, D) fp32, labels (R,) int64 or None, dlogits (R, V) fp32 or None, dloss a
    float or None (no gradient through the loss)."""
    S, R, D = h.shape
    V = W.shape[0]
    hdt = h.dtype
    H, Wd = h.double(), W.double()
    z, az = H[0] @ Wd.t(), H[0].abs() @ Wd.abs().t()
    if S == 2:
        z, az = z + H[1] @ Wd[comp].t(), az + H[1].abs() @ Wd[comp].abs().t()
    e_z = gam(S * D + 2) * az + S * D * UF
    out = {"logits": (z, e_z)}
    G, e_G = torch.zeros_like(z), torch.zeros_like(z)
    if labels is not None:
        valid = (labels != ign) & (labels >= 0) & (labels < V)
        mx = z.max(-1).values
        lse = torch.logsumexp(z, -1)
        p = torch.softmax(z, -1)
        lab = labels.clamp(0, V - 1)
        row = lse - z.gather(1, lab[:, None])[:, 0]
        E = e_z.max(-1).values
        spread = (z - mx[:, None]).abs().max(-1).values + 2 * E
        rho_e = 2 * U * EXP_ULPS + U * (spread + 1)
        rho_se = rho_e + gam(V) + V * UF
        e_row = E + e_z.gather(1, lab[:, None])[:, 0] + rho_se * (1 + rho_se) + 2 * U * LOG_ULPS * (lse - mx).abs() + U * lse.abs() + \
            U * row.abs() + 2 * U * E
        cnt = int(valid.sum())
        tot, e_tot = row[valid].sum(), e_row[valid].sum()
        loss = tot / cnt if cnt else torch.tensor(float("nan"), dtype=torch.float64)
        e_loss = (e_tot + gam(cnt + 3) * (tot + e_tot)) / max(cnt, 1) + 2 * U * (tot / max(cnt, 1)).abs()
        out["loss"] = (loss.reshape(1), e_loss.reshape(1))
        if dloss is not None and cnt:
            coef = dloss / cnt
            oh = torch.zeros_like(z).scatter_(1, lab[:, None], 1.0)
            rho_p = torch.expm1(2 * E + 2 * rho_e + gam(V + 2))[:, None]
            e_p = p * rho_p + UF
            vm = valid[:, None].double()
            G = vm * (p - oh) * coef
            e_G = vm * (e_p * abs(coef) + gam(4) * ((p - oh).abs() + e_p) * abs(coef))
    if dlogits is not None:
        G = G + dlogits.double()
        e_G = e_G + U * (G.abs() + e_G)
    uh = UO[hdt]
    e_W = torch.zeros_like(Wd)
    if torch_path and hdt != F32:
        e_G = e_G + uh * (G.abs() + e_G) + FLOOR[hdt]
        e_W = uh * Wd.abs()
    G_up, W_up = G.abs() + e_G, Wd.abs() + e_W
    dh, tol_dh, dW, tol_dW = [], [], torch.zeros_like(Wd), torch.zeros_like(Wd)
    n = R * S
    for s in range(S):
        Ws, W_ups, e_Ws = (Wd, W_up, e_W) if s == 0 else (Wd[comp], W_up[comp], e_W[comp])
        v = G @ Ws
        e = e_G @ Ws.abs() + G_up @ e_Ws + gam(V + 2) * (G_up @ W_ups) + V * UF
        dh.append(v)
        tol_dh.append(e + uh * (v.abs() + e) + FLOOR[hdt])
        d = G.t() @ H[s]
        e = e_G.t() @ H[s].abs() + gam(n + 2) * (G_up.t() @ H[s].abs()) + n * UF
        if torch_path and hdt != F32:
            e = e + uh * (d.abs() + e) + FLOOR[hdt]  # each strand's product is a 16-bit matrix product there
        if s == 0:
            dW, tol_dW = dW + d, tol_dW + e
        else:
            dW.index_add_(0, comp, d)
            tol_dW.index_add_(0, comp, e)
    out["dhidden"] = (torch.stack(dh), torch.stack(tol_dh))
    out["dW"] = (dW, tol_dW)
    return out


def lm_inputs(S, R, D, V, dtype, seed, frac_counted=0.2, ign=4, comp=COMP, heavy=()):
    """Hidden rows carry a signal of their label's weight row: the logits favour the label and the dW sums are coherent (|sum| a sizeable
    part of sum |terms|), so that a dropped tile moves dW by far more than the bound.  heavy: row ranges in which EVERY label counts --
    the walk tests put them on the tiles of the few waves that take a second tile (first and later trips) and count 2 % elsewhere, so
    that what such a wave carries from tile to tile is a tenth of the loss and of dW, not 0.3 % (below the worst-case bounds)."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(V, D, generator=g)
    labels = torch.randint(0, V, (R,), generator=g)
    h = torch.randn(S, R, D, generator=g) + (1.5 / math.sqrt(D)) * torch.stack([W[labels]] + ([W[comp][labels]] if S == 2 else []))
    skip = torch.rand(R, generator=g) >= frac_counted
    for lo, hi in heavy:
        skip[lo:hi] = False
    labels[skip] = ign
    # (small against the loss gradient of a counted row, ~1e-3: its incoherent terms would otherwise dominate sum |terms| of dW)
    dlog = 2.0 ** -16 * torch.randn(R, V, generator=g)
    return h.to(dtype), W, labels, dlog


def lm_check(backend, h, W, comp, labels, ign, dlogits, dloss, torch_path, tag="lmhead"):
    name, dev = backend
    S, R, D = h.shape
    V = W.shape[0]
    hd, wd = h.clone().to(dev).reshape(S, 1, R, D).requires_grad_(True), W.clone().to(dev).requires_grad_(True)
    cd = None if comp is None else comp.to(dev)
    logits, loss = ops.lm_head(hd, wd, cd, None if labels is None else labels.to(dev).reshape(1, R), ign)
    ref = lm_reference(h, W, comp, labels, ign, dlogits, dloss, torch_path)
    hold(name, f"{tag}.logits", logits, *ref["logits"], F32)
    if labels is not None:
        hold(name, f"{tag}.loss", loss.reshape(1), *ref["loss"], F32)
    roots, grads = [], []
    if dloss is not None:
        roots.append(loss), grads.append(torch.tensor(dloss, dtype=F32, device=dev))
    if dlogits is not None:
        roots.append(logits), grads.append(dlogits.to(dev).reshape(logits.shape))
    if not roots:
        return
    torch.autograd.backward(roots, grads)
    hold(name, f"{tag}.dhidden", hd.grad, *ref["dhidden"], h.dtype)
    hold(name, f"{tag}.dW", wd.grad, *ref["dW"], F32)


def _comp(V, S):
    return None if S == 1 else (COMP if V == 16 else COMP12)


def test_complement_maps_are_involutions():
    for c in (COMP, COMP12):
        assert torch.equal(c[c], torch.arange(c.numel())) and not torch.equal(c, torch.arange(c.numel()))


ROWS2 = 32768 + 5 * 16 + 7    # 512 workgroups x 4 waves x 16 tokens = 32768 per trip: 6 tiles more, the last one ragged
ROWS3 = 65536 + 16 + 3        # a third trip for two waves
HEAVY2 = ((0, 96), (32768, ROWS2))                       # the six walking waves' first tiles, and their second ones
HEAVY3 = ((0, 32), (32768, 32768 + 32), (65536, ROWS3))  # the two waves that take three tiles


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("dtype", LM_TYPES)
@pytest.mark.parametrize("D", [128, 256])
def test_lm_head_two_tile_walk(backend, D, dtype, S):
    """Matrix-core forward and backward where some waves take two 16-token tiles and most take one: next-tile prefetch, loss / count
    carried across tiles, dW accumulators and the wave's LDS G tile reused, 512 loss partials folded in two trips of 256.  The loss is
    checked with an upstream dlogits (here) and without (test_lm_head_three_tile_walk, the edge values)."""
    lib = L.get_lib()
    # the matrix-core forward and backward share one grid formula, capped at 512 workgroups: 512 loss partials, two trips of the fold
    assert lib.cad_lm_head_bwd_partials(ROWS2) == 512 > 256 and ((ROWS2 + 15) // 16 + 3) // 4 > 512
    assert lib.cad_lm_head_partials(ROWS2) // 2 >= 512  # (the caller's buffer, sized for the general kernel's grid)
    assert (ROWS2 + 15) // 16 > 512 * 4 and ROWS2 % 16 != 0
    h, W, labels, dlog = lm_inputs(S, ROWS2, D, 16, dtype, 5 * D + S, frac_counted=0.02, heavy=HEAVY2)
    lm_check(backend, h, W, _comp(16, S), labels, 4, dlog, 0.75, False, tag="lmhead-mfma")


def test_lm_head_three_tile_walk(backend):
    name, dev = backend
    assert (ROWS3 + 15) // 16 > 2 * 512 * 4
    h, W, labels, dlog = lm_inputs(2, ROWS3, 128, 16, BF, 77, frac_counted=0.02, heavy=HEAVY3)
    lm_check(backend, h, W, COMP, labels, 4, None, 1.0, False, tag="lmhead-mfma")


def test_lm_head_small_vocabulary_walk(backend):
    """V = 12 < the 16-column tile, two tiles per wave, both strands."""
    h, W, labels, dlog = lm_inputs(2, ROWS2, 256, 12, F32, 78, comp=COMP12, frac_counted=0.02, heavy=HEAVY2)
    lm_check(backend, h, W, COMP12, labels, 4, dlog, 1.0, False, tag="lmhead-mfma")


def test_lm_head_d512_multi_tile(backend):
    """bf16, d_model 512: the NJ = 16 forward, and the backward as two launches over 256-channel blocks with ld = 512."""
    h, W, labels, dlog = lm_inputs(2, ROWS2, 512, 16, BF, 79, frac_counted=0.02, heavy=HEAVY2)
    lm_check(backend, h, W, COMP, labels, 4, dlog, 1.0, False, tag="lmhead-mfma")


@pytest.mark.parametrize("D,dtype", [(40, F32), (40, BF), (40, HF), (512, F32)], ids=["D40-f32", "D40-bf16", "D40-f16", "D512-f32"])
def test_lm_head_general_kernel_walk(backend, D, dtype):
    """One wave per row, 4096 workgroups of 4: at 16384 + 13 rows thirteen waves take a second row, and the 4096 loss partials take 16
    trips of the fold.  D = 40: the backward is the torch path; D = 512 fp32: the two-launch matrix-core backward."""
    R = 16384 + 13
    assert L.get_lib().cad_lm_head_partials(R) // 2 == 4096 > 256 and R > 4096 * 4
    h, W, labels, dlog = lm_inputs(2, R, D, 16, dtype, 80 + D, frac_counted=0.02, heavy=((0, 13), (16384, R)))
    lm_check(backend, h, W, COMP, labels, 4, dlog, 1.0, D == 40, tag="lmhead-general")


LM_EDGES = ["spread60", "shifted+100", "shifted-120", "label-on-smallest", "all-ignored", "one-counted-last-tile", "labels-out-of-range",
            "dlogits-no-labels", "zero-rows"]


@pytest.mark.parametrize("kind", LM_EDGES)
@pytest.mark.parametrize("D", [128, 40])
@pytest.mark.parametrize("dtype", LM_TYPES)
def test_lm_head_edge_values(backend, kind, D, dtype):
    """One matrix-core D and the general kernel (torch backward).  37 rows: two full tiles and a ragged one."""
    S, R, V, ign = 2, 37, 16, -100
    g = torch.Generator().manual_seed(LM_EDGES.index(kind) * 100 + D)
    h, W, labels, dlog = lm_inputs(S, R, D, V, dtype, 900 + D, frac_counted=0.7, ign=ign)
    dloss, dlogits = 1.0, None
    if kind in ("spread60", "shifted+100", "shifted-120", "label-on-smallest"):
        # logits tens of units apart: W[v] = target[v] e for one unit direction e, h = e / 2 in both strands: logit v = (target[v] + target[comp v]) / 2
        target = torch.linspace(-60, 60, V)[torch.randperm(V, generator=g)]
        if kind == "shifted+100":
            target = target / 4 + 100  # every logit above fp32's exp range: a softmax without the max subtraction overflows
        if kind == "shifted-120":
            target = target / 4 - 120  # every exp underflows without it
        e = torch.randn(D, generator=g)
        e = e / e.norm()
        W = target[:, None] * e[None, :] + 0.01 * torch.randn(V, D, generator=g)
        h = (0.5 * e[None, None, :] * torch.ones(S, R, 1) + 0.01 * torch.randn(S, R, D, generator=g)).to(dtype)
        if kind == "label-on-smallest":
            z = lm_reference(h, W, COMP, None, ign, None, None, False)["logits"][0]
            labels = z.argmin(-1)
    elif kind == "all-ignored":
        labels = torch.full((R,), ign)
    elif kind == "one-counted-last-tile":
        labels = torch.full((R,), ign)
        labels[R - 2] = 5
    elif kind == "labels-out-of-range":
        labels[::3] = V
        labels[1::5] = -1
        labels[2::7] = 1 << 40
    elif kind == "dlogits-no-labels":
        labels, dloss, dlogits = None, None, dlog
    elif kind == "zero-rows":
        h = h.clone()
        h[:, ::2] = 0
    lm_check(backend, h, W, COMP, labels, ign, dlogits, dloss, D == 40, tag="lmhead-edge")


def test_lm_head_all_ignored_matches_cross_entropy():
    """The reference convention itself: F.cross_entropy in fp64 with every label ignored gives a NaN loss and ZERO gradients."""
    z = torch.randn(5, 16, dtype=torch.float64, requires_grad=True)
    loss = torch.nn.functional.cross_entropy(z, torch.full((5,), -100), ignore_index=-100)
    loss.backward()
    assert bool(torch.isnan(loss)) and bool((z.grad == 0).all())
    h, W, _, _ = lm_inputs(1, 5, 40, 16, F32, 1)
    ref = lm_reference(h, W, None, torch.full((5,), -100), -100, None, 1.0, False)
    assert bool(torch.isnan(ref["loss"][0]).all()) and bool((ref["dW"][0] == 0).all())


@pytest.mark.parametrize("dtype", LM_TYPES)
@pytest.mark.parametrize("D", [128, 256])
def test_lm_head_misaligned(backend, D, dtype):
    """hidden one element into its buffer: cad_lm_head_fwd takes the general kernel (hidden % 32), the backward the torch path (% 16).
    Logits go into a sentinel-surrounded view, through the C entry point; then the whole op through ops.lm_head."""
    name, dev = backend
    S, R, V = 2, 37, 16
    h, W, labels, dlog = lm_inputs(S, R, D, V, dtype, 600 + D, frac_counted=0.7)
    A = Arena(dev, 1)
    hd, wd, logits = A.put(h), W.to(dev), A.put(shape=(R, V), dtype=F32)
    assert hd.data_ptr() % 16 != 0 and hd.is_contiguous()
    acc = torch.zeros(2, dtype=F32, device=dev)
    lab, cd = labels.to(dev), COMP.to(dev)
    parts = torch.empty(L.get_lib().cad_lm_head_partials(R), dtype=F32, device=dev)
    stream = L.stream_and_check(hd, wd, cd, lab, logits, acc, parts)
    a = L.LmHeadArgs(L.ptr(hd), L.ptr(wd), L.ptr(cd), L.ptr(lab), L.ptr(logits), C.c_void_p(acc.data_ptr()), C.c_void_p(acc.data_ptr() + 4),
                     R, D, V, S, 4, L.dtype_code(dtype), L.ptr(parts))
    L.check(L.get_lib().cad_lm_head_fwd(C.byref(a), stream), "cad_lm_head_fwd")
    ref = lm_reference(h, W, COMP, labels, 4, None, None, False)
    hold(name, "lmhead-misaligned.logits", logits, *ref["logits"], F32)
    hold(name, "lmhead-misaligned.loss", (acc[0] / acc[1]).reshape(1), *ref["loss"], F32)
    A.intact()
    # the whole op on the misaligned view (ops keeps a contiguous view as it is)
    hv = A.put(h).reshape(S, 1, R, D).requires_grad_(True)
    wl = W.clone().to(dev).requires_grad_(True)
    lg, loss = ops.lm_head(hv, wl, cd, lab.reshape(1, R), 4)
    torch.autograd.backward([loss, lg], [torch.tensor(0.75, device=dev), dlog.to(dev).reshape(lg.shape)])
    ref = lm_reference(h, W, COMP, labels, 4, dlog, 0.75, True)
    hold(name, "lmhead-misaligned.logits", lg, *ref["logits"], F32)
    hold(name, "lmhead-misaligned.loss", loss.reshape(1), *ref["loss"], F32)
    hold(name, "lmhead-misaligned.dhidden", hv.grad, *ref["dhidden"], dtype)
    hold(name, "lmhead-misaligned.dW", wl.grad, *ref["dW"], F32)


def test_zz_report_worst_ratios(backend):
    """Prints the worst err / tol per output and type recorded by the tests above (run with -s to see it)."""
    name, dev = backend
    for (bk, key) in sorted(WORST):
        if bk == name:
            print(f"[fp64 summary] {bk} {key}: {WORST[(bk, key)]:.3f}")
    assert all(v <= 1.0 for (bk, _), v in WORST.items() if bk == name)
