"""Causal conv1d + SiLU (csrc/conv1d.hip) and the embedding (csrc/embed.hip) held to float64, element by element, at the row lengths and
row counts where their tile walks start and end, for every tap count, on misaligned operands and at edge values.

In the manner of test_norm_head_fp64.py (whose helpers are imported, not copied): references are written here in torch.float64 and start
from the inputs AS STORED (after their rounding to bf16 / fp16); every output element must satisfy |out - ref| <= tol with a tol DERIVED
below from how the kernel rounds; nothing in it is fitted to a result.  Notation as there: u = 2^-24, g(n) = n u / (1 - n u) (n fp32
roundings in a row, any order, fused or not), uo = 0 / 2^-8 / 2^-11 for an fp32 / bf16 / fp16 OUTPUT, floor = half the spacing of the
output format's subnormals, UF = 2^-126 per fp32 operation whose result may underflow (gradual underflow or flush-to-zero).

Approximate instructions (carried explicitly as constants, as RSQ_ULPS is there):
  EXP2_ULPS = 1   cad_exp2 is v_exp_f32 on the device (exp2f on the emulator, < 1 ulp).
  RCP_ULPS  = 1   cad_rcp is v_rcp_f32 on the device (a correctly rounded 1 / x on the emulator).
                  The micro-architecture notes give the instructions' cost only, no accuracy: 1 ulp (= 2 u relative) is assumed for each.
                  Both flush subnormal results to zero on the device: an absolute UF each.

conv1d.  Per row, in the row's own direction (rows below `split` run in direction rev_lo, the others in rev_hi; a right-to-left row is
realised here by an explicit flip, the convolution of a left-to-right row, and a flip back), K taps w_0 .. w_{K-1}, bias b (0 if None):
  pre[l] = b + sum_k w_k x[l - (K-1) + k]      x = 0 before the row
  out    = pre sigma(pre)
  dpre   = dout sigma (1 + pre (1 - sigma))
  dx[m]  = sum over the sets of sum_k w_k dpre[m + (K-1) - k]   (+ the addend when `accumulate` is set)
  dw_k   = sum over the channel's rows and positions of dpre[l] x[l - (K-1) + k],   dbias = sum dpre
Bounds (P = pre, s = sigma(P), q = 1 - s = sigma(-P), both evaluated in fp64 without cancellation):
  pre    the kernel holds the taps aligned to four (the missing leading taps have the weight 0: exact zeros that add no error) and runs a
         chain of explicit fused multiply-adds from b: K roundings,  e_P = g(K) (|b| + sum_k |w_k x|) + K UF.
  sigma  = rcp(1 + exp2(t)), t = fl(-pre^ fl(log2 e)): the constant and the product are rounded, the error of pre^ goes through:
         |t - (-P log2 e)| <= d = log2e (e_P (1 + g(2)) + g(2) |P|) + UF;   exp2: E^ = E (1 + r), E = exp(-P),
         |r| <= rho = 2^d (1 + 2 u EXP2_ULPS) - 1, or E^ flushed (absolute UF);   the denominator 1 + E^ is off by the relative
         dd = q rho + UF + u (1 + q rho + UF)  (E / (1 + E) = q; one rounding of the add);   rcp: 2 u RCP_ULPS relative, absolute UF:
         e_s = s ((1 + 2 u RCP_ULPS) / (1 - dd) - 1) + 2 UF.
         Where exp2 overflows to +inf (t >= 128, P below -88.7), sigma^ = rcp(inf) = 0 exactly and out = -0: the true sigma is then
         below 2^(-128 + d) < UF, which the absolute UF terms carry (e_out >= (|P| + e_P) 2 UF there; for an fp32 output this is ABOVE
         the format's floor 2^-150: sigma(-88.7) ~ 2^-128 is an fp32 subnormal, not zero -- the bound says so instead of a floor).
  out    = fl(pre^ sigma^):   e_out = (|P| + e_P)(s + e_s)(1 + u) - |P| s + UF;   tol = e_out + uo (|out| + e_out) + floor.
  1 - sigma^   one rounding:  e_q = e_s + u (q + e_s).  Near sigma = 1 this is an ABSOLUTE error of ~3 u on a q that may be far smaller.
  dpre   T = 1 + P q:  e_T = ((|P| + e_P)(q + e_q) - |P| q) + g(2) (1 + (|P| + e_P)(q + e_q)) + UF  -- the term |P| e_q is the
         absolute error of 1 - sigma^ multiplied by |pre|: at pre = 1e4 it is ~1e-3 of dout, and the bound carries it as such.
         dpre = dout sigma T:  e_dpre = |dout| (s + e_s)(|T| + e_T)(1 + g(2)) - |dout| s |T| + 2 UF
         (upper bounds multiplied through, the true magnitude subtracted, two roundings of the two products).
  dx     per set a chain of K fused multiply-adds from 0, one add per set, one for the addend: with R = sum over the sets of (K + 1) + 1,
         e_dx = sum_sets sum_k |w_k| e_dpre + g(R) (sum_sets sum_k |w_k| (|dpre| + e_dpre) + |addend|) + R UF;
         tol = e_dx + uo (|dx| + e_dx) + floor.  The addend is read as stored.
  dw_k, dbias   n = rows x positions terms of the channel, in ANY association order (lane, wave butterfly, LDS fold of the four waves,
         slot fold or fp32 atomics):  sum |x| e_dpre + g(n + 8) sum (|dpre| + e_dpre) |x| + n UF   (dbias: x = 1).  fp32 outputs.
  Inputs (conv_inputs): dout correlates with the row's own window of x and has a mean, so that the dw / dbias sums are coherent (|sum| is
  a sizeable part of sum |terms|, which the bound scales with): a tile counted twice or dropped moves them by far more than the bound.
  One row in 16 is 2^12 times larger than the others, so that single rows matter to the sums.

  Misaligned operands (contiguous views one element into a larger buffer, which .contiguous() keeps) take the scalar kernels at
  L % 8 == 0 too (the launchers' `vec`).  The FORWARD result must equal the aligned (vector) call bit for bit: per element it is the same
  chain of explicit fmaf and one product pre * sigma, and nothing else in it can be contracted.  The BACKWARD is held to the bounds
  only: 1 + pre (1 - sigma), o += ..., part += dpre * x are expressions that -ffp-contract may fuse differently in the two
  instantiations, so bit equality of dx / dw is not a property of the source.
  Non-finite x (one +inf, one NaN per placement): everything whose window does not contain the value keeps its bounds -- outputs outside
  [p - 3, p + 3] of the row, dx outside [p - 6, p + 6], other rows' dx, other channels' dw / dbias (the reference is computed with the
  value replaced by 0: none of those depend on it).  Outputs inside the causal window of the row's direction (K positions) must be
  non-finite; the class (inf / NaN) is not asserted.  For K < 4 the kernel multiplies the missing leading taps' ZERO weights with the
  window (0 * inf = NaN), so a non-finite value reaches one to three positions more than the K taps do: the K = 4 window (+-3, +-6)
  is asserted for every K, and the kernel is left as it is.

Embedding.  Forward: a gather and one conversion, so the output EQUALS W[ids] (strand 1: W[comp[ids]]) converted with torch's own cast
(round to nearest even, as from_f32); ids outside [0, V) are clamped to 0 / V - 1 first, in the forward and in the backward alike.
Backward: dW[v] = sum of dout (as stored) over the tokens mapped to v; with n_v terms in any order (wave tables, their sum, slot fold)
tol = g(n_v + 2) sum |dout| + floor(fp32); a 16-bit table's gradient is rounded to the table's type once more (uo, floor of that type).
A word no token maps to has a row that is exactly 0.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from caduceus_amd import _lib as L
from caduceus_amd import mixer, ops
from test_norm_head_fp64 import COMP, COMP12, FLOOR, OVER, TAG, U, UF, UO, WORST, gam, hold  # noqa: F401

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
EXP2_ULPS, RCP_ULPS = 1, 1
LOG2E = 1.4426950408889634
TYPES = [pytest.param(F32, id="f32"), pytest.param(BF, id="bf16"), pytest.param(HF, id="f16")]
TILE = 496          # positions per wave tile (62 lanes x 8)
FWD_WG = 4 * 4      # virtual tiles per forward workgroup (4 waves x 4 tiles)
BWD_WG = 4 * 8      # ... per backward workgroup


# =========================================================================================================================================
# conv1d: reference
# =========================================================================================================================================
def _rev_rows(SB, split, dirs):
    return torch.where(torch.arange(SB) < split, bool(dirs[0]), bool(dirs[1]))


def _dir(t, rev):
    """Rows that run right-to-left flipped along L (an involution): row frame <-> the row's own direction."""
    return torch.where(rev[None, :, None], t.flip(-1), t)


def _behind(t, K):
    """(E, SB, L) -> (E, SB, L, K): [..., l, k] = t[l - (K-1) + k], 0 before the row."""
    return F.pad(t, (K - 1, 0)).unfold(-1, K, 1)


def _ahead(t, K):
    """[..., m, j] = t[m + j], 0 behind the row."""
    return F.pad(t, (0, K - 1)).unfold(-1, K, 1)


def sigmoid_bounds(P, e_P):
    """sigma, 1 - sigma in fp64 and the bounds e_s, e_q of the header."""
    s, q = torch.sigmoid(P), torch.sigmoid(-P)
    d = LOG2E * (e_P * (1 + gam(2)) + gam(2) * P.abs()) + UF
    rho = torch.exp(math.log(2.0) * d) * (1 + 2 * U * EXP2_ULPS) - 1
    dd = q * rho + UF
    dd = dd + U * (1 + dd)
    assert float(dd.max()) < 0.5, "the sigmoid bound is void"
    e_s = s * ((1 + 2 * U * RCP_ULPS) / (1 - dd) - 1) + 2 * UF
    e_q = e_s + U * (q + e_s)
    return s, q, e_s, e_q


def conv_reference(x, sets, split, douts=None, addend=None):
    """fp64 values and tolerances.  x (E, SB, L) as stored; sets: [(w (E, K) fp32, b (E,) fp32 or None, (rev_lo, rev_hi))]; douts: one
    (E, SB, L) tensor as stored per set; addend: the pre-filled dx of an accumulating call, as stored.
    Returns {"pre": [P], "out": [(ref, tol)], "dx": (ref, tol), "dw": [(ref, tol)], "db": [(ref, tol)]}, all in the row frame."""
    E, SB, Lq = x.shape
    dt = x.dtype
    X = x.double()
    res = {"pre": [], "out": [], "dw": [], "db": []}
    dx, e_dx, up_dx, R = torch.zeros_like(X), torch.zeros_like(X), torch.zeros_like(X), 1
    for i, (w, b, dirs) in enumerate(sets):
        K = w.shape[1]
        rev = _rev_rows(SB, split, dirs)
        W = w.double()[:, None, None, :]
        Bv = (torch.zeros(E, dtype=torch.float64) if b is None else b.double())[:, None, None]
        win = _behind(_dir(X, rev), K)
        P = Bv + (win * W).sum(-1)
        e_P = gam(K) * (Bv.abs() + (win.abs() * W.abs()).sum(-1)) + K * UF
        s, q, e_s, e_q = sigmoid_bounds(P, e_P)
        o = P * s
        e_o = (P.abs() + e_P) * (s + e_s) * (1 + U) - o.abs() + UF
        res["pre"].append(_dir(P, rev))
        res["out"].append((_dir(o, rev), _dir(e_o + UO[dt] * (o.abs() + e_o) + FLOOR[dt], rev)))
        if douts is None:
            continue
        G = _dir(douts[i].double(), rev)
        Pq_up = (P.abs() + e_P) * (q + e_q)
        T = 1 + P * q
        e_T = (Pq_up - P.abs() * q) + gam(2) * (1 + Pq_up) + UF
        dpre = G * s * T
        e_dp = G.abs() * (s + e_s) * (T.abs() + e_T) * (1 + gam(2)) - dpre.abs() + 2 * UF
        dp_up = dpre.abs() + e_dp
        Wf = W.flip(-1)  # dx[m] = sum_j w[K-1-j] dpre[m + j]
        dx += _dir((_ahead(dpre, K) * Wf).sum(-1), rev)
        e_dx += _dir((_ahead(e_dp, K) * Wf.abs()).sum(-1), rev)
        up_dx += _dir((_ahead(dp_up, K) * Wf.abs()).sum(-1), rev)
        R += K + 1
        n = SB * Lq
        dw = torch.einsum("esl,eslk->ek", dpre, win)
        t_dw = torch.einsum("esl,eslk->ek", e_dp, win.abs()) + gam(n + 8) * torch.einsum("esl,eslk->ek", dp_up, win.abs()) + n * UF
        res["dw"].append((dw, t_dw))
        res["db"].append((dpre.sum((1, 2)), e_dp.sum((1, 2)) + gam(n + 8) * dp_up.sum((1, 2)) + n * UF))
    if douts is not None:
        if addend is not None:
            dx, up_dx = dx + addend.double(), up_dx + addend.double().abs()
        e = e_dx + gam(R) * up_dx + R * UF
        res["dx"] = (dx, e + UO[dt] * (dx.abs() + e) + FLOOR[dt])
    return res


def conv_inputs(E, SB, Lq, Ks, dtype, split, dirs_list, seed, bias=True, xscale=1.0):
    """x, [(w, b, dirs)], [dout]: see the header (coherent dw / dbias sums, one row in 16 a factor 2^12 larger)."""
    g = torch.Generator().manual_seed(seed)
    x = (xscale * torch.randn(E, SB, Lq, generator=g)).clamp(-6e4, 6e4).to(dtype)  # (inside fp16's range)
    rows = torch.arange(E * SB).view(E, SB, 1)
    scale = torch.where(rows % 16 == 5, 1.0, 2.0 ** -12)
    sets, douts = [], []
    for K, dirs in zip(Ks, dirs_list):
        w = 0.5 * torch.randn(E, K, generator=g)
        b = 0.2 * torch.randn(E, generator=g) if bias else None
        rev = _rev_rows(SB, split, dirs)
        sw = _behind(_dir(x.float(), rev), K).sum(-1) / (xscale if xscale else 1.0)
        dout = _dir(scale * (0.5 * sw + 0.25 + torch.randn(E, SB, Lq, generator=g)), rev).to(dtype)
        sets.append((w, b, dirs))
        douts.append(dout)
    return x, sets, douts


def conv_check(backend, x, wset, split, dout, tag="conv", xdev=None, doutdev=None):
    """Through ops.causal_conv1d and autograd (the production path: slotted dw / dbias), every output against conv_reference.
    Returns (out, dx, dw, dbias) as computed."""
    name, dev = backend
    w, b, dirs = wset
    E, K = w.shape
    xd = (x.clone().to(dev) if xdev is None else xdev).requires_grad_(dout is not None)
    wd = w.clone().to(dev).view(E, 1, K).requires_grad_(dout is not None)
    bd = None if b is None else b.clone().to(dev).requires_grad_(dout is not None)
    out = ops.causal_conv1d(xd, wd, bd, split, *dirs)
    ref = conv_reference(x, [wset], split, None if dout is None else [dout])
    hold(name, f"{tag}.out", out, *ref["out"][0], x.dtype)
    if dout is None:
        return out.detach(), None, None, None
    out.backward(dout.to(dev) if doutdev is None else doutdev)
    hold(name, f"{tag}.dx", xd.grad, *ref["dx"], x.dtype)
    hold(name, f"{tag}.dw", wd.grad.view(E, K), *ref["dw"][0], F32)
    if bd is not None:
        hold(name, f"{tag}.dbias", bd.grad, *ref["db"][0], F32)
    return out.detach(), xd.grad, wd.grad, None if bd is None else bd.grad


def _bwd_slots(SB, Lq):
    a = L.Conv1dBwdArgs(None, None, None, None, None, None, None, SB, Lq, 0, 1, 4, 0, 0, 0, 0)
    return L.get_lib().cad_conv1d_bwd_slots(C.byref(a))


BOTH = [(0, 1), (1, 0)]


# ---- row-length edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq", [1, 2, 3, 4, 7, 8, 9, 495, 496, 497, 504, 992, 993, 1000])
@pytest.mark.parametrize("dtype", TYPES)
def test_conv1d_row_lengths(backend, Lq, dtype):
    """One lane, one vector, the exact end of a tile (496, 992), one element past it, vector (L % 8 == 0) and scalar kernels.  Two rows per
    channel in opposite directions, both assignments."""
    for k, dirs in enumerate(BOTH):
        x, sets, douts = conv_inputs(2, 2, Lq, [4], dtype, 1, [dirs], 10 * Lq + k)
        conv_check(backend, x, sets[0], 1, douts[0])


# ---- walks ------------------------------------------------------------------------------------------------------------------------------
WALKS = [(3, 11, 1000, 4), (3, 11, 1001, 4), (2, 1, 2488, 1)]  # E, SB, L, split


@pytest.mark.parametrize("E,SB,Lq,split", WALKS, ids=[f"E{c[0]}-SB{c[1]}-L{c[2]}" for c in WALKS])
@pytest.mark.parametrize("dtype", TYPES)
def test_conv1d_walks(backend, E, SB, Lq, split, dtype):
    """(3, 11, 1000): 3 tiles per row, 33 virtual tiles per channel -- forward waves take a second and third tile in other rows and across
    the split (three workgroups, the last with one tile), the backward has two workgroups, the second with a single tile and three idle
    waves.  L = 1001: the same walk in the scalar kernels (and a fourth, one-element tile per row).  (2, 1, 2488): six tiles of one row,
    a wave's second tile lies in the same row."""
    tpr = (Lq + TILE - 1) // TILE
    nvt = SB * tpr
    assert _bwd_slots(SB, Lq) == (nvt + BWD_WG - 1) // BWD_WG
    if SB == 11:
        assert nvt > 2 * FWD_WG and _bwd_slots(SB, Lq) == 2 and (Lq != 1000 or nvt == BWD_WG + 1)
    else:
        assert tpr == 6 and 4 < nvt < FWD_WG
    for k, dirs in enumerate(BOTH):
        x, sets, douts = conv_inputs(E, SB, Lq, [4], dtype, split, [dirs], 3 * Lq + k)
        conv_check(backend, x, sets[0], split, douts[0], tag="conv-walk")


@pytest.mark.parametrize("dtype", TYPES)
def test_conv1d_walk_is_deterministic(backend, dtype):
    """The walks case twice: dw and dbias (two workgroups' slots, folded in a fixed order) have identical bits."""
    x, sets, douts = conv_inputs(3, 11, 1000, [4], dtype, 4, [(0, 1)], 77)
    a = conv_check(backend, x, sets[0], 4, douts[0], tag="conv-walk")
    b = conv_check(backend, x, sets[0], 4, douts[0], tag="conv-walk")
    for u_, v_ in zip(a, b):
        assert torch.equal(u_, v_)


@pytest.mark.parametrize("dtype", TYPES)
def test_conv1d_zero_dout_workgroup(backend, dtype):
    """dout = 0 over the whole second backward workgroup of the walks case (virtual tile 32: row 10, positions 992 ..): its sums are
    exactly 0, it skips its slot store and the slot keeps its initial zero.  Then dout = 0 everywhere: dw, dbias and dx exactly 0."""
    E, SB, Lq, split = 3, 11, 1000, 4
    assert SB * 3 == BWD_WG + 1 and _bwd_slots(SB, Lq) == 2
    x, sets, douts = conv_inputs(E, SB, Lq, [4], dtype, split, [(1, 0)], 78)
    d = douts[0].clone()
    d[:, 10, 2 * TILE:] = 0
    conv_check(backend, x, sets[0], split, d, tag="conv-edge")
    _, dx, dw, db = conv_check(backend, x, sets[0], split, torch.zeros_like(d), tag="conv-edge")
    assert bool((dw == 0).all()) and bool((db == 0).all()) and bool((dx == 0).all())


# ---- taps -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", TYPES)
def test_conv1d_taps(backend, K, dtype):
    """Every tap count with and without a bias, vector (L = 504, two tiles) and scalar (L = 75) kernels, both directions."""
    for Lq in (504, 75):
        for k, bias in enumerate((False, True)):
            x, sets, douts = conv_inputs(3, 2, Lq, [K], dtype, 1, [BOTH[k]], 100 * K + Lq + k, bias=bias)
            conv_check(backend, x, sets[0], 1, douts[0], tag="conv-taps")


# ---- two parameter sets, the accumulate flag --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq", [1000, 1001], ids=["vector", "scalar"])
@pytest.mark.parametrize("dtype", TYPES)
def test_conv1d_two_sets_and_accumulate(backend, Lq, dtype):
    """mixer._conv_fwd2 / _conv_bwd2: two sets (K = 4 and 3) in opposite directions on one x, dx summed.  Then the C entry points with
    accumulate = 1 on a pre-filled dx, with one set and with two."""
    name, dev = backend
    E, SB, split = 2, 3, 2
    x, sets, douts = conv_inputs(E, SB, Lq, [4, 3], dtype, split, BOTH, 5 * Lq)
    xd = x.to(dev)
    params = [(w.to(dev), b.to(dev)) for w, b, _ in sets]
    dd = [d.to(dev) for d in douts]
    outs = mixer._conv_fwd2(xd, params, split, BOTH)
    dx = torch.empty_like(xd)
    grads = mixer._conv_bwd2(xd, params, dd, dx, split, BOTH)
    ref = conv_reference(x, sets, split, douts)
    for i in range(2):
        hold(name, "conv-2sets.out", outs[i], *ref["out"][i], dtype)
        hold(name, "conv-2sets.dw", grads[i][0], *ref["dw"][i], F32)
        hold(name, "conv-2sets.dbias", grads[i][1], *ref["db"][i], F32)
    hold(name, "conv-2sets.dx", dx, *ref["dx"], dtype)
    g = torch.Generator().manual_seed(9)
    addend = torch.randn(E, SB, Lq, generator=g).to(dtype)
    lib = L.get_lib()
    for n in (1, 2):
        dxa = addend.clone().to(dev)
        args = (L.Conv1dBwdArgs * n)()
        bufs = []
        for i in range(n):
            wf, bf = params[i]
            dw, db = torch.zeros_like(wf), torch.zeros_like(bf)
            stream = L.stream_and_check(xd, wf, bf, dd[i], dxa, dw, db)
            args[i] = L.Conv1dBwdArgs(L.ptr(xd), L.ptr(wf), L.ptr(bf), L.ptr(dd[i]), L.ptr(dxa), L.ptr(dw), L.ptr(db), SB, Lq, split, E,
                                      wf.shape[1], BOTH[i][0], BOTH[i][1], L.dtype_code(dtype), 1)
            bufs.append((dw, db))
        L.check(lib.cad_conv1d_bwd_multi(args, n, stream), "cad_conv1d_bwd_multi")
        ref = conv_reference(x, sets[:n], split, douts[:n], addend)
        hold(name, "conv-accumulate.dx", dxa, *ref["dx"], dtype)
        for i in range(n):
            hold(name, "conv-accumulate.dw", bufs[i][0], *ref["dw"][i], F32)
            hold(name, "conv-accumulate.dbias", bufs[i][1], *ref["db"][i], F32)


# ---- misaligned -------------------------------------------------------------------------------------------------------------------------
def _off1(t, dev):
    """A contiguous view one element into a larger buffer."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t.to(dev))
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("dtype", TYPES)
def test_conv1d_misaligned(backend, dtype):
    """x and dout one element into their buffers at L = 1000: the scalar kernels (see the header).  Same bounds; the forward equals the
    aligned (vector) call bit for bit."""
    name, dev = backend
    for k, dirs in enumerate(BOTH):
        x, sets, douts = conv_inputs(2, 3, 1000, [4], dtype, 1 + k, [dirs], 500 + k)
        mis = conv_check(backend, x, sets[0], 1 + k, douts[0], tag="conv-misaligned", xdev=_off1(x, dev), doutdev=_off1(douts[0], dev))
        ali = conv_check(backend, x, sets[0], 1 + k, douts[0], tag="conv")
        assert torch.equal(mis[0].float().cpu(), ali[0].float().cpu()), "the scalar and the vector forward differ"


# ---- edge values ------------------------------------------------------------------------------------------------------------------------
CONV_EDGES = ["zero-x", "zero-w", "pre20", "pre80", "pre100", "pre1e4", "subnormal-x"]
SUBNORMAL = {F32: (2.0 ** -140, 2.0 ** -126), BF: (2.0 ** -130, 2.0 ** -126), HF: (2.0 ** -20, 2.0 ** -14)}  # scale, smallest normal


@pytest.mark.parametrize("kind", CONV_EDGES)
@pytest.mark.parametrize("Lq", [1000, 75])
@pytest.mark.parametrize("dtype", TYPES)
def test_conv1d_edge_values(backend, kind, Lq, dtype):
    """pre<X>: x scaled so that pre reaches beyond +-X on both sides -- sigmoid saturation, the 1 - sigma cancellation (+20 and up), exp2
    overflow (below -88.7: -100 and -1e4; fp16 outputs beyond 65504 come out as inf where the fp64 value rounds to it)."""
    E, SB, split = 2, 3, 1 + (Lq == 75)
    seed = 1000 * CONV_EDGES.index(kind) + Lq
    for k, bias in enumerate((True, False)):
        xscale = float(kind[3:]) if kind.startswith("pre") else 1.0
        x, sets, douts = conv_inputs(E, SB, Lq, [4], dtype, split, [BOTH[k]], seed + k, bias=bias, xscale=xscale)
        w, b, dirs = sets[0]
        if kind == "zero-x":
            x = torch.zeros_like(x)
        elif kind == "zero-w":
            w = torch.zeros_like(w)
        elif kind == "subnormal-x":
            g = torch.Generator().manual_seed(seed)
            x = (SUBNORMAL[dtype][0] * torch.randn(E, SB, Lq, generator=g)).to(dtype)
            sub = (x != 0) & (x.double().abs() < SUBNORMAL[dtype][1])
            assert int(sub.sum()) > x.numel() // 2
        if kind.startswith("pre"):
            P = conv_reference(x, [(w, b, dirs)], split)["pre"][0]
            assert float(P.max()) > xscale and float(P.min()) < -xscale
        conv_check(backend, x, (w, b, dirs), split, douts[0], tag="conv-edge")  # (zero-x, zero-w: pre = b, out = silu(b))


# ---- non-finite containment -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("Lq", [1000, 1001], ids=["vector", "scalar"])
@pytest.mark.parametrize("dtype", TYPES)
def test_conv1d_nonfinite_is_contained(backend, K, Lq, dtype):
    """+inf mid-row and at the last position of a tile, NaN mid-row and at the first position of a tile; channel 2 and one row of each
    other channel are clean.  See the header for what is asserted."""
    name, dev = backend
    E, SB, split, dirs = 3, 3, 1, (0, 1)
    x, sets, douts = conv_inputs(E, SB, Lq, [K], dtype, split, [dirs], 40 + K)
    w, b, _ = sets[0]
    spots = [(0, 0, 300, float("inf")), (0, 2, TILE - 1, float("inf")), (1, 1, 700, float("nan")), (1, 2, TILE, float("nan"))]
    x0, xb = x.clone(), x.clone()
    keep_out, keep_dx = torch.ones(E, SB, Lq, dtype=torch.bool), torch.ones(E, SB, Lq, dtype=torch.bool)
    must = torch.zeros(E, SB, Lq, dtype=torch.bool)
    rev = _rev_rows(SB, split, dirs)
    for e, sb, p, v in spots:
        x0[e, sb, p], xb[e, sb, p] = 0.0, v
        keep_out[e, sb, max(0, p - 3): p + 4] = False
        keep_dx[e, sb, max(0, p - 6): p + 7] = False
        if bool(rev[sb]):
            must[e, sb, max(0, p - K + 1): p + 1] = True
        else:
            must[e, sb, p: p + K] = True
    ref = conv_reference(x0, sets, split, douts)
    xd = xb.clone().to(dev).requires_grad_(True)
    wd, bd = w.clone().to(dev).view(E, 1, K).requires_grad_(True), b.clone().to(dev).requires_grad_(True)
    out = ops.causal_conv1d(xd, wd, bd, split, *dirs)
    out.backward(douts[0].to(dev))
    oc, dxc = out.detach().cpu(), xd.grad.cpu()
    assert not bool(torch.isfinite(oc[must]).any()), "a finite output inside the causal window of a non-finite input"
    hold(name, "conv-nonfinite.out", oc[keep_out], ref["out"][0][0][keep_out], ref["out"][0][1][keep_out], dtype)
    hold(name, "conv-nonfinite.dx", dxc[keep_dx], ref["dx"][0][keep_dx], ref["dx"][1][keep_dx], dtype)
    hold(name, "conv-nonfinite.dw", wd.grad.view(E, K)[2], ref["dw"][0][0][2], ref["dw"][0][1][2], F32)
    hold(name, "conv-nonfinite.dbias", bd.grad[2:], ref["db"][0][0][2:], ref["db"][0][1][2:], F32)


# =========================================================================================================================================
# embedding
# =========================================================================================================================================
EMB_PAIRS = [pytest.param(F32, F32, id="f32-f32"), pytest.param(F32, BF, id="f32-bf16"), pytest.param(F32, HF, id="f32-f16"),
             pytest.param(BF, BF, id="bf16-bf16"), pytest.param(BF, F32, id="bf16-f32"), pytest.param(HF, HF, id="f16-f16")]
# (12, 320): the vector kernels with a second c4 trip;  (16, 512): 32 KB per table -- four of them do not fit, the scalar backward with a
# second column trip (forward: vector for an fp32 table);  (16, 50): the scalar kernels
EMB_SHAPES = [(12, 320), (16, 512), (16, 50)]


def emb_table(V, D, wdt, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(V, D, generator=g)
    W.view(-1)[:4] = torch.tensor([1e5, 1e-7, -0.0, -7e4])  # beyond fp16's range, an fp16 subnormal, a signed zero
    return W.to(wdt)


def emb_check(backend, ids, W, S, odt, seed=0, backward=True, tag="embed"):
    """ops.embed and autograd: the forward equal to the gather, the backward within the bound of the header."""
    name, dev = backend
    V, D = W.shape
    comp = COMP if V == 16 else COMP12
    wd = W.clone().to(dev).requires_grad_(backward)
    out = ops.embed(ids.to(dev), wd, comp.to(dev) if S == 2 else None, S, odt)
    idc = ids.clamp(0, V - 1)
    maps = [idc] + ([comp[idc]] if S == 2 else [])
    assert torch.equal(out.detach().cpu(), torch.stack([W[m] for m in maps]).to(odt)), f"{tag}: the forward is not the gather"
    if not backward:
        return
    g = torch.Generator().manual_seed(seed + 1)
    big = torch.where(torch.rand(S, *ids.shape, 1, generator=g) < 1 / 16, 1.0, 2.0 ** -12)
    dout = (big * (0.25 + torch.randn(S, *ids.shape, D, generator=g))).to(odt)
    out.backward(dout.to(dev))
    G = dout.double()
    ref, asum = torch.zeros(V, D, dtype=torch.float64), torch.zeros(V, D, dtype=torch.float64)
    cnt = torch.zeros(V, dtype=torch.float64)
    for s, m in enumerate(maps):
        ref.index_add_(0, m.reshape(-1), G[s].reshape(-1, D))
        asum.index_add_(0, m.reshape(-1), G[s].reshape(-1, D).abs())
        cnt += torch.bincount(m.reshape(-1), minlength=V).double()
    tol = gam(cnt + 2)[:, None] * asum + FLOOR[F32]
    if W.dtype != F32:
        tol = tol + UO[W.dtype] * (ref.abs() + tol) + FLOOR[W.dtype]
    got = wd.grad
    assert got.dtype == W.dtype
    hold(name, f"{tag}.dW", got, ref, tol, W.dtype)
    assert bool((got.cpu()[cnt == 0] == 0).all()), "a word that no token maps to has a non-zero gradient"


@pytest.mark.parametrize("V,D", EMB_SHAPES, ids=[f"V{v}-D{d}" for v, d in EMB_SHAPES])
@pytest.mark.parametrize("wdt,odt", EMB_PAIRS)
def test_embed_token_counts(backend, V, D, wdt, odt):
    """1 and 3 tokens: blocks with fewer tokens than waves; 255 / 256 / 257: one short of, exactly and one past the vector backward's
    block; 700: a ragged last block (and two blocks of the scalar backward).  Every type pair of cad_embed_fwd's dispatch; the backward's
    dout has the output's type."""
    for n in (1, 3, 255, 256, 257, 700):
        for S in (1, 2):
            g = torch.Generator().manual_seed(31 * n + S)
            ids = torch.randint(0, V, (1, n), generator=g)
            emb_check(backend, ids, emb_table(V, D, wdt, n + D), S, odt, seed=n + S)


@pytest.mark.parametrize("V,D", EMB_SHAPES, ids=[f"V{v}-D{d}" for v, d in EMB_SHAPES])
@pytest.mark.parametrize("pattern", ["one-id", "one-missing", "out-of-range"])
@pytest.mark.parametrize("odt", TYPES)
def test_embed_id_patterns(backend, V, D, pattern, odt):
    """one-id: every token the same word, the deepest single sum (every other row exactly 0);  one-missing: a word that never occurs
    (nor its complement);  out-of-range: ids -1 and V + 3 are clamped to 0 and V - 1, in the forward and in the backward alike."""
    n = 700
    g = torch.Generator().manual_seed(V + D)
    ids = torch.randint(0, V, (1, n), generator=g)
    comp = COMP if V == 16 else COMP12
    if pattern == "one-id":
        ids = torch.full((1, n), 7)
    elif pattern == "one-missing":
        ids[(ids == 8) | (ids == int(comp[8]))] = 2
    else:
        ids[0, ::5], ids[0, 1::7] = -1, V + 3
    for S in (1, 2):
        emb_check(backend, ids, emb_table(V, D, F32, D), S, odt, seed=S, tag="embed-ids")


@pytest.mark.parametrize("odt", TYPES)
def test_embed_forward_second_trip_vector(backend, odt):
    """32768 + 5 tokens at D = 4: the vector forward's 8192 workgroups of 4 waves cover 32768 tokens per trip, five waves take a second."""
    n = 8192 * 4 + 5
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 16, (1, n), generator=g)
    emb_check(backend, ids, emb_table(16, 4, F32, 4), 2, odt, tag="embed-stride")


@pytest.mark.parametrize("wdt,odt", [pytest.param(F32, F32, id="f32-f32")])
def test_embed_forward_second_trip_scalar(backend, wdt, odt):
    """16384 * 256 + 3 elements at D = 1: the scalar forward's 16384 workgroups of 256 threads cover 4194304 elements per trip, three
    threads take a second.  Forward only (the largest tensor of this file: 4 M elements)."""
    n = 16384 * 256 + 3
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 16, (1, n), generator=g)
    emb_check(backend, ids, emb_table(16, 1, wdt, 1), 1, odt, backward=False, tag="embed-stride")


def test_zz_report_worst_ratios(backend):
    """Prints the worst err / tol per output and type recorded by the tests above (run with -s to see it)."""
    name, dev = backend
    mine = {k: v for k, v in WORST.items() if k[0] == name and k[1].startswith(("conv", "embed"))}
    for (bk, key) in sorted(mine):
        print(f"[fp64 summary] {bk} {key}: {mine[(bk, key)]:.3f}")
    assert all(v <= 1.0 for v in mine.values())
