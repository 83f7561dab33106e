"""The opt-in fp16 kernels (CAD_F16): binary16 activations in HBM, fp32 arithmetic inside.  Every kernel family's fp16 entry point,
fed fp16-rounded inputs, against the fp32 oracle at an fp16 tolerance, and -- on the same inputs -- clearly more accurate than the
bf16 kernel (a bf16-internal shortcut would not be).  Runs on the emulator (CPU) and on the GPU."""
import ctypes

import numpy as np
import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops
from oracle import oracle_model as om
from test_kernels import SCAN_CASES, _ref_add_norm, _rows_oracle, _scan_inputs, leaf

F16 = torch.float16
F16_TOL = dict(rtol=4e-3, atol=4e-3)  # (the bf16 tests use 3e-2 / 5e-2)
ORDER = 3.0  # the fp16 error must be at least this many times below the bf16 kernel's error on the same inputs


def _err(got, ref):
    """max |got - ref| / max(1, max |ref|)"""
    ref = ref.detach().float().cpu()
    return float((got.detach().float().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def _check_order(e16, ebf, what):
    assert e16 * ORDER < ebf, f"{what}: fp16 error {e16:.3g} is not clearly below the bf16 error {ebf:.3g}"


def _special_values(n, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 20, (n,), generator=g).float())
    specials = torch.tensor([65504.0, 65519.99, 65520.0, 70000.0, 1e9, -65520.0, -1e30, float("inf"), float("-inf"), float("nan"),
                             -float("nan"), 0.0, -0.0, 6.0e-8, 2.98e-8, 2.9802322e-08, 1e-10, -3e-6, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,
                             2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 0.1, 1.0 / 3.0])
    v[:specials.numel()] = specials
    return v


@pytest.mark.parametrize("D", [48, 50])
def test_f16_conversion_bit_identical_to_torch(backend, D):
    """fp32 -> fp16 (embed forward, F32 weight -> F16 out; D = 48 the vector kernel's packed stores, D = 50 the scalar kernel): bit for
    bit torch's .to(float16) -- round to nearest even, subnormals, > 65504 -> inf (never saturated), +-inf, NaN stays NaN.
    fp16 -> fp32 (embed backward with F16 dout, each row gathered once): exact."""
    _, dev = backend
    V = 64
    W = _special_values(V * D, 3).view(V, D)
    ids = torch.arange(V).view(1, V)
    out = ops.embed(ids.to(dev), W.to(dev), None, 1, out_dtype=F16)
    assert out.dtype == F16
    want = W.to(F16)
    got = out[0, 0].cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16))
    assert torch.isinf(got).sum() >= 6  # the overflowing values became infinities, none saturated to 65504
    # widening: dW[v] = dout[v] exactly (0 + x in fp32)
    w = leaf(torch.zeros(V, D), dev)
    o = ops.embed(ids.to(dev), w, None, 1, out_dtype=F16)
    dout = _special_values(V * D, 4).view(1, 1, V, D).to(F16)
    o.backward(dout.to(dev))
    torch.testing.assert_close(w.grad.cpu(), dout[0, 0].float(), rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize("S,R,D,swap", [(2, 300, 256, 1), (1, 77, 128, 0), (2, 40, 50, 1)])
@pytest.mark.parametrize("xdt", [torch.float32, F16])
def test_add_norm_f16(backend, S, R, D, swap, xdt):
    """(x F32, y F16) -- the first layer's fp32 embedding -- and (F16, F16), with the strand swap; forward and backward."""
    _, dev = backend
    g = torch.Generator().manual_seed(1)
    x = torch.randn(S, R, D, generator=g).to(xdt).float()
    res = torch.randn(S, R, D, generator=g)
    w, dy = 1 + 0.1 * torch.randn(D, generator=g), torch.randn(S, R, D, generator=g)
    errs = {}
    for ydt in (F16, torch.bfloat16):
        xin = xdt if ydt == F16 or xdt == torch.float32 else torch.bfloat16
        ins = [leaf(x, dev, xin), leaf(res, dev), leaf(w, dev)]
        y, ro = ops.add_norm(ins[0], ins[1], ins[2], None, 1e-5, True, bool(swap), ydt)
        assert y.dtype == ydt
        (y.float() * dy.to(dev)).sum().backward()
        rins = [leaf(x, "cpu"), leaf(res, "cpu"), leaf(w, "cpu")]
        ry, rro = _ref_add_norm(rins[0], rins[1], rins[2], None, 1e-5, True, bool(swap))
        (ry * dy).sum().backward()
        errs[ydt] = [_err(y, ry), _err(ins[0].grad, rins[0].grad), _err(ins[1].grad, rins[1].grad)]
        if ydt == F16:
            torch.testing.assert_close(ro.cpu(), rro.detach(), rtol=1e-6, atol=1e-6)
            assert max(errs[ydt]) < 4e-3, errs[ydt]
            torch.testing.assert_close(ins[2].grad.cpu(), rins[2].grad, rtol=2e-3, atol=2e-3 * float(rins[2].grad.abs().max()))
    _check_order(errs[F16][0], errs[torch.bfloat16][0], "y")


@pytest.mark.parametrize("case", [(5, 2, 75, 4, 1, 0, 1), (4, 3, 2100, 3, 1, 0, 1), (6, 2, 4096, 4, 2, 1, 0)])
def test_causal_conv1d_f16(backend, case):
    name, dev = backend
    E, SB, L, K, split, rl, rh = case
    g = torch.Generator().manual_seed(5)
    x = torch.randn(E, SB, L, generator=g).to(F16).float()
    w, b = 0.5 * torch.randn(E, 1, K, generator=g), 0.2 * torch.randn(E, generator=g)
    dout = torch.randn(E, SB, L, generator=g)
    rx, rw, rb = leaf(x, "cpu"), leaf(w, "cpu"), leaf(b, "cpu")
    ref = _rows_oracle(lambda x_: om.causal_conv1d_silu(x_, rw.squeeze(1), rb), [rx], split, rl, rh)
    (ref * dout).sum().backward()
    errs = {}
    for dt in (F16, torch.bfloat16):
        ins = [leaf(x, dev, dt), leaf(w, dev), leaf(b, dev)]
        out = ops.causal_conv1d(*ins, split, rl, rh)
        assert out.dtype == dt
        (out.float() * dout.to(dev)).sum().backward()
        errs[dt] = (_err(out, ref), _err(ins[0].grad, rx.grad))
        if dt == F16:
            torch.testing.assert_close(out.float().cpu(), ref.detach(), **F16_TOL)
            torch.testing.assert_close(ins[0].grad.float().cpu(), rx.grad, **F16_TOL)
            torch.testing.assert_close(ins[1].grad.cpu(), rw.grad, rtol=4e-3, atol=4e-3 * max(1, L / 64))
            torch.testing.assert_close(ins[2].grad.cpu(), rb.grad, rtol=4e-3, atol=4e-3 * max(1, L / 64))
    _check_order(errs[F16][0], errs[torch.bfloat16][0], "conv out")
    _check_order(errs[F16][1], errs[torch.bfloat16][1], "conv dx")


def test_causal_conv1d_golden_f16(backend, golden_dir):
    _, dev = backend
    z = {k: torch.from_numpy(v) for k, v in np.load(f"{golden_dir}/conv_op.npz").items()}
    cm = lambda t: t.permute(1, 0, 2).contiguous()
    x16 = cm(z["x"]).to(F16)
    x, w, b = leaf(x16, dev), leaf(z["w"].unsqueeze(1), dev), leaf(z["b"], dev)
    out = ops.causal_conv1d(x, w, b, x.shape[1], 0, 0)
    assert out.dtype == F16
    torch.testing.assert_close(cm(out.detach().float().cpu()), z["out"], **F16_TOL)
    (out.float() * cm(z["dout"]).to(dev)).sum().backward()
    torch.testing.assert_close(cm(x.grad.float().cpu()), z["dx"], **F16_TOL)
    torch.testing.assert_close(w.grad.cpu().squeeze(1), z["dw"], rtol=4e-3, atol=4e-3 * max(1.0, float(z["dw"].abs().max())))


def _scan_errs(dev, t, case, dt):
    E, SB, L, N, split, rl, rh = case
    order = ("u", "delta", "A", "B", "C", "D", "z", "bias")
    act = {"u", "delta", "B", "C", "z"}
    ins = [leaf(t[k], dev, dt if k in act else torch.float32) for k in order]
    out = ops.selective_scan(*ins, split, rl, rh)
    assert out.dtype == dt
    (out.float() * t["w"].to(dev)).sum().backward()
    return out, ins


@pytest.mark.parametrize("case", SCAN_CASES)
def test_selective_scan_f16(backend, case):
    """Forward + backward (generic / unrolled d_state 16 / tails, both directions) against the fp32 oracle on fp16-rounded inputs, and
    the output's and the activation gradients' errors clearly below the bf16 kernel's.  (dB / dC pass through the bf16 partial slots
    by design -- include/caduceus_hip.h, cad_scan_bwd -- and are held to the fp16 tolerance only.)"""
    _, dev = backend
    E, SB, L, N, split, rl, rh = case
    t = _scan_inputs(E, SB, L, N, 11, dev, F16)
    order = ("u", "delta", "A", "B", "C", "D", "z", "bias")
    ref_ins = [leaf(t[k], "cpu") for k in order]
    u, d, A, B, C, D, z, b = ref_ins
    ref = _rows_oracle(lambda u_, d_, B_, C_, z_: om.selective_scan(u_, d_, A, B_, C_, D, z_, b), [u, d, B, C, z], split, rl, rh)
    (ref * t["w"]).sum().backward()
    out, ins = _scan_errs(dev, t, case, F16)
    outb, insb = _scan_errs(dev, t, case, torch.bfloat16)
    torch.testing.assert_close(out.float().cpu(), ref.detach(), **F16_TOL)
    e16, ebf = [_err(out, ref)], [_err(outb, ref)]
    for k, a, ab, r in zip(order, ins, insb, ref_ins):
        scale = max(1.0, float(r.grad.abs().max()))
        torch.testing.assert_close(a.grad.float().cpu(), r.grad, rtol=F16_TOL["rtol"], atol=F16_TOL["atol"] * scale,
                                   msg=lambda m, k=k: f"d{k}: {m}")
        if k in ("u", "delta", "z"):
            e16.append(_err(a.grad, r.grad))
            ebf.append(_err(ab.grad, r.grad))
    if L >= 64:  # (a handful of values: both errors are at the rounding of a few numbers)
        _check_order(max(e16), max(ebf), "scan outputs / activation gradients")


@pytest.mark.parametrize("shape", ["1x64x64x16", "2x32x200x16", "1x16x37x8"])
def test_selective_scan_golden_f16(backend, shape, golden_dir):
    _, dev = backend
    z = {k: torch.from_numpy(v) for k, v in np.load(f"{golden_dir}/scan_op_{shape}.npz").items()}
    cm = lambda t: t.permute(1, 0, 2).contiguous()
    act = [cm(z["u"]), cm(z["delta"]), cm(z["B"]), cm(z["C"]), cm(z["z"])]
    rounded = [a.to(F16).float() for a in act]
    errs = {}
    for dt in (F16, torch.bfloat16):
        ins = [leaf(t, dev, dt) for t in rounded]
        u, d, B, C, zz = ins
        A, D, bias = leaf(z["A"], dev), leaf(z["D"], dev), leaf(z["delta_bias"], dev)
        out = ops.selective_scan(u, d, A, B, C, D, zz, bias, u.shape[1], 0, 0)
        (out.float() * cm(z["dout"]).to(dev)).sum().backward()
        got = {"out": cm(out.detach().float().cpu()), "du": cm(u.grad.float().cpu()), "ddelta": cm(d.grad.float().cpu()),
               "dB": cm(B.grad.float().cpu()), "dC": cm(C.grad.float().cpu()), "dz": cm(zz.grad.float().cpu()),
               "dA": A.grad.cpu(), "dD": D.grad.cpu(), "ddelta_bias": bias.grad.cpu()}
        errs[dt] = {k: _err(v, z[k]) for k, v in got.items()}
        if dt == F16:
            for k, v in got.items():  # (the golden vectors are the fp32 inputs: the fp16 rounding of the inputs is part of the error)
                torch.testing.assert_close(v, z[k], rtol=1e-2, atol=1e-2 * max(1.0, float(z[k].abs().max())), msg=lambda m, k=k: f"{k}: {m}")
    order_keys = ("out", "du", "ddelta", "dz")  # (dB / dC: the bf16 partial slots, see test_selective_scan_f16)
    assert max(errs[F16][k] for k in order_keys) * ORDER < max(errs[torch.bfloat16][k] for k in order_keys), errs


@pytest.mark.parametrize("cut", [300, 512])
def test_scan_carries_f16(backend, cut):
    """h0 / hT / dhT / dh0 in fp16 mode: a row scanned as two chained segments equals the row scanned at once."""
    _scan_carries_f16(backend, cut, "suite")


@pytest.mark.parametrize("cut", [300, 512])
def test_scan_carries_f16_long_memory(backend, cut):
    """... with inputs whose state outlives the cut (regime "long_memory" of test_kernels._scan_inputs)."""
    _scan_carries_f16(backend, cut, "long_memory")


def _scan_carries_f16(backend, cut, regime):
    _, dev = backend
    E, SB, L, N = 5, 1, 1100, 16
    t = _scan_inputs(E, SB, L, N, 31, dev, F16, regime)
    order = ("u", "delta", "A", "B", "C", "D", "z", "bias")
    act = {"u", "delta", "B", "C", "z"}
    mk = lambda: [leaf(t[k], dev, F16 if k in act else torch.float32) for k in order]
    w = t["w"].to(dev)
    ref_in = mk()
    ref = ops.selective_scan(*ref_in, 1, 0, 0)
    (ref.float() * w).sum().backward()
    ins = mk()
    u, d, A, B, C, D, z, b = ins
    f = lambda x, s: x[..., s]
    lo, hi = slice(0, cut), slice(cut, L)
    o1, h = ops.selective_scan_stateful(f(u, lo), f(d, lo), A, f(B, lo), f(C, lo), D, f(z, lo), b, None, 1, 0, 0)
    o2, _ = ops.selective_scan_stateful(f(u, hi), f(d, hi), A, f(B, hi), f(C, hi), D, f(z, hi), b, h, 1, 0, 0)
    out = torch.cat([o1, o2], -1)
    assert out.dtype == F16
    (out.float() * w).sum().backward()
    torch.testing.assert_close(out.float(), ref.float(), **F16_TOL)
    for k, a_, r_ in zip(order, ins, ref_in):
        scale = max(1.0, float(r_.grad.abs().max()))
        torch.testing.assert_close(a_.grad.float(), r_.grad.float(), rtol=4e-3, atol=4e-3 * scale, msg=lambda m, k=k: f"d{k}: {m}")


@pytest.mark.parametrize("n,npart", [(4096, 16), (1000, 3)])
def test_reduce_partials_f16_destination(backend, n, npart):
    """cad_reduce_partials(_multi) with an F16 destination read bf16 slots (the scan backward's fp16-mode dB / dC slots, whose sums may
    exceed binary16's range before the fold): one fp32 sum rounded once, bit-identical between the single and the multi fold."""
    _, dev = backend
    lib = L.get_lib()
    g = torch.Generator().manual_seed(3)
    src = [(torch.randn(npart, n, generator=g) * 1000).to(torch.bfloat16).to(dev) for _ in range(2)]
    src[0][0, :4] = 60000.0  # (two of these overflow binary16, the sum of them does not fit either: +inf)
    dst = [torch.empty(n, dtype=F16, device=dev) for _ in range(2)]
    stream = L.stream_and_check(*src, *dst)
    for s, d in zip(src, dst):
        L.check(lib.cad_reduce_partials(L.ptr(s), npart, n, L.ptr(d), L.CAD_F16, stream), "cad_reduce_partials")
    for s, d in zip(src, dst):
        want = s.cpu().double().sum(0).float()
        torch.testing.assert_close(d.float().cpu(), want.to(F16).float(), rtol=1e-3, atol=1e-2)
    multi = [torch.empty(n, dtype=F16, device=dev) for _ in range(2)]
    jobs = (L.ReduceJob * 2)(*[L.ReduceJob(L.ptr(s), L.ptr(m)) for s, m in zip(src, multi)])
    L.check(lib.cad_reduce_partials_multi(jobs, 2, npart, n, L.CAD_F16, stream), "cad_reduce_partials_multi")
    for a, b in zip(dst, multi):
        assert torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("n_strands", [1, 2])
@pytest.mark.parametrize("V,D,B,L", [(16, 40, 2, 300), (16, 256, 2, 301), (12, 128, 1, 75), (16, 512, 1, 200)])
def test_lm_head_f16_hidden(backend, n_strands, V, D, B, L):
    """LM head + loss with fp16 hidden states (logits stay fp32): general kernel, matrix-core kernel, two-launch backward."""
    name, dev = backend
    g = torch.Generator().manual_seed(2)
    comp = torch.tensor([0, 1, 2, 3, 4, 5, 6, 10, 9, 8, 7, 11, 12, 13, 14, 15])[:V]
    W = torch.randn(V, D, generator=g)
    h = torch.randn(n_strands, B, L, D, generator=g).to(F16).float()
    labels = torch.randint(0, V, (B, L), generator=g)
    labels[torch.rand(B, L, generator=g) < 0.8] = 4
    hd, wd = leaf(h, dev, F16), leaf(W, dev)
    logits, loss = ops.lm_head(hd, wd, comp.to(dev) if n_strands == 2 else None, labels.to(dev), 4)
    assert logits.dtype == torch.float32
    (loss + 0.01 * logits.square().mean()).backward()
    rh, rw = leaf(h, "cpu"), leaf(W, "cpu")
    rl = torch.nn.functional.linear(rh[0], rw) + (torch.nn.functional.linear(rh[1], rw[comp]) if n_strands == 2 else 0)
    rloss = om.cross_entropy(rl, labels, 4)
    (rloss + 0.01 * rl.square().mean()).backward()
    torch.testing.assert_close(logits.cpu(), rl.detach(), rtol=6e-4, atol=2e-3)
    torch.testing.assert_close(loss.cpu(), rloss.detach(), rtol=6e-4, atol=2e-3)
    assert hd.grad.dtype == F16
    torch.testing.assert_close(hd.grad.float().cpu(), rh.grad, rtol=4e-3, atol=4e-3 * max(1.0, float(rh.grad.abs().max())))
    torch.testing.assert_close(wd.grad.cpu(), rw.grad, rtol=2e-3, atol=2e-3)


# ---- the MFMA projections (csrc/gemm_f16.hip on the headers of csrc/gemm.hip): each mode against an fp32 product of the same fp16 operands ----------------------------------
def _operands(shapes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(scale * torch.randn(*s, generator=g)).to(F16).float() for s in shapes]


def _both(fn, ops_in, dev):
    """fn(*operands in dt) for dt = fp16 and bf16 (the same fp16-rounded values, rounded again to bf16 for the bf16 kernel)."""
    return {dt: fn(*[o.to(dev).to(dt) for o in ops_in]) for dt in (F16, torch.bfloat16)}


def _proj_check(res, ref, what, tol=3e-3):
    got = res[F16]
    got = got if isinstance(got, torch.Tensor) else got
    assert got.dtype in (F16, torch.float32), got.dtype
    e16, ebf = _err(got, ref), _err(res[torch.bfloat16], ref)
    assert e16 < tol, (what, e16)
    _check_order(e16, ebf, what)


@pytest.mark.parametrize("M,K,T", [(512, 256, 1000), (1024, 512, 256), (100, 64, 77)])
def test_proj_wxT_f16(backend, M, K, T):
    _, dev = backend
    W, X = _operands([(M, K), (T, K)], 1, 0.1)
    res = _both(lambda w, x: ops.proj_wxT(w, x), [W, X], dev)
    assert res[F16].dtype == F16
    _proj_check(res, W @ X.t(), "proj_wxT")


def test_proj_wx_f16_thin_k_softplus_and_addend(backend):
    """dt_proj (thin K, softplus + bias epilogue, fp32) and the x_proj input gradient (thin K with the addend, one rounding)."""
    _, dev = backend
    M, K, T = 512, 16, 1024
    W, X, Acc = _operands([(M, K), (K, T), (M, T)], 2, 0.5)
    bias = torch.randn(M, generator=torch.Generator().manual_seed(9)) - 3.0
    res = _both(lambda w, x: ops.proj_wx(w, x, softplus_bias=bias.to(dev)), [W, X], dev)
    assert res[F16].dtype == F16
    _proj_check(res, torch.nn.functional.softplus(W @ X + bias[:, None]), "proj_wx softplus")
    res = _both(lambda w, x, a: ops.proj_wx(w, x, acc=a), [W, X, Acc], dev)
    _proj_check(res, W @ X + Acc, "proj_wx acc")


@pytest.mark.parametrize("M,K", [(48, 512), (40, 1024)])
def test_proj_wx_f16_thin_m_deep_k(backend, M, K):
    """x_proj (thin M, deep K), and at K = 1024 the two K halves with the first as the addend of the second."""
    _, dev = backend
    T = 640
    W, X = _operands([(M, K), (K, T)], 3, 0.1)

    def run(w, x):
        if K <= 512:
            return ops.proj_wx(w, x)
        out = ops.proj_wx(w[:, :K // 2].contiguous(), x[:K // 2])
        return ops.proj_wx(w[:, K // 2:].contiguous(), x[K // 2:], out=out, acc=out)
    res = _both(run, [W, X], dev)
    assert res[F16].dtype == F16
    _proj_check(res, W @ X, "proj_wx thin-M")


@pytest.mark.parametrize("M,K", [(16, 256), (32, 512)])
def test_proj_wx_wgrad_f16(backend, M, K):
    """d(dt_lr) = W_dt^T d(delta) and dW_dt from one pass (cad_proj_wx_wgrad_f16), and the weight-gradient-only form."""
    _, dev = backend
    T = 1024
    W, X, Y = _operands([(M, K), (K, T), (M, T)], 4, 0.5)
    res = _both(lambda w, x, y: ops.proj_wx_wgrad(w, x, y), [W, X, Y], dev)
    _proj_check({k: v[0] for k, v in res.items()}, W @ X, "proj_wx_wgrad out")
    _proj_check({k: v[1] for k, v in res.items()}, X @ Y.t(), "proj_wx_wgrad dW")
    res = _both(lambda x, y: ops.proj_wgrad_only(x, y), [X, Y], dev)
    _proj_check(res, Y @ X.t(), "proj_wgrad_only")


@pytest.mark.parametrize("M,K", [(256, 512), (128, 256)])
def test_proj_xTw_f16(backend, M, K):
    """out_proj on both directions' scan outputs: token-major fp16 result of X^T W^T + X2^T W^T (one fp32 accumulation)."""
    _, dev = backend
    T = 520
    W, X, X2 = _operands([(M, K), (K, T), (K, T)], 5, 0.1)
    res = _both(lambda w, x, x2: ops.proj_xTw(w, x, x2), [W, X, X2], dev)
    assert res[F16].dtype == F16
    _proj_check(res, (X + X2).t() @ W.t(), "proj_xTw")


def test_gemm_stream_f16(backend):
    """cad_gemm_stream_f16: the fp32 partial tiles of a weight gradient (K split over all tokens) and the token-major fp16 product."""
    _, dev = backend
    M, N, T = 256, 256, 2048
    A, B = _operands([(M, T), (T, N)], 6, 0.1)
    res = _both(lambda a, b: ops.wgrad_cm_tm(a, b), [A, B], dev)
    assert res[F16] is not None and res[F16].dtype == torch.float32
    _proj_check(res, A @ B, "gemm_stream partials")
    Wt, X = _operands([(256, 512), (512, T)], 7, 0.1)
    res = _both(lambda w, x: ops.proj_xTw_stream(w, x), [Wt, X], dev)
    assert res[F16] is not None and res[F16].dtype == F16
    _proj_check(res, X.t() @ Wt.t(), "gemm_stream out_t")


def test_proj_f16_overflow_is_inf_not_saturated(backend):
    """A product beyond 65504 rounds to +-inf in the fp16 epilogue (GradScaler depends on seeing it), a NaN operand stays NaN."""
    _, dev = backend
    W = torch.full((128, 32), 64.0)
    X = torch.full((64, 32), 64.0)
    X[1] = -64.0
    X[2, 0] = float("nan")
    out = ops.proj_wxT(W.to(dev).to(F16), X.to(dev).to(F16)).cpu()
    assert torch.isposinf(out[:, 0]).all() and torch.isneginf(out[:, 1]).all() and torch.isnan(out[:, 2]).all()


def test_mixed_projection_operands_are_refused(backend):
    _, dev = backend
    W = torch.randn(128, 64).to(dev)
    with pytest.raises(TypeError):
        ops.proj_wxT(W.to(F16), W.to(torch.bfloat16))
