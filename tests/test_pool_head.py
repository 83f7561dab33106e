"""The pool head (csrc/pool.hip, cad_pool_head) held to float64, element by element: final add + norm and pooling over the sequence in
one pass, at the row counts where its chunk walk, its pieces and its combining launch start, at every width class and type pair, on
misaligned operands, at window edges and at edge values.

Reference and tolerances.  The reference starts from the inputs AS STORED and is torch.float64 throughout.  Per row, y and its bound
tol_y are test_norm_head_fp64.an_reference's "y" (derived there from how cad_add_norm_fwd rounds: statistics, v_rsq, scale, the rounding
to y_dtype); with weight NULL there is no norm, y = t = x + residual and tol_y = u |t| (0 without a residual).  The pooled bounds follow,
with nothing fitted (u = 2^-24, g(n) = n u / (1 - n u), the notation of that module):

  mean / window   out = (1 / n) sum_l c_l y_l over the m distinct rows of the window, c_l their multiplicities, n = sum c_l.
                  Perturbed terms:    sum c_l tol_y / n.
                  fp32 arithmetic:    a row with c_l > 1 costs one product (c_l is an exact fp32 integer, n < 2^24), the sum m - 1
                                      additions in ANY association order (waves, pieces, fused or not), the end one division by n, and n
                                      itself one rounding once L > 2^24: at most n + 2 roundings on any element's path, each relative to
                                      a partial sum bounded by sum c_l (|y_l| + tol_y):  g(n + 2) sum c_l (|y_l| + tol_y) / n.
                  Last rounding of a subnormal result: FLOOR[F32] = 2^-150.
  max             max is 1-Lipschitz in the sup norm and exact in fp32:  max_l tol_y.
Non-finite classes must match as in `hold`: a NaN row (a NaN or inf input under a norm makes its statistics NaN) contributes NaN to every
channel; without a norm a NaN or inf stays in its channel.

Geometry (csrc/pool.hip): the rows are walked from both ends at once, in chunks of cad_pool_head_chunk_rows rows (half of them from
either end), cad_pool_head_pieces pieces per (s, b) pair, at most 256; beyond 256 chunks a workgroup walks several chunks.
"""
import ctypes as C

import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops
from test_norm_head_fp64 import AN_TYPES, FLOOR, Arena, U, UO, an_inputs, an_reference, gam, hold  # noqa: F401

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
MODE = {"mean": L.POOL_MEAN, "max": L.POOL_MAX, "window": L.POOL_WINDOW}
EPS = 1e-5


def chunk_rows(D=256, dt=F32):
    return int(L.get_lib().cad_pool_head_chunk_rows(D, L.dtype_code(dt)))


def pool_direct(dev, off, x, res, w, b, is_rms, ydt, mode, centre=None, half=0, eps=EPS):
    """cad_pool_head on operands placed by an Arena (off = 1: one element into their buffers); sentinels around everything checked."""
    S, B, Lq, D = x.shape
    A = Arena(dev, off)
    lib = L.get_lib()
    xd, rd, wd, bd = A.put(x), A.put(res), A.put(w), A.put(b)
    cd = None if centre is None else centre.to(dev)
    out = A.put(shape=(S, B, D), dtype=F32)
    n = lib.cad_pool_head_scratch_floats(S, B, Lq, D, MODE[mode], half)
    assert n == S * B * D * lib.cad_pool_head_pieces(Lq, MODE[mode], half) and n > 0
    scratch = A.put(shape=(n,), dtype=F32)
    stream = L.stream_and_check(xd, rd, wd, bd, cd, out, scratch)
    a = L.PoolHeadArgs(L.ptr(xd), L.ptr(rd), L.ptr(wd), L.ptr(bd), L.ptr(cd), L.ptr(out), L.ptr(scratch), B, Lq, half, S, D, float(eps),
                       int(is_rms), L.dtype_code(x.dtype), L.dtype_code(ydt), MODE[mode])
    L.check(lib.cad_pool_head(C.byref(a), stream), "cad_pool_head")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    A.intact()
    return out.clone()


def rows_reference(x, res, w, b, is_rms, ydt, eps=EPS):
    """fp64 y (S, B, L, D) and tol_y of every row.  Rows with a non-finite input are NaN under a norm (their statistics are) and are
    kept out of an_reference, whose bound is void there."""
    S, B, Lq, D = x.shape
    if w is None:
        t = x.double()
        if res is None:
            return t, torch.zeros_like(t)
        t = t + res.double()
        return t, torch.nan_to_num(U * t.abs(), nan=0.0, posinf=0.0)
    tin = x.double() if res is None else x.double() + res.double()
    bad = ~torch.isfinite(tin).all(-1, keepdim=True)
    xs = torch.where(bad, torch.ones_like(x), x)
    rs = None if res is None else torch.where(bad, torch.zeros_like(res), res)
    y, tol = an_reference(xs.reshape(S, B * Lq, D), None if rs is None else rs.reshape(S, B * Lq, D), w, b, eps, is_rms, False, ydt)["y"]
    y, tol = y.reshape(S, B, Lq, D), tol.reshape(S, B, Lq, D)
    return torch.where(bad, torch.full_like(y, float("nan")), y), torch.where(bad, torch.zeros_like(tol), tol)


def window_index(centre, half, Lq):
    """(S, B, 2 half + 1) rows clamp(centre + k, 0, L - 1)."""
    k = torch.arange(-half, half + 1)
    return (centre.unsqueeze(-1) + k).clamp(0, Lq - 1)


def pool_reference(y, tol_y, mode, centre=None, half=0):
    """fp64 pooled value and its bound (header) from per-row y and tol_y."""
    S, B, Lq, D = y.shape
    if mode == "max":
        ref = y.max(2).values
        ref = torch.where(torch.isnan(y).any(2), torch.full_like(ref, float("nan")), ref)  # torch.max's NaN rule, stated outright
        return ref, tol_y.max(2).values
    if mode == "window":
        idx = window_index(centre, half, Lq).unsqueeze(-1).expand(S, B, 2 * half + 1, D)
        y, tol_y = y.gather(2, idx), tol_y.gather(2, idx)
    n = y.shape[2]
    mag = torch.where(torch.isfinite(y), y.abs(), torch.zeros_like(y)) + tol_y
    return y.sum(2) / n, tol_y.sum(2) / n + gam(n + 2) * mag.sum(2) / n + FLOOR[F32]


def check(backend, x, res, w, b, is_rms, ydt, modes=("mean", "max"), centre=None, half=0, off=0, tag="pool"):
    name, dev = backend
    y, tol_y = rows_reference(x, res, w, b, is_rms, ydt)
    outs = {}
    for mode in modes:
        kw = dict(centre=centre, half=half) if mode == "window" else {}
        out = pool_direct(dev, off, x, res, w, b, is_rms, ydt, mode, **kw)
        ref, tol = pool_reference(y, tol_y, mode, **kw)
        hold(name, f"{tag}.{mode}", out, ref, tol, F32)
        outs[mode] = out
    return outs


def inputs(S, B, Lq, D, xdt, ydt, has_res, has_bias, seed):
    x, res, w, b, _, _ = an_inputs(S, B * Lq, D, xdt, ydt, has_res, has_bias, seed, backward=False)
    return x.reshape(S, B, Lq, D), (None if res is None else res.reshape(S, B, Lq, D)), w, b


def centres(S, B, Lq):
    c = torch.tensor([0, Lq - 1, Lq // 2, -1, Lq + 5, 3], dtype=torch.int64)
    return c[:S * B].reshape(S, B)


# ---- widths, type pairs, norms, L on the chunk edges ------------------------------------------------------------------------------------
WIDTHS = [(40, None), (64, None), (256, None), (512, BF)]


@pytest.mark.parametrize("xdt,ydt", AN_TYPES)
@pytest.mark.parametrize("D,only", WIDTHS, ids=[f"D{d}" for d, _ in WIDTHS])
def test_pool_widths_types_chunk_edges(backend, D, only, xdt, ydt):
    """D 40 takes the scalar walk, 64 / 256 / 512 the vector walk with one and two 256-channel steps (512 in bf16 only).  L one below,
    at and one above a multiple of the chunk, and L = 1; RMSNorm and LayerNorm, with and without bias and residual; S 1 / 2, B 1 / 3."""
    if only is not None and ydt != only:
        return
    ch = chunk_rows(D, xdt)
    cases = [(True, True, False, 2, 3, 3 * ch - 1), (False, False, True, 1, 1, 3 * ch), (False, True, True, 2, 1, 3 * ch + 1),
             (True, False, True, 1, 3, 1), (False, True, False, 1, 1, ch + 1)]
    for k, (is_rms, has_res, has_bias, S, B, Lq) in enumerate(cases):
        x, res, w, b = inputs(S, B, Lq, D, xdt, ydt, has_res, has_bias, 31 * D + k)
        check(backend, x, res, w, b, is_rms, ydt, ("mean", "max", "window"), centres(S, B, Lq), 1 if Lq > 1 else 0)


WALK = [(40, F32, F32, 1, True), (256, BF, BF, 2, False), (64, F32, HF, 1, False)]


@pytest.mark.parametrize("D,xdt,ydt,S,is_rms", WALK, ids=[f"D{c[0]}-S{c[3]}" for c in WALK])
def test_pool_workgroup_walks_three_chunks(backend, D, xdt, ydt, S, is_rms):
    """The smallest L at which a workgroup walks three chunks: more than twice the pieces' maximum of chunks, ragged at the end."""
    lib = L.get_lib()
    ch = chunk_rows(D, xdt)
    pmax = int(lib.cad_pool_head_pieces(1 << 40, L.POOL_MEAN, 0))  # the cap on pieces
    Lq = 2 * pmax * ch + ch + 1
    pieces = int(lib.cad_pool_head_pieces(Lq, L.POOL_MEAN, 0))
    chunks = -(-Lq // ch)
    assert -(-chunks // pieces) == 3 and 1 < pieces <= pmax and Lq % ch == 1, (pieces, chunks)
    x, res, w, b = inputs(S, 1, Lq, D, xdt, ydt, True, not is_rms, 5 * D)
    check(backend, x, res, w, b, is_rms, ydt, ("mean", "max"), tag="pool-walk")


def test_pool_weight_null_pools_rows_as_they_are(backend):
    for k, (D, xdt, has_res) in enumerate([(64, BF, True), (40, F32, False), (256, HF, True)]):
        x, res, _, _ = inputs(2, 3, 35, D, xdt, xdt, has_res, False, 900 + k)
        check(backend, x, res, None, None, True, xdt, ("mean", "max", "window"), centres(2, 3, 35), 4, tag="pool-nonorm")


@pytest.mark.parametrize("D", [40, 64])
@pytest.mark.parametrize("xdt,ydt", AN_TYPES)
def test_pool_misaligned_operands(backend, D, xdt, ydt):
    """Every operand one element into its buffer: the scalar walk at both widths; nothing outside a view is written."""
    x, res, w, b = inputs(2, 2, 50, D, xdt, ydt, True, True, 77 + D)
    check(backend, x, res, w, b, False, ydt, ("mean", "max", "window"), centres(2, 2, 50), 3, off=1, tag="pool-misaligned")


# ---- window ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq,half", [(37, 0), (37, 1), (37, 40), (2000, 768), (1, 5)], ids=lambda v: str(v))
def test_pool_window_edges(backend, Lq, half):
    """Centres 0, L - 1, mid, -1, L + 5 and 3, a different one per (s, b); half 0 (a gather), 1, >= L (every weight on the two edge rows
    or on all rows), 768 at L 2000 (the VEP window, several pieces).  Then centres far outside, where the whole weight is on one end."""
    D = 64
    x, res, w, b = inputs(2, 3, Lq, D, BF, BF, True, False, 11 * Lq + half)
    check(backend, x, res, w, b, True, BF, ("window",), centres(2, 3, Lq), half, tag="pool-window")
    far = torch.tensor([[-2 ** 62, 2 ** 62, -Lq - half - 1], [Lq + half, -half, Lq - 1 + half]], dtype=torch.int64)
    out = check(backend, x, res, w, b, True, BF, ("window",), far, half, tag="pool-window-far")["window"]
    one = check(backend, x, res, w, b, True, BF, ("window",), torch.tensor([[0, Lq - 1, 0], [Lq - 1, 0, Lq - 1]]), 0)["window"]
    if half > 0 and Lq > 1:  # all 2 half + 1 offsets on one row: c y / c, within two roundings of the row itself
        sel = [(0, 0), (0, 1), (0, 2), (1, 0)]
        for s, bb in sel:
            assert torch.allclose(out[s, bb].cpu(), one[s, bb].cpu(), rtol=4 * U, atol=0), (s, bb)


# ---- edge values -----------------------------------------------------------------------------------------------------------------------------
def test_pool_nan_and_inf(backend):
    """Without a norm a NaN / +inf / -inf stays in its channel (mean and max; a window that misses the row is clean); under a norm the
    row's statistics are NaN and so is every channel of the pooled value."""
    name, dev = backend
    S, B, Lq, D = 1, 2, 40, 64
    for val in (float("nan"), float("inf"), float("-inf")):
        x, res, w, b = inputs(S, B, Lq, D, F32, F32, True, True, 5)
        x[0, 0, 17, 9] = val
        cen = torch.tensor([[30, 30]])
        outs = check(backend, x, res, None, None, True, F32, ("mean", "max", "window"), cen, 5, tag="pool-nonfinite")
        for mode in ("mean", "max"):
            o = outs[mode].cpu()
            fin = torch.isfinite(o)
            assert not bool(fin[0, 0, 9]) or (mode == "max" and val == float("-inf"))
            fin[0, 0, 9] = True
            assert bool(fin.all()), mode
        assert bool(torch.isfinite(outs["window"]).all())
        outs = check(backend, x, res, w, b, False, F32, ("mean", "max", "window"), cen, 5, tag="pool-nonfinite")
        assert bool(torch.isnan(outs["mean"][0, 0]).all()) and bool(torch.isnan(outs["max"][0, 0]).all())
        assert bool(torch.isfinite(outs["mean"][0, 1]).all()) and bool(torch.isfinite(outs["window"]).all())
    # +inf and -inf in one channel: the mean is NaN there, the max +inf
    x, res, _, _ = inputs(S, B, Lq, D, F32, F32, False, False, 6)
    x[0, 1, 3, 2], x[0, 1, 30, 2] = float("inf"), float("-inf")
    outs = check(backend, x, None, None, None, True, F32, tag="pool-nonfinite")
    assert bool(torch.isnan(outs["mean"][0, 1, 2])) and float(outs["max"][0, 1, 2]) == float("inf")


@pytest.mark.parametrize("xdt,ydt", AN_TYPES)
def test_pool_mean_1e3_and_subnormals(backend, xdt, ydt):
    """A row mean of 1e3 under LayerNorm (carried by the fp32 residual: the two-pass variance), and subnormal inputs."""
    g = torch.Generator().manual_seed(12)
    S, B, Lq, D = 2, 1, 33, 64
    w, b = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    x = (0.1 * torch.randn(S, B, Lq, D, generator=g)).to(xdt)
    res = 1e3 + 0.1 * torch.randn(S, B, Lq, D, generator=g)
    check(backend, x, res, w, b, False, ydt, ("mean", "max", "window"), centres(S, B, Lq), 2, tag="pool-mean1e3")
    tiny = (torch.randn(S, B, Lq, D, generator=g) * 2.0 ** -130)
    xs = tiny.to(xdt) if xdt != HF else (torch.randn(S, B, Lq, D, generator=g) * 2.0 ** -20).to(HF)  # binary16's subnormals
    for is_rms in (True, False):
        check(backend, xs, tiny, w, None if is_rms else b, is_rms, ydt, ("mean", "max", "window"), centres(S, B, Lq), 2, tag="pool-subnormal")
    check(backend, xs, tiny, None, None, True, ydt, ("mean", "max"), tag="pool-subnormal")


# ---- identities ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,xdt,ydt", [(64, BF, BF), (40, F32, F32), (256, F32, HF)])
def test_pool_row_bits_do_not_depend_on_neighbours_or_run(backend, D, xdt, ydt):
    name, dev = backend
    Lq = 4 * chunk_rows(D, xdt) + 3
    x, res, w, b = inputs(2, 3, Lq, D, xdt, ydt, True, True, 3 * D)
    cen = centres(2, 3, Lq)
    for mode in ("mean", "max", "window"):
        kw = dict(centre=cen, half=7) if mode == "window" else {}
        full = pool_direct(dev, 0, x, res, w, b, False, ydt, mode, **kw)
        again = pool_direct(dev, 0, x, res, w, b, False, ydt, mode, **kw)
        assert torch.equal(full.view(torch.int32), again.view(torch.int32)), mode
        for s, bb in ((0, 1), (1, 2)):
            kw1 = dict(centre=cen[s:s + 1, bb:bb + 1], half=7) if mode == "window" else {}
            alone = pool_direct(dev, 0, x[s:s + 1, bb:bb + 1], res[s:s + 1, bb:bb + 1], w, b, False, ydt, mode, **kw1)
            assert torch.equal(alone.view(torch.int32)[0, 0], full.view(torch.int32)[s, bb]), (mode, s, bb)


@pytest.mark.parametrize("D,xdt,ydt", [(64, BF, BF), (40, F32, F32), (256, F32, BF)])
def test_pool_bits_do_not_depend_on_the_direction_of_the_rows(backend, D, xdt, ydt):
    """Rows in the opposite order, centres mirrored to L - 1 - c: equal bits (what reverse-complementing an RCPS model's input does to a
    strand).  Even and odd row counts, clamped windows on both ends, several pieces."""
    name, dev = backend
    for Lq in (5 * chunk_rows(D, xdt) + 2, 5 * chunk_rows(D, xdt) + 3):
        x, res, w, b = inputs(2, 3, Lq, D, xdt, ydt, True, True, 3 * D + Lq)
        cen = centres(2, 3, Lq)
        for mode, half in (("mean", 0), ("max", 0), ("window", 0), ("window", 7), ("window", Lq // 2)):
            kw = dict(centre=cen, half=half) if mode == "window" else {}
            kwr = dict(centre=Lq - 1 - cen, half=half) if mode == "window" else {}
            fwd = pool_direct(dev, 0, x, res, w, b, False, ydt, mode, **kw)
            rev = pool_direct(dev, 0, x.flip(2).contiguous(), res.flip(2).contiguous(), w, b, False, ydt, mode, **kwr)
            assert torch.equal(fwd.view(torch.int32), rev.view(torch.int32)), (mode, half, Lq)


@pytest.mark.parametrize("D,xdt,ydt,is_rms", [(64, BF, BF, True), (40, F32, BF, False), (256, F32, F32, False), (512, BF, BF, True),
                                              (64, HF, HF, False)])
def test_pool_of_add_norm_fwd_own_rows(backend, D, xdt, ydt, is_rms):
    """Against the fp64 pooling of the y cad_add_norm_fwd itself stores.  On the emulator the head reproduces that kernel's row bits
    (same order, no fused multiply-adds), so only the summation term of the bound remains and max is exact; on the device the two
    translations may differ in a statistic's last bit ("Decode token") and tol_y applies to both sides."""
    name, dev = backend
    S, B, Lq = 2, 2, 3 * chunk_rows(D, xdt) + 5
    x, res, w, b = inputs(S, B, Lq, D, xdt, ydt, True, not is_rms, 17 * D)
    y, _ = ops.add_norm(x.to(dev), res.to(dev), w.to(dev), None if b is None else b.to(dev), EPS, is_rms, False, ydt)
    y = y.double().cpu()
    _, tol_y = rows_reference(x, res, w, b, is_rms, ydt)
    tol_y = torch.zeros_like(tol_y) if name == "emu" else 2 * tol_y
    cen = centres(S, B, Lq)
    for mode in ("mean", "max", "window"):
        kw = dict(centre=cen, half=9) if mode == "window" else {}
        out = pool_direct(dev, 0, x, res, w, b, is_rms, ydt, mode, **kw)
        ref, tol = pool_reference(y, tol_y, mode, **kw)
        hold(name, f"pool-own-rows.{mode}", out, ref, tol, F32)
        if name == "emu" and mode == "max":
            assert torch.equal(out.double().cpu(), ref)


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------
def test_pool_unsupported_arguments_return_before_a_launch(backend):
    """CAD_ERR_UNSUPPORTED (2) with `out` untouched; ops.pool_head raises PoolUnsupported, and refuses tensors that require grad."""
    name, dev = backend
    lib = L.get_lib()
    S, B, Lq = 1, 1, 8

    def call(D, xdt, ydt, mode, half, cen=True):
        x = torch.zeros(S, B, Lq, D, dtype=xdt, device=dev)
        w = torch.ones(D, device=dev)
        out = torch.full((S, B, D), -7.0, device=dev)
        scratch = torch.zeros(max(1, S * B * D * 4), device=dev)
        c = torch.zeros(S, B, dtype=torch.int64, device=dev) if cen else None
        a = L.PoolHeadArgs(L.ptr(x), None, L.ptr(w), None, L.ptr(c), L.ptr(out), L.ptr(scratch), B, Lq, half, S, D, EPS, 1,
                           L.dtype_code(xdt), L.dtype_code(ydt), mode)
        st = lib.cad_pool_head(C.byref(a), L.stream_and_check(x, w, out, scratch))
        if dev.type == "cuda":
            torch.cuda.synchronize()
        assert bool((out == -7.0).all()) or st == 0
        return st
    assert call(64, F32, F32, L.POOL_MEAN, 0) == 0
    assert call(1028, F32, F32, L.POOL_MEAN, 0) == 2
    assert call(64, BF, F32, L.POOL_MEAN, 0) == 2 and call(64, BF, HF, L.POOL_MAX, 0) == 2 and call(64, HF, BF, L.POOL_MAX, 0) == 2
    assert call(64, F32, F32, 3, 0) == 2 and call(64, F32, F32, -1, 0) == 2
    assert call(64, F32, F32, L.POOL_WINDOW, -1) == 2 and call(64, F32, F32, L.POOL_WINDOW, 1 << 22) == 2
    assert call(64, F32, F32, L.POOL_WINDOW, 0, cen=False) == 1  # a window without centres: a bad argument
    assert not lib.cad_pool_head_supported(0, 0, 0, 0, 0) and lib.cad_pool_head_supported(1024, 1, 1, 2, (1 << 22) - 1)
    x = torch.zeros(1, 1, 8, 1028, device=dev)
    with pytest.raises(ops.PoolUnsupported):
        ops.pool_head(x, None, torch.ones(1028, device=dev), None, EPS, True, F32, "mean")
    assert issubclass(ops.PoolUnsupported, ValueError)
    with pytest.raises(ops.PoolUnsupported):
        ops.pool_head(x[..., :64].contiguous().to(BF), None, None, None, EPS, True, F32, "max")
    with pytest.raises(ValueError):
        ops.pool_head(x[..., :64].contiguous(), None, None, None, EPS, True, F32, "median")
    with pytest.raises(TypeError):
        ops.pool_head(x[..., :64].contiguous(), None, None, None, EPS, True, F32, "window")
    wg = torch.ones(64, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="no backward"):
        ops.pool_head(x[..., :64].contiguous(), None, wg, None, EPS, True, F32, "mean")
    with torch.no_grad():
        out = ops.pool_head(x[..., :64].contiguous() + 1, None, wg, None, EPS, True, F32, "mean")
    assert out.shape == (1, 1, 64) and out.dtype == F32
