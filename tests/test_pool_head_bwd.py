"""The pool head's backward (csrc/pool_bwd.hip, cad_pool_head_bwd / cad_pool_head_max_rows, ops.pool_head_grad) held to float64, element
by element: dx, dres_in, dweight and dbias at the row counts where its chunk walk and its pieces start, at every width class and type pair,
on misaligned operands, at window edges, with ties and NaN rows under MAX; then the identities (row exchange, run to run, neighbours,
forward bits).

Reference and tolerances.  The kernel forms the gradient of a row's normed value as
    dy[s,b,r,c] = m(r) * (g[s,b,c] / n)        MEAN / WINDOW: one IEEE fp32 division, one rounded product with the exact integer m(r)
    dy[s,b,r,c] = g[s,b,c] if r == rows[s,b,c] else 0        MAX
and then follows cad_add_norm_bwd's sequence.  `dy32` below restates these two operations in torch fp32 on the CPU (tensor / tensor, so that
the division is a division, and tensor * tensor): it has the kernel's bits, so it enters test_norm_head_fp64.an_reference as the dy "as
stored", and that reference's dx / dres_in / dweight / dbias bounds apply as they stand (dro = None).  Nothing is fitted.  With weight NULL
there is no norm: dres_in must equal dy32 and dx its rounding to x_dtype, exactly.  Rows outside a window must be exactly 0.

MAX.  rows[s,b,c] is the lowest row whose recomputed y has the bits of out[s,b,c].  The fp64 reference cannot recompute bits, so: (1) the
row the kernel reports must attain the maximum within tol_y of that row (|y64[row] - out| <= tol_y) and lie inside [0, L); (2) with an fp32
y (no rounding ties between distinct rows) it must be the first argmax of the fp64 rows, also where rows are duplicated on purpose (equal
inputs give equal fp64 and equal fp32 rows, so the tie is certain on both sides and the lowest must win); (3) the routing is asserted
directly as a count: without a norm dx is dy, so exactly one row per channel is non-zero; under a norm a routed row's dx is dense, so the
rows of a pair with a non-zero dx are exactly the distinct rows reported for it; (4) dx and the sums are held to the bound with dy32 routed
to the reported rows.
"""
import ctypes as C

import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops
from test_norm_head_fp64 import AN_TYPES, Arena, an_reference, hold
from test_pool_head import EPS, MODE, centres, inputs, pool_direct, rows_reference, window_index

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


def grad_of(S, B, D, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return 0.25 + torch.randn(S, B, D, generator=g)


def bwd_direct(dev, off, x, res, w, b, is_rms, ydt, mode, g, centre=None, half=0, want=(True, True), eps=EPS):
    """cad_pool_head_bwd on operands and outputs placed by an Arena (off = 1: one element into their buffers; the scratch and the int64
    rows are 8-byte aligned by contract); sentinels around everything checked.  For MAX the forward's out comes from cad_pool_head on
    equally placed operands."""
    S, B, Lq, D = x.shape
    lib = L.get_lib()
    out = pool_direct(dev, off, x, res, w, b, is_rms, ydt, mode, centre, half, eps) if mode == "max" else None
    A, A0 = Arena(dev, off), Arena(dev, 0)
    xd, rd, wd, bd, gd, od = A.put(x), A.put(res), A.put(w), A.put(b), A.put(g), A.put(out)
    cd = None if centre is None or mode != "window" else centre.to(dev)
    dx = A.put(shape=x.shape, dtype=x.dtype)
    dri = None if res is None else A.put(shape=x.shape, dtype=F32)
    dw = A.put(shape=(D,), dtype=F32) if w is not None and want[0] else None
    db = A.put(shape=(D,), dtype=F32) if b is not None and want[1] else None
    rows = A0.put(shape=(S, B, D), dtype=torch.int64) if mode == "max" else None
    n = lib.cad_pool_head_bwd_scratch_floats(S, B, Lq, D, MODE[mode], half)
    assert n == 2 * S * B * D * lib.cad_pool_head_bwd_pieces(Lq) and n > 0
    scratch = A0.put(shape=(n,), dtype=F32)
    stream = L.stream_and_check(xd, rd, wd, bd, cd, gd, od, dx, dri, dw, db, rows, scratch)
    a = L.PoolHeadBwdArgs(L.ptr(xd), L.ptr(rd), L.ptr(wd), L.ptr(bd), L.ptr(cd), L.ptr(gd), L.ptr(od), L.ptr(dx), L.ptr(dri), L.ptr(dw),
                          L.ptr(db), L.ptr(rows), L.ptr(scratch), B, Lq, half if mode == "window" else 0, S, D, float(eps), int(is_rms),
                          L.dtype_code(x.dtype), L.dtype_code(ydt), MODE[mode])
    L.check(lib.cad_pool_head_bwd(C.byref(a), stream), "cad_pool_head_bwd")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    A.intact()
    A0.intact()

    def host(t):
        return None if t is None else t.clone().cpu()
    return {"dx": host(dx), "dres_in": host(dri), "dweight": host(dw), "dbias": host(db), "rows": host(rows), "out": host(out)}


def multiplicity(S, B, Lq, mode, centre, half):
    """m(r) (S, B, L) fp32: how many of the window's offsets land on row r (1 everywhere for mean), and n."""
    if mode != "window":
        return torch.ones(S, B, Lq), Lq
    idx = window_index(centre, half, Lq)
    m = torch.zeros(S, B, Lq).scatter_add_(2, idx, torch.ones(idx.shape))
    return m, 2 * half + 1


def dy32_of(g, S, B, Lq, D, mode, centre=None, half=0, rows=None):
    """The kernel's dy restated in torch fp32 (module docstring)."""
    if mode == "max":
        hot = torch.arange(Lq).view(1, 1, Lq, 1) == rows.view(S, B, 1, D)
        return torch.where(hot, g.view(S, B, 1, D).expand(S, B, Lq, D), torch.zeros(()))
    m, n = multiplicity(S, B, Lq, mode, centre, half)
    gd = g / torch.full_like(g, float(n))
    return gd.view(S, B, 1, D) * m.view(S, B, Lq, 1)


def check_rows(name, x, res, w, b, is_rms, ydt, got, tag):
    """MAX: the reported rows attain the maximum (module docstring, (1) and (2))."""
    S, B, Lq, D = x.shape
    rows, out = got["rows"], got["out"].double()
    assert bool(((rows >= 0) & (rows < Lq)).all()), f"{tag}: a row outside [0, L)"
    y, tol_y = rows_reference(x, res, w, b, is_rms, ydt)
    at = rows.view(S, B, 1, D)
    assert bool(((y.gather(2, at).view(S, B, D) - out).abs() <= tol_y.gather(2, at).view(S, B, D)).all()), f"{tag}: the row does not attain out"
    if ydt == F32:
        first = (y == y.max(2, keepdim=True).values).int().argmax(2)
        assert torch.equal(first, rows), f"{tag}: not the lowest row of the maximum"


def check(backend, x, res, w, b, is_rms, ydt, modes=("mean", "max"), centre=None, half=0, off=0, seed=0, tag="pool-bwd"):
    name, dev = backend
    S, B, Lq, D = x.shape
    g = grad_of(S, B, D, seed)
    outs = {}
    for mode in modes:
        kw = dict(centre=centre, half=half) if mode == "window" else {}
        got = bwd_direct(dev, off, x, res, w, b, is_rms, ydt, mode, g, **kw)
        if mode == "max":
            check_rows(name, x, res, w, b, is_rms, ydt, got, f"{tag}.{mode}")
        dy32 = dy32_of(g, S, B, Lq, D, mode, rows=got["rows"], **kw)
        if mode == "window":  # rows outside the window: exact zeros, written
            outside = multiplicity(S, B, Lq, mode, centre, half)[0] == 0
            assert bool((got["dx"][outside] == 0).all()) and (res is None or bool((got["dres_in"][outside] == 0).all())), tag
        if mode == "max":  # the rows with a non-zero gradient are the reported ones and no others (g != 0 everywhere)
            nz = (got["dx"].float() != 0).any(-1)  # (S, B, L)
            routed = torch.zeros(S, B, Lq, dtype=torch.bool).scatter_(2, got["rows"], torch.ones(S, B, D, dtype=torch.bool))
            assert torch.equal(nz, routed), f"{tag}: gradient on a row MAX did not choose"
        if w is None:
            assert torch.equal(got["dx"], dy32.to(x.dtype)), f"{tag}.{mode}: dx is not dy"
            assert res is None or torch.equal(got["dres_in"], dy32), f"{tag}.{mode}: dres_in is not dy"
            if mode == "max":
                assert bool(((got["dx"].float() != 0).sum(2) == (g != 0).to(torch.int64)).all()), f"{tag}: not one row per channel"
        else:
            ref = an_reference(x.reshape(S, B * Lq, D), None if res is None else res.reshape(S, B * Lq, D), w, b, EPS, is_rms, False, ydt,
                               dy=dy32.reshape(S, B * Lq, D), dro=None)
            hold(name, f"{tag}.{mode}.dx", got["dx"], *ref["dx"], x.dtype)
            if res is not None:
                hold(name, f"{tag}.{mode}.dres_in", got["dres_in"], *ref["dres_in"], F32)
            hold(name, f"{tag}.{mode}.dweight", got["dweight"], *ref["dweight"], F32)
            if b is not None:
                hold(name, f"{tag}.{mode}.dbias", got["dbias"], *ref["dbias"], F32)
        outs[mode] = got
    return outs


# ---- chunk and piece edges, widths, type pairs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdt,ydt", AN_TYPES)
@pytest.mark.parametrize("D", [64, 260])
def test_bwd_types_and_chunk_edges(backend, D, xdt, ydt):
    """The five type pairs at a vector width and a scalar one; L on both sides of the 16-row chunk and of one row; RMSNorm and LayerNorm
    with bias, with and without residual; S 1 / 2, B 1 / 3."""
    cases = [(True, True, False, 2, 3, 15), (False, False, True, 1, 1, 16), (False, True, True, 2, 1, 17), (True, False, False, 1, 3, 1),
             (False, True, True, 1, 1, 2), (True, True, False, 2, 1, 33)]
    for k, (is_rms, has_res, has_bias, S, B, Lq) in enumerate(cases):
        x, res, w, b = inputs(S, B, Lq, D, xdt, ydt, has_res, has_bias, 31 * D + k)
        check(backend, x, res, w, b, is_rms, ydt, ("mean", "max", "window"), centres(S, B, Lq), 1 if Lq > 1 else 0, seed=k)


WIDTHS = [(40, F32, F32), (256, BF, BF), (512, F32, BF), (516, HF, HF), (1024, BF, BF)]


@pytest.mark.parametrize("D,xdt,ydt", WIDTHS, ids=[f"D{c[0]}" for c in WIDTHS])
def test_bwd_widths(backend, D, xdt, ydt):
    """The scalar walk at 40 and 516, the vector walk with one, two and four 256-channel steps."""
    for k, (is_rms, Lq) in enumerate([(True, 17), (False, 33)]):
        x, res, w, b = inputs(2, 1, Lq, D, xdt, ydt, True, not is_rms, 7 * D + k)
        check(backend, x, res, w, b, is_rms, ydt, ("mean", "max", "window"), centres(2, 1, Lq), 3, seed=D + k)


def test_bwd_workgroup_walks_several_chunks(backend):
    """4096 + 17 rows at D = 64: more chunks than pieces, so a workgroup walks two chunks and the last piece is ragged."""
    lib = L.get_lib()
    Lq = 4096 + 17
    pieces = int(lib.cad_pool_head_bwd_pieces(Lq))
    assert 1 < pieces < -(-Lq // 16), pieces
    x, res, w, b = inputs(1, 1, Lq, 64, BF, BF, True, False, 4113)
    check(backend, x, res, w, b, True, BF, ("mean", "max"), tag="pool-bwd-walk")
    x, res, w, b = inputs(2, 1, Lq, 64, F32, F32, True, True, 4114)
    check(backend, x, res, w, b, False, F32, ("window",), torch.tensor([[2000], [4100]]), 700, tag="pool-bwd-walk")


def test_bwd_weight_null_is_dy_itself(backend):
    for k, (D, xdt, has_res) in enumerate([(64, BF, True), (40, F32, False), (256, HF, True)]):
        x, res, _, _ = inputs(2, 3, 35, D, xdt, xdt, has_res, False, 900 + k)
        check(backend, x, res, None, None, True, xdt, ("mean", "max", "window"), centres(2, 3, 35), 4, seed=k, tag="pool-bwd-nonorm")


@pytest.mark.parametrize("D", [40, 64])
@pytest.mark.parametrize("xdt,ydt", AN_TYPES)
def test_bwd_misaligned_operands(backend, D, xdt, ydt):
    """Every operand and output one element into its buffer: the scalar walk at both widths; nothing outside a view is written."""
    x, res, w, b = inputs(2, 2, 37, D, xdt, ydt, True, True, 77 + D)
    check(backend, x, res, w, b, False, ydt, ("mean", "max", "window"), centres(2, 2, 37), 3, off=1, tag="pool-bwd-misaligned")


# ---- window ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq,half", [(37, 0), (37, 1), (37, 40), (1, 5)], ids=lambda v: str(v))
def test_bwd_window_edges(backend, Lq, half):
    """Centres -100, 0, L - 1 and L + 100 (and two inside): a gather, a clamped window on either end, every offset on one edge row."""
    D = 64
    cen = torch.tensor([[-100, 0, Lq - 1], [Lq + 100, Lq // 2, 3 % Lq]], dtype=torch.int64)
    x, res, w, b = inputs(2, 3, Lq, D, BF, BF, True, False, 11 * Lq + half)
    check(backend, x, res, w, b, True, BF, ("window",), cen, half, tag="pool-bwd-window")
    x, res, w, b = inputs(2, 3, Lq, D, F32, F32, True, True, 13 * Lq + half)
    check(backend, x, res, w, b, False, F32, ("window",), cen.flip(0), half, tag="pool-bwd-window")


# ---- MAX: ties and NaN -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,xdt,ydt", [(64, F32, F32), (40, F32, F32), (64, BF, BF)])
def test_bwd_max_ties_go_to_the_lowest_row(backend, D, xdt, ydt):
    """Every row occurs twice (rows r and r + 20 are equal), so every channel's maximum is attained on two rows with equal bits: the
    gradient must go to the lower one alone."""
    S, B, Lq = 2, 2, 40
    x, res, w, b = inputs(S, B, Lq, D, xdt, ydt, True, True, 5 * D)
    x[:, :, 20:], res[:, :, 20:] = x[:, :, :20], res[:, :, :20]
    for ww, bb in ((w, b), (None, None)):
        got = check(backend, x, res, ww, bb, False, ydt if ww is not None else xdt, ("max",), seed=D, tag="pool-bwd-ties")["max"]
        assert bool((got["rows"] < 20).all())
        assert bool((got["dres_in"][:, :, 20:] == 0).all()) and bool((got["dx"][:, :, 20:].float() == 0).all())


def test_bwd_max_nan_rows(backend):
    """Without a norm a NaN stays in its channel: out is NaN there and the gradient goes to the lowest NaN row.  Under a norm a NaN row's
    statistics are NaN: every channel of out is NaN, every channel's gradient goes to the lowest NaN row, dx is NaN on the NaN rows
    (their rstd is) and exactly 0 on every other row of the pair; the other pair is untouched by it."""
    name, dev = backend
    S, B, Lq, D = 1, 2, 40, 64
    x, res, w, b = inputs(S, B, Lq, D, F32, F32, True, True, 5)
    x[0, 0, 17, 9] = float("nan")
    x[0, 0, 29, 9] = float("nan")
    g = grad_of(S, B, D, 3)
    got = bwd_direct(dev, 0, x, res, None, None, True, F32, "max", g)
    assert int(got["rows"][0, 0, 9]) == 17 and torch.isnan(got["out"][0, 0, 9])
    dy32 = dy32_of(g, S, B, Lq, D, "max", rows=got["rows"])
    assert torch.equal(got["dx"], dy32) and torch.equal(got["dres_in"], dy32)
    got = bwd_direct(dev, 0, x, res, w, b, False, F32, "max", g)
    assert bool((got["rows"][0, 0] == 17).all()) and bool(torch.isnan(got["out"][0, 0]).all())
    nan_rows = torch.isnan(got["dx"][0, 0]).all(-1)
    assert nan_rows.nonzero().flatten().tolist() == [17, 29]
    assert bool((got["dx"][0, 0][~nan_rows] == 0).all()) and bool((got["dres_in"][0, 0][~nan_rows] == 0).all())
    alone = bwd_direct(dev, 0, x[:, 1:], res[:, 1:], w, b, False, F32, "max", g[:, 1:])
    assert torch.equal(alone["dx"][0, 0], got["dx"][0, 1]) and torch.equal(alone["rows"][0, 0], got["rows"][0, 1])


# ---- identities ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,xdt,ydt", [(64, BF, BF), (40, F32, F32), (256, F32, BF)])
def test_bwd_rows_in_the_opposite_order_give_the_reversed_gradient(backend, D, xdt, ydt):
    """Rows reversed, centres mirrored to L - 1 - c: dx and dres_in come back reversed, bit for bit (a row's gradient depends on the row,
    its multiplicity and g alone).  MAX with an fp32 y only: ties between distinct rows would go to the other row."""
    name, dev = backend
    for Lq in (50, 51):
        x, res, w, b = inputs(2, 3, Lq, D, xdt, ydt, True, True, 3 * D + Lq)
        cen, g = centres(2, 3, Lq), grad_of(2, 3, D, Lq)
        modes = [("mean", 0), ("window", 0), ("window", 7), ("window", Lq // 2)] + ([("max", 0)] if ydt == F32 else [])
        for mode, half in modes:
            fwd = bwd_direct(dev, 0, x, res, w, b, False, ydt, mode, g, cen, half)
            rev = bwd_direct(dev, 0, x.flip(2).contiguous(), res.flip(2).contiguous(), w, b, False, ydt, mode, g, Lq - 1 - cen, half)
            for key in ("dx", "dres_in"):
                assert torch.equal(fwd[key].view(torch.int16 if fwd[key].element_size() == 2 else torch.int32),
                                   rev[key].flip(2).view(torch.int16 if fwd[key].element_size() == 2 else torch.int32)), (mode, half, Lq, key)


@pytest.mark.parametrize("D,xdt,ydt", [(64, BF, BF), (40, F32, F32), (256, F32, HF)])
def test_bwd_weight_gradient_bits_do_not_depend_on_the_run_or_on_a_silent_pair(backend, D, xdt, ydt):
    """dweight / dbias: equal bits over two runs, and unchanged when an unrelated pair whose g is 0 is appended to the batch (its slots
    hold exact zeros and the fold's chains keep their shape).  dx of the first pair does not depend on the second either."""
    name, dev = backend
    Lq = 16 * 20 + 3  # 21 pieces: the fold's 16 chains take one and two slots
    x, res, w, b = inputs(2, 2, Lq, D, xdt, ydt, True, True, 3 * D)
    g = grad_of(2, 2, D, D)
    g[:, 1] = 0
    cen = centres(2, 2, Lq)
    for mode in ("mean", "max", "window"):
        kw = dict(centre=cen, half=7) if mode == "window" else {}
        kw1 = dict(centre=cen[:, :1].contiguous(), half=7) if mode == "window" else {}
        both = bwd_direct(dev, 0, x, res, w, b, False, ydt, mode, g, **kw)
        again = bwd_direct(dev, 0, x, res, w, b, False, ydt, mode, g, **kw)
        alone = bwd_direct(dev, 0, x[:, :1].contiguous(), res[:, :1].contiguous(), w, b, False, ydt, mode, g[:, :1].contiguous(), **kw1)
        for key in ("dweight", "dbias"):
            assert torch.equal(both[key].view(torch.int32), again[key].view(torch.int32)), (mode, key)
            assert torch.equal(both[key].view(torch.int32), alone[key].view(torch.int32)), (mode, key)
        assert torch.equal(both["dx"][:, :1].float(), alone["dx"].float()) and bool((both["dx"][:, 1].float() == 0).all()), mode


def test_pool_head_grad_is_pool_head_and_its_backward_is_the_kernel(backend):
    """ops.pool_head_grad: the forward's bits are ops.pool_head's; autograd delivers cad_pool_head_bwd's bits, dweight / dbias in the
    parameters' dtype; ops.pool_head still refuses tensors that require grad."""
    name, dev = backend
    S, B, Lq, D = 2, 2, 37, 64
    for xdt, pdt in ((BF, BF), (F32, F32)):
        x, res, w, b = inputs(S, B, Lq, D, xdt, xdt, True, True, 21)
        cen = centres(S, B, Lq)
        g = grad_of(S, B, D, 9)
        for mode in ("mean", "max", "window"):
            kw = dict(centre=cen.to(dev), half=2) if mode == "window" else {}
            leaves = [t.detach().clone().to(dev).requires_grad_(True) for t in (x, res, w.to(pdt), b.to(pdt))]
            with torch.no_grad():
                plain = ops.pool_head(*leaves, EPS, False, xdt, mode, **kw)
                assert torch.equal(ops.pool_head_grad(*leaves, EPS, False, xdt, mode, **kw), plain)
            with pytest.raises(RuntimeError, match="no backward"):
                ops.pool_head(*leaves, EPS, False, xdt, mode, **kw)
            out = ops.pool_head_grad(*leaves, EPS, False, xdt, mode, **kw)
            assert out.requires_grad and torch.equal(out.detach(), plain)
            out.backward(g.to(dev))
            kd = dict(centre=cen, half=2) if mode == "window" else {}
            got = bwd_direct(dev, 0, x, res, w.to(pdt).float(), b.to(pdt).float(), False, xdt, mode, g, **kd)
            assert torch.equal(leaves[0].grad.cpu(), got["dx"]) and torch.equal(leaves[1].grad.cpu(), got["dres_in"]), mode
            assert leaves[2].grad.dtype == pdt and leaves[3].grad.dtype == pdt
            assert torch.equal(leaves[2].grad.cpu(), got["dweight"].to(pdt)) and torch.equal(leaves[3].grad.cpu(), got["dbias"].to(pdt)), mode
    # only x asks for a gradient, no norm: no scratch, no sums
    xg = x.detach().clone().to(dev).requires_grad_(True)
    ops.pool_head_grad(xg, None, None, None, EPS, True, F32, "mean").sum().backward()
    assert torch.equal(xg.grad.cpu(), torch.full_like(x, 1.0) / torch.full_like(x, float(Lq)))


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------
def test_bwd_unsupported_arguments_return_before_a_launch(backend):
    """CAD_ERR_UNSUPPORTED (2) with dx untouched for D = 1025 and half = 2^22; the domain is the forward's."""
    name, dev = backend
    lib = L.get_lib()
    S, B, Lq = 1, 1, 8

    def call(D, mode, half):
        x = torch.zeros(S, B, Lq, D, device=dev)
        w, g = torch.ones(D, device=dev), torch.ones(S, B, D, device=dev)
        dx = torch.full((S, B, Lq, D), -7.0, device=dev)
        dw = torch.full((D,), -7.0, device=dev)
        scratch = torch.zeros(max(2, 2 * S * B * D), device=dev)
        c = torch.zeros(S, B, dtype=torch.int64, device=dev)
        a = L.PoolHeadBwdArgs(L.ptr(x), None, L.ptr(w), None, L.ptr(c), L.ptr(g), None, L.ptr(dx), None, L.ptr(dw), None, None, L.ptr(scratch),
                              B, Lq, half, S, D, EPS, 1, L.CAD_F32, L.CAD_F32, mode)
        st = lib.cad_pool_head_bwd(C.byref(a), L.stream_and_check(x, w, g, dx, dw, scratch))
        if dev.type == "cuda":
            torch.cuda.synchronize()
        assert st == 0 or (bool((dx == -7.0).all()) and bool((dw == -7.0).all()))
        return st
    assert call(64, L.POOL_MEAN, 0) == 0
    assert call(1025, L.POOL_MEAN, 0) == 2 and call(64, L.POOL_WINDOW, 1 << 22) == 2 and call(64, 3, 0) == 2
    assert call(64, L.POOL_MAX, 0) == 1  # MAX without out / rows: a bad argument
    for args in ((1024, 1, 1, 2, (1 << 22) - 1), (1025, 0, 0, 0, 0), (64, 1, 0, 0, 0), (64, 0, 0, 2, 1 << 22)):
        assert bool(lib.cad_pool_head_bwd_supported(*args)) == bool(lib.cad_pool_head_supported(*args))
    x = torch.zeros(1, 1, 8, 1028, device=dev, requires_grad=True)
    with pytest.raises(ops.PoolUnsupported):
        ops.pool_head_grad(x, None, torch.ones(1028, device=dev), None, EPS, True, F32, "mean")
