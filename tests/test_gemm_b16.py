"""cad_gemm_b16 (csrc/gemm_b16.hip), the strided bf16 MFMA GEMM of the generic engine, held to EXACT sums by the method of
tests/test_proj_exact.py (whose helpers are used as they are): integer-valued bf16 operands whose partial sums stay below 2^24 in any
order (asserted from |A| @ |B|) make fp32 accumulation exact, so a bf16 result must equal the fp64 product rounded ONCE to nearest even,
bit for bit, and an fp32 result (out_f32) the product itself.  Every case counts >= 100 rounding ties and >= 100 non-tie inexact sums on
its reference; addend cases >= 100 elements in which one rounding and two differ.

A "case" of the shape walk is one (operand views, tile configuration, placement) combination over the five shapes that cross every tile
edge -- (1, 1, 1) has one element, so the counts are asserted on the case's reference as a whole and, besides, on every shape of at least
4096 elements alone.  The shapes also walk both load paths (16-byte vectors need a pitch of 8 elements: K = 32, 264, 8 compact, or the
poisoned placement's pitch; K = 75 and the one-element-off placement take the 2-byte path) and both store paths (N = 64, 136 vector; 70,
1, 300-in-a-padded-view 2-byte)."""
import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops
from test_mixer_schedule import _Recorder
from test_proj_exact import (BF, F32, PBITS, Place, _amp, _assert_decided, _bits, _cast, _check_bound, _exact_bound, _illcond, _ints, _rne,
                             _run_twice, _same_bits, _tie_counts, cu)  # noqa: F401  (cu: the CU-count override fixture)

SHAPES = [(129, 70, 75), (64, 64, 32), (200, 136, 264), (1, 1, 1), (17, 300, 8)]
# (CU count, poison): the real count selects the 64 x 64 tiles for every small shape; one CU the 128 x 128 tiles wherever M, N > 64
VARIANTS = [pytest.param(None, False, id="tile64-compact"), pytest.param(1, True, id="tile128-poison"), pytest.param(None, True, id="tile64-poison")]


def _operands(M, N, K, seed):
    """Integer operands for an exact (M, K) @ (K, N): amplitudes as in test_proj_exact (_amp), rows of A / columns of B in sign groups."""
    if (M, N, K) == (1, 1, 1):
        return torch.tensor([[3.0]]).double(), torch.tensor([[171.0]]).double()  # 513: a tie between 512 and 514
    a = _amp(K, BF)
    Am, Bm = _ints(M, K, a, seed), _ints(K, N, a, seed + 1, by_cols=True)
    _exact_bound(Am, Bm)
    return Am, Bm


def _view(P, m, transposed):
    """m as a bf16 device operand: row-major, or the transposed view of its row-major transpose (unit stride along the rows)."""
    return P.operand(_cast(m.t().contiguous(), BF)).t() if transposed else P.operand(_cast(m, BF))


@pytest.mark.parametrize("grid,poison", VARIANTS)
@pytest.mark.parametrize("ta,tb", [(False, False), (True, False), (False, True), (True, True)])
def test_gemm_b16_exact_shapes_and_views(backend, cu, ta, tb, grid, poison):
    """All four plain / transposed operand combinations over the five shapes, both tile configurations, compact and inside NaN-filled
    operand buffers / sentinel-filled output buffers: bf16 D = the product rounded once, out_f32 D = the product."""
    name, dev = backend
    cu(grid)
    ties = inexact = 0
    for q, (M, N, K) in enumerate(SHAPES):
        Am, Bm = _operands(M, N, K, 5000 + 10 * q)
        S = Am @ Bm
        t, i = _tie_counts(S, BF)
        ties, inexact = ties + t, inexact + i
        if M * N >= 4096:
            _assert_decided(S, BF)

        def run(P):
            A, B = _view(P, Am, ta), _view(P, Bm, tb)
            out, out32 = P.output((M, N), BF), P.output((M, N), F32)
            ops.mm_b16(A, B, out=out)
            ops.bmm_b16(A.unsqueeze(0), B.unsqueeze(0), out=out32.unsqueeze(0), out_f32=True)
            return out.cpu(), out32.cpu()
        out, out32 = _run_twice(dev, poison, run)
        assert _same_bits(out, _rne(S, BF)), (M, N, K)
        assert torch.equal(out32.double(), S), (M, N, K)
    assert ties >= 100 and inexact >= 100, (ties, inexact)


def test_gemm_b16_real_grid_selects_the_large_tiles(backend):
    """2944 x 2944 x 96 at the real CU count: 23 x 23 = 529 tiles of 128 x 128 >= 2 * 256 CUs, the launcher's large configuration on its
    real grid (flattened onto grid.x), K = 3 chunks."""
    name, dev = backend
    if name == "emu":
        pytest.skip("real-grid case: device only")
    M = N = 2944
    K = 96
    assert ((M + 127) // 128) * ((N + 127) // 128) >= 2 * ops._cu_count()
    Am, Bm = _operands(M, N, K, 5100)
    S = Am @ Bm
    _assert_decided(S, BF)
    out = ops.mm_b16(_cast(Am, BF).to(dev), _cast(Bm.t().contiguous(), BF).to(dev).t())
    assert _same_bits(out.cpu(), _rne(S, BF))


@pytest.mark.parametrize("grid", [pytest.param(None, id="tile64"), pytest.param(1, id="tile128")])
def test_gemm_b16_output_views(backend, cu, grid):
    """Padded and transposed output views inside sentinel-filled buffers: a row-major view with an odd pitch, the transposed view of a
    column-major buffer (unit stride along the rows: no operand swap in the launcher), and one with 8-byte aligned columns."""
    name, dev = backend
    cu(grid)
    M, N, K = 200, 136, 264
    Am, Bm = _operands(M, N, K, 5200)
    S = Am @ Bm
    _assert_decided(S, BF)
    expect = _rne(S, BF)
    A, B = _cast(Am, BF).to(dev), _cast(Bm, BF).to(dev)
    # (buffer shape, first row, first column, transposed): a row-major view with an odd pitch (145); the transposed view of a column-major
    # buffer with 8-byte aligned columns (pitch 208); the same with an odd pitch and offset
    for shape, r0, c0, tr in (((M + 5, N + 9), 3, 5, False), ((N + 4, M + 8), 2, 4, True), ((N + 4, M + 7), 1, 3, True)):
        buf = torch.full(shape, 0x5A5A, dtype=torch.int16).view(BF).to(dev)
        view = buf[r0:r0 + N, c0:c0 + M].t() if tr else buf[r0:r0 + M, c0:c0 + N]
        ops.mm_b16(A, B, out=view)
        assert _same_bits(view.cpu().contiguous(), expect)
        after = buf.cpu().view(torch.int16).clone()
        if tr:
            after[r0:r0 + N, c0:c0 + M] = 0x5A5A
        else:
            after[r0:r0 + M, c0:c0 + N] = 0x5A5A
        assert bool((after == 0x5A5A).all()), "bytes outside the output view were written"


@pytest.mark.parametrize("grid", [pytest.param(None, id="tile64"), pytest.param(1, id="tile128")])
def test_gemm_b16_batch_of_three_with_batch_strides(backend, cu, grid):
    """Batch 3 (grid.z) on views with non-trivial batch strides: the permuted K slices of channel-major operands (batch stride Kc inside a
    row, as mm_b16 builds them) and a padded batched output."""
    name, dev = backend
    cu(grid)
    M, N, n, Kc = 130, 90, 3, 72
    a = _amp(Kc, BF)
    Ym, Xm = _ints(M, n * Kc, a, 5300), _ints(N, n * Kc, a, 5301)
    _exact_bound(Ym, Xm.t())
    S = torch.stack([Ym[:, s * Kc:(s + 1) * Kc] @ Xm[:, s * Kc:(s + 1) * Kc].t() for s in range(n)])
    _assert_decided(S, BF)
    y, x = _cast(Ym, BF).to(dev), _cast(Xm, BF).to(dev)
    ya, xb = y.unflatten(1, (n, Kc)).permute(1, 0, 2), x.unflatten(1, (n, Kc)).permute(1, 2, 0)
    buf = torch.full((n, M + 3, N + 6), 0x5A5A, dtype=torch.int16).view(BF).to(dev)
    out = buf[:, 1:1 + M, 2:2 + N]
    ops.bmm_b16(ya, xb, out=out)
    assert _same_bits(out.cpu().contiguous(), _rne(S, BF))
    after = buf.cpu().view(torch.int16).clone()
    after[:, 1:1 + M, 2:2 + N] = 0x5A5A
    assert bool((after == 0x5A5A).all())
    assert torch.equal(ops.bmm_b16(ya, xb, out_f32=True).cpu().double(), S)


@pytest.mark.parametrize("ta,tb", [(False, False), (True, True)])
def test_gemm_b16_one_element_off_alignment(backend, cu, ta, tb):
    """Operands and output starting one element (2 bytes) off 16-byte alignment take the 2-byte load / store paths: bit-identical to
    the aligned call (16-byte loads, 8-byte stores), which equals the reference."""
    name, dev = backend
    cu(1)
    M, N, K = 200, 136, 264
    Am, Bm = _operands(M, N, K, 5400)
    S = Am @ Bm
    _assert_decided(S, BF)

    def shifted(t):  # the same values, same strides, one element further on
        flat = torch.empty(t.numel() + 9, dtype=BF, device=dev)
        v = flat[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 2
        return v
    A0 = _cast(Am.t().contiguous(), BF).to(dev) if ta else _cast(Am, BF).to(dev)
    B0 = _cast(Bm.t().contiguous(), BF).to(dev) if tb else _cast(Bm, BF).to(dev)
    assert A0.data_ptr() % 16 == 0 and B0.data_ptr() % 16 == 0
    tr = lambda t, f: t.t() if f else t
    aligned = ops.mm_b16(tr(A0, ta), tr(B0, tb))
    off_out = shifted(torch.zeros(M, N, dtype=BF, device=dev))
    ops.mm_b16(tr(shifted(A0), ta), tr(shifted(B0), tb), out=off_out)
    assert _same_bits(aligned, _rne(S, BF)) and _same_bits(off_out.cpu().contiguous(), aligned.cpu())


@pytest.mark.parametrize("grid,poison", VARIANTS[:2])
@pytest.mark.parametrize("addend", ["acc", "alias"])
@pytest.mark.parametrize("M,N,K", [(129, 70, 75), (200, 136, 264)])
def test_gemm_b16_addend_inside_the_one_rounding(backend, cu, M, N, K, addend, grid, poison):
    """bf16 D = round(S + addend): the widened addend joins the fp32 sum BEFORE the one rounding, also when it aliases D; out_f32 with an
    fp32 addend holds S + addend exactly."""
    name, dev = backend
    Am, Bm = _operands(M, N, K, 5500 + K)
    acc = _ints(M, N, 2 ** PBITS[BF], 5502 + K, signed_groups=False)
    _exact_bound(Am, Bm, acc)
    S = Am @ Bm
    _assert_decided(S + acc, BF)
    expect = _rne(S + acc, BF)
    twice = (_rne(S, BF).float() + acc.float()).to(BF)
    assert int((_bits(expect) != _bits(twice)).sum()) >= 100, "the case does not tell one rounding from two"
    cu(grid)

    def run(P):
        A, B = P.operand(_cast(Am, BF)), P.operand(_cast(Bm, BF))
        if addend == "alias":
            out = P.output((M, N), BF, init=_cast(acc, BF))
            ops.mm_b16(A, B, out=out, addend=out)
            out32 = P.output((M, N), F32, init=acc.float())
            ops._gemm_strided("gemm_b16", BF, F32, A.unsqueeze(0), B.unsqueeze(0), out32.unsqueeze(0), out32.unsqueeze(0))
        else:
            out = P.output((M, N), BF)
            ad = P.output((M, N), BF, init=_cast(acc, BF))  # (an addend with out's strides, in a buffer of its own)
            ops.mm_b16(A, B, out=out, addend=ad)
            out32, ad32 = P.output((M, N), F32), P.output((M, N), F32, init=acc.float())
            ops._gemm_strided("gemm_b16", BF, F32, A.unsqueeze(0), B.unsqueeze(0), out32.unsqueeze(0), ad32.unsqueeze(0))
        return out.cpu(), out32.cpu()
    out, out32 = _run_twice(dev, poison, run)
    assert _same_bits(out, expect)
    assert torch.equal(out32.double(), S + acc)


@pytest.mark.parametrize("ta,tb", [(False, False), (True, True)])
def test_gemm_b16_nonfinite_values_stay_in_their_row_or_column(backend, cu, ta, tb):
    """A NaN in one column of B and an inf in one row of A: exactly that output column / row is non-finite, every other element keeps
    its bits (ragged shape, both tile configurations)."""
    name, dev = backend
    g = torch.Generator().manual_seed(5600)
    M, N, K = 150, 139, 75
    Ac, Bc = (torch.randn(M, K, generator=g) + 0.01).to(BF), (torch.randn(K, N, generator=g) + 0.01).to(BF)
    row, col = M - 1, N - 3
    Ap, Bp = Ac.clone(), Bc.clone()
    Bp[3, col] = float("nan")
    Ap[row, 70] = float("inf")
    put = lambda m, f: m.t().contiguous().to(dev).t() if f else m.to(dev)
    for n_cu in (None, 1):
        cu(n_cu)
        clean = ops.mm_b16(put(Ac, ta), put(Bc, tb)).cpu()
        bad = ops.mm_b16(put(Ap, ta), put(Bp, tb)).cpu()
        mask = torch.zeros(M, N, dtype=torch.bool)
        mask[row, :] = True
        mask[:, col] = True
        assert bool(torch.isfinite(clean.float()).all())
        assert bool((~torch.isfinite(bad.float()))[mask].all()) and bool(torch.isnan(bad.float())[:, col].all())
        assert torch.equal(_bits(bad)[~mask], _bits(clean)[~mask])


def test_gemm_b16_sums_beyond_the_bf16_range_become_inf(backend, cu):
    """A finite fp32 sum beyond bf16's range is +-inf: powers of two added up to max + half an ulp (a tie that nearest-even rounds to
    2^128 = inf; truncation would keep the largest finite value), every partial sum exact and finite in fp32.  out_f32 keeps the sum."""
    name, dev = backend
    cu(1)
    p, e_hi = PBITS[BF], 127
    ew = e_hi // 2 + 1
    ex = e_hi - ew
    M, N, K, r_pos, r_neg, c_big = 130, 139, 40, 3, 129, 137
    Lm, Rm = torch.full((M, K), 2.0 ** -3, dtype=torch.float64), torch.full((K, N), 2.0 ** -3, dtype=torch.float64)
    Lm[r_pos], Lm[r_neg], Rm[:, c_big] = 0.0, 0.0, 0.0
    for i in range(p + 1):
        Lm[r_pos, i], Lm[r_neg, i], Rm[i, c_big] = 2.0 ** ew, -(2.0 ** ew), 2.0 ** (ex - i)
    S = Lm @ Rm
    assert float(S[r_pos, c_big]) == 2.0 ** (e_hi + 1) - 2.0 ** (e_hi - p)
    expect = S.float().to(BF)
    assert float(expect[r_pos, c_big]) == float("inf") and float(expect[r_neg, c_big]) == float("-inf")
    assert int(torch.isinf(expect.float()).sum()) == 2
    A, B = _cast(Lm, BF).to(dev), _cast(Rm, BF).to(dev)
    assert _same_bits(ops.mm_b16(A, B).cpu(), expect)
    assert torch.equal(ops.bmm_b16(A.unsqueeze(0), B.unsqueeze(0), out_f32=True)[0].cpu().double(), S)


def test_gemm_b16_illconditioned_against_the_derived_bound(backend, cu):
    """Non-integer, ill-conditioned operands (test_proj_exact's _illcond: rows / columns scaled by 2^+-20, cancelling sums) held per element
    to that module's derived bound  u |S| (1 + u) + (K + 2) 2^-24 sum |a b| + K 2^-126  (u = 2^-8; 0 for the out_f32 form)."""
    name, dev = backend
    cu(2)
    for ta, tb in ((False, False), (True, True)):
        Ld, Rd = _illcond(130, 200, 257, BF, 5700)
        A = Ld.t().contiguous().to(dev).t() if ta else Ld.to(dev)
        B = Rd.t().contiguous().to(dev).t() if tb else Rd.to(dev)
        _check_bound("gemm_b16", ops.mm_b16(A, B).cpu(), Ld, Rd, BF, 200)
        _check_bound("gemm_b16 out_f32", ops.bmm_b16(A.unsqueeze(0), B.unsqueeze(0), out_f32=True)[0].cpu(), Ld, Rd, F32, 200)


# ---- ops._MmB16: gradients through the same kernel ----------------------------------------------------------------------------------------
def _grads(dev, Am, Bm, Gm, addend=None):
    a, b = _cast(Am, BF).to(dev).requires_grad_(True), _cast(Bm, BF).to(dev).requires_grad_(True)
    ad = None if addend is None else _cast(addend, BF).to(dev).requires_grad_(True)
    real, calls = L.get_lib(), []
    L._lib = _Recorder(real, calls)
    try:
        out = ops.mm(a, b, own_b16=True) if ad is None else ops.addmm(ad, a, b, own_b16=True)
        out.backward(_cast(Gm, BF).to(dev))
    finally:
        L._lib = real
    return out.detach().cpu(), a.grad.cpu(), b.grad.cpu(), (None if ad is None else ad.grad.cpu()), calls


def test_mm_b16_gradients_are_exact(backend, cu):
    """ops.mm / ops.addmm with own_b16: out, da = g b^T and db = a^T g of integer operands equal the exact products rounded once; the
    addend's gradient is g.  Ragged shape, transposed views inside the backward."""
    name, dev = backend
    cu(1)
    M, K, N = 129, 75, 70
    a = _amp(K, BF)
    Am, Bm, Gm = _ints(M, K, a, 5800), _ints(K, N, a, 5801, by_cols=True), _ints(M, N, a, 5802)
    acc = _ints(M, N, 2 ** PBITS[BF], 5803, signed_groups=False)
    _exact_bound(Am, Bm, acc), _exact_bound(Gm, Bm.t()), _exact_bound(Am.t(), Gm)
    for S in (Am @ Bm, Gm @ Bm.t(), Am.t() @ Gm):
        assert sum(_tie_counts(S, BF)) >= 100  # every product holds sums that bf16 has to round
    out, da, db, _, calls = _grads(dev, Am, Bm, Gm)
    assert calls == ["cad_gemm_b16"] * 3
    assert _same_bits(out, _rne(Am @ Bm, BF)) and _same_bits(da, _rne(Gm @ Bm.t(), BF)) and _same_bits(db, _rne(Am.t() @ Gm, BF))
    out, da, db, dacc, calls = _grads(dev, Am, Bm, Gm, addend=acc)
    assert calls == ["cad_gemm_b16"] * 3
    assert _same_bits(out, _rne(Am @ Bm + acc, BF)) and _same_bits(da, _rne(Gm @ Bm.t(), BF)) and _same_bits(db, _rne(Am.t() @ Gm, BF))
    assert _same_bits(dacc, _cast(Gm, BF))


@pytest.fixture
def four_cus(backend, cu, monkeypatch):
    """Four CUs on both sides: the library's launchers (cad_debug_set_cu_count) and, on the device, the count ops sizes its K slices with
    (the entry of its per-device cache, put back afterwards; without a device ops assumes 256 CUs, which slices as well)."""
    name, dev = backend
    cu(4)
    if dev.type == "cuda":
        ops._cu_count()
        monkeypatch.setitem(ops._CU_COUNT, torch.cuda.current_device(), 4)


def test_mm_b16_weight_gradient_takes_the_k_slices(backend, four_cus):
    """An engine weight gradient: W (24 x 10) @ X (10 x 8192) has dW = g X^T with (M, N, K) = (24, 10, 8192) -- one 64 x 64 tile and a
    long reduction, cut into K slices (4 of 2048 at four CUs): ONE batched out_f32 launch, the fp32 partial tiles summed by
    cad_fold_f32_multi, one rounding.  Exact on integer operands."""
    name, dev = backend
    M, K, T = 24, 10, 8192
    Wm, Xm, Gm = _ints(M, K, 32, 5900), _ints(K, T, 32, 5901), _ints(M, T, 32, 5902)
    _exact_bound(Wm, Xm), _exact_bound(Gm, Xm.t()), _exact_bound(Wm.t(), Gm)
    assert ops._f32_kslices(M, K, T) > 1
    out, dW, dX, _, calls = _grads(dev, Wm, Xm, Gm)
    assert calls == ["cad_gemm_b16", "cad_gemm_b16", "cad_fold_f32_multi", "cad_gemm_b16"], calls  # forward, dW slices + fold, dX
    assert _same_bits(out, _rne(Wm @ Xm, BF)) and _same_bits(dX, _rne(Wm.t() @ Gm, BF))
    assert _same_bits(dW, _rne(Gm @ Xm.t(), BF))
    assert int((_rne(Gm @ Xm.t(), BF).double() != Gm @ Xm.t()).sum()) >= 100  # the one rounding is visible in the weight gradient


def test_mm_b16_k_slices_with_an_odd_result_and_an_addend(backend, four_cus):
    """The K-slice path where the fold kernel does not apply (M N = 23 x 9 = 207, no multiple of 4: the partial tiles are summed by an
    element-wise fp32 sum) and with an addend, which joins the fp32 sum before the ONE rounding; an output view is filled in place."""
    name, dev = backend
    M, N, K = 23, 9, 8192
    Am, Bm = _ints(M, K, 32, 5950), _ints(K, N, 32, 5951, by_cols=True)
    acc = _ints(M, N, 2 ** PBITS[BF], 5952, signed_groups=False)
    _exact_bound(Am, Bm, acc)
    assert ops._f32_kslices(M, N, K) > 1
    S = Am @ Bm
    expect = _rne(S + acc, BF)
    assert int((_bits(expect) != _bits((_rne(S, BF).float() + acc.float()).to(BF))).sum()) >= 20  # (207 elements: one rounding, not two)
    A, B, ad = _cast(Am, BF).to(dev), _cast(Bm, BF).to(dev), _cast(acc, BF).to(dev)
    real, calls = L.get_lib(), []
    L._lib = _Recorder(real, calls)
    try:
        plain, with_acc = ops.mm_b16(A, B), ops.mm_b16(A, B, addend=ad)
        out = torch.zeros(M, N + 3, dtype=BF, device=dev)[:, 1:1 + N]
        ops.mm_b16(A, B, out=out, addend=ad)
    finally:
        L._lib = real
    assert calls == ["cad_gemm_b16"] * 3, calls  # one batched out_f32 launch each, no fold kernel
    assert _same_bits(plain.cpu(), _rne(S, BF)) and _same_bits(with_acc.cpu(), expect) and _same_bits(out.cpu().contiguous(), expect)
