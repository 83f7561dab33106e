"""The MFMA projections (csrc/gemm.hip with its headers proj_wstat.h / proj_ring.h / gemm_stream.h, gemm_fp8.hip, gemm_f32.hip) held to EXACT sums, with several blocks per workgroup.

A  exact sums: integer operands whose partial sums stay below 2^24 in any order (asserted from abs(L) @ abs(R)), so fp32 accumulation is
   exact whatever the MFMA's internal order: 16-bit outputs must equal the fp64 product rounded ONCE to nearest even, bit for bit, fp32
   outputs the product itself.  Every case counts its rounding ties and its non-tie inexact elements on the reference (>= 100 each), so
   the rounding mode is decided.  Addends follow the sequences stated in include/caduceus_hip.h (thin K: round(round(W X) + acc);
   thin M / deep K: round(W X + acc)).
B  several blocks per workgroup: (1) cad_debug_set_cu_count lowers the CU count the launchers size their grids with, so that one or two
   workgroups walk 5 .. 20 blocks plus a ragged tail -- double-buffer parity, ring slots and counted waits over many wraps, on the
   emulator and on the GPU; (2) on the GPU only, the real grid with T = 3 * CUs * 128 + a ragged tail (or the matching item count):
   every workgroup takes at least three blocks through real asynchronous DMA.
C  poisoned surroundings: every operand a view inside a NaN-filled buffer (pitch columns, rows past M, tokens past T), every output a
   view inside a sentinel-filled buffer: the result must be bit-identical to the compact call, every sentinel byte unchanged.
D  non-integer, ill-conditioned operands (rows / columns scaled by powers of two, cancelling sums) against a per-element DERIVED bound
   |out - S| <= u |S| (1 + u) + (K + 2) 2^-24 sum|w x| + K 2^-126   (u = 2^-8 bf16, 2^-11 fp16, 0 for fp32 outputs);
   NaN / inf in one token or channel appears in exactly that column / row; a finite sum beyond the output range becomes +-inf.
"""
import ctypes as C

import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
PBITS = {BF: 8, HF: 11}          # significand bits (with the hidden one)
UNIT = {BF: 2.0 ** -8, HF: 2.0 ** -11, F32: 0.0}
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(HF, id="f16")]
INT_OF = {BF: torch.int16, HF: torch.int16, F32: torch.int32, torch.uint8: torch.uint8}
SENT = {torch.int16: 0x5A5A, torch.int32: 0x5A5A5A5A, torch.uint8: 0x5A}
WORST = {}                        # section D: kernel -> worst err / tol (printed by the last test of the module)


# ---- infrastructure ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def cu(backend):
    """The test-only CU-count override (cad_debug_set_cu_count); always restored."""
    lib = L.get_lib()

    def set_count(n):
        L.check(lib.cad_debug_set_cu_count(int(n or 0)), "cad_debug_set_cu_count")
    yield set_count
    lib.cad_debug_set_cu_count(0)


# (grid, poison): the plain call on the real grid at a small T (one block per workgroup); two workgroups walking many blocks on poisoned
# views; ONE workgroup walking all blocks
VARIANTS = [pytest.param(None, False, id="real-compact"), pytest.param(2, True, id="cu2-poison"), pytest.param(1, False, id="cu1-compact")]


class Place:
    """Puts operands on the device -- compact, or (poison) as views inside larger NaN-filled buffers that still satisfy the launchers'
    alignment checks: two rows before, three after, 16 bytes of pitch before and 32 after every row -- and outputs as views inside
    sentinel-filled buffers whose bytes outside the view are checked by check()."""

    def __init__(self, dev, poison):
        self.dev, self.poison, self.outs = dev, poison, []

    def operand(self, t):
        if t is None:
            return None
        if not self.poison:
            return t.contiguous().to(self.dev)
        q = 16 // t.element_size()
        fill = 0x7F if t.dtype == torch.uint8 else float("nan")  # (0x7f: the e4m3 NaN)
        if t.dim() == 1:
            buf = torch.full((t.numel() + 3 * q,), fill, dtype=t.dtype)
            buf[q:q + t.numel()] = t
            return buf.to(self.dev)[q:q + t.numel()]
        r, c = t.shape
        buf = torch.full((r + 5, c + 3 * q), fill, dtype=t.dtype)
        buf[2:2 + r, q:q + c] = t
        return buf.to(self.dev)[2:2 + r, q:q + c]

    def output(self, shape, dtype, init=None, full_rows=False):
        """full_rows: the rows stay contiguous (slot buffers); sentinel rows before and after only."""
        r, c = shape
        ity = INT_OF[dtype]
        if not self.poison:
            out = torch.full((r, c), SENT[ity], dtype=ity).view(dtype).to(self.dev)
            if init is not None:
                out.copy_(init.to(self.dev))
            return out
        q = 0 if full_rows else 16 // torch.empty((), dtype=dtype).element_size()
        buf = torch.full((r + 5, c + 3 * q), SENT[ity], dtype=ity).view(dtype).to(self.dev)
        view = buf[2:2 + r, q:q + c]
        if init is not None:
            view.copy_(init.to(self.dev))
        self.outs.append((buf, r, c, q, ity))
        return view

    def check(self):
        for buf, r, c, q, ity in self.outs:
            after = buf.cpu().view(ity).clone()
            after[2:2 + r, q:q + c] = SENT[ity]
            assert bool((after == SENT[ity]).all()), "bytes outside the output view were written"


def _bits(t):
    return t.detach().cpu().contiguous().view(INT_OF[t.dtype])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _amp(K, dtype):
    """Power-of-two integer amplitude a: the typical one-signed sum K a^2 / 4 reaches 4 * 2^p, so sums spread over the exactly
    representable integers (< 2^p), the binade of pure ties (odd sums in [2^p, 2^(p+1))) and the binades with non-tie inexact sums."""
    a = 2
    while K * a * a / 4 < 4 * 2 ** PBITS[dtype]:
        a *= 2
    return a


def _ints(rows, cols, a, seed, signed_groups=True, by_cols=False):
    """Integers in [-a, a]; every third row (column, by_cols) non-negative, every third non-positive: their products sum up."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(-a, a + 1, (rows, cols), generator=g).double()
    if signed_groups:
        k = torch.arange(cols if by_cols else rows) % 3
        if by_cols:
            m[:, k == 1], m[:, k == 2] = m[:, k == 1].abs(), -m[:, k == 2].abs()
        else:
            m[k == 1], m[k == 2] = m[k == 1].abs(), -m[k == 2].abs()
    return m


def _exact_bound(Lm, Rm, acc=None):
    """Every partial sum, in any order, stays below 2^24 in magnitude: fp32 accumulation of the integer products is exact."""
    b = float((Lm.abs() @ Rm.abs()).max()) + (0.0 if acc is None else float(acc.abs().max()))
    assert b < 2 ** 24, b


def _rne(S, dtype):
    """An fp64 tensor of values exact in fp32 (integers < 2^24 here) rounded ONCE to nearest even."""
    assert torch.equal(S.float().double(), S)
    return S.float().to(dtype)


def _tie_counts(S, dtype):
    """(ties, non-tie inexact elements) of rounding the exact sums S to dtype."""
    r = _rne(S, dtype).double()
    inexact = (r != S) & torch.isfinite(r)
    _, e = torch.frexp(S)
    half_ulp = torch.ldexp(torch.ones_like(S), e - PBITS[dtype] - 1)
    tie = inexact & ((r - S).abs() == half_ulp)
    return int(tie.sum()), int((inexact & ~tie).sum())


def _assert_decided(S, dtype):
    ties, inexact = _tie_counts(S, dtype)
    assert ties >= 100 and inexact >= 100, (ties, inexact)


def _ties_round_to_even_sanity():
    S = torch.tensor([257.0, 259.0, 258.0, 1027.0]).double()
    assert _rne(S, BF).tolist() == [256.0, 260.0, 258.0, 1024.0] and _tie_counts(S, BF) == (2, 1)


def test_reference_rounding_helpers():
    """257 -> 256 and 259 -> 260 in bf16 (ties to even); 1027 is inexact but no tie."""
    _ties_round_to_even_sanity()
    S = torch.tensor([2049.0, 2051.0, 4097.0]).double()
    assert _rne(S, HF).tolist() == [2048.0, 2052.0, 4096.0] and _tie_counts(S, HF) == (2, 1)


def _cast(m, dtype):
    t = m.float().to(dtype)
    assert torch.equal(t.double(), m), "operand not exactly representable"
    return t


# ---- raw launches (the ops wrappers take no output views for these) ---------------------------------------------------------------------
def _gemm_stream(A, B, out, R, Cc, K, nslices, mode, col_fastest):
    stream = L.stream_and_check(A, B, out, contiguous=False)
    a = L.GemmStreamArgs(L.ptr(A), L.ptr(B), L.ptr(out), R, Cc, K, A.stride(0), B.stride(0), out.stride(0) if mode else 0, nslices, mode,
                         int(col_fastest))
    L.check(ops._proj_fn("cad_gemm_stream", A.dtype)(C.byref(a), stream), "cad_gemm_stream")


def _wgrad_slots(T):
    return int(L.get_lib().cad_proj_wx_wgrad_partials(int(T)))


# =========================================================================================================================================
# A + B (override) + C: exact integer sums
# =========================================================================================================================================
def _run_twice(dev, poison, fn):
    """fn(Place) -> result(s).  With poison: the compact call as well, and the two must agree bit for bit; sentinels are checked."""
    P = Place(dev, poison)
    res = fn(P)
    P.check()
    if poison:
        P0 = Place(dev, False)
        res0 = fn(P0)
        for a, b in zip(res if isinstance(res, tuple) else (res,), res0 if isinstance(res0, tuple) else (res0,)):
            assert _same_bits(a, b), "poisoned surroundings changed the result"
    return res


@pytest.mark.parametrize("grid,poison", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [32, 64, 128, 256, 512])
def test_wxT_exact(backend, cu, dtype, K, grid, poison):
    """cad_proj_wxT for every supported K: ragged M (not a multiple of 16 nor of the wave's rows), ragged T (any T is allowed)."""
    name, dev = backend
    assert ops.proj_supported(torch.empty(0, dtype=dtype), K) and not ops.proj_supported(torch.empty(0, dtype=dtype), K + 8)
    NT = 32 if K == 512 else 64
    M, T = (150 if K < 512 else 77), (3 * NT + 13 if grid is None else 9 * NT + NT // 2 + 5)
    a = _amp(K, dtype)
    Lm, Rm = _ints(M, K, a, 100 + K), _ints(K, T, a, 200 + K, by_cols=True)
    _exact_bound(Lm, Rm)
    S = Lm @ Rm
    _assert_decided(S, dtype)
    cu(grid)

    def run(P):
        W, X = P.operand(_cast(Lm, dtype)), P.operand(_cast(Rm.t().contiguous(), dtype))
        out = P.output((M, T), dtype)
        ops.proj_wxT(W, X, out=out)
        return out.cpu()
    out = _run_twice(dev, poison, run)
    assert _same_bits(out, _rne(S, dtype))


@pytest.mark.parametrize("grid,poison", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [8, 24, 40, 64])
@pytest.mark.parametrize("addend", ["none", "acc", "alias"])
def test_wx_thin_k_exact(backend, cu, dtype, K, addend, grid, poison):
    """cad_proj_wx, thin K (K below the padded 32 / 64 rows of the tile): plain, with an addend, with the addend aliasing the output.
    The addend sequence is the header's: the fp32 sums are rounded to the element type, the widened addend is added in fp32, the result
    rounded again -- the integer addends make round(round(S) + acc) and round(S + acc) differ in at least a hundred elements."""
    name, dev = backend
    M, T = 130, (200 if grid is None else 9 * 64 + 24)
    assert ops.proj_wx_supported(torch.empty(0, dtype=dtype), K, T)
    a = _amp(K, dtype)
    Lm, Rm = _ints(M, K, a, 300 + K), _ints(K, T, a, 400 + K, by_cols=True)
    S = Lm @ Rm
    _assert_decided(S, dtype)
    acc = None
    if addend != "none":
        acc = _ints(M, T, 2 ** PBITS[dtype], 500 + K, signed_groups=False)
        _exact_bound(Lm, Rm, acc)
        expect = (_rne(S, dtype).float() + acc.float()).to(dtype)      # the header's sequence: two roundings
        once = _rne(torch.where(torch.isfinite(_rne(S, dtype).double()), S + acc, S), dtype)
        assert int((_bits(once) != _bits(expect)).sum()) >= 100, "the case does not tell one rounding from two"
    else:
        _exact_bound(Lm, Rm)
        expect = _rne(S, dtype)
    cu(grid)

    def run(P):
        W, X = P.operand(_cast(Lm, dtype)), P.operand(_cast(Rm, dtype))
        if addend == "alias":
            out = P.output((M, T), dtype, init=_cast(acc, dtype))
            ops.proj_wx(W, X, out=out, acc=out)
        else:
            out = P.output((M, T), dtype)
            ops.proj_wx(W, X, out=out, acc=None if acc is None else P.operand(_cast(acc, dtype)))
        return out.cpu()
    out = _run_twice(dev, poison, run)
    assert _same_bits(out, expect)


@pytest.mark.parametrize("grid,poison", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K", [(48, 512), (33, 128), (13, 192), (64, 256)])
@pytest.mark.parametrize("addend", ["none", "acc"])
def test_wx_thin_m_exact(backend, cu, dtype, M, K, addend, grid, poison):
    """cad_proj_wx, thin M / deep K through the 4-slot DMA ring; the addend is added to the fp32 sums BEFORE the one rounding."""
    name, dev = backend
    T = 520 if grid is None else 7 * 128 + 40
    assert ops.proj_wx_supported(torch.empty(0, dtype=dtype), K, T, M=M) and not L.get_lib().cad_proj_wx_supported(K, T)
    a = _amp(K, dtype)
    Lm, Rm = _ints(M, K, a, 600 + K), _ints(K, T, a, 700 + K, by_cols=True)
    acc = _ints(M, T, 2 ** PBITS[dtype], 800 + K, signed_groups=False) if addend == "acc" else None
    _exact_bound(Lm, Rm, acc)
    S = Lm @ Rm
    _assert_decided(S, dtype)
    expect = _rne(S if acc is None else S + acc, dtype)
    if acc is not None:
        assert int((_bits(expect) != _bits((_rne(S, dtype).float() + acc.float()).to(dtype))).sum()) >= 100
    cu(grid)

    def run(P):
        W, X = P.operand(_cast(Lm, dtype)), P.operand(_cast(Rm, dtype))
        out = P.output((M, T), dtype)
        ops.proj_wx(W, X, out=out, acc=None if acc is None else P.operand(_cast(acc, dtype)))
        return out.cpu()
    out = _run_twice(dev, poison, run)
    assert _same_bits(out, expect)


@pytest.mark.parametrize("grid,poison", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_wx_two_k_halves_exact(backend, cu, dtype, grid, poison):
    """x_proj at d_inner 1024: the whole product is refused (asserted), the mixer's two K halves -- views of one W / X, the second with the
    first as its aliasing addend -- give round(S2 + round(S1))."""
    name, dev = backend
    M, K, T = 64, 1024, (264 if grid is None else 5 * 128 + 24)
    assert not ops.proj_wx_supported(torch.empty(0, dtype=dtype), K, T, M=M)
    assert ops.proj_wx_supported(torch.empty(0, dtype=dtype), K // 2, T, M=M)
    a = _amp(K // 2, dtype)
    Lm, Rm = _ints(M, K, a, 901), _ints(K, T, a, 902, by_cols=True)
    _exact_bound(Lm, Rm)
    h = K // 2
    S1, S2 = Lm[:, :h] @ Rm[:h], Lm[:, h:] @ Rm[h:]
    _assert_decided(S1, dtype)
    first = _rne(S1, dtype)
    expect = _rne(torch.where(torch.isfinite(first.double()), S2 + first.double(), S2), dtype)
    expect = torch.where(torch.isfinite(first), expect, first)
    _assert_decided(torch.where(torch.isfinite(first.double()), S2 + first.double(), S2), dtype)
    cu(grid)

    def run(P):
        W, X = P.operand(_cast(Lm, dtype)), P.operand(_cast(Rm, dtype))
        out = P.output((M, T), dtype)
        ops.proj_wx(W[:, :h], X[:h], out=out)
        mid = out.cpu().clone()
        ops.proj_wx(W[:, h:], X[h:], out=out, acc=out)
        return mid, out.cpu()
    mid, out = _run_twice(dev, poison, run)
    assert _same_bits(mid, first) and _same_bits(out, expect)


@pytest.mark.parametrize("grid,poison", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K", [(16, 256), (32, 512), (16, 512)])
def test_wx_wgrad_fused_exact(backend, cu, dtype, M, K, grid, poison):
    """cad_proj_wx_wgrad, fused: out = round(W X) and dW (K, M) = X Y^T exactly (fp32 slots, summed); whole 128-token blocks only
    (a ragged T is refused, asserted)."""
    name, dev = backend
    T = 128 * 3 if grid is None else 128 * 7
    x0 = torch.empty(0, dtype=dtype)
    assert ops.proj_wx_wgrad_supported(x0, M, K, T) and not ops.proj_wx_wgrad_supported(x0, M, K, T + 8)
    assert not ops.proj_wx_wgrad_supported(x0, 48, K, T) and not ops.proj_wx_wgrad_supported(x0, M, 128, T)
    a = _amp(K, dtype)
    Wm, Xm, Ym = _ints(M, K, a, 1000 + K), _ints(K, T, a, 1001 + K, by_cols=True), _ints(M, T, 4, 1002 + K)
    _exact_bound(Wm, Xm)
    _exact_bound(Xm, Ym.t())
    S = Wm @ Xm
    _assert_decided(S, dtype)
    cu(grid)
    nslot = _wgrad_slots(T)
    assert nslot == (T // 128 if grid is None else grid)

    def run(P):
        W, X, Y = P.operand(_cast(Wm, dtype)), P.operand(_cast(Xm, dtype)), P.operand(_cast(Ym, dtype))
        out = P.output((M, T), dtype)
        part = P.output((nslot, K * M), F32, full_rows=True)
        ops.proj_wx_wgrad(W, X, Y, out=out, part=part.view(nslot, K, M))
        return out.cpu(), part.cpu()
    out, part = _run_twice(dev, poison, run)
    assert _same_bits(out, _rne(S, dtype))
    assert torch.equal(part.view(nslot, K, M).double().sum(0), Xm @ Ym.t())


@pytest.mark.parametrize("grid,poison", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K", [(48, 512), (7, 256), (64, 512), (40, 256)])
def test_wgrad_only_exact(backend, cu, dtype, M, K, grid, poison):
    """cad_proj_wx_wgrad with W == NULL: dW = Y X^T alone, any M <= 64 (rows >= M of the Y tile re-read row M - 1: never stored)."""
    name, dev = backend
    T = 128 * 2 if grid is None else 128 * 9
    x0 = torch.empty(0, dtype=dtype)
    assert ops.proj_wgrad_only_supported(x0, M, K, T) and not ops.proj_wgrad_only_supported(x0, 65, K, T)
    assert not ops.proj_wgrad_only_supported(x0, M, K, T + 64)
    Xm, Ym = _ints(K, T, 8, 1100 + K), _ints(M, T, 8, 1101 + M, by_cols=True)
    _exact_bound(Xm, Ym.t())
    cu(grid)
    nslot = _wgrad_slots(T)

    def run(P):
        X, Y = P.operand(_cast(Xm, dtype)), P.operand(_cast(Ym, dtype))
        part = P.output((nslot, K * M), F32, full_rows=True)
        ops.proj_wgrad_only(X, Y, part=part.view(nslot, K, M))
        return part.cpu()
    part = _run_twice(dev, poison, run)
    assert torch.equal(part.view(nslot, K, M).double().sum(0), Xm @ Ym.t())


@pytest.mark.parametrize("grid,poison", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,panels", [(128, 256, 1), (256, 512, 2), (128, 512, 2), (256, 256, 1)])
def test_xTw_exact(backend, cu, dtype, M, K, panels, grid, poison):
    """cad_proj_xTw, one panel and two: fp32 accumulation over both panels and all of K, one rounding."""
    name, dev = backend
    T = 200 if grid is None else 6 * 128 + 72
    x0 = torch.empty(0, dtype=dtype)
    assert ops.proj_xTw_supported(x0, M, K, T) and not ops.proj_xTw_supported(x0, 192, K, T) and not ops.proj_xTw_supported(x0, M, K, T + 4)
    a = _amp(K * panels, dtype)
    Wm = _ints(M, K, a, 1200 + K)
    Xs = [_ints(K, T, a, 1201 + K + p, by_cols=True) for p in range(panels)]
    S = sum(X.t() @ Wm.t() for X in Xs)
    _exact_bound(torch.cat([X.t() for X in Xs], 1), torch.cat([Wm.t()] * panels, 0))
    _assert_decided(S, dtype)
    cu(grid)

    def run(P):
        W = P.operand(_cast(Wm, dtype))
        X = [P.operand(_cast(x, dtype)) for x in Xs]
        out = P.output((T, M), dtype)
        ops.proj_xTw(W, X[0], X[1] if panels == 2 else None, out=out)
        return out.cpu()
    out = _run_twice(dev, poison, run)
    assert _same_bits(out, _rne(S, dtype))


@pytest.mark.parametrize("grid,poison", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("col_fastest", [0, 1])
def test_gemm_stream_out_t_exact(backend, cu, dtype, col_fastest, grid, poison):
    """cad_gemm_stream / CAD_GEMM_OUT_T_BF16: out (C, R) = round((A B)^T), 2 x 3 tiles of 256 x 256 -- under the override one workgroup
    owns three or six items (the ring and its counted waits run across item boundaries and store bursts)."""
    name, dev = backend
    R, Cc, K = 512, 768, 96
    lib = L.get_lib()
    assert lib.cad_gemm_stream_supported(R, Cc, K, 1) and not lib.cad_gemm_stream_supported(R, Cc + 128, K, 1)
    assert not lib.cad_gemm_stream_supported(R, Cc, K + 16, 1)
    a = _amp(K, dtype)
    Am, Bm = _ints(R, K, a, 1300), _ints(K, Cc, a, 1301, by_cols=True)
    _exact_bound(Am, Bm)
    S = Am @ Bm
    _assert_decided(S, dtype)
    cu(grid)

    def run(P):
        A, B = P.operand(_cast(Am, dtype)), P.operand(_cast(Bm, dtype))
        out = P.output((Cc, R), dtype)
        _gemm_stream(A, B, out, R, Cc, K, 1, ops.GEMM_OUT_T_BF16, col_fastest)
        return out.cpu()
    out = _run_twice(dev, poison, run)
    assert _same_bits(out, _rne(S.t().contiguous(), dtype))


@pytest.mark.parametrize("grid,poison", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("col_fastest", [0, 1])
def test_gemm_stream_partials_exact(backend, cu, dtype, col_fastest, grid, poison):
    """cad_gemm_stream / CAD_GEMM_PARTIALS: 2 x 1 tiles x 5 K slices of 3 chunks (shorter than the ring) resp. 6 chunks; the sum of the
    fp32 tiles is the product exactly.  The slice count is the caller's (python side at the REAL CU count) while the C side is lowered:
    one workgroup owns five or ten (tile, slice) items."""
    name, dev = backend
    R, Cc, ns = 512, 256, 5
    K = ns * 32 * (3 if col_fastest else 6)
    assert L.get_lib().cad_gemm_stream_supported(R, Cc, K, ns) and not L.get_lib().cad_gemm_stream_supported(R, Cc, K, 4)
    Am, Bm = _ints(R, K, 8, 1400), _ints(K, Cc, 8, 1401, by_cols=True)
    _exact_bound(Am, Bm)
    cu(grid)

    def run(P):
        A, B = P.operand(_cast(Am, dtype)), P.operand(_cast(Bm, dtype))
        out = P.output((ns, R * Cc), F32, full_rows=True)
        _gemm_stream(A, B, out, R, Cc, K, ns, ops.GEMM_PARTIALS, col_fastest)
        return out.cpu()
    out = _run_twice(dev, poison, run)
    assert torch.equal(out.view(ns, R, Cc).double().sum(0), Am @ Bm)
    kp = K // ns
    for s in range(ns):  # every slice is its own k range
        assert torch.equal(out.view(ns, R, Cc)[s].double(), Am[:, s * kp:(s + 1) * kp] @ Bm[s * kp:(s + 1) * kp])


def test_gemm_stream_partials_through_ops_at_the_real_cu_count(backend, cu):
    """ops.wgrad_cm_tm keeps sizing its K slices with the real CU count while the launcher's grid is lowered to two workgroups."""
    name, dev = backend
    M, N, T = 256, 256, 32 * 12
    Am, Bm = _ints(M, T, 8, 1500), _ints(T, N, 8, 1501, by_cols=True)
    _exact_bound(Am, Bm)
    assert ops.gemm_stream_slices(M, N, T) == 12
    cu(2)
    out = ops.wgrad_cm_tm(_cast(Am, BF).to(dev), _cast(Bm, BF).to(dev))
    assert out is not None and torch.equal(out.cpu().double(), Am @ Bm)
    assert ops.wgrad_cm_tm(_cast(Am, BF).to(dev)[:200], _cast(Bm, BF).to(dev)) is None


def _e4m3_ints(rows, cols, seed, by_cols=False):
    """Integers exactly representable in e4m3 (|v| <= 16: four significand bits)."""
    return _ints(rows, cols, 16, seed, by_cols=by_cols)


def _fp8_bytes(m):
    q = m.float().to(ops.FP8)
    assert torch.equal(q.double(), m)
    return q.view(torch.uint8)


@pytest.mark.parametrize("grid,poison", VARIANTS)
@pytest.mark.parametrize("K", [256, 512])
def test_wxT_fp8_exact(backend, cu, K, grid, poison):
    """cad_proj_wxT_fp8 with power-of-two scales: out = round(S * sw[m] * sx[t]) exactly (the scaling is exact, one rounding to bf16)."""
    name, dev = backend
    assert ops.fp8_proj_supported(torch.empty(0, dtype=BF), K) and not ops.fp8_proj_supported(torch.empty(0, dtype=BF), 128)
    NT = 64
    M, T = 150, (3 * NT + 13 if grid is None else 9 * NT + 37)
    Lm, Rm = _e4m3_ints(M, K, 1600 + K), _e4m3_ints(K, T, 1601 + K, by_cols=True)
    _exact_bound(Lm, Rm)
    S = Lm @ Rm
    _assert_decided(S, BF)
    g = torch.Generator().manual_seed(K)
    sw = torch.ldexp(torch.ones(M), torch.randint(-12, 13, (M,), generator=g)).float()
    sx = torch.ldexp(torch.ones(T), torch.randint(-12, 13, (T,), generator=g)).float()
    expect = (_rne(S, BF).double() * sw.double()[:, None] * sx.double()[None, :]).float().to(BF)  # (power-of-two scaling commutes with the rounding)
    assert torch.equal(expect.double(), _rne(S, BF).double() * sw.double()[:, None] * sx.double()[None, :])
    cu(grid)

    def run(P):
        Wq, Xq = P.operand(_fp8_bytes(Lm)), P.operand(_fp8_bytes(Rm.t().contiguous()))
        out = P.output((M, T), BF)
        ops.proj_wxT_fp8(Wq, P.operand(sw), Xq, P.operand(sx), out=out)
        return out.cpu()
    out = _run_twice(dev, poison, run)
    assert _same_bits(out, expect)


@pytest.mark.parametrize("grid,poison", VARIANTS)
@pytest.mark.parametrize("ta,tb", [(False, False), (True, False), (False, True), (True, True)])
def test_gemm_f32_exact(backend, cu, ta, tb, grid, poison):
    """cad_gemm_f32, plain and transposed operand views, ragged in all three dimensions, with an integer addend: the product exactly.
    (One tile per workgroup: the CU count only selects the tile configuration -- lowered, the 128 x 128 one.)"""
    name, dev = backend
    M, N, K = 130, 257, 33 if grid is None else 200
    Am, Bm, Dm = _ints(M, K, 64, 1700), _ints(K, N, 64, 1701, by_cols=True), _ints(M, N, 1000, 1702, signed_groups=False)
    _exact_bound(Am, Bm, Dm)
    cu(grid)

    def run(P):
        A = P.operand(Am.t().contiguous().float()).t() if ta else P.operand(Am.float())
        B = P.operand(Bm.t().contiguous().float()).t() if tb else P.operand(Bm.float())
        out = P.output((M, N), F32)
        ops.mm_f32(A, B, out=out, addend=None)
        out2 = P.output((M, N), F32, init=Dm.float())
        ops.mm_f32(A, B, out=out2, addend=out2)
        return out.cpu(), out2.cpu()
    out, out2 = _run_twice(dev, poison, run)
    assert torch.equal(out.double(), Am @ Bm) and torch.equal(out2.double(), Am @ Bm + Dm)


@pytest.mark.parametrize("grid,poison", VARIANTS)
def test_gemm_f32_batched_exact(backend, cu, grid, poison):
    """The batched form on the permuted channel-major views the mixer builds for the K slices of a weight gradient."""
    name, dev = backend
    M, N, n, Kc = 70, 90, 3, 64
    Ym, Xm = _ints(M, n * Kc, 64, 1800), _ints(N, n * Kc, 64, 1801)
    _exact_bound(Ym, Xm.t())
    cu(grid)

    def run(P):
        y, x = P.operand(Ym.float()), P.operand(Xm.float())
        ya = y.unflatten(1, (n, Kc)).permute(1, 0, 2)
        xb = x.unflatten(1, (n, Kc)).permute(1, 2, 0)
        return ops.bmm_f32(ya, xb).cpu()
    part = _run_twice(dev, poison, run)
    for s in range(n):
        assert torch.equal(part[s].double(), Ym[:, s * Kc:(s + 1) * Kc] @ Xm[:, s * Kc:(s + 1) * Kc].t())


# =========================================================================================================================================
# B, real grid (GPU only): every workgroup takes >= 3 blocks / items through real asynchronous DMA; still integers, still bit-exact
# =========================================================================================================================================
def _long_T(name, tail):
    if name == "emu":
        pytest.skip("real-grid long stream: device only")
    return 3 * ops._cu_count() * 128 + tail


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [64, 512])
def test_wxT_real_grid(backend, dtype, K):
    name, dev = backend
    T, M = _long_T(name, 72 + 5), 96
    a = _amp(K, dtype)
    Lm, Rm = _ints(M, K, a, 2000 + K), _ints(K, T, a, 2001 + K, by_cols=True)
    _exact_bound(Lm, Rm)
    S = Lm @ Rm
    _assert_decided(S, dtype)
    out = ops.proj_wxT(_cast(Lm, dtype).to(dev), _cast(Rm.t().contiguous(), dtype).to(dev))
    assert _same_bits(out.cpu(), _rne(S, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("addend", ["none", "alias"])
def test_wx_thin_k_real_grid(backend, dtype, addend):
    name, dev = backend
    T, M, K = _long_T(name, 72), 130, 24
    a = _amp(K, dtype)
    Lm, Rm = _ints(M, K, a, 2100), _ints(K, T, a, 2101, by_cols=True)
    acc = _ints(M, T, 2 ** PBITS[dtype], 2102, signed_groups=False) if addend == "alias" else None
    _exact_bound(Lm, Rm, acc)
    S = Lm @ Rm
    _assert_decided(S, dtype)
    W, X = _cast(Lm, dtype).to(dev), _cast(Rm, dtype).to(dev)
    if acc is None:
        out, expect = ops.proj_wx(W, X), _rne(S, dtype)
    else:
        out = _cast(acc, dtype).to(dev)
        ops.proj_wx(W, X, out=out, acc=out)
        expect = (_rne(S, dtype).float() + acc.float()).to(dtype)
    assert _same_bits(out.cpu(), expect)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,addend", [(48, 256, False), (64, 512, True)])
def test_wx_thin_m_real_grid(backend, dtype, M, K, addend):
    name, dev = backend
    T = _long_T(name, 72)
    a = _amp(K, dtype)
    Lm, Rm = _ints(M, K, a, 2200 + K), _ints(K, T, a, 2201 + K, by_cols=True)
    acc = _ints(M, T, 2 ** PBITS[dtype], 2202, signed_groups=False) if addend else None
    _exact_bound(Lm, Rm, acc)
    S = Lm @ Rm
    _assert_decided(S, dtype)
    out = ops.proj_wx(_cast(Lm, dtype).to(dev), _cast(Rm, dtype).to(dev), acc=None if acc is None else _cast(acc, dtype).to(dev))
    assert _same_bits(out.cpu(), _rne(S if acc is None else S + acc, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fused", [True, False])
def test_wx_wgrad_real_grid(backend, dtype, fused):
    name, dev = backend
    T, K = _long_T(name, 128 * 5), 256
    M = 16 if fused else 40
    assert _wgrad_slots(T) == 256 and T // 128 >= 3 * 256
    a = _amp(K, dtype)
    Wm, Xm, Ym = _ints(M, K, a, 2300), _ints(K, T, a, 2301, by_cols=True), _ints(M, T, 4, 2302)
    _exact_bound(Xm, Ym.t())
    X, Y = _cast(Xm, dtype).to(dev), _cast(Ym, dtype).to(dev)
    if fused:
        _exact_bound(Wm, Xm)
        S = Wm @ Xm
        _assert_decided(S, dtype)
        out, dW = ops.proj_wx_wgrad(_cast(Wm, dtype).to(dev), X, Y)
        assert _same_bits(out.cpu(), _rne(S, dtype))
        assert torch.equal(dW.cpu().double(), Xm @ Ym.t())
    else:
        dW = ops.proj_wgrad_only(X, Y)
        assert torch.equal(dW.cpu().double(), Ym @ Xm.t())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("panels", [1, 2])
def test_xTw_real_grid(backend, dtype, panels):
    name, dev = backend
    T, M, K = _long_T(name, 72), 128, 256
    a = _amp(K * panels, dtype)
    Wm = _ints(M, K, a, 2400)
    Xs = [_ints(K, T, a, 2401 + p, by_cols=True) for p in range(panels)]
    S = sum(X.t() @ Wm.t() for X in Xs)
    _exact_bound(torch.cat([X.t() for X in Xs], 1), torch.cat([Wm.t()] * panels, 0))
    _assert_decided(S, dtype)
    Xd = [_cast(x, dtype).to(dev) for x in Xs]
    out = ops.proj_xTw(_cast(Wm, dtype).to(dev), Xd[0], Xd[1] if panels == 2 else None)
    assert _same_bits(out.cpu(), _rne(S, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,col_fastest", [("out_t", 0), ("out_t", 1), ("partials", 0), ("partials", 1)])
def test_gemm_stream_real_grid(backend, dtype, mode, col_fastest):
    """3 * CUs + 2 work items: OUT_T as 2 row tiles x (items / 2) column tiles, PARTIALS as one tile x items K slices of four chunks."""
    name, dev = backend
    if name == "emu":
        pytest.skip("real-grid long stream: device only")
    items = 3 * ops._cu_count() + 2
    if mode == "out_t":
        R, Cc, K, ns = 512, 256 * (items // 2), 64, 1
    else:
        R, Cc, ns = 256, 256, items
        K = ns * 128
    a = _amp(K, dtype) if mode == "out_t" else 4
    Am, Bm = _ints(R, K, a, 2500), _ints(K, Cc, a, 2501, by_cols=True)
    _exact_bound(Am, Bm)
    S = Am @ Bm
    A, B = _cast(Am, dtype).to(dev), _cast(Bm, dtype).to(dev)
    if mode == "out_t":
        _assert_decided(S, dtype)
        out = torch.empty((Cc, R), dtype=dtype, device=dev)
        _gemm_stream(A, B, out, R, Cc, K, 1, ops.GEMM_OUT_T_BF16, col_fastest)
        assert _same_bits(out.cpu(), _rne(S.t().contiguous(), dtype))
    else:
        out = torch.empty((ns, R, Cc), dtype=F32, device=dev)
        _gemm_stream(A, B, out, R, Cc, K, ns, ops.GEMM_PARTIALS, col_fastest)
        assert torch.equal(out.double().sum(0).cpu(), S)


def test_wxT_fp8_real_grid(backend):
    name, dev = backend
    T, M, K = _long_T(name, 72 + 5), 96, 256
    Lm, Rm = _e4m3_ints(M, K, 2600), _e4m3_ints(K, T, 2601, by_cols=True)
    _exact_bound(Lm, Rm)
    S = Lm @ Rm
    _assert_decided(S, BF)
    out = ops.proj_wxT_fp8(_fp8_bytes(Lm).to(dev), torch.ones(M, device=dev), _fp8_bytes(Rm.t().contiguous()).to(dev),
                           torch.full((T,), 0.5, device=dev))
    assert _same_bits(out.cpu(), _rne(S * 0.5, BF))


# =========================================================================================================================================
# D: ill-conditioned non-integer operands, derived per-element bound; NaN / inf placement; overflow
# =========================================================================================================================================
def _illcond(rows, K, cols, dtype, seed):
    """L (rows, K), R (K, cols) in dtype: rows of L and columns of R scaled by powers of two (2^+-20 for bf16; binary16's own range
    2^-24 .. 2^15 leaves 2^-6 .. 2^4 per operand), and in every second row of L the odd k repeat the even k up to a 2^-5 relative
    perturbation while the odd rows of R negate the even ones: these sums cancel to ~2^-6 of sum |l r|."""
    g = torch.Generator().manual_seed(seed)
    Lm, Rm = torch.randn(rows, K, generator=g), torch.randn(K, cols, generator=g)
    Rm[1::2] = -Rm[0::2][: Rm[1::2].shape[0]]
    pert = 1.0 + torch.randn(rows, K // 2, generator=g) * 2.0 ** -5
    Lm[::2, 1:2 * (K // 2):2] = Lm[::2, 0:2 * (K // 2):2] * pert[::2]
    lo, hi = (-20, 21) if dtype != HF else (-6, 5)
    Lm = torch.ldexp(Lm, torch.randint(lo, hi, (rows, 1), generator=g))
    Rm = torch.ldexp(Rm, torch.randint(lo, hi, (1, cols), generator=g))
    return Lm.to(dtype), Rm.to(dtype)


def _check_bound(kernel, out, Ld, Rd, dtype_out, red_len, acc=None, first_rounding=False):
    """|out - S| <= u |S| (1 + u) + (red_len + 2) 2^-24 (sum |l r| + |acc|) + red_len 2^-126, per element; fp16 outputs add half the
    spacing of binary16's subnormals (2^-25: below 2^-14 the format's error is absolute).  first_rounding: the thin-K addend path rounds
    the product before the addition (include/caduceus_hip.h) -- its first rounding adds u |W X| (1 + u)."""
    L64, R64 = Ld.double(), Rd.double()
    P = L64 @ R64
    S = P if acc is None else P + acc.double()
    A = L64.abs() @ R64.abs() + (0 if acc is None else acc.double().abs())
    u = UNIT[dtype_out]
    tol = u * S.abs() * (1 + u) + (red_len + 2) * 2.0 ** -24 * A + red_len * 2.0 ** -126
    if dtype_out == HF:
        tol = tol + 2.0 ** -25
    if first_rounding:
        tol = tol + u * P.abs() * (1 + u) + (2.0 ** -25 if dtype_out == HF else 0.0)
    o = out.double()
    assert bool(torch.isfinite(o).all())
    cancel = float((S.abs() / A.clamp_min(1e-300)).min())
    assert cancel < 2.0 ** -8, cancel  # the case does contain cancelling sums
    ratio = float(((o - S).abs() / tol).max())
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print(f"[section D] {kernel}: worst err / tol = {ratio:.3f}")
    assert ratio <= 1.0, (kernel, ratio)


@pytest.mark.parametrize("dtype", DTYPES)
def test_illconditioned_16bit_projections(backend, cu, dtype):
    """Every 16-bit-output projection at the derived bound, two workgroups walking several blocks."""
    name, dev = backend
    cu(2)
    tag = "bf16" if dtype == BF else "f16"
    d = lambda t: t.to(dev)
    # cad_proj_wxT
    for K in (64, 512):
        Ld, Rd = _illcond(70, K, 5 * 64 + 29, dtype, 3000 + K)
        _check_bound(f"proj_wxT[{tag}]", ops.proj_wxT(d(Ld), d(Rd.t().contiguous())).cpu(), Ld, Rd, dtype, K)
    # cad_proj_wx thin K, plain and with the addend (two roundings)
    for K in (24, 64):
        Ld, Rd = _illcond(130, K, 5 * 64 + 24, dtype, 3100 + K)
        _check_bound(f"proj_wx thin-K[{tag}]", ops.proj_wx(d(Ld), d(Rd)).cpu(), Ld, Rd, dtype, K)
        acc = (-(Ld.double() @ Rd.double()) * (1 + 2.0 ** -4 * torch.randn(130, Rd.shape[1], generator=torch.Generator().manual_seed(K)))).to(dtype)
        _check_bound(f"proj_wx thin-K + acc[{tag}]", ops.proj_wx(d(Ld), d(Rd), acc=d(acc)).cpu(), Ld, Rd, dtype, K, acc=acc, first_rounding=True)
    # cad_proj_wx thin M / deep K, plain and with the addend (one rounding)
    for M, K in ((48, 256), (33, 512)):
        Ld, Rd = _illcond(M, K, 5 * 128 + 40, dtype, 3200 + K)
        _check_bound(f"proj_wx thin-M[{tag}]", ops.proj_wx(d(Ld), d(Rd)).cpu(), Ld, Rd, dtype, K)
        acc = (-(Ld.double() @ Rd.double()) * (1 + 2.0 ** -4 * torch.randn(M, Rd.shape[1], generator=torch.Generator().manual_seed(K)))).to(dtype)
        _check_bound(f"proj_wx thin-M + acc[{tag}]", ops.proj_wx(d(Ld), d(Rd), acc=d(acc)).cpu(), Ld, Rd, dtype, K, acc=acc)
    # cad_proj_xTw, two panels: canonical L = [X1^T X2^T] (T, 2K), R = [W^T ; W^T]
    M, K, T = 128, 256, 5 * 128 + 40
    Ld, Rd = _illcond(T, 2 * K, M, dtype, 3300)
    Rd[K:] = Rd[:K]
    X1, X2, W = Ld[:, :K].t().contiguous(), Ld[:, K:].t().contiguous(), Rd[:K].t().contiguous()
    S, A = Ld.double() @ Rd.double(), Ld.double().abs() @ Rd.double().abs()
    if float((S.abs() / A).min()) < 2.0 ** -8:  # (tying the two W copies keeps the cancellation inside each panel)
        _check_bound(f"proj_xTw[{tag}]", ops.proj_xTw(d(W), d(X1), d(X2)).cpu(), Ld, Rd, dtype, 2 * K)
    else:
        raise AssertionError("xTw case without cancellation")
    # cad_gemm_stream, OUT_T
    R_, Cc, K = 256, 512, 128
    Ld, Rd = _illcond(R_, K, Cc, dtype, 3400)
    out = torch.empty((Cc, R_), dtype=dtype, device=dev)
    _gemm_stream(d(Ld), d(Rd), out, R_, Cc, K, 1, ops.GEMM_OUT_T_BF16, 1)
    _check_bound(f"gemm_stream out_t[{tag}]", out.cpu().t(), Ld, Rd, dtype, K)
    # fp32 outputs: the weight-gradient slots and the CAD_GEMM_PARTIALS tiles after their sum (u = 0, K = the reduction length)
    K, M, T = 256, 40, 128 * 6
    Yd, Xt = _illcond(M, T, K, dtype, 3500)       # dW (M, K) = Y (M, T) X^T
    dW = ops.proj_wgrad_only(d(Xt.t().contiguous()), d(Yd))
    _check_bound(f"proj_wgrad_only[{tag}]", dW.cpu(), Yd, Xt, F32, T + 2)
    Ld, Rd = _illcond(256, 32 * 12, 256, dtype, 3600)
    out = ops.wgrad_cm_tm(d(Ld), d(Rd))
    _check_bound(f"gemm_stream partials[{tag}]", out.cpu(), Ld, Rd, F32, 32 * 12 + 12)


def test_illconditioned_fp8_and_f32(backend, cu):
    name, dev = backend
    cu(2)
    K, M, T = 256, 70, 5 * 64 + 29
    g = torch.Generator().manual_seed(3700)
    Ld, Rd = _illcond(M, K, T, BF, 3700)
    Lq = (Ld.float() / Ld.float().abs().amax(1, keepdim=True) * 400).to(ops.FP8)
    Rq = (Rd.float() / Rd.float().abs().amax(0, keepdim=True) * 400).to(ops.FP8)
    sw = torch.ldexp(torch.rand(M, generator=g) + 0.5, torch.randint(-20, 21, (M,), generator=g)).float()
    sx = torch.ldexp(torch.rand(T, generator=g) + 0.5, torch.randint(-20, 21, (T,), generator=g)).float()
    out = ops.proj_wxT_fp8(Lq.view(torch.uint8).to(dev), sw.to(dev), Rq.t().contiguous().view(torch.uint8).to(dev), sx.to(dev))
    # canonical operands with the scales folded in (exact in fp64); the scale product and its application are two more fp32 roundings
    _check_bound("proj_wxT_fp8", out.cpu(), Lq.double() * sw.double()[:, None], Rq.double() * sx.double()[None, :], BF, K + 2)
    for ta, tb in ((False, False), (True, True)):
        Ld, Rd = _illcond(130, 200, 257, F32, 3800)
        A = Ld.t().contiguous().to(dev).t() if ta else Ld.to(dev)
        B = Rd.t().contiguous().to(dev).t() if tb else Rd.to(dev)
        _check_bound("gemm_f32", ops.mm_f32(A, B).cpu(), Ld, Rd, F32, 200)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_values_stay_in_their_row_or_column(backend, cu, dtype):
    """A NaN in one token and an inf in one channel: exactly that output column / row is non-finite, every other element keeps its bits."""
    name, dev = backend
    cu(2)
    d = lambda t: t.to(dev)
    g = torch.Generator().manual_seed(4000)
    rnd = lambda *s: (torch.randn(*s, generator=g) + 0.01).to(dtype)

    def check(run, Lc, Rc, row, col, transposed=False):
        """run(L, R) -> out in canonical orientation; NaN goes into column `col` of R (a token), inf into row `row` of L (a channel)."""
        clean = run(Lc, Rc)
        Lp, Rp = Lc.clone(), Rc.clone()
        Rp[3, col] = float("nan")
        Lp[row, 5] = float("inf")
        bad = run(Lp, Rp)
        mask = torch.zeros(clean.shape, dtype=torch.bool)
        mask[row, :] = True
        mask[:, col] = True
        assert bool(torch.isfinite(clean.float()).all())
        assert bool((~torch.isfinite(bad.float()))[mask].all()) and bool(torch.isnan(bad.float())[:, col].all())
        assert torch.equal(_bits(bad)[~mask], _bits(clean)[~mask])

    T = 5 * 64 + 24
    check(lambda l, r: ops.proj_wxT(d(l), d(r.t().contiguous())).cpu(), rnd(70, 64), rnd(64, T), 17, T - 3)
    check(lambda l, r: ops.proj_wx(d(l), d(r)).cpu(), rnd(130, 24), rnd(24, T), 129, T - 1)
    T = 5 * 128 + 40
    check(lambda l, r: ops.proj_wx(d(l), d(r)).cpu(), rnd(33, 128), rnd(128, T), 32, T - 9)
    check(lambda l, r: ops.proj_xTw(d(r.t().contiguous()), d(l.t().contiguous())).cpu(), rnd(T, 256), rnd(256, 128), T - 2, 77)
    check(lambda l, r: ops.proj_wgrad_only(d(r.t().contiguous()), d(l)).cpu(), rnd(40, 128 * 5), rnd(128 * 5, 256), 39, 200)

    def gs(l, r):
        out = torch.empty((r.shape[1], l.shape[0]), dtype=dtype, device=dev)
        _gemm_stream(d(l), d(r), out, l.shape[0], r.shape[1], l.shape[1], 1, ops.GEMM_OUT_T_BF16, 0)
        return out.cpu().t()
    check(gs, rnd(256, 64), rnd(64, 512), 255, 300)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_beyond_the_output_range_become_inf(backend, cu, dtype):
    """A finite fp32 sum beyond the output type's range is +-inf -- not NaN, not the largest finite value.  The sums are powers of two
    added up to max + half an ulp (a tie: nearest-even rounds it to 2^emax+1 = inf, truncation would keep the largest finite value);
    every partial sum is exact in fp32 and finite."""
    name, dev = backend
    cu(2)
    d = lambda t: t.to(dev)
    p = PBITS[dtype]
    e_hi = 127 if dtype == BF else 15
    ew = e_hi // 2 + 1
    ex = e_hi - ew

    def operands(rows, K, cols, r_pos, r_neg, c_big):
        """row r_pos (r_neg) of L times column c_big of R = +-(2^(e_hi+1) - 2^(e_hi-p)); everything else small."""
        Lm, Rm = torch.full((rows, K), 2.0 ** -3, dtype=torch.float64), torch.full((K, cols), 2.0 ** -3, dtype=torch.float64)
        Lm[r_pos], Lm[r_neg], Rm[:, c_big] = 0.0, 0.0, 0.0
        for i in range(p + 1):  # 2^e_hi + 2^(e_hi-1) + ... + 2^(e_hi-p)
            Lm[r_pos, i], Lm[r_neg, i], Rm[i, c_big] = 2.0 ** ew, -(2.0 ** ew), 2.0 ** (ex - i)
        return _cast(Lm, dtype), _cast(Rm, dtype)

    def check(out, Ld, Rd, r_pos, r_neg, c_big):
        S = Ld.double() @ Rd.double()
        assert float(S[r_pos, c_big]) == 2.0 ** (e_hi + 1) - 2.0 ** (e_hi - p) and float(S[r_pos, c_big]) < 3.4028234e38 * 1.0000001
        expect = S.float().to(dtype)
        assert float(expect[r_pos, c_big]) == float("inf") and float(expect[r_neg, c_big]) == float("-inf")
        assert int(torch.isinf(expect.float()).sum()) == 2
        assert _same_bits(out, expect)

    T = 5 * 64 + 24
    Ld, Rd = operands(70, 64, T, 3, 69, T - 2)
    check(ops.proj_wxT(d(Ld), d(Rd.t().contiguous())).cpu(), Ld, Rd, 3, 69, T - 2)
    Ld, Rd = operands(130, 24, T, 3, 129, T - 2)
    check(ops.proj_wx(d(Ld), d(Rd)).cpu(), Ld, Rd, 3, 129, T - 2)
    T = 5 * 128 + 40
    Ld, Rd = operands(33, 128, T, 0, 32, T - 2)
    check(ops.proj_wx(d(Ld), d(Rd)).cpu(), Ld, Rd, 0, 32, T - 2)
    Ld, Rd = operands(T, 256, 128, 1, T - 1, 100)
    check(ops.proj_xTw(d(Rd.t().contiguous()), d(Ld.t().contiguous())).cpu(), Ld, Rd, 1, T - 1, 100)
    Ld, Rd = operands(256, 64, 512, 2, 255, 511)
    out = torch.empty((512, 256), dtype=dtype, device=dev)
    _gemm_stream(d(Ld), d(Rd), out, 256, 512, 64, 1, ops.GEMM_OUT_T_BF16, 1)
    check(out.cpu().t().contiguous(), Ld, Rd, 2, 255, 511)


def test_zz_report_section_d(backend):
    """Prints the worst err / tol per kernel collected by the section D tests of this run (pytest -s)."""
    for k in sorted(WORST):
        print(f"[section D] worst err / tol  {k}: {WORST[k]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
