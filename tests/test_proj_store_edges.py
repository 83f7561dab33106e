"""The store side of the d_model-256 projection kernels at its edges: cad_proj_xTw (out_proj) after its 8-byte output pieces became 16-byte
stores built by a lane exchange (csrc/cad_stream.h: cad_d_pair16), with cad_gemm_stream in its token-major mode (d(x2d), the same result
layout, 8-byte stores) and the two channel-major writers cad_proj_wxT (in_proj, d(y)) and thin-K cad_proj_wx (dt_proj) beside it.  Bit for bit against exact sums, on the
host emulator and on the GPU: integer operands whose partial sums stay below 2^24 in any order (asserted), so the fp64 product rounded
once IS the result, whatever moves the bytes.

What can go wrong in the new code, and the smallest shapes that show it:
 * the exchange pairs the wrong accumulator tiles or lane rows, or a lane's 16 bytes land at the wrong offset of the 64-byte run: any
   full block shows it -- T = one store instruction's 16 tokens, one tile, one tile -+ 8 tokens (the entry points take T % 8 == 0: a
   token-quad is not a legal step for them; the channel-major writers, which take any T, also get tile -+ 4);
 * the counted waits behind a store burst allow for cad_proj_xTw's new number of store instructions (half as many): only several blocks / items in
   ONE workgroup on the GPU reach that wait, so the CU count the launchers size their grids with is lowered to 1 and 2
   (cad_debug_set_cu_count) and the walks get grid - 1, grid and grid + 1 blocks, the last one ragged; with K = 512 and two panels every
   block of cad_proj_xTw runs through all ring slots four times;
 * the 16-byte form is only taken for 16-byte aligned output rows: a row pitch of 8 k + 4 elements and a base 8 bytes off take the
   8-byte form under waits sized for the 16-byte one; bytes around the output view must stay untouched;
 * cad_gemm_stream: one and two K chunks (items shorter than the ring drain everything) and four (the counted waits);
 * dt_proj with and without the softplus + bias epilogue.  With every pre-activation >= 40 the bf16 epilogue max(x, 0) + exp(-|x|)
   is x itself in fp32 (exp(-40) < 2^-57, below half an ulp of any x >= 40), so the exact reference is round(W X + bias).
The tile, ring and wave constants are read from the headers."""
import ctypes as C
import os
import re

import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops

BF = torch.bfloat16
CSRC = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "csrc")


def _const(header, struct, name):
    """`name = <int>` inside `struct <struct> { ... }` of csrc/<header>."""
    src = open(os.path.join(CSRC, header)).read()
    body = src[src.index("struct " + struct):]
    body = body[:body.index("};")]
    m = re.search(r"\b%s = (\d+)\b" % name, body)
    assert m, (header, struct, name)
    return int(m.group(1))


GT_NT, GT_KC, GT_RING = (_const("proj_ring.h", "GtCfg", n) for n in ("NT", "KC", "RING"))          # cad_proj_xTw: 128 tokens, 64 rows, 4 slots
GS_RT, GS_CT, GS_KC, GS_RING = (_const("gemm_stream.h", "GsCfg", n) for n in ("RT", "CT", "KC", "RING"))
GX_NT = _const("proj_wstat.h", "GxCfg", "NT")                                                       # thin-K cad_proj_wx: 64 tokens
GP_NT = 64                                                                                          # cad_proj_wxT at K < 512 (GpCfg::NT)
assert re.search(r"NT = KS >= 16 \? GP_NT16 : %d;" % GP_NT, open(os.path.join(CSRC, "proj_wstat.h")).read())
PIECE = 16   # tokens (cad_proj_xTw) / output rows (cad_gemm_stream) of one store instruction: the 16 columns of an MFMA D tile
E, D, R = 512, 256, 16


@pytest.fixture
def cu(backend):
    """The test-only CU-count override (cad_debug_set_cu_count); always restored."""
    lib = L.get_lib()

    def set_count(n):
        L.check(lib.cad_debug_set_cu_count(int(n or 0)), "cad_debug_set_cu_count")
    yield set_count
    lib.cad_debug_set_cu_count(0)


def _ints(rows, cols, a, seed, lo=None):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-a if lo is None else lo, a + 1, (rows, cols), generator=g).double()


def _bf(m):
    t = m.float().to(BF)
    assert torch.equal(t.double(), m), "operand not exactly representable"
    return t


def _exact(Lm, Rm, extra=0.0):
    b = float((Lm.abs() @ Rm.abs()).max()) + extra
    assert b < 2 ** 24, b


def _rne(S):
    assert torch.equal(S.float().double(), S)
    return S.float().to(BF)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16))


SENT = 0x5A5A


def _out_view(rows, cols, dev, layout):
    """A (rows, cols) bf16 output inside a sentinel-filled buffer.  "aligned": pitch cols + 8, base 16 bytes in; "pitch4": pitch
    cols + 12 (rows alternate between 16-byte aligned and 8 bytes off); "base8": pitch cols + 8, base 8 bytes off 16-byte alignment."""
    pitch, lead = {"aligned": (cols + 8, 8), "pitch4": (cols + 12, 8), "base8": (cols + 8, 4)}[layout]
    buf = torch.full(((rows + 2) * pitch,), SENT, dtype=torch.int16).view(BF).to(dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[pitch + lead:pitch + lead + rows * pitch].view(rows, pitch)[:, :cols]
    return buf, view, (pitch, lead)


def _check_out(buf, view, geom, expect):
    assert _same_bits(view, expect)
    pitch, lead = geom
    rows, cols = expect.shape
    after = buf.cpu().view(torch.int16).clone()
    after[pitch + lead:pitch + lead + rows * pitch].view(rows, pitch)[:, :cols] = SENT
    assert bool((after == SENT).all()), "bytes outside the output view were written"


_REF = {}


def _ref(key, make):
    """References are computed once per shape, shared and never modified."""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


# ---- cad_proj_xTw (out_proj) ------------------------------------------------------------------------------------------------------------
def _xTw_case(M, K, T, panels):
    def make():
        Wm = _ints(M, K, 8, 100 + M)
        Xs = [_ints(K, T, 8, 101 + p) for p in range(panels)]
        _exact(torch.cat([X.t() for X in Xs], 1), torch.cat([Wm.t()] * panels, 0))
        S = sum(X.t() @ Wm.t() for X in Xs)
        assert int((_rne(S).double() != S).sum()) >= 100 or T < 64  # the rounding is exercised
        return Wm, Xs, _rne(S)
    return _ref(("xTw", M, K, T, panels), make)


# (CU override, T): the real grid with one block or less per workgroup; ONE workgroup walking all blocks; two workgroups with
# grid - 1, grid and grid + 1 blocks (the last block of the walk ragged)
XTW_WALKS = [(None, PIECE), (None, GT_NT - 8), (None, GT_NT), (None, GT_NT + 8),
             (1, (GT_RING + 1) * GT_NT + 8), (2, GT_NT), (2, 2 * GT_NT), (2, 2 * GT_NT + 8), (2, 5 * GT_NT - 8)]


@pytest.mark.parametrize("grid,T", XTW_WALKS)
def test_xTw_store_edges(backend, cu, grid, T):
    """out_proj at the real channel counts (D = 256 features: the paired 16-byte stores; K = E = 512, two panels)."""
    name, dev = backend
    Wm, Xs, expect = _xTw_case(D, E, T, 2)
    cu(grid)
    buf, view, geom = _out_view(T, D, dev, "aligned")
    ops.proj_xTw(_bf(Wm).to(dev), _bf(Xs[0]).to(dev), _bf(Xs[1]).to(dev), out=view)
    _check_out(buf, view, geom, expect)


@pytest.mark.parametrize("layout", ["pitch4", "base8"])
@pytest.mark.parametrize("M,K,panels", [(D, E, 2), (D, 256, 1), (128, 256, 1)])
def test_xTw_unaligned_rows_and_narrow_waves(backend, cu, layout, M, K, panels):
    """Output rows that are not 16-byte aligned (8-byte pieces under the waits of the 16-byte form), and M = 128 (one accumulator tile per
    wave: no pair to exchange), several blocks in one workgroup."""
    name, dev = backend
    T = (GT_RING + 1) * GT_NT + 8
    Wm, Xs, expect = _xTw_case(M, K, T, panels)
    cu(1)
    buf, view, geom = _out_view(T, M, dev, layout)
    ops.proj_xTw(_bf(Wm).to(dev), _bf(Xs[0]).to(dev), _bf(Xs[1]).to(dev) if panels == 2 else None, out=view)
    _check_out(buf, view, geom, expect)


# ---- cad_gemm_stream, CAD_GEMM_OUT_T_BF16 (d(x2d)) --------------------------------------------------------------------------------------
def _gemm_stream_out_t(A, B, out, R_, Cc, K, col_fastest):
    stream = L.stream_and_check(A, B, out, contiguous=False)
    a = L.GemmStreamArgs(L.ptr(A), L.ptr(B), L.ptr(out), R_, Cc, K, A.stride(0), B.stride(0), out.stride(0), 1, ops.GEMM_OUT_T_BF16,
                         int(col_fastest))
    L.check(ops._proj_fn("cad_gemm_stream", A.dtype)(C.byref(a), stream), "cad_gemm_stream")


def _gs_case(R_, Cc, K):
    def make():
        Am, Bm = _ints(R_, K, 16, 200 + K), _ints(K, Cc, 16, 201 + K)
        _exact(Am, Bm)
        S = (Am @ Bm).t().contiguous()
        return Am, Bm, _rne(S)
    return _ref(("gs", R_, Cc, K), make)


# K chunks per item: 1, 2 (shorter than the ring: every wait drains), RING (the counted waits behind the store burst);
# (CU override, column tiles): one item; ONE workgroup walking three items; two workgroups with grid - 1, grid, grid + 1 items
# the unaligned layouts only where a workgroup walks several items
GS_CASES = [(nk, grid, ntiles, "aligned") for nk in (1, 2, GS_RING) for grid, ntiles in [(None, 1), (1, 3), (2, 1), (2, 2), (2, 3)]]
GS_CASES += [(nk, grid, 3, layout) for nk in (1, GS_RING) for grid in (1, 2) for layout in ("pitch4", "base8")]


@pytest.mark.parametrize("nk,grid,ntiles,layout", GS_CASES)
def test_gemm_stream_out_t_store_edges(backend, cu, nk, grid, ntiles, layout):
    """d(x2d): out (C, R) token-major = (A (R, K) . B (K, C))^T with R = d_model = one row tile."""
    name, dev = backend
    R_, Cc, K = GS_RT, ntiles * GS_CT, nk * GS_KC
    Am, Bm, expect = _gs_case(R_, Cc, K)
    cu(grid)
    buf, view, geom = _out_view(Cc, R_, dev, layout)
    _gemm_stream_out_t(_bf(Am).to(dev), _bf(Bm).to(dev), view, R_, Cc, K, col_fastest=ntiles & 1)
    _check_out(buf, view, geom, expect)


def test_gemm_stream_out_t_two_row_tiles(backend, cu):
    """R = 2 row tiles: a workgroup's 256-byte runs are the first or the second half of the 1 KB output rows."""
    name, dev = backend
    R_, Cc, K = 2 * GS_RT, 2 * GS_CT, GS_RING * GS_KC
    Am, Bm, expect = _gs_case(R_, Cc, K)
    cu(1)
    buf, view, geom = _out_view(Cc, R_, dev, "aligned")
    _gemm_stream_out_t(_bf(Am).to(dev), _bf(Bm).to(dev), view, R_, Cc, K, col_fastest=0)
    _check_out(buf, view, geom, expect)


# ---- the channel-major writers: cad_proj_wxT (in_proj, d(y)) and thin-K cad_proj_wx (dt_proj) --------------------------------------------
CM_WALKS = [(None, 8), (None, GP_NT - 4), (None, GP_NT), (None, GP_NT + 4), (1, 5 * GP_NT + 8), (2, GP_NT), (2, 2 * GP_NT),
            (2, 2 * GP_NT + 8), (2, 5 * GP_NT - 4)]


@pytest.mark.parametrize("grid,T", CM_WALKS)
def test_wxT_store_edges(backend, cu, grid, T):
    """in_proj: out (M, T) channel-major = W (M, D) X (T, D)^T; any T is allowed; M = 150 leaves the second wave's rows ragged."""
    name, dev = backend
    M = 150

    def make():
        Wm, Xm = _ints(M, D, 8, 300), _ints(T, D, 8, 301)
        _exact(Wm, Xm.t())
        return Wm, Xm, _rne(Wm @ Xm.t())
    Wm, Xm, expect = _ref(("wxT", T), make)
    cu(grid)
    buf, view, geom = _out_view(M, T, dev, "aligned")
    ops.proj_wxT(_bf(Wm).to(dev), _bf(Xm).to(dev), out=view)
    _check_out(buf, view, geom, expect)


assert GX_NT == GP_NT


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("grid,T", [(g, t) for g, t in CM_WALKS if t % 8 == 0] + [(None, GX_NT - 8), (None, GX_NT + 8)])
def test_dt_proj_store_edges(backend, cu, grid, T, bias):
    """dt_proj: out (E, T) = W (E, R) X (R, T) [softplus(. + bias)], thin K = dt_rank."""
    name, dev = backend

    def make():
        Wm, Xm = _ints(E, R, 8, 400, lo=0), _ints(R, T, 8, 401, lo=0)   # non-negative: pre-activations >= the bias
        bm = 40.0 + torch.arange(E).double() % 7
        _exact(Wm, Xm, extra=float(bm.max()))
        S = Wm @ Xm
        return Wm, Xm, bm, _rne(S), _rne(S + bm[:, None])
    Wm, Xm, bm, plain, biased = _ref(("dt", T), make)
    cu(grid)
    buf, view, geom = _out_view(E, T, dev, "aligned")
    ops.proj_wx(_bf(Wm).to(dev), _bf(Xm).to(dev), out=view, softplus_bias=bm.float().to(dev) if bias else None)
    _check_out(buf, view, geom, biased if bias else plain)
