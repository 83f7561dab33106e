"""The ring-chunk loaders of csrc/proj_ring.h after the change of their cache policy (streaming LDS-DMA loads of the channel-major operand):
cad_proj_wx thin M / deep K, cad_proj_wx_wgrad (fused and weight gradient alone) and cad_proj_xTw at the real channel counts
(D = 256, E = 512, R + 2N = 48, R = 16), bit for bit against the exact sums of tests/test_proj_exact.py (integer operands whose partial
sums stay below 2^24 in any order: the fp64 product rounded once IS the result, whatever moves the bytes).

Tile token extent Tt = 128, ring depth r = 4:  T in {Tt - 8, Tt, Tt + 8, r Tt + 8}; the weight-gradient kernels take whole blocks only
(T in {Tt, r Tt}; a ragged T is refused, asserted).  The thin kernel's addend is checked with `out` aliasing `acc`."""
import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TT, RING = 128, 4
E, D, R, N = 512, 256, 16, 16
T_ALL = [TT - 8, TT, TT + 8, RING * TT + 8]
T_BLOCKS = [TT, RING * TT]


@pytest.fixture(scope="module")
def dev():
    L.use_library_for_testing(None)
    assert torch.cuda.is_available() and L.is_device_build()
    return torch.device("cuda:0")


def _ints(rows, cols, a, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-a, a + 1, (rows, cols), generator=g).double()


def _bf(m):
    t = m.float().to(BF)
    assert torch.equal(t.double(), m), "operand not exactly representable"
    return t


def _exact(Lm, Rm, acc=None):
    b = float((Lm.abs() @ Rm.abs()).max()) + (0.0 if acc is None else float(acc.abs().max()))
    assert b < 2 ** 24, b


def _rne(S):
    assert torch.equal(S.float().double(), S)
    return S.float().to(BF)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16))


_CASES = {}


def _operands(M, K, T, seed):
    """Shared per (M, K, T): computed once, never modified."""
    key = (M, K, T, seed)
    if key not in _CASES:
        Wm, Xm = _ints(M, K, 16, seed), _ints(K, T, 16, seed + 1)
        _exact(Wm, Xm)
        S = Wm @ Xm
        assert int((_rne(S).double() != S).sum()) >= 100  # the rounding is exercised
        _CASES[key] = (Wm, Xm, S)
    return _CASES[key]


@pytest.mark.parametrize("T", T_ALL)
@pytest.mark.parametrize("M", [R + 2 * N, R])
def test_thin_m_deep_k(dev, M, T):
    """x_proj (M = 48) and d(dt_lr) (M = 16) over K = E."""
    Wm, Xm, S = _operands(M, E, T, 10 + M)
    assert ops.proj_wx_supported(torch.empty(0, dtype=BF), E, T, M=M)
    out = ops.proj_wx(_bf(Wm).to(dev), _bf(Xm).to(dev))
    assert _same_bits(out, _rne(S))


@pytest.mark.parametrize("T", [TT + 8, RING * TT + 8])
def test_thin_m_deep_k_addend_aliasing_the_output(dev, T):
    """out = round(W X + acc) with out == acc (one rounding of the fp32 sum: include/caduceus_hip.h)."""
    M = R + 2 * N
    Wm, Xm, S = _operands(M, E, T, 10 + M)
    acc = _ints(M, T, 256, 77)
    _exact(Wm, Xm, acc)
    out = _bf(acc).to(dev)
    ops.proj_wx(_bf(Wm).to(dev), _bf(Xm).to(dev), out=out, acc=out)
    assert _same_bits(out, _rne(S + acc))


@pytest.mark.parametrize("T", T_BLOCKS)
def test_wgrad_fused(dev, T):
    """d(dt_lr) = W_dt^T d(delta) and dW_dt = d(delta) dt_lr^T from one pass over d(delta)."""
    M = R
    Wm, Xm, S = _operands(M, E, T, 10 + M)
    Ym = _ints(M, T, 4, 31)
    _exact(Xm, Ym.t())
    x0 = torch.empty(0, dtype=BF)
    assert ops.proj_wx_wgrad_supported(x0, M, E, T) and not ops.proj_wx_wgrad_supported(x0, M, E, T + 8)
    out, dW = ops.proj_wx_wgrad(_bf(Wm).to(dev), _bf(Xm).to(dev), _bf(Ym).to(dev))
    assert _same_bits(out, _rne(S))
    assert torch.equal(dW.cpu().double(), Xm @ Ym.t())


@pytest.mark.parametrize("T", T_BLOCKS)
def test_wgrad_only(dev, T):
    """dW_x = d(dbc) xc^T (M = R + 2N rows of Y)."""
    M = R + 2 * N
    Xm, Ym = _ints(E, T, 8, 41), _ints(M, T, 8, 42)
    _exact(Ym, Xm.t())
    x0 = torch.empty(0, dtype=BF)
    assert ops.proj_wgrad_only_supported(x0, M, E, T) and not ops.proj_wgrad_only_supported(x0, M, E, T + 8)
    dW = ops.proj_wgrad_only(_bf(Xm).to(dev), _bf(Ym).to(dev))
    assert torch.equal(dW.cpu().double(), Ym @ Xm.t())


@pytest.mark.parametrize("T", T_ALL)
@pytest.mark.parametrize("panels", [1, 2])
def test_xTw(dev, T, panels):
    """out_proj: out (T, D) = W_out (y_f + y_r), fp32 accumulation over both panels, one rounding."""
    Wm = _ints(D, E, 16, 51)
    Xs = [_ints(E, T, 16, 52 + p) for p in range(panels)]
    _exact(torch.cat([X.t() for X in Xs], 1), torch.cat([Wm.t()] * panels, 0))
    S = sum(X.t() @ Wm.t() for X in Xs)
    assert int((_rne(S).double() != S).sum()) >= 100
    X = [_bf(x).to(dev) for x in Xs]
    out = ops.proj_xTw(_bf(Wm).to(dev), X[0], X[1] if panels == 2 else None)
    assert _same_bits(out, _rne(S))
