"""The selective scans where the rest of the suite does not look: long memory and edge values, against float64.

Reference: oracle.oracle_model.selective_scan on float64 copies of exactly the dtype-rounded values the kernel sees, every row in its
own direction by explicit flips (test_kernels._rows_oracle); chains with an entry state use `scan64` below, the same recurrence with
h0 / hT, which test_reference_with_state_equals_the_oracle ties to the oracle.

A. LONG MEMORY.  Every other scan test draws A = -(0.5 + 15.5 rand), dt ~ 0.1 (test_kernels._scan_inputs, regime "suite"): the decay
product of one 512-position chunk, exp(A sum_dt), has a median of 5e-152 over the (channel, state) pairs and a maximum of 2e-15, so
whatever moves state across whole chunks, L-split segments or ranks is multiplied by zero.  Regime "long_memory" (A = -(0.02 + rand),
every fourth state fast, dt ~ 4e-3) has a median product of 0.23, a largest one of 0.96, 70 % of the pairs >= 0.1 and a smallest of
2e-15; `assert_long_memory` asserts these conditions on the inputs of every case.  Mutation controls (emulator, fp32, E 8 / L 4096 for
the L-split and E 5 / L 1100 / cut 512 for the chain; the figure is the worst err / tol of this module's comparison, > 1 fails;
intact kernels: 1.2e-4 .. 3.6e-4):

    mutation                                          suite recipe              long_memory
    P := 0 in ops.compose_segments (L-split k = 4)    passes (1.2e-4, unmoved)  raises (41)
    h0 withheld from the 2nd segment of a chain       raises (28)               raises (265)
    dhT withheld in the chain's backward              raises (20)               raises (83)

The old inputs cannot see a wrong decay product or composition at all -- the comparison does not move by one bit.  A state withheld AT
a cut is seen by both recipes (the few dozen positions behind the cut still remember it); with long memory the whole segment does.
test_mutations_are_seen_only_with_long_memory asserts the table's verdicts.
No sequence-parallel (two-process gloo) case on long-memory weights: tests/test_seqpar.py's `_worker` calls `_setup_model(name)` inside the
spawned process and loads the golden state dict there, so `A_log` / `dt_proj.bias` cannot be set without changing that harness.

Bounds of part A: the project's tolerance classes per element, |got - ref| <= rtol |ref| + atol max(1, max |ref|) (FP32 6e-4 / 2e-3,
BF16 3e-2 / 5e-2, F16_TOL 4e-3 / 4e-3) AND a relative error norm per tensor: 1e-5 (fp32: ~100 fp32 roundings), 2e-2 (bf16: the figure
test_scan_backward_lean_production_instantiation uses; ~5 bf16 roundings), 2e-3 (fp16: ~4 roundings of 2^-11; dB / dC of fp16 pass
through bf16 slots by design and take the bf16 figure).

B. EDGE VALUES, element-wise with a LOCAL scale: |got - ref| <= rtol |ref| + atol s_i, s_i from the float64 reference of that very
position: out, du, d(delta): max(1, |ref_i|); dz: max(1, |dout_i| sum_sets |y_i|) (y the un-gated output: the gate gradient is
recovered from the STORED gated outputs, whose rounding is relative to each set's own y, also where the two cancel).  The
per-channel / per-position sums (dA, dD, d(bias), dB, dC) keep the tensor-wide scale of the existing tests.  A whole-tensor atol
scale (17.8 in a probe) is what let an fp16 gate gradient that was wrong by 0.13 pass.  Planted: gates 0, the dtype's smallest
subnormal, +-2^-k through fp16's subnormal range, ~1e-3, +-8, +-30; raw delta + bias across the softplus threshold 20 in dtype
steps, 28, [-17.5, -16] (softplus' `d == 0` branch), -40; as dt: 0, the smallest subnormal, both sides of 2^-9 and 1/16, > 20;
A = -16 under dt = 28 (a decay of exactly 0) next to slow states; zero u, zero B / C columns; two sets under one gate with a position
where their outputs cancel exactly.  All planted values are finite numbers of their dtype.

Found by B and fixed in csrc/scan_bwd.hip (sc_gate_lost: fp16 gates |z| <= 2^-15 and every |z| < 2^-100 join the z == 0 worklist): on the parent commit the fp16 gate gradient at small non-zero gates was off
by up to |dout y| / 2 (emulator: dz 0.0 for fp64 0.1316 at z = 2^-24, 0.1776 for 0.0928 at z = 2e-7), and a gate at the smallest
fp32 / bf16 subnormal gave inf / NaN (1 / z overflows).  `test_bound_rejects_the_old_gate_error` shows the local bound refuses
errors of that size.  Nothing in B needed more than its class: no extra term was added to any bound."""
import numpy as np
import pytest
import torch

from caduceus_amd import _lib as CL
from caduceus_amd import ops
from oracle import oracle_model as om
from test_fp16_kernels import F16_TOL
from test_kernels import BF16, FP32, _rows_oracle, _scan_inputs, leaf
from test_scan_bwd_sums import fold, run_device

F32, B16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, B16, F16]
TOL = {F32: FP32, B16: BF16, F16: F16_TOL}
RELN = {F32: 1e-5, B16: 2e-2, F16: 2e-3}
ORDER = ("u", "delta", "A", "B", "C", "D", "z", "bias")
ACT = {"u", "delta", "B", "C", "z"}
CHUNK = 512
WORST = {}  # (part, dtype) -> worst err / tol, printed at the end of every test (pytest -s / the job log)


def _name(dtype):
    return str(dtype).split(".")[-1]


def check(what, got, ref, dtype, scale=None, reln=True, part="A"):
    """|got - ref| <= rtol |ref| + atol scale (scale: a tensor of local scales, or None = max(1, max |ref|)); returns err / tol."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    tol = TOL[dtype]
    s = max(1.0, float(ref.abs().max())) if scale is None else scale.double()
    bound = tol["rtol"] * ref.abs() + tol["atol"] * s
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    ratio = err / bound
    worst = float(ratio.max())
    key = (part, _name(dtype))
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= 1.0:
        i = int(torch.argmax(ratio))
        idx = tuple(int(x) for x in np.unravel_index(i, tuple(ratio.shape)))
        raise AssertionError(f"{what}{list(idx)} = {float(got.flatten()[i]):.9g}, fp64 {float(ref.flatten()[i]):.9g}: |err| "
                             f"{float(err.flatten()[i]):.3g} > bound {float(bound.flatten()[i]):.3g} (err/tol {worst:.3g}, "
                             f"{int((ratio > 1).sum())} of {ratio.numel()} out of bounds)")
    if reln:
        lim = RELN[B16] if (dtype == F16 and what.split()[-1] in ("dB", "dC")) else RELN[dtype]
        rn = float((got - ref).norm() / ref.norm().clamp_min(1e-300))
        assert rn <= lim, f"{what}: relative error norm {rn:.3g} > {lim:.3g}"
    return worst


def decay_products(t, L):
    """exp(A * sum of dt over one chunk) per (channel, state), float64, from the inputs alone (mean chunk sum over rows and chunks)."""
    dt = torch.nn.functional.softplus(t["delta"].double() + t["bias"].double()[:, None, None])
    per_chunk = dt.sum(-1).mean(1) * (min(L, CHUNK) / L)  # (E)
    return torch.exp(t["A"].double() * per_chunk[:, None])


def assert_long_memory(t, L):
    P = decay_products(t, L)
    assert float((P >= 0.1).double().mean()) >= 0.5 and float(P.max()) >= 0.5, (float((P >= 0.1).double().mean()), float(P.max()))
    assert float(P.min()) < 1e-3, "keep a spread: some states must still decay fast"
    return P


def scan64(u, delta, A, B, C, D, z, bias, h0, rev):
    """One row, float64: u, delta, z (E, L); A (E, N); B, C (N, L); h0 (E, N) or None.  Returns (out, y, hT), the row taken right to
    left when rev."""
    f = (lambda x: x.flip(-1)) if rev else (lambda x: x)
    u_, d_, z_, B_, C_ = f(u), f(delta), f(z), f(B), f(C)
    dt = torch.nn.functional.softplus(d_ + bias[:, None])
    h = torch.zeros(A.shape, dtype=u.dtype) if h0 is None else h0
    ys = []
    for l in range(u.shape[-1]):
        h = torch.exp(dt[:, l, None] * A) * h + dt[:, l, None] * B_[None, :, l] * u_[:, l, None]
        ys.append((h * C_[None, :, l]).sum(-1))
    y = torch.stack(ys, -1) + u_ * D[:, None]
    return f(y * torch.nn.functional.silu(z_)), f(y), h


def leaves64(t, order=ORDER):
    return [t[k].detach().double().clone().requires_grad_(True) for k in order]


def oracle64(ins, split, rl, rh):
    u, d, A, B, C, D, z, b = ins
    return _rows_oracle(lambda u_, d_, B_, C_, z_: om.selective_scan(u_, d_, A, B_, C_, D, z_, b), [u, d, B, C, z], split, rl, rh)


def inv_softplus64(dt):
    dt = dt.double()
    return torch.where(dt > 0, dt + torch.log(-torch.expm1(-dt)), torch.full_like(dt, -200.0))


def report(tag):
    print(f"\n[scan regimes] {tag}: worst err/tol so far " + ", ".join(f"{p}/{d} {v:.3f}" for (p, d), v in sorted(WORST.items())))


def test_reference_with_state_equals_the_oracle():
    t = _scan_inputs(3, 1, 40, 5, 3, None, F32, "long_memory")
    for rev in (0, 1):
        ins = leaves64(t)
        u, d, A, B, C, D, z, b = ins
        ref = oracle64(ins, 1, rev, rev)
        out, _, _ = scan64(u[:, 0], d[:, 0], A, B[:, 0], C[:, 0], D, z[:, 0], b, None, rev)
        torch.testing.assert_close(out, ref[:, 0], rtol=1e-12, atol=1e-12)


# ---- A. long memory -------------------------------------------------------------------------------------------------------------------
def run_unsplit(dev, t, dtype, split, rl, rh, tag):
    ins = [leaf(t[k], dev, dtype if k in ACT else F32) for k in ORDER]
    out = ops.selective_scan(*ins, split, rl, rh)
    (out.float() * t["w"].to(dev)).sum().backward()
    rins = leaves64(t)
    ref = oracle64(rins, split, rl, rh)
    (ref * t["w"].double()).sum().backward()
    check(f"{tag} out", out, ref, dtype)
    for k, a, r in zip(ORDER, ins, rins):
        check(f"{tag} d{k}", a.grad, r.grad, dtype)


@pytest.mark.parametrize("case", [(9, 2, 1100, 16, 1, 0, 1), (10, 2, 1544, 5, 1, 1, 0)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_long_memory_unsplit(backend, case, dtype):
    """Several chunks with a ragged tail (1100: element path; 1544: vector path), both directions in one launch, a second workgroup,
    d_state 16 and odd."""
    _, dev = backend
    E, SB, L, N, split, rl, rh = case
    t = _scan_inputs(E, SB, L, N, 41, dev, dtype, "long_memory")
    assert_long_memory(t, L)
    run_unsplit(dev, t, dtype, split, rl, rh, f"unsplit {case} {_name(dtype)}")
    report(f"unsplit {case} {_name(dtype)}")


def run_multi(dev, ts, z, dtype, split, dirs, is_dt, tag, part="A", local=False):
    """selective_scan_multi (one gate for all sets) against the oracle.  is_dt: t["delta"] holds dt; the oracle gets softplus^-1(dt) in
    float64 and bias 0 (d raw = d dt * sigmoid(raw))."""
    order = ("u", "delta", "A", "B", "C", "D", "bias")
    zd = leaf(z, dev, dtype)
    dsets = [tuple(leaf(t[k], dev, dtype if k in ACT else F32) for k in order) for t in ts]
    outs = ops.selective_scan_multi(dsets, zd, split, dirs, delta_is_dt=is_dt)
    sum((o.float() * t["w"].to(dev)).sum() for o, t in zip(outs, ts)).backward()
    zr = z.detach().double().clone().requires_grad_(True)
    rsets, refs = [], []
    for i, t in enumerate(ts):
        tt = dict(t)
        if is_dt:
            tt["delta"], tt["bias"] = inv_softplus64(t["delta"]), torch.zeros_like(t["bias"])
        u, d, A, B, C, D, b = leaves64(tt, order)
        rsets.append((u, d, A, B, C, D, b))
        refs.append(oracle64((u, d, A, B, C, D, zr, b), split, *dirs[i]))
    sum((r * t["w"].double()).sum() for r, t in zip(refs, ts)).backward()
    loc = lambda r: r.detach().abs().clamp_min(1.0) if local else None
    for i in range(len(ts)):
        check(f"{tag} set {i} out", outs[i], refs[i], dtype, loc(refs[i]), part=part)
        for k, a, r in zip(order, dsets[i], rsets[i]):
            check(f"{tag} set {i} d{k}", a.grad, r.grad, dtype, loc(r.grad) if k in ("u", "delta") else None, part=part, reln=not local)
    return zd, zr, refs


@pytest.mark.parametrize("nsets", [1, 2])
def test_long_memory_lean_production_instantiation(backend, nsets):
    """bf16, d_state 16, L % 8 == 0, delta_is_dt: scan_bwd_kernel<bf16, true, false, 8, true>; one and two sets under a shared gate."""
    _, dev = backend
    E, SB, L, N, split = 9, 2, 1544, 16, 1
    dirs = [(0, 1), (1, 0)][:nsets]
    ts = []
    for i in range(nsets):
        t = _scan_inputs(E, SB, L, N, 51 + i, dev, B16, "long_memory")
        assert_long_memory(t, L)
        t["delta"] = torch.nn.functional.softplus(t["delta"] + t["bias"][:, None, None]).to(B16).float()
        ts.append(t)
    zd, zr, _ = run_multi(dev, ts, ts[0]["z"], B16, split, dirs, True, f"lean nsets={nsets}")
    check("lean dz", zd.grad, zr.grad, B16)
    report(f"lean nsets={nsets}")


def run_lsplit(dev, monkeypatch, dtype, k, regime, L):
    E, SB, N, split = 8, 2, 16, 1
    ts = [_scan_inputs(E, SB, L, N, 31 + i, dev, dtype, regime) for i in range(2)]
    if regime == "long_memory":
        for t in ts:
            assert_long_memory(t, L)
    monkeypatch.setenv("CADUCEUS_AMD_LSPLIT", str(k))
    assert ops.lsplit_factor(E, SB, L, 2) == k
    zd, zr, _ = run_multi(dev, ts, ts[0]["z"], dtype, split, [(0, 1), (1, 0)], False, f"lsplit k={k} {regime} {_name(dtype)}")
    check("lsplit dz", zd.grad, zr.grad, dtype)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_long_memory_lsplit(backend, monkeypatch, dtype, k):
    """L-split k = 2, 4, two sets with opposite directions under one gate (the BiMamba launch): both outputs and every gradient."""
    _, dev = backend
    run_lsplit(dev, monkeypatch, dtype, k, "long_memory", 1024 * k)
    report(f"lsplit k={k} {_name(dtype)}")


def run_chain(dev, dtype, cut, regime, mutate=None):
    """Each row as two chained selective_scan_stateful segments (row 0 left to right, row 1 right to left), a random state entering
    the first: outputs, the state between the segments, the final state and every gradient, dh0 included."""
    E, SB, L, N = 5, 2, 1100, 16
    t = _scan_inputs(E, SB, L, N, 31, dev, dtype, regime)
    if regime == "long_memory":
        assert_long_memory(t, L)
    g = torch.Generator().manual_seed(77)
    h0m, wh = torch.randn(E, SB, N, generator=g), torch.randn(E, SB, N, generator=g)
    ins = [leaf(t[k], dev, dtype if k in ACT else F32) for k in ORDER]
    h0 = leaf(h0m, dev)
    u, d, A, B, C, D, z, b = ins
    lo, hi = slice(0, cut), slice(cut, L)
    outs, mids, ends = {}, {}, {}
    for row, rev in ((0, 0), (1, 1)):
        first, second = (lo, hi) if rev == 0 else (hi, lo)
        r = slice(row, row + 1)
        f = lambda x, s: x[:, r][..., s]
        o1, h1 = ops.selective_scan_stateful(f(u, first), f(d, first), A, f(B, first), f(C, first), D, f(z, first), b, h0[:, r], 1, rev, rev)
        hin = None if mutate == "drop_h0" else (h1.detach() if mutate == "drop_dhT" else h1)
        o2, h2 = ops.selective_scan_stateful(f(u, second), f(d, second), A, f(B, second), f(C, second), D, f(z, second), b, hin, 1, rev, rev)
        outs[row] = torch.cat([o1, o2], -1) if rev == 0 else torch.cat([o2, o1], -1)
        mids[row], ends[row] = h1, h2
    out, hT = torch.cat([outs[0], outs[1]], 1), torch.cat([ends[0], ends[1]], 1)
    ((out.float() * t["w"].to(dev)).sum() + (hT * wh.to(dev)).sum()).backward()
    # float64
    rins = leaves64(t)
    rh0 = h0m.double().clone().requires_grad_(True)
    ru, rd, rA, rB, rC, rD, rz, rb = rins
    routs, rmids, rends = [], [], []
    for row, rev in ((0, 0), (1, 1)):
        first, second = (lo, hi) if rev == 0 else (hi, lo)
        f = lambda x, s: x[:, row][..., s]
        o1, _, h1 = scan64(f(ru, first), f(rd, first), rA, f(rB, first), f(rC, first), rD, f(rz, first), rb, rh0[:, row], rev)
        o2, _, h2 = scan64(f(ru, second), f(rd, second), rA, f(rB, second), f(rC, second), rD, f(rz, second), rb, h1, rev)
        routs.append(torch.cat([o1, o2], -1) if rev == 0 else torch.cat([o2, o1], -1))
        rmids.append(h1), rends.append(h2)
    rout, rhT = torch.stack(routs, 1), torch.stack(rends, 1)
    ((rout * t["w"].double()).sum() + (rhT * wh.double()).sum()).backward()
    tag = f"chain cut={cut} {regime} {_name(dtype)}"
    # the carried states are fp32 whatever the activation dtype, but they are sums of dtype-rounded-input products computed from the
    # same rounded inputs as the reference: the activation class applies
    check(f"{tag} out", out, rout, dtype)
    check(f"{tag} h between the segments", torch.cat([mids[0], mids[1]], 1), torch.stack(rmids, 1), dtype)
    check(f"{tag} hT", hT, rhT, dtype)
    for k, a, r in zip(ORDER, ins, rins):
        check(f"{tag} d{k}", a.grad, r.grad, dtype)
    check(f"{tag} dh0", h0.grad, rh0.grad, dtype)


@pytest.mark.parametrize("cut", [512, 700, 37])
@pytest.mark.parametrize("dtype", DTYPES)
def test_long_memory_stateful_chain(backend, dtype, cut):
    _, dev = backend
    run_chain(dev, dtype, cut, "long_memory")
    report(f"chain cut={cut} {_name(dtype)}")


def compose64(P, S, k, split, rev_lo, rev_hi, towards_end):
    """Sequential composition in float64: the value entering segment q of every row, the chain starting from 0 at the row's logical
    start (towards_end=False) or end (True)."""
    E, SBk, N = S.shape
    SB = SBk // k
    P, S = P.double().view(E, SB, k, N), S.double().view(E, SB, k, N)
    out = torch.zeros_like(S)
    for r in range(SB):
        rev = rev_lo if r < split else rev_hi
        logical = list(range(k)) if not rev else list(range(k - 1, -1, -1))  # physical segment index in logical order
        walk = logical[::-1] if towards_end else logical
        v = torch.zeros(E, N, dtype=torch.float64)
        for q in walk:
            out[:, r, q] = v
            v = P[:, r, q] * v + S[:, r, q]
    return out.view(E, SBk, N)


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("towards_end", [False, True])
@pytest.mark.parametrize("dirs", [(0, 1), (1, 0)])
def test_compose_segments_against_sequential_float64(k, towards_end, dirs):
    """ops.compose_segments alone (host): decay products of order one, `split` inside the rows; exact to fp32 rounding (k - 1 fused
    steps: (k + 1) 2^-24 relative to the sum of the magnitudes).  With P := 0 the same comparison fails."""
    g = torch.Generator().manual_seed(9)
    E, SB, N, split = 4, 3, 5, 2
    P = 0.3 + 0.69 * torch.rand(E, SB * k, N, generator=g)
    S = torch.randn(E, SB * k, N, generator=g)
    ref = compose64(P, S, k, split, *dirs, towards_end)
    mag = compose64(P, S.abs(), k, split, *dirs, towards_end)
    bound = (k + 1) * 2.0 ** -24 * mag
    got = ops.compose_segments(P, S, k, split, *dirs, towards_end).double()
    assert bool(((got - ref).abs() <= bound).all()), float(((got - ref).abs() - bound).max())
    bad = ops.compose_segments(torch.zeros_like(P), S, k, split, *dirs, towards_end).double()
    assert not bool(((bad - ref).abs() <= bound).all())


MUTATION_L = 4096


def _with_zero_P(monkeypatch):
    orig = ops.compose_segments
    monkeypatch.setattr(ops, "compose_segments", lambda P, S, *a, **kw: orig(torch.zeros_like(P), S, *a, **kw))


def test_mutations_are_seen_only_with_long_memory(monkeypatch):
    """The three mutations of the module docstring, emulator, fp32: each must raise on the long-memory inputs; P := 0 in the segment
    composition -- the gap this module closes -- passes on the suite's recipe."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    from build_emu import build_emu
    CL.use_library_for_testing(build_emu())
    saved = dict(WORST)
    try:
        dev = torch.device("cpu")
        for mut in ("drop_h0", "drop_dhT"):
            with pytest.raises(AssertionError):
                run_chain(dev, F32, 512, "long_memory", mutate=mut)
        with monkeypatch.context() as m:
            _with_zero_P(m)
            run_lsplit(dev, m, F32, 4, "suite", MUTATION_L)
            with pytest.raises(AssertionError):
                run_lsplit(dev, m, F32, 4, "long_memory", MUTATION_L)
    finally:
        CL.use_library_for_testing(None)
        WORST.clear()
        WORST.update(saved)  # (the mutated runs are not kernel errors)


# ---- B. edge values -------------------------------------------------------------------------------------------------------------------
def smallest_subnormal(dtype):
    return {F32: 2.0 ** -149, B16: 2.0 ** -133, F16: 2.0 ** -24}[dtype]


def q(x, dtype):
    return x.to(dtype).float() if dtype != F32 else x.float()


GATE_POS = 40  # planted gates start here, in every row of channels 0 .. 3


def edge_inputs(E, SB, L, N, dtype, nsets, is_dt, seed=7):
    """Ordinary inputs (dt ~ 0.1 .. 0.3, half of the states slow) with the edge values of the module docstring planted."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    tiny = smallest_subnormal(dtype)
    gates = [0.0, tiny, -tiny] + [s * 2.0 ** -k for k in range(13, 25) for s in (1.0, -1.0)] + \
            [1e-5, 1e-6, 2e-7, -2e-7, 1e-3, -1e-3, 8.0, -8.0, 30.0, -30.0]
    z = r(E, SB, L)
    z[:4, :, GATE_POS:GATE_POS + 2 * len(gates):2] = torch.tensor(gates)   # every other position: next to ordinary gates
    z[4, :, 600:600 + len(gates)] = torch.tensor(gates)                     # ... and a run of them in the second chunk
    z[:, :, L - 1] = tiny
    z = q(z, dtype)
    ts = []
    for i in range(nsets):
        A = -(0.02 + torch.rand(E, N, generator=g))
        A[:, 1::2] = -(0.5 + 15.5 * torch.rand(E, (N + 1) // 2, generator=g))[:, :N // 2]
        A[:, 0] = -16.0
        bias = 0.3 * r(E) - 1.0
        bias[0], bias[1] = 0.0, -3.0
        raw = 0.5 * r(E, SB, L) - 1.0
        # raw + bias at the planted points (channels 0 and 1: exact sums)
        pts = [19.5 + j / 16 for j in range(17)] + [20.0 - 2.0 ** -6, 20.0 + 2.0 ** -6, 24.0, 28.0,
                                                    -17.5, -17.0, -16.75, -16.625, -16.5, -16.0, -40.0]
        for e in (0, 1):
            raw[e, :, 100:100 + len(pts)] = torch.tensor(pts) - bias[e]
            raw[e, :, 700:700 + 3 * len(pts):3] = torch.tensor(pts) - bias[e]
        raw[2, :, 200:216] = 28.0 - bias[2]   # a run of dt = 28: A dt = -448 underflows to a decay of exactly 0 for state 0
        raw = q(raw, dtype)
        t = dict(u=r(E, SB, L), A=A, B=r(N, SB, L), C=r(N, SB, L), D=r(E), bias=bias, w=r(E, SB, L))
        t["u"][3, :, 300:340] = 0.0
        t["B"][:, :, 310:330] = 0.0
        t["C"][:, :, 320:350] = 0.0
        if is_dt:
            dt = torch.nn.functional.softplus(raw.double() + bias.double()[:, None, None]).float()
            dts = [0.0, tiny, 2.0 ** -9, 2.0 ** -9 * (1 - 2.0 ** -7), 2.0 ** -9 * (1 + 2.0 ** -7), 0.0625, 0.0625 * (1 - 2.0 ** -7),
                   0.0625 * (1 + 2.0 ** -7), 2.0 ** -12, 20.5, 28.0]
            dt[5, :, 400:400 + len(dts)] = torch.tensor(dts)
            dt[5, :, 900:900 + 2 * len(dts):2] = torch.tensor(dts)
            t["delta"] = q(dt, dtype)
        else:
            t["delta"] = raw
        for k in ("u", "B", "C"):
            t[k] = q(t[k], dtype)
        ts.append(t)
    if nsets == 2:  # a position where the two un-gated outputs cancel exactly: C = 0 there, so y = D u in both sets
        ts[1]["u"][0, :, 325] = ts[0]["u"][0, :, 325]
        ts[1]["D"][0] = -ts[0]["D"][0]
    dout = q(r(E, SB, L), dtype)
    return ts, z, dout


def edge_reference(ts, z, dout, split, dirs, is_dt):
    """float64: per set out, the un-gated y and every gradient for the loss sum(out_i * dout) over the sets (one dout, one gate)."""
    zr = z.double().clone().requires_grad_(True)
    order = ("u", "delta", "A", "B", "C", "D", "bias")
    res, loss = [], 0.0
    for i, t in enumerate(ts):
        tt = dict(t)
        if is_dt:
            tt["delta"], tt["bias"] = inv_softplus64(t["delta"]), torch.zeros_like(t["bias"])
        lv = leaves64(tt, order)
        u, d, A, B, C, D, b = lv
        out = oracle64((u, d, A, B, C, D, zr, b), split, *dirs[i])
        loss = loss + (out * dout.double()).sum()
        res.append(dict(out=out, leaves=dict(zip(order, lv))))
    loss.backward()
    SB = z.shape[1]
    for i, (t, r) in enumerate(zip(ts, res)):
        ys = []
        for sb in range(SB):
            rev = dirs[i][0] if sb < split else dirs[i][1]
            lv = {k: v.detach() for k, v in r["leaves"].items()}
            ys.append(scan64(lv["u"][:, sb], lv["delta"][:, sb], lv["A"], lv["B"][:, sb], lv["C"][:, sb], lv["D"], z.double()[:, sb],
                             lv["bias"], None, rev)[1])
        r["y"] = torch.stack(ys, 1)
    return res, zr.grad


@pytest.mark.parametrize("nsets", [1, 2])
@pytest.mark.parametrize("is_dt", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_values(backend, dtype, is_dt, nsets):
    """The C-ABI launch of the training step (set 0 writes the gate gradient of both sets from out + out2; the fix-up launch behind it).
    N 16 and L % 8 == 0: bf16 with is_dt is the lean instantiation, everything else the generic / unrolled ones."""
    _, dev = backend
    E, SB, L, N, split = 9, 2, 1104, 16, 1
    dirs = [(0, 1), (1, 0)][:nsets]
    ts, z, dout = edge_inputs(E, SB, L, N, dtype, nsets, is_dt)
    res, dz_ref = edge_reference(ts, z, dout, split, dirs, is_dt)
    ds, dz, run = run_device(dev, ts, z, dout, split, dirs, dtype, is_dt)
    run["launch"]()
    CL.check(run["lib"].cad_scan_bwd_gate_fix(run["ba"], nsets, run["stream"]), "gate fix")
    fold(ds, run, "reduce")
    tag = f"edge {_name(dtype)} is_dt={int(is_dt)} nsets={nsets}"
    loc = lambda r: r.detach().abs().clamp_min(1.0)
    ysum = sum(r["y"].abs() for r in res)
    check(f"{tag} dz", dz, dz_ref, dtype, (dout.double().abs() * ysum).clamp_min(1.0), reln=False, part="B")
    for i, (d, r) in enumerate(zip(ds, res)):
        g = {k: v.grad for k, v in r["leaves"].items()}
        check(f"{tag} set {i} out", d["out"], r["out"], dtype, loc(r["out"]), reln=False, part="B")
        check(f"{tag} set {i} du", d["du"], g["u"], dtype, loc(g["u"]), reln=False, part="B")
        check(f"{tag} set {i} ddelta", d["ddelta"], g["delta"], dtype, loc(g["delta"]), reln=False, part="B")
        for name, k in (("dA", "A"), ("dD", "D"), ("dbias", "bias"), ("dB", "B"), ("dC", "C")):
            check(f"{tag} set {i} {name}", d[name], g[k], dtype, reln=False, part="B")
    if dtype == F16 and dev.type == "cuda":  # what the device stored for the output under the planted z = 2^-24 (kept or flushed)
        p = GATE_POS + 2 * (3 + 2 * 11)
        print(f"\n[scan regimes] fp16 out at z = {float(z[0, 0, p]):.3g}: stored {float(ds[0]['out'][0, 0, p]):.6g}, "
              f"fp64 {float(res[0]['out'][0, 0, p]):.6g}")
    report(tag)


def test_bound_rejects_the_old_gate_error():
    """Host only: the local dz bound refuses the fp16 gate-gradient errors of the parent commit at positions with |dout y| <= 1 (dz
    0.0 written for 0.1316, 0.1776 for 0.0928, -0.7847 for -0.7655) and accepts an fp16 rounding of the same references."""
    ref = torch.tensor([0.13161, 0.09276, -0.76549])
    for i, old in enumerate((0.0, 0.17761, -0.78467)):
        got = ref.clone()
        got[i] = old
        with pytest.raises(AssertionError):
            check("old dz", got, ref, F16, torch.ones(3), reln=False, part="control")
    check("rounded dz", ref.to(F16), ref, F16, torch.ones(3), reln=False, part="control")
    WORST.pop(("control", "float16"), None)


@pytest.mark.parametrize("dtype", [B16, F16])
def test_proj_wx_softplus_epilogue_at_the_edges(backend, dtype):
    """cad_proj_wx's softplus + bias epilogue with pre-activations planted on both sides of the threshold 20, well above it, in
    [-17.5, -16] and at -40: K = 16 with a one-hot X column per planted value, so W X + bias is the planted number exactly."""
    _, dev = backend
    M, K, T = 512, 16, 1024
    g = torch.Generator().manual_seed(3)
    pts = [19.5, 19.75, 19.875, 20.0, 20.125, 20.25, 20.5, 24.0, 28.0, -17.5, -17.0, -16.75, -16.5, -16.0, -40.0]
    W = q(0.5 * torch.randn(M, K, generator=g), dtype)
    X = q(0.5 * torch.randn(K, T, generator=g), dtype)
    bias = torch.zeros(M)
    bias[1::2] = -3.0
    W[:, 0] = q(torch.tensor(pts).repeat(M // len(pts) + 1)[:M] - bias, dtype)
    X[:, :64] = 0.0
    X[0, :64] = 1.0   # columns 0 .. 63: pre-activation = W[:, 0] + bias
    got = ops.proj_wx(W.to(dev).to(dtype), X.to(dev).to(dtype), softplus_bias=bias.to(dev))
    ref = torch.nn.functional.softplus(W.double() @ X.double() + bias.double()[:, None])
    check(f"proj_wx softplus {_name(dtype)}", got, ref, dtype, ref.abs().clamp_min(1.0), reln=False, part="B")
    # relative at the planted columns too: softplus(-17) = 4e-8 must not be an absolute-tolerance pass.  The epilogue is evaluated in fp32
    # and rounded once: two unit roundoffs of the dtype (bf16 2^-8, fp16 2^-10) -- a wrong small-argument branch would not fit
    rel = ((got.double().cpu()[:, :64] - ref[:, :64]).abs() / ref[:, :64].abs().clamp_min(1e-30))
    keep = ref[:, :64] >= smallest_subnormal(dtype) * 2 ** 12   # (values the dtype holds with full precision)
    once = {B16: 2.0 ** -8, F16: 2.0 ** -10}[dtype]
    assert float(rel[keep].max()) <= once, float(rel[keep].max())
    report(f"proj_wx softplus {_name(dtype)}")
