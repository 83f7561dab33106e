"""Sequence parallelism (caduceus_amd/seqpar.py) at three and four ranks, against float64, on inputs that remember.

tests/test_seqpar.py runs the module at world size 2 on weights that forget a segment (decay product of a 550-position segment: median
1e-14 .. 1e-23).  At W = 2 `seqpar._compose` visits at most one segment before `rank`, so every decay product P = exp(A sum_dt) is
multiplied by zero, no rank has two neighbours, and both `+=` of the halo backward are never active together.  This module closes that:

A. `seqpar._compose` alone (host): W = 2 .. 5, every rank, against the sequential float64 chain written out from the definition; in
   float64 it must equal ops.compose_segments on the same maps; control: with P := 0 the comparison fails exactly at the ranks that have
   two or more segments in front of them in some row -- none at W = 2.
B. `sum_dt` and `hT` of cad_scan_fwd, full pass and map_only: sum_dt against the float64 row sum of dt at the kernel's rounding point
   (test_kernels.test_fused_softplus_rounding_point_against_oracle: the RAW delta is rounded to the activation type and softplus is
   evaluated in fp32 inside the scan; with delta_is_dt the rounded dt itself is summed), rtol 6e-4 of the sum (all terms positive); hT
   against scan64's final state in the activation's class.
C. seqpar.selective_scan_multi over W = 3, 4 gloo ranks (one and two parameter sets under one gate, the BiMamba launch) against
   oracle64 on the whole rows: outputs, activation gradients concatenated along L, parameter gradients summed over the ranks.
   Inputs: test_kernels._scan_inputs(..., "long_memory"); `assert_segments_remember` asserts on the reference inputs alone that every
   segment's decay product exp(A sum of dt over the segment) has >= half of its (channel, row, state) entries >= 0.1, a maximum >= 0.5
   and a minimum < 1e-3.  Measured (float64, the same for the three dtypes to two digits; share >= 0.1 / max / median, worst segment):
       W 3, L 2100 (700 each: a chunk and a ragged tail)      0.58 / 0.94 / 0.16
       W 4, L 1100 (275 each: below a chunk)                  0.76 / 0.97 / 0.48
       W 4, L 2080 (520 each: a chunk + 8, the vector path)   0.66 / 0.93 / 0.24
       W 4, L 1101 (275, 275, 275, 276)                       0.76 / 0.97 / 0.42
       W 2, L 1100 (the mutation table's W = 2 column)        0.66 / 0.93 / 0.23
   Planted gates in every case, in the first, an interior and the last rank's segment, at the segment's first and last position and
   in its middle: exact 0, the dtype's smallest subnormal, and in fp16 +-2^-15, +-2^-20, +-2^-24.  dz there is held with the local scale
   of test_scan_regimes.test_edge_values, max(1, sum over the sets of |dout_i y_i|) (one dout per set here: the loss is sum out_i w_i).
   GATE GRADIENT, the finding: `_ScanSeqPar.backward` ran the scan backward without the worklist of lost gates and without
   cad_scan_bwd_gate_fix, so dz at a lost gate stayed at the main kernel's 0 contribution.  On the parent commit (emulator; err / tol
   of the local bound at the planted gates, W = 3, L 2100; one and two sets alike):
       fp32   err / tol 217    dz -0.0 returned where float64 has -2.1746; 35 of the 36 planted positions out of bounds
       bf16   err / tol 7.7    dz 0.0 for 1.1282;  25 .. 33 of 36
       fp16   err / tol 83     dz -0.0 for -3.9544; 137 .. 142 of 144 (the +-2^-15 .. 2^-24 gates too)
   With the worklist handed to the second backward pass and cad_scan_bwd_gate_fix behind it, the worst |err| at the same positions is
   4.2e-07 (fp32), 1.8e-02 (bf16, on |dz| up to 4.1) and 2.2e-03 (fp16): err / tol 1.7e-04, 0.046, 0.061 (emulator).
   Mutation controls (emulator, fp32, two sets; the worker patches seqpar._compose; one spawn per W carries that W's column):
       mutation                                  W = 2, long_memory   W = 3, suite   W = 3, long_memory
       maps_P := 0                               passes               passes         fails
       maps_P := 1                                                                   fails
       h0 := 0 entering the last rank                                                fails
       dhT := 0                                                                      fails
   test_compose_mutations asserts the verdicts.
D. seqpar.causal_conv1d in the same spawns: E 5, SB 3, split 1, d_conv 4 with bias, both direction assignments, local lengths 3
   (the minimum), 4 and 5 (the two `+=` of _HaloExchange.backward overlap), 7, and one unequal cut (W 3: 5, 6, 6; W 4: 5, 6, 5, 6), fp32
   and bf16, against test_conv_embed_fp64.conv_reference on the whole rows with that file's bounds.  Controls: the right halo zeroed,
   and the left halo zeroed, must both fail.
   FINDING, fixed in seqpar.causal_conv1d: bf16 dx at the three positions on either side of a cut (test_conv_dx_at_the_cuts_*) missed
   that file's bound on the parent commit, worst err / tol 98 (W = 3, L 16: -4.1008e-05 returned for -4.0844e-05, tol 1.6e-07, the
   same on the emulator and the MI355X).  The bound allows ONE rounding of the fp32 sum to bf16.  Every rank's conv backward stored
   its part of dx as bf16 -- the halo positions' part too -- and _HaloExchange.backward added the neighbour's bf16 part with `+=` in
   bf16: three roundings, two of them relative to the parts, which may cancel.  All other bf16 elements met the bound.  16-bit
   segments now run the conv and the halo exchange in fp32 on the same stored values and round once.
E. The golden ps_fused model at W = 3 with every A_log / dt_proj.bias overwritten from a fixed seed (A = -(0.02 + rand), every fourth
   state left as it is, softplus(bias) = dt0 (0.75 + 0.5 rand)) against the single-process run, with test_seqpar.py's bounds of the same
   backend.  The decay condition of part C is asserted per mixer from the overwritten weights, with dt taken from the bias ALONE (the
   data-dependent part dt_proj(x) of the pre-activation is left out).  Emulator: L = 3 x 352, dt0 = 4e-3.  GPU: L = 3 x 1408; at
   dt0 = 4e-3 a 1408-position segment has only 0.29 of its entries >= 0.1, so the condition -- which is not lowered -- is met with
   dt0 = 1.5e-3 (the length is kept: two chunks and a tail per segment).

Worst err / tol measured (bound = 1; C / B through test_scan_regimes.check, D through test_norm_head_fp64.hold):
    part                               emulator  fp32 / bf16 / fp16          MI355X  fp32 / bf16 / fp16
    B sum_dt (rtol 6e-4)               3.1e-04 / 3.4e-04 / 3.4e-04           3.3e-04 / 3.8e-04 / 3.4e-04
    B hT                               7.9e-05 / 3.3e-06 / 2.5e-05           6.2e-05 / 4.3e-06 / 3.9e-05
    C outputs and gradients            3.8e-04 / 0.071 / 0.41                1.0e-03 / 0.071 / 0.41
    C dz at the planted gates          1.7e-04 / 0.046 / 0.061               4.1e-04 / 0.046 / 0.061
    D out                              0.31 / 0.98                           0.34 / 0.98
    D dx away from the cuts            0.21 / 0.96                           0.19 / 0.96
    D dx at the cuts                   0.18 / 0.99 (parent: 98)              0.24 / 0.99 (parent: 98)
    D dw, dbias (fp32 sums)            0.029, 0.024                          0.033, 0.018
    E logits, worst |difference|       1.9e-05 (atol 2e-4)                   2.0e-05 (atol 4e-4)
    E gradients                        1.2e-03                               1.1e-03
    B: the full pass and map_only gave the same hT and sum_dt bit for bit in all 26 cases, on both backends.
    E decay per mixer from the bias alone (share >= 0.1 / max / median): emulator 0.77 / 0.97 / 0.38, MI355X 0.74 / 0.96 / 0.24.
"""
import contextlib
import ctypes as C
import os
import sys
from datetime import timedelta

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from caduceus_amd import _lib as CL
from caduceus_amd import ops
from conftest import ROOT
from test_conv_embed_fp64 import conv_inputs, conv_reference
from test_kernels import _scan_inputs, leaf
from test_norm_head_fp64 import WORST as HOLD_WORST
from test_norm_head_fp64 import hold
from test_scan_regimes import RELN, TOL, WORST, check, decay_products, inv_softplus64, leaves64, oracle64, report, scan64  # noqa: F401
from test_seqpar import _free_port, _long_batch, _setup_model

F32, B16, F16 = torch.float32, torch.bfloat16, torch.float16
DT = {"float32": F32, "bfloat16": B16, "float16": F16}
NAMES = list(DT)
ACT = {"u", "delta", "B", "C", "z"}
SET_ORDER = ("u", "delta", "A", "B", "C", "D", "bias")
DIRS = [(0, 1), (1, 0)]
SCAN_E, SCAN_SB, SCAN_N = 9, 2, 16
SCAN_CASES = {3: [2100], 4: [1100, 2080, 1101]}   # W -> whole-row lengths, cut as rank * L // W


def _emu():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    from build_emu import build_emu
    return build_emu()


def figures(tag):
    """test_scan_regimes.report, and this module's parts once more with three significant digits (fp32 ratios are ~1e-4)."""
    report(tag)
    print("[seqpar chain] worst err/tol so far " + ", ".join(f"{p}/{d} {v:.3g}" for (p, d), v in sorted(WORST.items()) if p[0] in "BC"))


def cuts(L, W):
    return [r * L // W for r in range(W + 1)]


# ---- A. _compose alone ------------------------------------------------------------------------------------------------------------------
def entering64(P, S, rank, split, dirs, towards_end):
    """float64, from the definition: every row's segments are visited one after the other in the row's logical direction (ascending
    ranks for a left-to-right row), or against it for a state gradient (towards_end), from a zero value, up to but not including
    `rank`; a visited segment q maps v -> P[q] v + S[q].  The value that arrives is the one entering `rank`."""
    W = len(P)
    E, SB, N = S[0].shape
    out = torch.zeros(E, SB, N, dtype=torch.float64)
    for row in range(SB):
        rev = dirs[0] if row < split else dirs[1]
        logical = list(range(W - 1, -1, -1)) if rev else list(range(W))
        walk = logical[::-1] if towards_end else logical
        v = torch.zeros(E, N, dtype=torch.float64)
        for q in walk:
            if q == rank:
                break
            v = P[q][:, row].double() * v + S[q][:, row].double()
        out[:, row] = v
    return out


def segments_in_front(W, rank, SB, split, dirs, towards_end):
    """The largest number of segments visited before `rank` over the rows."""
    most = 0
    for row in range(SB):
        rev = dirs[0] if row < split else dirs[1]
        ascending = (rev == 0) != towards_end
        most = max(most, rank if ascending else W - 1 - rank)
    return most


@pytest.mark.parametrize("towards_end", [False, True])
@pytest.mark.parametrize("dirs", [(0, 1), (1, 0), (0, 0)])
@pytest.mark.parametrize("W", [2, 3, 4, 5])
def test_compose_against_the_sequential_chain(W, dirs, towards_end):
    """Every rank, `split` strictly inside the rows and once at 0 and at SB.  Bound: (W + 1) 2^-24 times the same chain run on |S| (the
    derivation of test_scan_regimes.test_compose_segments_against_sequential_float64).  In float64 _compose equals ops.compose_segments
    on the maps stacked as k = W segments.  Control: P := 0 fails exactly where two or more segments lie in front of `rank` in some row
    -- an interior or far rank of W >= 3, no rank of W = 2."""
    from caduceus_amd import seqpar
    g = torch.Generator().manual_seed(100 * W + 10 * dirs[0] + dirs[1])
    E, SB, N = 4, 3, 5
    P = [0.3 + 0.69 * torch.rand(E, SB, N, generator=g) for _ in range(W)]
    S = [torch.randn(E, SB, N, generator=g) for _ in range(W)]
    Z = [torch.zeros_like(p) for p in P]
    seen_fail = False
    for split in (1, 2, 0, SB):
        P64, S64 = [p.double() for p in P], [s.double() for s in S]
        stacked = ops.compose_segments(torch.stack(P64, 2).reshape(E, SB * W, N), torch.stack(S64, 2).reshape(E, SB * W, N), W, split,
                                       *dirs, towards_end).view(E, SB, W, N)
        for rank in range(W):
            ref = entering64(P, S, rank, split, dirs, towards_end)
            mag = entering64(P, [s.abs() for s in S], rank, split, dirs, towards_end)
            bound = (W + 1) * 2.0 ** -24 * mag
            got = seqpar._compose(P, S, rank, split, *dirs, towards_end)
            assert got.dtype == F32
            assert bool(((got.double() - ref).abs() <= bound).all()), (W, rank, split, float(((got.double() - ref).abs() - bound).max()))
            got64 = seqpar._compose(P64, S64, rank, split, *dirs, towards_end)
            assert torch.equal(got64, stacked[:, :, rank]), (W, rank, split)
            assert bool(((got64 - ref).abs() <= (W + 1) * 2.0 ** -53 * mag).all())
            bad = seqpar._compose(Z, S, rank, split, *dirs, towards_end).double()
            fails = not bool(((bad - ref).abs() <= bound).all())
            assert fails == (segments_in_front(W, rank, SB, split, dirs, towards_end) >= 2), (W, rank, split, fails)
            seen_fail = seen_fail or fails
    assert seen_fail == (W >= 3)


# ---- B. sum_dt and hT of cad_scan_fwd ---------------------------------------------------------------------------------------------------
def run_fwd_maps(dev, t, dtype, split, dirs, map_only, is_dt):
    """cad_scan_fwd through ops.scan_fwd_args as _ScanSeqPar (full pass) and ops.scan_fwd_launch (map_only) build it."""
    lib = CL.get_lib()
    (E, SB, Lq), N = t["u"].shape, t["A"].shape[1]
    d = {k: t[k].to(dev).to(dtype if k in ACT else F32).contiguous() for k in ("u", "delta", "A", "B", "C", "D", "z", "bias")}
    hT = torch.full((E, SB, N), float("nan"), dtype=F32, device=dev)
    sdt = torch.full((E, SB), float("nan"), dtype=F32, device=dev)
    out = None if map_only else torch.empty_like(d["u"])
    state = None if map_only else torch.empty((lib.cad_scan_state_floats(E, SB, Lq, N),), dtype=F32, device=dev)
    a, stream = ops.scan_fwd_args(E, SB, Lq, N, split, dirs, dtype, delta_is_dt=is_dt, u=d["u"], delta=d["delta"], A=d["A"], Bm=d["B"],
                                  Cm=d["C"], D=d["D"], z=None if map_only else d["z"], delta_bias=d["bias"], out=out, chunk_state=state,
                                  hT=hT, sum_dt=sdt)
    a.map_only = int(map_only)
    CL.check(lib.cad_scan_fwd(C.byref(a), stream), "cad_scan_fwd")
    return hT.cpu(), sdt.cpu()


def fwd_maps_case(dev, E, SB, L, N, dtype, is_dt, seed=71):
    split, dirs = 1, (0, 1)
    t = _scan_inputs(E, SB, L, N, seed, dev, dtype, "long_memory")
    bias64 = t["bias"].double()[:, None, None]
    tt = dict(t)
    if is_dt:  # the rounded dt is what the kernel reads and sums
        t["delta"] = torch.nn.functional.softplus(t["delta"] + t["bias"][:, None, None]).to(dtype).float()
        dt64 = t["delta"].double()
        tt["delta"], tt["bias"] = inv_softplus64(t["delta"]), torch.zeros_like(t["bias"])
    else:      # the raw delta is rounded, softplus is evaluated behind it
        dt64 = torch.nn.functional.softplus(t["delta"].double() + bias64)
    sum_ref = dt64.sum(-1)
    hs = []
    for sb in range(SB):
        rev = dirs[0] if sb < split else dirs[1]
        hs.append(scan64(tt["u"][:, sb].double(), tt["delta"][:, sb].double(), tt["A"].double(), tt["B"][:, sb].double(),
                         tt["C"][:, sb].double(), tt["D"].double(), tt["z"][:, sb].double(), tt["bias"].double(), None, rev)[2])
    h_ref = torch.stack(hs, 1)
    tag = f"fwd maps L={L} N={N} {str(dtype).split('.')[-1]} is_dt={int(is_dt)}"
    got = {}
    for map_only in (False, True):
        hT, sdt = run_fwd_maps(dev, t, dtype, split, dirs, map_only, is_dt)
        mode = "map_only" if map_only else "full"
        ratio = ((sdt.double() - sum_ref).abs() / (6e-4 * sum_ref)).max()
        key = ("B sum_dt", str(dtype).split(".")[-1])
        WORST[key] = max(WORST.get(key, 0.0), float(ratio))
        print(f"\n[seqpar chain] {tag} {mode}: sum_dt worst err / tol {float(ratio):.3g}")
        assert float(ratio) <= 1.0 and bool(torch.isfinite(sdt).all()), (tag, mode, float(ratio))
        check(f"{tag} {mode} hT", hT, h_ref, dtype, part="B hT")
        got[map_only] = (hT, sdt)
    print(f"[seqpar chain] {tag}: full pass and map_only agree bit for bit: hT {torch.equal(got[False][0], got[True][0])}, "
          f"sum_dt {torch.equal(got[False][1], got[True][1])}")


@pytest.mark.parametrize("L", [37, 512, 1100, 1544])
@pytest.mark.parametrize("N", [16, 5])
@pytest.mark.parametrize("dtype", [F32, B16, F16])
def test_forward_segment_maps(backend, dtype, N, L):
    """Below a chunk, exactly one chunk, a ragged element-path tail, the vector path; both directions in one launch; two workgroups."""
    _, dev = backend
    fwd_maps_case(dev, 9, 2, L, N, dtype, False)
    figures(f"fwd maps {L} {N}")


@pytest.mark.parametrize("dtype", [B16, F16])
def test_forward_segment_maps_delta_is_dt(backend, dtype):
    _, dev = backend
    fwd_maps_case(dev, 9, 2, 1544, 16, dtype, True)
    figures("fwd maps delta_is_dt")


# ---- C / D. the ops across ranks --------------------------------------------------------------------------------------------------------
def planted_gates(dtype):
    tiny = {F32: 2.0 ** -149, B16: 2.0 ** -133, F16: 2.0 ** -24}[dtype]
    vals = [0.0, tiny]
    if dtype == F16:
        vals += [s * 2.0 ** -k for k in (15, 20, 24) for s in (1.0, -1.0)]
    return vals


def planted_positions(L, W):
    """[(value index, position)]: in the first, an interior and the last rank's segment, at its first and last position and in its
    middle.  Value j sits in channel j, in every row."""
    c = cuts(L, W)
    pos = []
    for r in sorted({0, W // 2 if W > 2 else 0, W - 1}):
        pos += [c[r], c[r + 1] - 1, (c[r] + c[r + 1]) // 2]
    return pos


def scan_case_inputs(L, W, regime, dtype, nsets):
    ts = [_scan_inputs(SCAN_E, SCAN_SB, L, SCAN_N, 61 + i, None, dtype, regime) for i in range(nsets)]
    z = ts[0]["z"].clone()
    for j, v in enumerate(planted_gates(dtype)):
        for p in planted_positions(L, W):
            z[j, :, p] = v
    z = z.to(dtype).float()
    assert float(z[0, 0, 0]) == 0.0 and float(z[1, 0, L - 1]) != 0.0   # (the subnormal survives the cast)
    return ts, z


def assert_segments_remember(ts, L, W):
    """On the reference inputs alone: every segment's decay product, float64."""
    c = cuts(L, W)
    figures = []
    for t in ts:
        dt = torch.nn.functional.softplus(t["delta"].double() + t["bias"].double()[:, None, None])
        for r in range(W):
            P = torch.exp(t["A"].double()[:, None, :] * dt[..., c[r]:c[r + 1]].sum(-1)[..., None])
            share = float((P >= 0.1).double().mean())
            assert share >= 0.5 and float(P.max()) >= 0.5 and float(P.min()) < 1e-3, (L, W, r, share, float(P.max()), float(P.min()))
            figures.append((share, float(P.max()), float(P.median())))
    return figures


_REFS = {}


def scan_reference(L, W, regime, dtype, nsets):
    """oracle64 on the whole rows, once per case (both backends read the same entry): outputs, gradients, the local dz scale."""
    key = (L, W, regime, dtype, nsets)
    if key in _REFS:
        return _REFS[key]
    ts, z = scan_case_inputs(L, W, regime, dtype, nsets)
    zr = z.double().clone().requires_grad_(True)
    rsets, refs = [], []
    for i, t in enumerate(ts):
        lv = leaves64(t, SET_ORDER)
        u, d, A, B, Cm, D, b = lv
        rsets.append(lv)
        refs.append(oracle64((u, d, A, B, Cm, D, zr, b), 1, *DIRS[i]))
    sum((r * t["w"].double()).sum() for r, t in zip(refs, ts)).backward()
    scale = torch.zeros_like(z, dtype=torch.float64)
    with torch.no_grad():
        for i, t in enumerate(ts):
            ys = [scan64(t["u"][:, sb].double(), t["delta"][:, sb].double(), t["A"].double(), t["B"][:, sb].double(), t["C"][:, sb].double(),
                         t["D"].double(), z[:, sb].double(), t["bias"].double(), None, DIRS[i][0] if sb < 1 else DIRS[i][1])[1]
                  for sb in range(SCAN_SB)]
            scale += t["w"].double().abs() * torch.stack(ys, 1).abs()
    ref = dict(outs=[r.detach() for r in refs], grads=[{k: v.grad for k, v in zip(SET_ORDER, lv)} for lv in rsets], dz=zr.grad,
               dz_scale=scale.clamp_min(1.0))
    _REFS[key] = ref
    return ref


def compare_scan(parts, L, W, regime, dtype, nsets, tag, part="C"):
    ref = scan_reference(L, W, regime, dtype, nsets)
    for i in range(nsets):
        check(f"{tag} set {i} out", torch.cat([p["outs"][i] for p in parts], -1), ref["outs"][i], dtype, part=part)
        for k in SET_ORDER:
            gs = [p["grads"][i][k].double() for p in parts]
            got = torch.cat(gs, -1) if k in ACT else sum(gs)
            check(f"{tag} set {i} d{k}", got, ref["grads"][i][k], dtype, part=part)
    dz = torch.cat([p["dz"] for p in parts], -1)
    nv = len(planted_gates(dtype))
    pos = torch.tensor(planted_positions(L, W))
    at = lambda x: x[:nv][..., pos]
    err = (at(dz).double() - at(ref["dz"])).abs()
    print(f"\n[seqpar chain] {tag}: dz at the planted gates: worst |err| {float(err.max()):.4g} (|fp64| there up to "
          f"{float(at(ref['dz']).abs().max()):.4g}, local scale up to {float(at(ref['dz_scale']).max()):.4g})")
    check(f"{tag} dz at the planted gates", at(dz), at(ref["dz"]), dtype, at(ref["dz_scale"]), reln=False, part=part + " dz planted")
    check(f"{tag} dz", dz, ref["dz"], dtype, part=part)


def conv_case_inputs(L, dirs, dtype, seed):
    x, sets, douts = conv_inputs(5, 3, L, [4], dtype, 1, [dirs], seed)
    return x, sets[0], douts[0]


def at_the_cuts(L, W):
    """Positions within three of an interior cut: where _HaloExchange.backward adds a neighbour's halo gradient."""
    m = torch.zeros(L, dtype=torch.bool)
    for c in cuts(L, W)[1:-1]:
        m[max(0, c - 3):c + 3] = True
    return m


def compare_conv(parts, L, W, dirs, dtype, seed, tag, name, which="rest"):
    """which = "rest": out, dw, dbias and dx away from the cuts; "cuts": dx at the cuts; "all": both."""
    x, wset, dout = conv_case_inputs(L, dirs, dtype, seed)
    ref = conv_reference(x, [wset], 1, [dout])
    E, K = wset[0].shape
    m = at_the_cuts(L, W)
    dx = torch.cat([p["dx"] for p in parts], -1)
    if which in ("cuts", "all"):
        hold(name, f"{tag}.dx at the cuts", dx[..., m], ref["dx"][0][..., m], ref["dx"][1][..., m], dtype)
    if which in ("rest", "all"):
        hold(name, f"{tag}.out", torch.cat([p["out"] for p in parts], -1), *ref["out"][0], dtype)
        hold(name, f"{tag}.dx", dx[..., ~m], ref["dx"][0][..., ~m], ref["dx"][1][..., ~m], dtype)
        hold(name, f"{tag}.dw", sum(p["dw"].double() for p in parts).view(E, K), *ref["dw"][0], F32)
        hold(name, f"{tag}.dbias", sum(p["db"].double() for p in parts), *ref["db"][0], F32)


class _MaskedHalo:
    """Control: _HaloExchange with one side's halo (and with it that side's gradient) zeroed."""

    def __init__(self, orig, side, halo):
        self.orig, self.side, self.halo = orig, side, halo

    def apply(self, x, group):
        ext = self.orig.apply(x, group)
        m = torch.ones(ext.shape[-1], dtype=ext.dtype, device=ext.device)
        if self.side == "right":
            m[-self.halo:] = 0
        else:
            m[:self.halo] = 0
        return ext * m


@contextlib.contextmanager
def _mutated(seqpar, mut, world):
    compose, halo = seqpar._compose, seqpar._HaloExchange
    if mut == "P0":
        seqpar._compose = lambda P, S, *a, **kw: compose([torch.zeros_like(p) for p in P], S, *a, **kw)
    elif mut == "P1":
        seqpar._compose = lambda P, S, *a, **kw: compose([torch.ones_like(p) for p in P], S, *a, **kw)
    elif mut == "drop_h0":   # the state entering the last rank withheld
        seqpar._compose = lambda P, S, rank, split, rl, rh, towards_end: (
            torch.zeros_like(S[0]) if (not towards_end and rank == world - 1) else compose(P, S, rank, split, rl, rh, towards_end))
    elif mut == "drop_dhT":
        seqpar._compose = lambda P, S, rank, split, rl, rh, towards_end: (
            torch.zeros_like(S[0]) if towards_end else compose(P, S, rank, split, rl, rh, towards_end))
    elif mut in ("halo_right", "halo_left"):
        seqpar._HaloExchange = _MaskedHalo(halo, mut.split("_")[1], seqpar.HALO)
    else:
        assert mut is None, mut
    try:
        yield
    finally:
        seqpar._compose, seqpar._HaloExchange = compose, halo


def _scan_job(seqpar, dev, rank, W, job):
    dtype, nsets, L = DT[job["dtype"]], job["nsets"], job["L"]
    ts, z = scan_case_inputs(L, W, job["regime"], dtype, nsets)
    c = cuts(L, W)
    seg = slice(c[rank], c[rank + 1])
    zd = leaf(z[..., seg], dev, dtype)
    dsets = [tuple(leaf(t[k][..., seg] if k in ACT else t[k], dev, dtype if k in ACT else F32) for k in SET_ORDER) for t in ts]
    outs = seqpar.selective_scan_multi(dsets, zd, 1, DIRS[:nsets])
    sum((o.float() * t["w"][..., seg].to(dev)).sum() for o, t in zip(outs, ts)).backward()
    return dict(outs=[o.detach().cpu() for o in outs], dz=zd.grad.cpu(),
                grads=[{k: a.grad.cpu() for k, a in zip(SET_ORDER, s)} for s in dsets])


def _conv_job(seqpar, dev, rank, W, job):
    dtype, L = DT[job["dtype"]], job["L"]
    x, (w, b, dirs), dout = conv_case_inputs(L, tuple(job["dirs"]), dtype, job["seed"])
    c = cuts(L, W)
    seg = slice(c[rank], c[rank + 1])
    xd = leaf(x[..., seg], dev)
    wd = leaf(w.view(w.shape[0], 1, -1), dev)
    bd = leaf(b, dev)
    out = seqpar.causal_conv1d(xd, wd, bd, 1, *dirs)
    out.backward(dout[..., seg].to(dev).contiguous())
    return dict(out=out.detach().cpu(), dx=xd.grad.cpu(), dw=wd.grad.cpu(), db=bd.grad.cpu())


def _worker(rank, world, port, out_dir, device, emu, plan):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))  # a dead peer ends the run
    from caduceus_amd import seqpar
    CL.use_library_for_testing(emu)   # None: the real gfx950 library
    dev = torch.device(device)
    results = {}
    with seqpar.sequence_parallel():
        for job in plan:
            with _mutated(seqpar, job.get("mut"), world):
                results[job["id"]] = (_scan_job if job["kind"] == "scan" else _conv_job)(seqpar, dev, rank, world, job)
    torch.save(results, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def spawn(world, device, plan, out_dir):
    """One spawn for the whole plan; returns the per-rank result dicts."""
    emu = _emu() if device == "cpu" else None
    os.makedirs(out_dir, exist_ok=True)
    mp.spawn(_worker, args=(world, _free_port(), str(out_dir), device, emu, plan), nprocs=world, join=True)
    return [torch.load(os.path.join(out_dir, f"rank{r}.pt")) for r in range(world)]


CONV_LLOC = [3, 4, 5, 7]


def conv_lengths(W):
    return [W * n for n in CONV_LLOC] + [5 * W + W // 2]   # the last one cut unequally (W 3: 5, 6, 6; W 4: 5, 6, 5, 6)


def scan_id(L, name, nsets):
    return f"scan L={L} {name} nsets={nsets}"


def conv_id(L, dirs, name):
    return f"conv L={L} dirs={dirs[0]}{dirs[1]} {name}"


def full_plan(W):
    plan = [dict(kind="scan", id=scan_id(L, n, ns), L=L, regime="long_memory", dtype=n, nsets=ns)
            for L in SCAN_CASES[W] for n in NAMES for ns in (1, 2)]
    plan += [dict(kind="conv", id=conv_id(L, d, n), L=L, dirs=d, dtype=n, seed=1000 * W + L)
             for L in conv_lengths(W) for d in DIRS for n in NAMES[:2]]
    return plan


def _runs(request, tmp_path_factory, W):
    device = "cpu" if request.param == "emu" else "cuda:0"
    return request.param, spawn(W, device, full_plan(W), tmp_path_factory.mktemp(f"chain_w{W}_{request.param}"))


BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]


@pytest.fixture(scope="module", params=BACKENDS)
def runs3(request, tmp_path_factory):
    return _runs(request, tmp_path_factory, 3)


@pytest.fixture(scope="module", params=BACKENDS)
def runs4(request, tmp_path_factory):
    return _runs(request, tmp_path_factory, 4)


def _scan_across(runs, W, L, name, nsets):
    backend, parts = runs
    dtype = DT[name]
    ts, _ = scan_case_inputs(L, W, "long_memory", dtype, nsets)
    assert_segments_remember(ts, L, W)
    tag = f"{backend} W={W} {scan_id(L, name, nsets)}"
    compare_scan([p[scan_id(L, name, nsets)] for p in parts], L, W, "long_memory", dtype, nsets, tag)
    figures(tag)


@pytest.mark.parametrize("nsets", [1, 2])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("L", SCAN_CASES[3])
def test_scan_three_ranks(runs3, L, name, nsets):
    _scan_across(runs3, 3, L, name, nsets)


@pytest.mark.parametrize("nsets", [1, 2])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("L", SCAN_CASES[4])
def test_scan_four_ranks(runs4, L, name, nsets):
    _scan_across(runs4, 4, L, name, nsets)


def _conv_across(runs, W, i, dirs, name, which="rest"):
    backend, parts = runs
    L = conv_lengths(W)[i]
    cid = conv_id(L, dirs, name)
    compare_conv([p[cid] for p in parts], L, W, dirs, DT[name], 1000 * W + L, f"seqpar W={W} {cid}", backend, which)


def _conv_dx_at_the_cuts(runs, W, name):
    """Every length and direction assignment of one (W, dtype); all of them are compared before the verdict."""
    failed = []
    for i in range(5):
        for dirs in DIRS:
            try:
                _conv_across(runs, W, i, dirs, name, "cuts")
            except AssertionError as ex:
                failed.append(str(ex))
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("name", NAMES[:2])
@pytest.mark.parametrize("dirs", DIRS)
@pytest.mark.parametrize("i", range(5))
def test_conv_three_ranks(runs3, i, dirs, name):
    _conv_across(runs3, 3, i, dirs, name)


@pytest.mark.parametrize("name", NAMES[:2])
@pytest.mark.parametrize("dirs", DIRS)
@pytest.mark.parametrize("i", range(5))
def test_conv_four_ranks(runs4, i, dirs, name):
    _conv_across(runs4, 4, i, dirs, name)


@pytest.mark.parametrize("name", NAMES[:2])
def test_conv_dx_at_the_cuts_three_ranks(runs3, name):
    """dx at the positions that receive a neighbour's halo gradient, same reference and bounds (the module docstring, part D, has what
    bfloat16 returned there before the two ranks' parts were added in fp32)."""
    _conv_dx_at_the_cuts(runs3, 3, name)


@pytest.mark.parametrize("name", NAMES[:2])
def test_conv_dx_at_the_cuts_four_ranks(runs4, name):
    """As test_conv_dx_at_the_cuts_three_ranks."""
    _conv_dx_at_the_cuts(runs4, 4, name)


# ---- controls ---------------------------------------------------------------------------------------------------------------------------
MUT_L = {2: 1100, 3: 2100}


def test_compose_mutations(tmp_path):
    """The table of the module docstring, emulator, fp32, two sets; each W's column in one spawn.  Also D's halo controls (W = 3, local
    length 5, both direction assignments): zeroing either side's halo must fail the conv comparison."""
    saved = dict(WORST)
    try:
        verdicts = {}
        for W, jobs in ((2, [("P0", "long_memory")]),
                        (3, [(None, "long_memory"), ("P0", "suite"), ("P0", "long_memory"), ("P1", "long_memory"),
                             ("drop_h0", "long_memory"), ("drop_dhT", "long_memory")])):
            L = MUT_L[W]
            plan = [dict(kind="scan", id=f"{m} {reg}", L=L, regime=reg, dtype="float32", nsets=2, mut=m) for m, reg in jobs]
            if W == 3:
                plan += [dict(kind="conv", id=f"{m} {d}", L=15, dirs=d, dtype="float32", seed=3015, mut=m)
                         for m in (None, "halo_right", "halo_left") for d in DIRS]
            parts = spawn(W, "cpu", plan, tmp_path / f"w{W}")
            for m, reg in jobs:
                if reg == "long_memory":
                    assert_segments_remember(scan_case_inputs(L, W, reg, F32, 2)[0], L, W)
                try:
                    compare_scan([p[f"{m} {reg}"] for p in parts], L, W, reg, F32, 2, f"mutation {m} W={W} {reg}", part="control")
                    verdicts[(m, W, reg)] = "passes"
                except AssertionError:
                    verdicts[(m, W, reg)] = "fails"
            if W == 3:
                for m in (None, "halo_right", "halo_left"):
                    for d in DIRS:
                        try:
                            compare_conv([p[f"{m} {d}"] for p in parts], 15, 3, d, F32, 3015, f"control {m} {d}", "control", "all")
                            verdicts[(m, "conv", d)] = "passes"
                        except AssertionError:
                            verdicts[(m, "conv", d)] = "fails"
        print("\n[seqpar chain] verdicts:", verdicts)
        assert verdicts[("P0", 2, "long_memory")] == "passes"
        assert verdicts[(None, 3, "long_memory")] == "passes"
        assert verdicts[("P0", 3, "suite")] == "passes"
        for m in ("P0", "P1", "drop_h0", "drop_dhT"):
            assert verdicts[(m, 3, "long_memory")] == "fails", m
        for d in DIRS:
            assert verdicts[(None, "conv", d)] == "passes"
            assert verdicts[("halo_right", "conv", d)] == "fails" and verdicts[("halo_left", "conv", d)] == "fails", d
    finally:
        WORST.clear()
        WORST.update(saved)   # (the mutated runs are not kernel errors)
        for key in [k for k in HOLD_WORST if k[0] == "control"]:
            del HOLD_WORST[key]


# ---- E. the model at W = 3 on long-memory weights ---------------------------------------------------------------------------------------
def make_long_memory(model, dt0, seed=123):
    """Overwrites every A_log and dt_proj.bias from a fixed seed: A = -(0.02 + rand), every fourth state left as it is;
    softplus(bias) = dt0 (0.75 + 0.5 rand)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("A_log"):
                new = torch.log(0.02 + torch.rand(p.shape, generator=g))
                new[:, 3::4] = p[:, 3::4].cpu()
                p.copy_(new)
            elif n.endswith("dt_proj.bias"):
                dt = (dt0 * (0.75 + 0.5 * torch.rand(p.shape, generator=g))).double()
                p.copy_((dt + torch.log(-torch.expm1(-dt))).float())


def assert_model_remembers(model, Lseg):
    """Part C's condition per mixer, float64, dt = softplus(dt_proj.bias) ALONE (without the data-dependent dt_proj(x))."""
    figures = []
    for n, m in model.named_modules():
        if hasattr(m, "A_log") and hasattr(m, "dt_proj"):
            A = -torch.exp(m.A_log.detach().double().cpu())
            dt = torch.nn.functional.softplus(m.dt_proj.bias.detach().double().cpu())
            P = torch.exp(A * (Lseg * dt)[:, None])
            share = float((P >= 0.1).double().mean())
            assert share >= 0.5 and float(P.max()) >= 0.5 and float(P.min()) < 1e-3, (n, share, float(P.max()), float(P.min()))
            figures.append((share, float(P.max()), float(P.median())))
    assert figures
    return figures


def _model_worker(rank, world, port, out_dir, name, L, dt0, device):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    from caduceus_amd import seqpar
    from caduceus_amd.dp import BucketedGradReducer
    model, rec = _setup_model(name, device)
    make_long_memory(model, dt0)
    reducer = BucketedGradReducer(model.parameters(), average=False)  # partial sums over each rank's tokens
    ids, labels = _long_batch(rec, L)
    ids, labels = ids.to(device), labels.to(device)
    seg = slice(rank * L // world, (rank + 1) * L // world)
    reducer.zero_grad()
    with seqpar.sequence_parallel():
        logits = model(ids[:, seg]).logits
        loss = seqpar.masked_lm_loss(logits, labels[:, seg], ignore_index=4)
    loss.backward()
    reducer.finish()
    total = loss.detach().clone()
    dist.all_reduce(total)
    torch.save({"logits": logits.detach().cpu(), "loss": total.cpu(),
                "grads": {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _model_three_ranks(tmp_path, device, L, dt0, logits_atol):
    world, name = 3, "ps_fused"
    if device == "cpu":
        _emu()
    mp.spawn(_model_worker, args=(world, _free_port(), str(tmp_path), name, L, dt0, device), nprocs=world, join=True)
    parts = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]
    model, rec = _setup_model(name, device)
    make_long_memory(model, dt0)
    print("\n[seqpar chain] model decay per mixer (share >= 0.1, max, median):", assert_model_remembers(model, L // world))
    ids, labels = _long_batch(rec, L)
    out = model(ids.to(device), labels=labels.to(device))
    out.loss.backward()
    logits = torch.cat([p["logits"] for p in parts], 1)
    print(f"[seqpar chain] model W=3 {device}: worst |logits - single process| {float((logits - out.logits.detach().cpu()).abs().max()):.3g}")
    torch.testing.assert_close(logits, out.logits.detach().cpu(), rtol=2e-4, atol=logits_atol)
    torch.testing.assert_close(parts[0]["loss"], out.loss.detach().cpu(), rtol=1e-5, atol=1e-6)
    worst = 0.0
    for n, p in model.named_parameters():
        g = p.grad.detach().cpu()
        scale = max(1.0, float(g.abs().max()))
        worst = max(worst, float(((parts[0]["grads"][n] - g).abs() / (2e-3 * g.abs() + 2e-4 * scale)).max()))
    print(f"[seqpar chain] model W=3 {device}: worst gradient err / tol {worst:.3g}")
    for n, p in model.named_parameters():
        g = p.grad.detach().cpu()
        scale = max(1.0, float(g.abs().max()))
        torch.testing.assert_close(parts[0]["grads"][n], g, rtol=2e-3, atol=2e-4 * scale, msg=lambda m, n=n: f"{n}: {m}")
        if device == "cpu":
            for r in (1, 2):
                assert torch.equal(parts[0]["grads"][n], parts[r]["grads"][n]), n


def test_model_three_ranks_long_memory(tmp_path):
    """Emulator: logits, loss and every parameter gradient equal the single-process run (bounds of
    test_seqpar.test_sequence_parallel_matches_single_process)."""
    try:
        _model_three_ranks(tmp_path, "cpu", 3 * 352, 4e-3, 2e-4)
    finally:
        CL.use_library_for_testing(None)


@pytest.mark.gpu
def test_model_three_ranks_long_memory_on_the_gpu(tmp_path):
    """Three processes on cuda:0 over gloo (bounds of test_seqpar.test_sequence_parallel_two_processes_on_the_gpu); segments of two
    chunks and a tail.  dt0 = 1.5e-3: see the module docstring."""
    _model_three_ranks(tmp_path, "cuda:0", 3 * 1408, 1.5e-3, 4e-4)
