"""The score head (csrc/score.hip, cad_lm_head_score) held to float64, element by element, from the same stored hidden state.

Bounds: the `logits` and `row loss` lines of the header of tests/test_norm_head_fp64.py, restated per scored row; the constants U, UF,
EXP_ULPS, LOG_ULPS and gam() are imported from there, nothing is fitted to a result.  A = the ids the mask allows (all V without one):
  z[v]            e_z[v] = g(S D + 2) sum |h w| + S D UF                    (the forward's logit row)
  lse over A      E = max_A e_z (lse is 1-Lipschitz in it); the exp terms carry rho_e = 2 u EXP_ULPS + u (spread + 1) relative,
                  spread = max_A |z - max_A z| + 2 E, their sum g(V) more: rho_se = rho_e + g(V) + V UF; logf 2 u LOG_ULPS |lse - max|;
                  the add of the maximum u |lse|:   e_lse = E + rho_se (1 + rho_se) + 2 u LOG_ULPS |lse - max| + u |lse| + 2 u E
  logp_all[v]     (z[v] + mask[v]) - lse:  tol = e_lse + e_z[v] + u |logp_all[v]|   for v in A (with v the label this is that header's
                  e_row, which is what `logp` is held to); exactly -inf outside A (non-finite classes must match)
  logp            0.0 exactly where the target is ignore_index or outside [0, V); -inf exactly where it is masked
  sum_A exp(logp_all) = 1 within g(V) + rho_se (summed in fp64 from the kernel's own outputs)
Masked ids take no part in lse, E or spread.
"""
import ctypes as C
import math
import os
import subprocess

import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops
from conftest import ROOT
from test_norm_head_fp64 import BF, COMP, COMP12, EXP_ULPS, F32, HF, LOG_ULPS, TAG, U, UF, Arena, gam, hold, lm_inputs

COMP5 = torch.tensor([0, 2, 1, 4, 3])  # 1 <-> 2, 3 <-> 4
COMPS = {16: COMP, 12: COMP12, 5: COMP5}
NEG_INF = float("-inf")
MFMA = [(128, F32), (128, BF), (128, HF), (256, F32), (256, BF), (256, HF), (512, BF)]
GENERAL = [(40, F32), (40, BF), (40, HF), (64, F32), (64, BF), (64, HF)]


def _mask(V, allowed):
    if allowed is None:
        return None
    m = torch.full((V,), NEG_INF)
    m[list(allowed)] = 0.0
    return m


def score_reference(h, W, comp, row_index, targets, mask, ign):
    """fp64 values and tolerances {name: (ref, tol)} for the scored rows.  h (S, R, D) as stored, W (V, D) fp32."""
    S, R, D = h.shape
    V = W.shape[0]
    idx = torch.arange(R) if row_index is None else row_index.reshape(-1)
    H, Wd = h.double()[:, idx], W.double()
    z, az = H[0] @ Wd.t(), H[0].abs() @ Wd.abs().t()
    if S == 2:
        z, az = z + H[1] @ Wd[comp].t(), az + H[1].abs() @ Wd[comp].abs().t()
    e_z = gam(S * D + 2) * az + S * D * UF
    allowed = torch.ones(V, dtype=torch.bool) if mask is None else mask == 0
    al = allowed[None, :].expand_as(z)
    zero = torch.zeros_like(z)
    zm = torch.where(al, z, torch.full_like(z, NEG_INF))
    mx = zm.max(-1).values
    lse = torch.logsumexp(zm, -1)
    E = torch.where(al, e_z, zero).max(-1).values
    spread = torch.where(al, (z - mx[:, None]).abs(), zero).max(-1).values + 2 * E
    rho_e = 2 * U * EXP_ULPS + U * (spread + 1)
    rho_se = rho_e + gam(V) + V * UF
    e_lse = E + rho_se * (1 + rho_se) + 2 * U * LOG_ULPS * (lse - mx).abs() + U * lse.abs() + 2 * U * E
    lp = zm - lse[:, None]
    tol = torch.where(al, e_lse[:, None] + e_z + U * torch.where(al, lp, zero).abs(), zero)
    out = {"logp_all": (lp, tol), "sum_bound": gam(V) + rho_se, "e_z": e_z, "E": E}
    if targets is not None:
        t = targets.reshape(-1)
        valid = (t != ign) & (t >= 0) & (t < V)
        tc = t.clamp(0, V - 1)[:, None]
        out["logp"] = (torch.where(valid, lp.gather(1, tc)[:, 0], torch.zeros_like(lse)),
                       torch.where(valid, tol.gather(1, tc)[:, 0], torch.zeros_like(lse)))
    return out


def run_score(dev, h, W, comp, targets=None, row_index=None, mask=None, want_all=True, ign=4):
    S, R, D = h.shape
    to = lambda t: None if t is None else t.to(dev)
    with torch.no_grad():
        res = ops.lm_head_score(h.to(dev), to(W), to(comp) if S == 2 else None, targets=to(targets), row_index=to(row_index),
                                logit_mask=to(mask), want_all=want_all, ignore_index=ign)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return res


def check(backend, tag, h, W, comp, targets, row_index, mask, ign=4, sum_to_one=True):
    """logp and logp_all of one call against score_reference, and the normalisation; returns (logp, logp_all)."""
    name, dev = backend
    ref = score_reference(h, W, comp, row_index, targets, mask, ign)
    logp, logp_all = run_score(dev, h, W, comp, targets, row_index, mask, True, ign)
    n = ref["logp_all"][0].shape[0]
    assert logp.shape == (tuple(row_index.shape) if row_index is not None else (h.shape[1],)) and logp_all.numel() == n * W.shape[0]
    hold(name, f"{tag}.logp_all", logp_all, *ref["logp_all"], F32)
    hold(name, f"{tag}.logp", logp, *ref["logp"], F32)
    # normalisation over the allowed ids, from the kernel's own outputs
    s = torch.exp(logp_all.double().cpu().reshape(n, -1)).sum(-1)
    dev1 = (s - 1).abs()
    print(f"[fp64] {name} {tag}: worst |sum exp(logp_all) - 1| / bound = {float((dev1 / ref['sum_bound']).max()):.3f}")
    if sum_to_one:
        assert bool((dev1 <= ref["sum_bound"]).all()), (tag, float(dev1.max()), float(ref["sum_bound"].min()))
    return logp, logp_all


def _targets(R, V, g, mask_allowed, ign=4):
    """Random ids, with ignore_index, -1, V and (if there is a mask) a forbidden id among them."""
    t = torch.randint(0, V, (R,), generator=g)
    specials = [ign, -1, V] + ([next(v for v in range(V) if v not in mask_allowed)] if mask_allowed is not None else [])
    for k, s in enumerate(specials):
        if k < R:
            t[(3 * k + 1) % R] = s
    return t


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("D,dtype", MFMA + GENERAL, ids=[f"D{d}-{TAG[t]}" for d, t in MFMA + GENERAL])
def test_score_rows_widths_vocabularies(backend, D, dtype, S):
    """n in {1, 15, 16, 17, 33} (below, at and above one 16-row tile; 33: a wave's workgroup holds three tiles, the last with one row)
    at every width class and dtype of both paths, V in {16, 12, 5}, with and without a mask."""
    lib = L.get_lib()
    assert lib.cad_lm_head_score_supported(D, 16, L.dtype_code(dtype)) == 1
    for k, n in enumerate([1, 15, 16, 17, 33]):
        for V in ((16, 12, 5) if n in (17, 33) else ((16, 12, 5)[k % 3],)):
            comp = COMPS[V]
            allowed = None if (k + V) % 2 else ([7, 8, 9, 10] if V > 10 else [1, 3, 4])
            g = torch.Generator().manual_seed(1000 * D + 10 * n + V + S)
            h, W, _, _ = lm_inputs(S, n, D, V, dtype, 17 * D + n + V, comp=comp)
            check(backend, f"score-D{D}-n{n}-V{V}-S{S}", h, W, comp, _targets(n, V, g, allowed), None, _mask(V, allowed))


def _cu_count(n):
    L.check(L.get_lib().cad_debug_set_cu_count(int(n)), "cad_debug_set_cu_count")


@pytest.mark.parametrize("D,dtype,S", [(128, BF, 2), (256, F32, 1), (512, BF, 2)], ids=["D128-bf16-S2", "D256-f32-S1", "D512-bf16-S2"])
def test_score_three_tile_walk(backend, D, dtype, S):
    """The matrix-core launcher sizes its grid by the CU count (two workgroups of four waves per CU at most).  With one CU, 8 waves walk
    18 tiles at n = 275: waves 0 and 1 take three tiles each (prefetch of the next tile's rows, W registers kept), wave 1's last one
    ragged with 3 rows.  Once on rows 0 .. n - 1 and once on a reversed gather of them."""
    n = 2 * 8 * 16 + 16 + 3
    g = torch.Generator().manual_seed(D + S)
    h, W, _, _ = lm_inputs(S, n, D, 16, dtype, 3 * D + S)
    t = _targets(n, 16, g, [7, 8, 9, 10])
    try:
        _cu_count(1)
        a = check(backend, f"score-walk-D{D}", h, W, COMP, t, None, _mask(16, [7, 8, 9, 10]))
        b = check(backend, f"score-walk-rev-D{D}", h, W, COMP, t.flip(0), torch.arange(n - 1, -1, -1), _mask(16, [7, 8, 9, 10]))
    finally:
        _cu_count(0)
    assert torch.equal(a[1].cpu(), b[1].cpu().flip(0)), "a row's result depends on its place in the walk"


def test_score_general_path_walk(backend):
    """One wave per scored row, 4096 workgroups of 4 at most: at 16384 + 13 scored rows thirteen waves take a second row (a gather with
    repeats over 1000 stored rows keeps the input small)."""
    n, R = 16384 + 13, 1000
    g = torch.Generator().manual_seed(5)
    h, W, _, _ = lm_inputs(2, R, 40, 12, BF, 91, comp=COMP12)
    idx = (torch.arange(n) * 7) % R
    check(backend, "score-general-walk", h, W, COMP12, torch.randint(0, 12, (n,), generator=g), idx, None)


@pytest.mark.parametrize("D,dtype", [(128, BF), (256, HF), (40, F32)], ids=["D128-bf16", "D256-f16", "D40-f32"])
@pytest.mark.parametrize("kind", ["identity", "reversed", "repeated", "sparse"])
def test_score_row_index(backend, kind, D, dtype):
    name, dev = backend
    R = 1000 if kind == "sparse" else 37
    g = torch.Generator().manual_seed(D)
    h, W, _, _ = lm_inputs(2, R, D, 16, dtype, 300 + D)
    idx = {"identity": torch.arange(R), "reversed": torch.arange(R - 1, -1, -1),
           "repeated": torch.tensor([5, 5, 0, 36, 5, 36, 36, 1, 0, 0, 5, 17, 17, 17, 17, 17, 17, 2, 5]),
           "sparse": torch.tensor([999, 0, 513, 16, 15, 700, 513])}[kind]
    t = _targets(idx.numel(), 16, g, None)
    logp, logp_all = check(backend, f"score-{kind}-D{D}", h, W, COMP, t, idx, None)
    if kind == "identity":  # the same rows without an index: the same bits
        logp0, all0 = run_score(dev, h, W, COMP, t)
        assert torch.equal(logp0, logp) and torch.equal(all0, logp_all)
    if kind == "repeated":  # a repeated row gives the same bits every time
        first = {}
        for i, r in enumerate(idx.tolist()):
            assert torch.equal(logp_all[i], logp_all[first.setdefault(r, i)])
    if kind == "sparse":    # a 2-d index shapes the outputs
        l2, a2 = run_score(dev, h, W, COMP, t[:6].reshape(2, 3), idx[:6].reshape(2, 3))
        assert l2.shape == (2, 3) and a2.shape == (2, 3, 16) and torch.equal(a2.reshape(6, 16), logp_all[:6])


@pytest.mark.parametrize("D,dtype", [(128, BF), (40, F32)], ids=["D128-bf16", "D40-f32"])
def test_score_sparse_gather_leaves_the_rest_untouched(backend, D, dtype):
    """Through the C entry point: 7 gathered rows written into the head of sentinel-filled outputs of 20 rows; the rest stays."""
    name, dev = backend
    R, n, V, SENT = 1000, 7, 16, -512.0
    h, W, _, _ = lm_inputs(2, R, D, V, dtype, 400 + D)
    idx = torch.tensor([999, 0, 513, 16, 15, 700, 513])
    t = torch.tensor([3, 4, 7, 0, 15, 9, 8])
    hd, wd, cd, idd, td = h.to(dev), W.to(dev), COMP.to(dev), idx.to(dev), t.to(dev)
    logp = torch.full((20,), SENT, device=dev)
    logp_all = torch.full((20, V), SENT, device=dev)
    stream = L.stream_and_check(hd, wd, cd, idd, td, logp, logp_all)
    a = L.LmScoreArgs(L.ptr(hd), L.ptr(wd), L.ptr(cd), L.ptr(idd), L.ptr(td), None, L.ptr(logp), L.ptr(logp_all), R, n, D, V, 2, 4,
                      L.dtype_code(dtype))
    L.check(L.get_lib().cad_lm_head_score(C.byref(a), stream), "cad_lm_head_score")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    ref = score_reference(h, W, COMP, idx, t, None, 4)
    hold(name, "score-sentinel.logp_all", logp_all[:n], *ref["logp_all"], F32)
    hold(name, "score-sentinel.logp", logp[:n], *ref["logp"], F32)
    assert bool((logp[n:] == SENT).all()) and bool((logp_all[n:] == SENT).all()), "rows beyond n were written"
    # logp alone, and logp_all alone
    for lp_on, all_on in ((True, False), (False, True)):
        lp2, all2 = torch.full((20,), SENT, device=dev), torch.full((20, V), SENT, device=dev)
        a.logp, a.logp_all = (L.ptr(lp2) if lp_on else None), (L.ptr(all2) if all_on else None)
        L.check(L.get_lib().cad_lm_head_score(C.byref(a), stream), "cad_lm_head_score")
        assert torch.equal(lp2, logp if lp_on else torch.full_like(lp2, SENT))
        assert torch.equal(all2, logp_all if all_on else torch.full_like(all2, SENT))


@pytest.mark.parametrize("D,dtype", [(128, F32), (256, BF), (64, HF)], ids=["D128-f32", "D256-bf16", "D64-f16"])
def test_score_special_targets_and_mask(backend, D, dtype):
    """ignore_index, -1, V and a masked id give 0.0, 0.0, 0.0 and -inf exactly; logp_all is -inf exactly at the masked ids."""
    name, dev = backend
    V, ign, allowed = 12, 4, [7, 8, 9, 10]
    h, W, _, _ = lm_inputs(2, 21, D, V, dtype, 500 + D, comp=COMP12)
    t = torch.tensor([ign, -1, V, 3, 7, 8, 9, 10, 1 << 40, 0, 11] + [7] * 10)
    logp, logp_all = check(backend, f"score-specials-D{D}", h, W, COMP12, t, None, _mask(V, allowed), ign)
    lp, la = logp.cpu(), logp_all.cpu()
    assert lp[:3].tolist() == [0.0, 0.0, 0.0] and lp[8].item() == 0.0
    assert lp[3].item() == NEG_INF and lp[9].item() == NEG_INF and lp[10].item() == NEG_INF
    assert bool(torch.isfinite(lp[4:8]).all()) and bool((lp[4:8] <= 0).all())
    forbidden = torch.tensor([v not in allowed for v in range(V)])
    assert bool((la[:, forbidden] == NEG_INF).all()) and bool(torch.isfinite(la[:, ~forbidden]).all())


@pytest.mark.parametrize("D,dtype", [(128, BF), (256, F32), (40, HF)], ids=["D128-bf16", "D256-f32", "D40-f16"])
def test_score_batch_independence(backend, D, dtype):
    """A row scored alone equals, bit for bit, the same row scored inside a batch (no cross-row state, no atomics)."""
    name, dev = backend
    h, W, _, _ = lm_inputs(2, 37, D, 16, dtype, 600 + D)
    t = torch.randint(0, 16, (37,), generator=torch.Generator().manual_seed(3))
    m = _mask(16, [7, 8, 9, 10])
    logp, logp_all = run_score(dev, h, W, COMP, t, None, m)
    for r in (0, 15, 16, 36):
        l1, a1 = run_score(dev, h[:, r:r + 1].contiguous(), W, COMP, t[r:r + 1], None, m)
        l2, a2 = run_score(dev, h, W, COMP, t[r:r + 1], torch.tensor([r]), m)
        assert torch.equal(l1[0], logp[r]) and torch.equal(a1[0], logp_all[r]), r
        assert torch.equal(l2[0], logp[r]) and torch.equal(a2[0], logp_all[r]), r


@pytest.mark.parametrize("D,dtype", [(128, F32), (128, BF), (40, F32), (40, HF)], ids=["D128-f32", "D128-bf16", "D40-f32", "D40-f16"])
@pytest.mark.parametrize("kind", ["one-80-above", "all-equal", "shifted+100"])
def test_score_edge_values(backend, kind, D, dtype):
    name, dev = backend
    S, R, V = 2, 19, 16
    g = torch.Generator().manual_seed(D + len(kind))
    e = torch.randn(D, generator=g)
    e = e / e.norm()
    if kind == "all-equal":  # the same weight row for every id: equal logits, bit for bit; logp_all = -log(number of allowed ids)
        W = (2.0 * e)[None, :].expand(V, D).contiguous()
        h = torch.randn(S, R, D, generator=g).to(dtype)
    else:  # logit v = (target[v] + target[comp v]) / 2 + noise; id 3 is a fixed point of COMP
        target = torch.zeros(V)
        target[3] = 80.0
        if kind == "shifted+100":
            target = torch.linspace(-15, 15, V) + 100  # every logit above fp32's exp range
        W = target[:, None] * e[None, :] + 0.01 * torch.randn(V, D, generator=g)
        h = (0.5 * e[None, None, :] * torch.ones(S, R, 1) + 0.01 * torch.randn(S, R, D, generator=g)).to(dtype)
    t = torch.randint(0, V, (R,), generator=g)
    for allowed in (None, [2, 3, 5, 11]):
        # (logits near 100: the rounding of lse itself, u |lse|, is outside what the normalisation bound counts)
        logp, logp_all = check(backend, f"score-{kind}-D{D}", h, W, COMP, t, None, _mask(V, allowed), sum_to_one=kind != "shifted+100")
        la = logp_all.cpu()
        keep = torch.ones(V, dtype=torch.bool) if allowed is None else torch.tensor([v in allowed for v in range(V)])
        assert bool(torch.isfinite(la[:, keep]).all()), "overflow"
        if kind == "one-80-above":
            others = keep.clone()
            others[3] = False
            assert bool((la[:, 3].abs() < 1e-6).all()) and bool((la[:, others] < -70).all())
        if kind == "all-equal":
            assert bool((la[:, keep] == la[:, keep][:, :1]).all())
            assert bool((la[:, keep] + math.log(int(keep.sum()))).abs().max() < 1e-6)


@pytest.mark.parametrize("dtype", [F32, BF, HF], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("D", [128, 256])
def test_score_misaligned_hidden_takes_the_general_path(backend, D, dtype):
    """hidden one element into its buffer: no 16-byte loads are possible, the launcher takes the one-wave-per-row kernel.  Same bounds,
    sentinels around the view intact; the aligned call (matrix cores) holds them too."""
    name, dev = backend
    S, R, V = 2, 37, 16
    h, W, _, _ = lm_inputs(S, R, D, V, dtype, 700 + D)
    t = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(D))
    A = Arena(dev, 1)
    hv = A.put(h)
    assert hv.data_ptr() % 16 != 0 and hv.is_contiguous()
    ref = score_reference(h, W, COMP, None, t, None, 4)
    with torch.no_grad():
        logp, logp_all = ops.lm_head_score(hv, W.to(dev), COMP.to(dev), targets=t.to(dev), want_all=True, ignore_index=4)
    hold(name, "score-misaligned.logp_all", logp_all, *ref["logp_all"], F32)
    hold(name, "score-misaligned.logp", logp, *ref["logp"], F32)
    A.intact()
    check(backend, "score-aligned", h, W, COMP, t, None, None)


def test_score_refusals(backend):
    name, dev = backend
    h, W, _, _ = lm_inputs(2, 5, 64, 16, F32, 1)
    hd, wd, cd = h.to(dev), W.to(dev), COMP.to(dev)
    lib = L.get_lib()
    assert lib.cad_lm_head_score_supported(64, 17, 0) == 0 and lib.cad_lm_head_score_supported(64, 16, 3) == 0
    assert lib.cad_lm_head_score_supported(1000, 1, 2) == 1
    with pytest.raises(ops.ScoreUnsupported, match="vocab_size 72"):
        ops.lm_head_score(hd, torch.zeros(72, 64, device=dev), None, want_all=True)
    with pytest.raises(RuntimeError, match="no backward"):
        ops.lm_head_score(hd, wd.clone().requires_grad_(True), cd, want_all=True)
    with torch.no_grad():  # (grad mode off: parameters are fine)
        ops.lm_head_score(hd, wd.clone().requires_grad_(True), cd, want_all=True)
    with pytest.raises(ValueError, match="targets"):
        ops.lm_head_score(hd, wd, cd)
    with pytest.raises(ValueError, match="targets holds"):
        ops.lm_head_score(hd, wd, cd, targets=torch.zeros(4, dtype=torch.int64, device=dev))
    # the C entry point: nothing to write, a missing complement map, targets missing beside logp, more rows than there are
    out = torch.zeros(5, device=dev)
    stream = L.stream_and_check(hd, wd, cd, out)
    mk = lambda **kw: L.LmScoreArgs(**{**dict(hidden=L.ptr(hd), weight=L.ptr(wd), comp=L.ptr(cd), row_index=None, targets=None, logit_mask=None,
                                              logp=None, logp_all=None, rows=5, n=5, D=64, V=16, n_strands=2, ignore_index=4, dtype=0), **kw})
    tg = torch.zeros(5, dtype=torch.int64, device=dev)
    for bad in (mk(), mk(logp=L.ptr(out)), mk(logp=L.ptr(out), targets=L.ptr(tg), comp=None), mk(logp=L.ptr(out), targets=L.ptr(tg), n=6)):
        assert lib.cad_lm_head_score(C.byref(bad), stream) == 1
    assert lib.cad_lm_head_score(C.byref(mk(logp=L.ptr(out), targets=L.ptr(tg), V=17)), stream) == 2
    if dev.type == "cpu":  # what the host holds is checked on the host
        with pytest.raises(ValueError, match="allows no id"):
            ops.lm_head_score(hd, wd, cd, want_all=True, logit_mask=torch.full((16,), NEG_INF))
        with pytest.raises(ValueError, match="row_index"):
            ops.lm_head_score(hd, wd, cd, want_all=True, row_index=torch.tensor([5]))


def test_score_struct_matches_the_compiler(tmp_path):
    """cad_lm_score_args as a C compiler lays it out equals the ctypes mirror, field for field."""
    fields = [f[0] for f in L.LmScoreArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "caduceus_hip.h"\nint main(){printf("%zu\\n", sizeof(cad_lm_score_args));' +
                   "".join(f'printf("%zu\\n", offsetof(cad_lm_score_args, {f}));' for f in fields) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got[0] == C.sizeof(L.LmScoreArgs)
    assert got[1:] == [getattr(L.LmScoreArgs, f).offset for f in fields]


@pytest.mark.parametrize("D,dtype,S", [(128, BF, 2), (256, HF, 1), (512, BF, 2), (40, F32, 2)],
                         ids=["D128-bf16-S2", "D256-f16-S1", "D512-bf16-S2", "D40-f32-S2"])
def test_score_is_the_negated_single_row_loss(backend, D, dtype, S):
    """The promise csrc/cad_head.h exists for: a sequence log-likelihood equals what the training loss saw.  One score call over 19 rows
    against 19 forward calls on the single-row slices with the row's target as the label: the loss of one counted row is
    (lse - z[t]) / 1, the exact negation of logp = z[t] - lse, so the two agree bit for bit (three matrix-core widths, and the one-wave-
    per-row path at D = 40)."""
    name, dev = backend
    R, V = 19, 16
    h, W, _, _ = lm_inputs(S, R, D, V, dtype, 800 + D)
    t = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(D + S))
    comp = COMP if S == 2 else None
    logp = run_score(dev, h, W, comp, t, want_all=False, ign=-100).cpu()
    hd, wd, cd, td = h.to(dev), W.to(dev), None if comp is None else comp.to(dev), t.to(dev)
    with torch.no_grad():
        loss = torch.stack([ops.lm_head(hd[:, r:r + 1].reshape(S, 1, 1, D), wd, cd, td[r:r + 1].reshape(1, 1), -100)[1] for r in range(R)]).cpu()
    print(f"[bits] {name} D{D} S{S}: max |logp + loss| = {float((logp.double() + loss.double()).abs().max()):.3e}")
    assert bool(torch.isfinite(logp).all()) and torch.equal(logp, -loss)
