"""The attribution head (csrc/attrib.hip, cad_embed_attrib) held to float64, element by element, from the same stored gradient.

Bounds: the `logits` line of the header of tests/test_norm_head_fp64.py, restated for g (the row is the same code, csrc/cad_head.h, with
dh as the hidden state and the embedding table E as the weight); the constants U, UF and gam() are imported from there, nothing is fitted
to a result.  A = the number of allowed ids, sums over A run over the allowed ids.
  g[v]            e_g[v] = g(S D + 2) sum |dh E| + S D UF                    (S D products, any order: lanes, butterfly, matrix cores)
  m = sum_A g / A A - 1 additions and one division on perturbed terms:
                  e_m = (1 + g(A)) mean_A e_g + g(A) mean_A |g| + UF         (centre off: m = 0 exactly, e_m = 0)
  c[v] = g[v] - m tol = e_g[v] + e_m + u (|c[v]| + e_g[v] + e_m)             (the subtraction rounds once; centre off: g - 0 is exact and
                                                                              tol = e_g[v])
  grad[i][k]      c[allowed[k]]
  gxi[i]          c[ids[i]] where ids[i] is allowed; exactly 0.0 elsewhere (tol 0: ids that are not allowed, equal to V, or -1)
  A = 1 centred   g - g / 1 = 0.0 exactly, everywhere
Exchanging the two strands of dh exchanges the two per-strand sums of every g[v] <-> g[comp v]; they meet in one commutative add, so the
results are the same bits.
"""
import ctypes as C
import os
import subprocess

import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops
from conftest import ROOT
from test_norm_head_fp64 import BF, COMP, COMP12, F32, HF, SENT, TAG, U, UF, Arena, gam, hold, lm_inputs

COMP5 = torch.tensor([0, 2, 1, 4, 3])  # 1 <-> 2, 3 <-> 4
COMPS = {16: COMP, 12: COMP12, 5: COMP5}
# per vocabulary: every id, four ids closed under the complement map, one id
ALLOWED = {16: (list(range(16)), [7, 8, 9, 10], [9]), 12: (list(range(12)), [3, 7, 8, 11], [7]), 5: (list(range(5)), [1, 2, 3, 4], [3])}
MFMA = [(128, F32), (128, BF), (128, HF), (256, F32), (256, BF), (256, HF), (512, BF)]
GENERAL = [(40, F32), (40, BF), (40, HF), (64, F32), (64, BF), (64, HF)]


def attrib_reference(dh, E, comp, ids, allowed, centre):
    """fp64 values and tolerances {name: (ref, tol)}.  dh (S, R, D) as stored, E (V, D) fp32."""
    S, R, D = dh.shape
    V, A = E.shape[0], len(allowed)
    H, W = dh.double(), E.double()
    g, ag = H[0] @ W.t(), H[0].abs() @ W.abs().t()
    if S == 2:
        g, ag = g + H[1] @ W[comp].t(), ag + H[1].abs() @ W[comp].abs().t()
    e_g = gam(S * D + 2) * ag + S * D * UF
    al = torch.tensor(allowed)
    ga, ea = g[:, al], e_g[:, al]
    if centre:
        m = ga.sum(1, keepdim=True) / A
        e_m = (1 + gam(A)) * ea.mean(1, keepdim=True) + gam(A) * ga.abs().mean(1, keepdim=True) + UF
        c = ga - m
        tol = ea + e_m
        tol = tol + U * (c.abs() + tol)
        if A == 1:
            c, tol = torch.zeros_like(c), torch.zeros_like(tol)
    else:
        c, tol = ga, ea
    col = torch.full((V + 2,), -1, dtype=torch.int64)  # id -> column of grad; V and -1 (index V + 1 from the end) stay -1
    col[al] = torch.arange(A)
    k = col[ids.clamp(-1, V)]
    own = k >= 0
    kc = k.clamp_min(0)[:, None]
    zero = torch.zeros(R, dtype=torch.float64)
    return {"grad": (c, tol), "gxi": (torch.where(own, c.gather(1, kc)[:, 0], zero), torch.where(own, tol.gather(1, kc)[:, 0], zero)),
            "own": own}


def _ids(R, V, g, allowed):
    """Random ids, with -1, V and (if there is one) an id that is not allowed among them."""
    t = torch.randint(0, V, (R,), generator=g)
    specials = [-1, V] + [v for v in range(V) if v not in allowed][:1]
    for k, s in enumerate(specials):
        if k < R:
            t[(3 * k + 1) % R] = s
    return t


def run_attrib(dev, dh, E, comp, ids, allowed, centre, want_grad=True, want_gxi=True):
    S = dh.shape[0]
    res = ops.embed_attrib(dh.to(dev), E.to(dev), comp.to(dev) if S == 2 else None, ids.to(dev), torch.tensor(allowed, device=dev), centre,
                           want_grad, want_gxi)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return res


def check(backend, tag, dh, E, comp, ids, allowed, centre):
    name, dev = backend
    ref = attrib_reference(dh, E, comp, ids, allowed, centre)
    grad, gxi = run_attrib(dev, dh, E, comp, ids, allowed, centre)
    assert grad.shape == (dh.shape[1], len(allowed)) and gxi.shape == (dh.shape[1],)
    hold(name, f"{tag}.grad", grad, *ref["grad"], F32)
    hold(name, f"{tag}.gxi", gxi, *ref["gxi"], F32)
    assert bool((gxi.cpu()[~ref["own"]] == 0.0).all()), "gxi at an id that is not allowed"
    return grad, gxi


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("D,dtype", MFMA + GENERAL, ids=[f"D{d}-{TAG[t]}" for d, t in MFMA + GENERAL])
def test_attrib_rows_widths_vocabularies(backend, D, dtype, S):
    """rows in {1, 15, 16, 17, 33} (below, at and above one 16-row tile; 33: three tiles, the last with one row) at every width class and
    dtype of both paths, V in {16, 12, 5}, allowed = every id / four ids closed under comp / one id, centred and not."""
    assert L.get_lib().cad_embed_attrib_supported(D, 16, L.dtype_code(dtype)) == 1
    for k, n in enumerate([1, 15, 16, 17, 33]):
        for V in ((16, 12, 5) if n in (17, 33) else ((16, 12, 5)[k % 3],)):
            comp = COMPS[V]
            g = torch.Generator().manual_seed(1000 * D + 10 * n + V + S)
            dh, E, _, _ = lm_inputs(S, n, D, V, dtype, 17 * D + n + V, comp=comp)
            for j, allowed in enumerate(ALLOWED[V]):
                for centre in ((True, False) if n == 33 else ((k + j + V) % 2 == 0,)):
                    grad, gxi = check(backend, f"attrib-D{D}-n{n}-V{V}-S{S}-A{len(allowed)}-c{int(centre)}", dh, E, comp,
                                      _ids(n, V, g, allowed), allowed, centre)
                    if centre and len(allowed) == 1:
                        assert bool((grad == 0.0).all()) and bool((gxi == 0.0).all()), "A = 1 centred is exactly 0.0"


def _cu_count(n):
    L.check(L.get_lib().cad_debug_set_cu_count(int(n)), "cad_debug_set_cu_count")


@pytest.mark.parametrize("D,dtype,S", [(128, BF, 2), (256, F32, 1), (512, BF, 2)], ids=["D128-bf16-S2", "D256-f32-S1", "D512-bf16-S2"])
def test_attrib_three_tile_walk(backend, D, dtype, S):
    """The matrix-core launcher sizes its grid by the CU count (two workgroups of four waves per CU at most).  With one CU, 8 waves walk
    18 tiles at 275 rows: waves 0 and 1 take three tiles each (the next tile's rows prefetched, the E registers kept), wave 1's last one
    ragged with 3 rows."""
    n = 2 * 8 * 16 + 16 + 3
    dh, E, _, _ = lm_inputs(S, n, D, 16, dtype, 3 * D + S)
    ids = _ids(n, 16, torch.Generator().manual_seed(D + S), [7, 8, 9, 10])
    try:
        _cu_count(1)
        a = check(backend, f"attrib-walk-D{D}", dh, E, COMP, ids, [7, 8, 9, 10], True)
    finally:
        _cu_count(0)
    b = check(backend, f"attrib-wide-D{D}", dh, E, COMP, ids, [7, 8, 9, 10], True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "a row's result depends on its place in the walk"


def test_attrib_general_path_walk(backend):
    """One wave per row, 4096 workgroups of 4 at most: at 16384 + 13 rows thirteen waves take a second row."""
    n = 16384 + 13
    dh, E, _, _ = lm_inputs(2, n, 40, 12, BF, 91, comp=COMP12)
    check(backend, "attrib-general-walk", dh, E, COMP12, _ids(n, 12, torch.Generator().manual_seed(5), [3, 7, 8, 11]), [3, 7, 8, 11], True)


@pytest.mark.parametrize("D,dtype", [(128, BF), (256, F32), (40, HF)], ids=["D128-bf16", "D256-f32", "D40-f16"])
def test_attrib_each_output_alone_and_guard_words(backend, D, dtype):
    """Through the C entry point, every operand a view into a sentinel-filled buffer: both outputs, grad alone, gxi alone.  A NULL
    output's buffer keeps its sentinel, the written ones equal the two-output call bit for bit, and no guard word around the outputs
    or the inputs changes: the launch writes its (rows, A) and (rows) outputs and nothing else."""
    name, dev = backend
    S, R, V, allowed = 2, 37, 16, [7, 8, 9, 10]
    dh, E, _, _ = lm_inputs(S, R, D, V, dtype, 400 + D)
    ids = _ids(R, V, torch.Generator().manual_seed(D), allowed)
    ar = Arena(dev, 0)
    dhd, Ed, cd, idd, ald = ar.put(dh), ar.put(E), ar.put(COMP), ar.put(ids), ar.put(torch.tensor(allowed))
    ref = attrib_reference(dh, E, COMP, ids, allowed, True)
    results = {}
    for g_on, x_on in ((True, True), (True, False), (False, True)):
        grad, gxi = ar.put(shape=(R, len(allowed)), dtype=F32), ar.put(shape=(R,), dtype=F32)
        grad.fill_(SENT)
        gxi.fill_(SENT)
        stream = L.stream_and_check(dhd, Ed, cd, idd, ald, grad, gxi)
        a = L.EmbedAttribArgs(L.ptr(dhd), L.ptr(Ed), L.ptr(cd), L.ptr(idd), L.ptr(ald), L.ptr(grad) if g_on else None,
                              L.ptr(gxi) if x_on else None, R, D, V, S, len(allowed), 1, L.dtype_code(dtype))
        L.check(L.get_lib().cad_embed_attrib(C.byref(a), stream), "cad_embed_attrib")
        if dev.type == "cuda":
            torch.cuda.synchronize()
        results[g_on, x_on] = (grad.clone(), gxi.clone())
    ar.intact()
    both = results[True, True]
    hold(name, "attrib-guard.grad", both[0], *ref["grad"], F32)
    hold(name, "attrib-guard.gxi", both[1], *ref["gxi"], F32)
    assert torch.equal(results[True, False][0], both[0]) and bool((results[True, False][1] == SENT).all())
    assert torch.equal(results[False, True][1], both[1]) and bool((results[False, True][0] == SENT).all())


@pytest.mark.parametrize("D,dtype,V", [(128, BF, 16), (256, F32, 12), (512, BF, 5), (40, F32, 16), (64, HF, 12)],
                         ids=["D128-bf16-V16", "D256-f32-V12", "D512-bf16-V5", "D40-f32-V16", "D64-f16-V12"])
def test_attrib_strand_exchange_is_bit_exact(backend, D, dtype, V):
    """g of the exchanged strands at column comp v is g at column v, bit for bit (both paths)."""
    name, dev = backend
    comp = COMPS[V]
    dh, E, _, _ = lm_inputs(2, 33, D, V, dtype, 900 + D, comp=comp)
    ids = torch.zeros(33, dtype=torch.int64)
    g = run_attrib(dev, dh, E, comp, ids, list(range(V)), False, want_gxi=False).cpu()
    gx = run_attrib(dev, dh.flip(0).contiguous(), E, comp, ids, list(range(V)), False, want_gxi=False).cpu()
    print(f"[bits] {name} D{D} V{V}: max |g(exchanged)[comp v] - g[v]| = {float((gx[:, comp] - g).abs().max()):.3e}")
    assert bool(torch.isfinite(g).all()) and torch.equal(gx[:, comp], g)


@pytest.mark.parametrize("dtype", [F32, BF, HF], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("D", [128, 256])
def test_attrib_misaligned_gradient_takes_the_scalar_row(backend, D, dtype):
    """dh one element into its buffer: no 16-byte loads are possible, the launcher takes the one-wave-per-row kernel.  Same bounds,
    sentinels around the view intact."""
    name, dev = backend
    S, R, V, allowed = 2, 37, 16, [7, 8, 9, 10]
    dh, E, _, _ = lm_inputs(S, R, D, V, dtype, 700 + D)
    ids = _ids(R, V, torch.Generator().manual_seed(D), allowed)
    ar = Arena(dev, 1)
    hv = ar.put(dh)
    assert hv.data_ptr() % 16 != 0 and hv.is_contiguous()
    ref = attrib_reference(dh, E, COMP, ids, allowed, True)
    grad, gxi = ops.embed_attrib(hv, E.to(dev), COMP.to(dev), ids.to(dev), torch.tensor(allowed, device=dev))
    hold(name, "attrib-misaligned.grad", grad, *ref["grad"], F32)
    hold(name, "attrib-misaligned.gxi", gxi, *ref["gxi"], F32)
    ar.intact()


def test_attrib_refusals(backend):
    name, dev = backend
    dh, E, _, _ = lm_inputs(2, 5, 64, 16, F32, 1)
    hd, wd, cd = dh.to(dev), E.to(dev), COMP.to(dev)
    ids, al = torch.zeros(5, dtype=torch.int64, device=dev), torch.tensor([7, 8, 9, 10], device=dev)
    lib = L.get_lib()
    assert lib.cad_embed_attrib_supported(64, 17, 0) == 0 and lib.cad_embed_attrib_supported(64, 16, 3) == 0
    assert lib.cad_embed_attrib_supported(1000, 1, 2) == 1
    assert issubclass(ops.AttribUnsupported, ValueError) and not ops.embed_attrib_supported(64, 16, torch.float64)
    with pytest.raises(ops.AttribUnsupported, match="vocab_size 72"):
        ops.embed_attrib(hd, torch.zeros(72, 64, device=dev), None, ids, al)
    with pytest.raises(ValueError, match="grad, gxi"):
        ops.embed_attrib(hd, wd, cd, ids, al, want_grad=False, want_gxi=False)
    with pytest.raises(ValueError, match="complement map"):
        ops.embed_attrib(hd, wd, None, ids, al)
    with pytest.raises(TypeError, match="ids holds 5"):
        ops.embed_attrib(hd, wd, cd, ids[:4], al)
    with pytest.raises(TypeError, match="allowed holds"):
        ops.embed_attrib(hd, wd, cd, ids, torch.zeros(17, dtype=torch.int64, device=dev))
    # a gradient that requires grad is detached, not refused: the head has no backward and builds no graph
    out = ops.embed_attrib(hd.clone().requires_grad_(True), wd, cd, ids, al, want_gxi=False)
    assert not out.requires_grad and out.shape == (5, 4)
    # the C entry point: nothing to write, a missing complement map, ids missing beside gxi, A outside [1, V]
    o = torch.zeros(5 * 16, device=dev)
    stream = L.stream_and_check(hd, wd, cd, ids, al, o)
    mk = lambda **kw: L.EmbedAttribArgs(**{**dict(dh=L.ptr(hd), weight=L.ptr(wd), comp=L.ptr(cd), ids=L.ptr(ids), allowed=L.ptr(al), grad=None,
                                                  gxi=None, rows=5, D=64, V=16, n_strands=2, A=4, centre=1, dtype=0), **kw})
    for bad in (mk(), mk(grad=L.ptr(o), comp=None), mk(gxi=L.ptr(o), ids=None), mk(grad=L.ptr(o), A=0), mk(grad=L.ptr(o), A=17),
                mk(grad=L.ptr(o), allowed=None), mk(grad=L.ptr(o), rows=0)):
        assert lib.cad_embed_attrib(C.byref(bad), stream) == 1
    assert lib.cad_embed_attrib(C.byref(mk(grad=L.ptr(o), V=17)), stream) == 2
    assert lib.cad_embed_attrib(C.byref(mk(grad=L.ptr(o), dtype=3)), stream) == 2
    if dev.type == "cpu":  # what the host holds is checked on the host
        for bad in ([8, 7], [7, 7], [7, 16], [-1, 7]):
            with pytest.raises(ValueError, match="ascending"):
                ops.embed_attrib(hd, wd, cd, ids, torch.tensor(bad))


def test_attrib_struct_matches_the_compiler(tmp_path):
    """cad_embed_attrib_args as a C compiler lays it out equals the ctypes mirror, field for field."""
    fields = [f[0] for f in L.EmbedAttribArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "caduceus_hip.h"\nint main(){printf("%zu\\n", sizeof(cad_embed_attrib_args));' +
                   "".join(f'printf("%zu\\n", offsetof(cad_embed_attrib_args, {f}));' for f in fields) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got[0] == C.sizeof(L.EmbedAttribArgs)
    assert got[1:] == [getattr(L.EmbedAttribArgs, f).offset for f in fields]
