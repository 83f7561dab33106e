"""The per-workgroup weight-gradient slots of conv1d / add + norm and their fold (ops.wgrad_slots, cad_reduce_partials):
  * the deep-and-narrow fp32 fold (slot groups in parallel, csrc/scan_fold.hip) sums in the library's ONE order (include/caduceus_hip.h:
    groups of CAD_FOLD_GROUP consecutive slots from 0, the group sums left to right from 0) -- bit for bit, at the depths either side of
    its threshold (64 slots), ragged last groups, more than one pass over the groups (> 512 slots) and its deepest admitted shape;
  * every slot the fold reads is WRITTEN by its producing workgroup: with the slots pre-filled with NaN instead of allocated empty, the
    gradients are finite and equal, bit for bit, those of zero-filled slots -- for the two kernels alone (vector and scalar variants, a
    last workgroup with fewer rows than the others) and for one whole BiMamba mixer layer."""

import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import mixer, ops
from caduceus_amd.mamba import Mamba

FOLD_GROUP = 8


def _fold_in_library_order(src):
    """(nparts, n) fp32 -> (n): IEEE fp32 additions in the library's order (CPU tensors: every `+` is one rounding)."""
    nparts, n = src.shape
    s = torch.zeros(n, dtype=torch.float32)
    for k0 in range(0, nparts, FOLD_GROUP):
        g = torch.zeros(n, dtype=torch.float32)
        for k in range(k0, min(nparts, k0 + FOLD_GROUP)):
            g = g + src[k]
        s = s + g
    return s


# (slots, n): 63 / 64 the threshold of the deep kernel, 65 / 1000 a ragged last group, 1024 x 256 the add + norm weight gradient of the
# flagship step (two passes over the groups), 4096 the deepest the kernel admits, 4104 past it (back on the plain kernel), n = 4 one
# column, 260 a last workgroup with one column of four, 258 not a multiple of four (plain kernel, scalar path)
@pytest.mark.parametrize("nparts,n", [(63, 256), (64, 256), (65, 260), (1000, 4), (1024, 256), (4096, 64), (4104, 64), (100, 258)])
def test_reduce_partials_f32_deep_matches_library_order(backend, nparts, n):
    name, dev = backend
    torch.manual_seed(nparts * 1000 + n)
    # values of mixed sign and magnitude: a different order of additions changes the last bits of almost every column
    src = (torch.randn(nparts, n) * torch.exp(3.0 * torch.randn(nparts, n))).float()
    want = _fold_in_library_order(src)
    s = src.to(dev).contiguous()
    dst = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    stream = L.stream_and_check(s, dst)
    L.check(L.get_lib().cad_reduce_partials(L.ptr(s), nparts, n, L.ptr(dst), L.CAD_F32, stream), "cad_reduce_partials")
    assert torch.equal(dst.cpu(), want)


def _nan_slots(monkeypatch):
    real = ops.wgrad_slots

    def slots(n_slots, n, device, zero=True):
        t = real(n_slots, n, device, zero=True)
        return t if zero else t.fill_(float("nan"))
    monkeypatch.setattr(ops, "wgrad_slots", slots)


def _zero_slots(monkeypatch):
    real = ops.wgrad_slots
    monkeypatch.setattr(ops, "wgrad_slots", lambda n_slots, n, device, zero=True: real(n_slots, n, device, zero=True))


def _both_ways(monkeypatch, run):
    with monkeypatch.context() as m:
        _zero_slots(m)
        want = run()
    with monkeypatch.context() as m:
        _nan_slots(m)
        got = run()
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.isfinite(a.float()).all(), f"gradient {i} read a slot nobody wrote"
        assert torch.equal(a, b), f"gradient {i} differs from the zero-filled run"


# D = 256 vector kernel, D = 36 vector kernel with idle lanes, D = 37 scalar kernel; 300 rows per strand: the last workgroup's waves run
# out of rows (rows_per_wave 8 -> 32 rows per workgroup, 19 workgroups)
@pytest.mark.parametrize("D,bias,rms", [(256, False, True), (36, True, False), (37, True, False)])
def test_add_norm_bwd_writes_every_slot(backend, monkeypatch, D, bias, rms):
    name, dev = backend
    torch.manual_seed(D)
    x0, r0 = torch.randn(2, 1, 300, D, device=dev), torch.randn(2, 1, 300, D, device=dev)
    w0 = torch.randn(D, device=dev)
    b0 = torch.randn(D, device=dev) if bias else None
    gy, gr = torch.randn(2, 1, 300, D, device=dev), torch.randn(2, 1, 300, D, device=dev)

    def run():
        x, r, w = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        b = None if b0 is None else b0.clone().requires_grad_(True)
        y, res = ops.add_norm(x, r, w, b, 1e-5, rms, True, torch.float32)
        (y * gy).sum().add((res * gr).sum()).backward()
        return [w.grad] + ([b.grad] if bias else [])
    _both_ways(monkeypatch, run)


# L = 1000 vector kernel, L = 1001 scalar kernel; 2 rows x 3 wave tiles: ONE workgroup per channel walks 6 of its 32 tiles.  L = 20000:
# 82 tiles, three workgroups per channel, the last one with 18 tiles
@pytest.mark.parametrize("Lq,bias", [(1000, True), (1001, False), (20000, True)])
def test_conv1d_bwd_writes_every_slot(backend, monkeypatch, Lq, bias):
    name, dev = backend
    E, SB, K = 8, 2, 4
    torch.manual_seed(Lq)
    x0 = torch.randn(E, SB, Lq, device=dev)
    w0, b0 = torch.randn(E, 1, K, device=dev), (torch.randn(E, device=dev) if bias else None)
    g = torch.randn(E, SB, Lq, device=dev)

    def run():
        x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        b = None if b0 is None else b0.clone().requires_grad_(True)
        (ops.causal_conv1d(x, w, b, 1, 0, 1) * g).sum().backward()
        return [w.grad] + ([b.grad] if bias else [])
    _both_ways(monkeypatch, run)


def test_mixer_layer_with_nan_slots(backend, monkeypatch):
    """One production layer (d_model 256, two strands, bf16; L = 2048 on the device, 256 in the emulator), forward + backward: the conv
    dw / dbias slots and the partial slots of dW_x / dW_dt pre-filled with NaN."""
    name, dev = backend
    Lq, d_model = (2048 if name == "hip" else 256), 256
    torch.manual_seed(0)
    mf, mr = Mamba(d_model, device=dev), Mamba(d_model, device=dev)
    mr.in_proj.weight = mf.in_proj.weight
    mr.out_proj.weight = mf.out_proj.weight
    hn0 = (torch.randn(2, 1, Lq, d_model, device=dev) * 0.5).to(torch.bfloat16)
    g = torch.randn(2, 1, Lq, d_model, device=dev).to(torch.bfloat16)
    params = list(dict.fromkeys(list(mf.parameters()) + list(mr.parameters())))
    real_partials = ops.wgrad_partials
    fill = [0.0]
    monkeypatch.setattr(ops, "wgrad_partials", lambda *a, **k: real_partials(*a, **k).fill_(fill[0]))

    def run():
        for p in params:
            p.grad = None
        hn = hn0.clone().requires_grad_(True)
        mixer.prepare_step_cache([(mf, mr)], torch.bfloat16)
        mixer.bimamba_mixer(hn, mf, mr, 1).backward(g)
        return [hn.grad.clone()] + [p.grad.clone() for p in params]

    with monkeypatch.context() as m:
        _zero_slots(m)
        want = run()
    fill[0] = float("nan")
    with monkeypatch.context() as m:
        _nan_slots(m)
        got = run()
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.isfinite(a.float()).all(), f"gradient {i} read a slot nobody wrote"
        assert torch.equal(a, b), f"gradient {i} differs from the zero-filled run"
