"""The generic per-op engine (caduceus_amd/engine.py) in bf16 on the own strided MFMA GEMM (cad_gemm_b16) behind engine._OWN_GEMM_B16:
no library matrix product is left on the un-tied, ew_multiply and uni-directional configurations; the error against the fp32 golden
vectors is that of the library branch (the yardstick) within the project's 1.5 factor; the schedule of an un-tied layer names the kernel
for every projection and every gradient product.  Every test sets the handle itself."""
import pytest
import torch

from caduceus_amd import _lib, engine
from caduceus_amd.mamba import Mamba
from conftest import load_golden_model  # noqa: F401
from test_mixer_schedule import _Recorder
from test_model_parity import build_model

ENGINE_VARIANTS = ["ps_fused_ewmul", "ps_fused_untied", "ps_fused_unidir"]
_LIBRARY_PRODUCTS = ("mm", "bmm", "addmm", "matmul", "baddbmm", "einsum")


def _no_library_products(mp):
    def boom(*a, **k):
        raise AssertionError("a library matrix product on the bf16 engine path")
    for fn in _LIBRARY_PRODUCTS:
        mp.setattr(torch, fn, boom)
    mp.setattr(torch.Tensor, "__matmul__", boom)
    mp.setattr(torch.Tensor, "addmm_", boom)
    mp.setattr(torch.nn.functional, "linear", boom)


def _bf16_step(name, dev):
    """Forward + loss + backward in bf16 autocast: (logits, loss, {parameter: gradient}) on the CPU, and the golden record."""
    model, cfg, sd, rec = build_model(name, dev)
    ids, labels = rec["input_ids"].to(dev), rec["labels"].to(dev)
    with torch.autocast(dev.type, dtype=torch.bfloat16):
        out = model(ids, labels=labels)
    out.loss.backward()
    grads = {k: p.grad.detach().float().cpu() for k, p in model.state_dict(keep_vars=True).items() if getattr(p, "grad", None) is not None}
    return out.logits.detach().float().cpu(), out.loss.detach().float().cpu(), grads, rec


@pytest.mark.parametrize("name", ENGINE_VARIANTS)
def test_bf16_engine_step_runs_without_a_library_gemm(backend, name, monkeypatch):
    """With the handle on, forward + loss + backward of the three golden variants the engine serves run with every torch matrix product
    made to raise (the pattern of test_fp32_training_step_runs_without_a_library_gemm); the result stays at the bf16 tolerance of
    test_model_bf16_autocast.  Without the routing, ops.mm's bf16 branch is torch.mm: this test fails."""
    _, dev = backend
    monkeypatch.setattr(engine, "_OWN_GEMM_B16", True)
    with monkeypatch.context() as mp:
        _no_library_products(mp)
        logits, loss, grads, rec = _bf16_step(name, dev)
    rel = float((logits - rec["logits"]).norm() / rec["logits"].norm())
    assert rel < 3e-2, rel
    assert abs(float(loss) - float(rec["loss"])) < 0.05 * max(1.0, float(rec["loss"]))
    assert len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads.values())


def _rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


@pytest.mark.parametrize("name", ENGINE_VARIANTS)
def test_bf16_engine_error_is_the_library_branch_s(backend, name, monkeypatch):
    """Logits, loss and every gradient against the fp32 golden vectors: the relative error norm with the handle on is at most 1.5 times
    the same norm with the handle off (the factor of test_fused_softplus_rounding_point_against_oracle).  The library branch is the
    yardstick, not the kernel under test."""
    _, dev = backend
    monkeypatch.setattr(engine, "_OWN_GEMM_B16", False)
    lg0, ls0, g0, rec = _bf16_step(name, dev)
    monkeypatch.setattr(engine, "_OWN_GEMM_B16", True)
    lg1, ls1, g1, _ = _bf16_step(name, dev)
    rows = [("logits", _rel(lg1, rec["logits"]), _rel(lg0, rec["logits"])), ("loss", _rel(ls1, rec["loss"]), _rel(ls0, rec["loss"]))]
    keys = [k for k in rec if k.startswith("grad/")]
    assert len(keys) > 10 and all(k[5:] in g0 and k[5:] in g1 for k in keys)
    rows += [(k, _rel(g1[k[5:]], rec[k]), _rel(g0[k[5:]], rec[k])) for k in keys]
    for what, on, off in rows:
        print(f"[engine b16] {name} {what}: own {on:.3e}  library {off:.3e}  ratio {on / max(off, 1e-300):.3f}")
    worse = [(what, on, off) for what, on, off in rows if not on <= 1.5 * off]
    assert not worse, worse


def test_untied_engine_layer_schedule_in_bf16(backend, monkeypatch):
    """One un-tied BiMamba layer ("add") through the engine in bf16, forward + backward, recorded by the _Recorder pattern of
    tests/test_mixer_schedule.py: cad_gemm_b16 for every projection (in_proj, x_proj, dt_proj, out_proj of both parameter sets: 8) and
    for both gradient products of each (16), no other GEMM entry point, no library product."""
    name, dev = backend
    monkeypatch.setattr(engine, "_OWN_GEMM_B16", True)
    torch.manual_seed(0)
    d_model, L = 64, 200
    mf, mr = Mamba(d_model, device=dev), Mamba(d_model, device=dev)
    hn = (torch.randn(2, 1, L, d_model, device=dev) * 0.5).to(torch.bfloat16).requires_grad_(True)
    g = torch.randn(2, 1, L, d_model, device=dev).to(torch.bfloat16)
    real, calls = _lib.get_lib(), []
    _lib._lib = _Recorder(real, calls)
    try:
        with monkeypatch.context() as mp:
            _no_library_products(mp)
            with torch.autocast(dev.type, dtype=torch.bfloat16):
                out = engine.bimamba_tframe(hn, mf, mr, "add", True)
            out.backward(g)
    finally:
        _lib._lib = real
    assert out.dtype == torch.bfloat16 and hn.grad is not None
    assert all(p.grad is not None for p in list(mf.parameters()) + list(mr.parameters()))
    gemms = [c for c in calls if "gemm" in c or "proj" in c]
    assert gemms == ["cad_gemm_b16"] * 24, gemms
    fwd = calls[:calls.index("cad_scan_fwd_multi")]
    assert fwd.count("cad_gemm_b16") == 6  # in_proj, x_proj, dt_proj of both sets ahead of the first scan; out_proj behind the scans
