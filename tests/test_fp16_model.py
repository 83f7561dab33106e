"""The opt-in fp16 compute path end to end: CaduceusConfig(fp16_kernels=True) / caduceus_amd.fp16_kernels() under fp16 autocast -- the
reference's own AMP precision -- against the fp32 golden vectors at a tolerance tighter than the bf16 model tests', with exact
RC-equivariance and no library GEMM on the hand-scheduled mixer's training step; without the opt-in nothing changes.  The AMP loop and
the full-size layer run on the GPU only."""
import pytest
import torch

from caduceus_amd import CaduceusConfig, CaduceusForMaskedLM, fp16_kernels
from caduceus_amd.mamba import act_dtype_of, as_requested
from conftest import MODEL_VARIANTS, load_golden_model

F16 = torch.float16
LOSS_SCALE = 2.0 ** 16  # (torch.amp.GradScaler's initial scale)


def build_model(name, dev, fp16=True):
    cfg, sd, rec = load_golden_model(name)
    head, emb = (("lm_head.lm_head.weight", "caduceus.backbone.embeddings.word_embeddings.embedding.weight")
                 if cfg["rcps"] else ("lm_head.weight", "caduceus.backbone.embeddings.word_embeddings.weight"))
    extra = {"fp16_kernels": True} if fp16 else {}
    config = CaduceusConfig(**cfg, tie_word_embeddings=bool(torch.equal(sd[head], sd[emb])), pad_token_id=4, **extra)
    model = CaduceusForMaskedLM(config)
    model.load_state_dict(sd, strict=True)
    return model.to(dev).train(), cfg, sd, rec


def test_switch_is_thread_local_and_scoped():
    x16, x32 = torch.zeros(2, dtype=F16), torch.zeros(2)
    assert act_dtype_of(x16) == torch.float32  # default: an fp16 request runs the fp32 kernels
    with fp16_kernels():
        assert act_dtype_of(x16) == F16 and act_dtype_of(x32) == torch.float32
        assert act_dtype_of(x16.bfloat16()) == torch.bfloat16
        with torch.autocast("cpu", dtype=F16):
            assert act_dtype_of(x32) == F16
        with fp16_kernels(False):
            assert act_dtype_of(x16) == torch.float32
        assert act_dtype_of(x16) == F16
        seen = []
        import threading
        th = threading.Thread(target=lambda: seen.append(act_dtype_of(x16)))
        th.start()
        th.join()
        assert seen == [torch.float32]
    assert act_dtype_of(x16) == torch.float32
    assert as_requested(x32, x16).dtype == F16


def test_config_serialises_unchanged_without_the_option():
    base = CaduceusConfig(d_model=64, n_layer=2)
    d = base.to_dict()
    assert "fp16_kernels" not in d and not hasattr(base, "fp16_kernels")
    on = CaduceusConfig(d_model=64, n_layer=2, fp16_kernels=True)
    d_on = on.to_dict()
    assert d_on.pop("fp16_kernels") is True
    assert d_on == d
    assert CaduceusConfig.from_dict(on.to_dict()).fp16_kernels is True


@pytest.mark.parametrize("name", MODEL_VARIANTS)
def test_model_fp16_kernels_vs_reference(backend, name):
    """Every golden variant under fp16 autocast with the opt-in: logits, loss and EVERY gradient against the fp32 reference vectors at
    1/3 of the bf16 model tests' tolerance (rtol 3e-2 / atol 5e-2 there); hidden states float16; not the fp32 run's bits."""
    _, dev = backend
    model, cfg, sd, rec = build_model(name, dev)
    ids, labels = rec["input_ids"].to(dev), rec["labels"].to(dev)
    with torch.autocast(dev.type, dtype=F16):
        out = model(ids, labels=labels, output_hidden_states=True)
    assert out.logits.dtype == torch.float32
    assert all(h.dtype == F16 for h in out.hidden_states)
    rel = float((out.logits.detach().cpu() - rec["logits"]).norm() / rec["logits"].norm())
    assert rel < 1e-2, rel
    assert not torch.equal(out.logits.detach().cpu(), rec["logits"])
    torch.testing.assert_close(out.loss.detach().cpu(), rec["loss"], rtol=5e-3, atol=5e-3)
    out.loss.backward()
    named = model.state_dict(keep_vars=True)
    checked = 0
    for k, g in rec.items():
        if not k.startswith("grad/"):
            continue
        got = named[k[5:]].grad
        assert got is not None and torch.isfinite(got).all(), k
        scale = max(1.0, float(g.abs().max()))
        torch.testing.assert_close(got.cpu(), g, rtol=1e-2, atol=1.5e-2 * scale, msg=lambda m, k=k: f"{k}: {m}")
        checked += 1
    assert checked > 10


@pytest.mark.parametrize("name", ["ps_fused", "ph_fused"])
def test_fp16_without_the_option_is_the_fp32_run(backend, name):
    """Off means off: an fp16 autocast step without the opt-in is bit-identical to the fp32 run (logits, loss, a gradient)."""
    _, dev = backend
    runs = []
    for amp in (False, True):
        model, cfg, sd, rec = build_model(name, dev, fp16=False)
        ids, labels = rec["input_ids"].to(dev), rec["labels"].to(dev)
        with torch.autocast(dev.type, dtype=F16, enabled=amp):
            out = model(ids, labels=labels)
        out.loss.backward()
        g = next(p.grad for k, p in model.named_parameters() if k.endswith("x_proj.weight"))
        runs.append((out.logits.detach().cpu(), out.loss.detach().cpu(), g.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["ps_fused", "ps_unfused"])
def test_fp16_kernels_rc_equivariance_exact(backend, name):
    _, dev = backend
    model, cfg, sd, rec = build_model(name, dev)
    comp = sd["lm_head.complement_map"].to(dev)
    ids = rec["input_ids"].to(dev)
    rc_ids = comp[torch.flip(ids, dims=[-1])]
    with torch.autocast(dev.type, dtype=F16), torch.no_grad():
        a, b = model(ids), model(rc_ids)
    assert torch.equal(a.logits, torch.flip(b.logits[..., comp], dims=[1]))


def test_context_manager_reaches_a_model_without_the_config_option(backend):
    _, dev = backend
    model, cfg, sd, rec = build_model("ps_fused", dev, fp16=False)
    ids = rec["input_ids"].to(dev)
    with torch.no_grad(), torch.autocast(dev.type, dtype=F16):
        plain = model(ids).logits
        with fp16_kernels():
            opted = model(ids).logits
        ref = build_model("ps_fused", dev)[0](ids).logits
    assert not torch.equal(plain, opted)
    assert torch.equal(opted, ref)


@pytest.mark.parametrize("name", ["ps_fused", "ph_fused"])
def test_fp16_training_step_runs_without_a_library_gemm(backend, name, monkeypatch):
    """The hand-scheduled mixer (tied, `add`) at fp16: forward + loss + backward with the torch matrix products made to raise, as the fp32
    and bf16 paths."""
    _, dev = backend
    model, cfg, sd, rec = build_model(name, dev)
    ids, labels = rec["input_ids"].to(dev), rec["labels"].to(dev)

    def boom(*a, **k):
        raise AssertionError("a library matrix product on the fp16 path")

    with monkeypatch.context() as mp:
        for fn in ("mm", "bmm", "addmm", "matmul", "baddbmm", "einsum"):
            mp.setattr(torch, fn, boom)
        mp.setattr(torch.Tensor, "__matmul__", boom)
        mp.setattr(torch.Tensor, "addmm_", boom)
        mp.setattr(torch.nn.functional, "linear", boom)
        with torch.autocast(dev.type, dtype=F16):
            out = model(ids, labels=labels)
        out.loss.backward()
    rel = float((out.logits.detach().cpu() - rec["logits"]).norm() / rec["logits"].norm())
    assert rel < 1e-2, rel


# ---- GPU only ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_amp_grad_scaler_loop_on_the_device():
    """torch.amp.GradScaler over the fp16 kernels: finite loss, parameters move; a huge init_scale overflows the scaled fp16 gradients
    (+-inf / NaN reach the scaler), that step is skipped -- parameters unchanged, scale reduced -- and later steps proceed."""
    from caduceus_amd import _lib
    _lib.use_library_for_testing(None)
    dev = torch.device("cuda:0")
    model, cfg, sd, rec = build_model("ps_fused", dev)
    ids, labels = rec["input_ids"].to(dev), rec["labels"].to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 60, backoff_factor=2.0 ** -20)
    params0 = [p.detach().clone() for p in model.parameters()]

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=F16):
            loss = model(ids, labels=labels).loss
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        return float(loss)

    loss0 = step()
    assert torch.isfinite(torch.tensor(loss0))
    assert scaler.get_scale() == 2.0 ** 40  # overflow seen -> scale backed off
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), params0))  # ... and the step skipped
    for _ in range(4):  # (2^40, 2^20 may overflow as well; 1.0 does not)
        if scaler.get_scale() <= 1.0:
            break
        step()
    moved = [p.detach().clone() for p in model.parameters()]
    losses = [step() for _ in range(3)]
    assert all(torch.isfinite(torch.tensor(losses)))
    assert scaler.get_scale() >= 1.0
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), moved))  # later steps proceed


@pytest.mark.gpu
def test_config2_one_layer_L131072_fp16_vs_oracle_and_memory():
    """One layer of the headline model (PS d_model 256, seqlen 131072) with the fp16 kernels against the fp32 C oracle -- logits, loss and
    every parameter gradient by relative error norm, as the bf16 one-layer test -- and the peak memory of the step: about the bf16 step's,
    well below the fp32 step's.  The fp16 backward runs on a scaled loss, as under torch.amp.GradScaler: a mean over 131072 tokens has
    per-token gradients below binary16's normal range (d(delta) ~ 1e-8), which an unscaled fp16 backward flushes to zero."""
    import bench
    from caduceus_amd import _lib
    from test_configs import _oracle_cfg, _oracle_step
    _lib.use_library_for_testing(None)
    dev = "cuda:0"
    ids, labels = bench.synthetic_batch(torch.Generator().manual_seed(9), 1, 131072, dev)
    peaks = {}
    for mode in ("fp32", "bf16", "fp16"):
        torch.manual_seed(77)
        model = CaduceusForMaskedLM(bench.make_config(256, 1)).to(dev).train()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        dt = {"fp32": None, "bf16": torch.bfloat16, "fp16": F16}[mode]
        with fp16_kernels(mode == "fp16"), torch.autocast("cuda", dtype=dt or torch.float32, enabled=dt is not None):
            out = model(ids, labels=labels)
        (out.loss * (LOSS_SCALE if mode == "fp16" else 1.0)).backward()
        torch.cuda.synchronize()
        peaks[mode] = torch.cuda.max_memory_allocated() - base
        if mode != "fp16":
            del model, out
    print("one-layer step peak memory (GB):", {k: round(v / 2 ** 30, 3) for k, v in peaks.items()})
    assert peaks["fp16"] < 1.25 * peaks["bf16"], peaks
    assert peaks["fp16"] < 0.8 * peaks["fp32"], peaks
    ref, sd = _oracle_step(model, _oracle_cfg(1, True), ids, labels)
    rel = float((out.logits.detach().float().cpu() - ref["logits"]).norm() / ref["logits"].norm())
    assert rel < 5e-3, rel
    assert abs(float(out.loss) - float(ref["loss"])) < 5e-3 * max(1.0, float(ref["loss"]))
    errs = {}
    for k, p in model.named_parameters():
        want = sd[k].grad
        assert want is not None and p.grad is not None and torch.isfinite(p.grad).all(), k
        if float(want.norm()) > 1e-9:
            errs[k] = float((p.grad.float().cpu() / LOSS_SCALE - want).norm() / want.norm())
    print("config2 one-layer fp16 gradient relative-norm errors:", {k: round(v, 5) for k, v in errs.items()})
    assert len(errs) >= 15
    for k, e in errs.items():
        assert e < 0.01, (k, e)  # (bf16: 0.025)
