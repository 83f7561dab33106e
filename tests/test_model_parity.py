"""End-to-end parity of the HIP engine (flip-free t-frame) against the golden vectors generated from the reference's
own classes, and against the CPU oracle, for every supported model variant.  Runs on the emulator (CPU) and on the GPU."""
import pytest
import torch
import torch.nn.functional as F

from caduceus_amd import CaduceusConfig, CaduceusForMaskedLM
from conftest import MODEL_VARIANTS, load_golden_model
from oracle import oracle_model as om

FP32 = dict(rtol=6e-4, atol=2e-3)
BF16 = dict(rtol=3e-2, atol=5e-2)


def build_model(name, dev, dtype=torch.float32):
    cfg, sd, rec = load_golden_model(name)
    head, emb = (("lm_head.lm_head.weight", "caduceus.backbone.embeddings.word_embeddings.embedding.weight")
                 if cfg["rcps"] else ("lm_head.weight", "caduceus.backbone.embeddings.word_embeddings.weight"))
    config = CaduceusConfig(**cfg, tie_word_embeddings=bool(torch.equal(sd[head], sd[emb])), pad_token_id=4)
    model = CaduceusForMaskedLM(config)
    model.load_state_dict(sd, strict=True)
    return model.to(dev).train(), cfg, sd, rec


@pytest.mark.parametrize("name", MODEL_VARIANTS)
def test_model_matches_reference_fp32(backend, name):
    _, dev = backend
    model, cfg, sd, rec = build_model(name, dev)
    ids, labels = rec["input_ids"].to(dev), rec["labels"].to(dev)
    out = model(ids, labels=labels)  # fused LM-head + CE kernel (ignore_index = pad_token_id = 4)
    torch.testing.assert_close(out.logits.cpu(), rec["logits"], **FP32)
    torch.testing.assert_close(out.loss.cpu(), rec["loss"], **FP32)
    hidden = model.caduceus(ids).last_hidden_state
    torch.testing.assert_close(hidden.cpu(), rec["hidden"], **FP32)
    out.loss.backward()
    named = model.state_dict(keep_vars=True)
    checked = 0
    for k, g in rec.items():
        if not k.startswith("grad/"):
            continue
        got = named[k[5:]].grad
        assert got is not None, k
        scale = max(1.0, float(g.abs().max()))
        torch.testing.assert_close(got.cpu(), g, rtol=6e-4, atol=2e-3 * scale, msg=lambda m, k=k: f"{k}: {m}")
        checked += 1
    assert checked > 10


@pytest.mark.parametrize("name", MODEL_VARIANTS)
def test_fp32_training_step_runs_without_a_library_gemm(backend, name, monkeypatch):
    """The fp32 path (north_star's "stated fp32 tolerance"; BASELINE configs[0]'s precision) multiplies on the own fp32 matrix-core kernel
    (cad_gemm_f32, csrc/gemm_f32.hip) since round 6: forward + loss + backward of every golden variant -- tied / un-tied, add / ew_multiply,
    uni-directional, LayerNorm, odd sizes: the hand-scheduled mixer AND the generic per-op engine -- with the torch matrix products made
    to raise, held to the reference's logits, loss and gradients at the reference tolerance."""
    _, dev = backend
    model, cfg, sd, rec = build_model(name, dev)
    ids, labels = rec["input_ids"].to(dev), rec["labels"].to(dev)

    def boom(*a, **k):
        raise AssertionError("a library matrix product on the fp32 path")

    with monkeypatch.context() as mp:
        for fn in ("mm", "bmm", "addmm", "matmul", "baddbmm", "einsum"):
            mp.setattr(torch, fn, boom)
        mp.setattr(torch.Tensor, "__matmul__", boom)
        mp.setattr(torch.Tensor, "addmm_", boom)
        mp.setattr(torch.nn.functional, "linear", boom)
        out = model(ids, labels=labels)
        out.loss.backward()
    torch.testing.assert_close(out.logits.cpu(), rec["logits"], **FP32)
    torch.testing.assert_close(out.loss.cpu(), rec["loss"], **FP32)
    named = model.state_dict(keep_vars=True)
    for k, g in rec.items():
        if k.startswith("grad/"):
            scale = max(1.0, float(g.abs().max()))
            torch.testing.assert_close(named[k[5:]].grad.cpu(), g, rtol=6e-4, atol=2e-3 * scale, msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("name", ["ps_fused", "ps_unfused", "ph_fused"])
def test_layer_trace_matches_reference(backend, name):
    """Per-layer (hidden, residual) of the reference, through the module-level reference-frame API."""
    _, dev = backend
    model, cfg, sd, rec = build_model(name, dev)
    bb = model.caduceus.backbone
    hidden = bb.embeddings(rec["input_ids"].to(dev))
    residual = None
    for i, layer in enumerate(bb.layers):
        hidden, residual = layer(hidden, residual)
        torch.testing.assert_close(hidden.cpu(), rec[f"trace/{i}/hidden"], **FP32)
        torch.testing.assert_close(residual.cpu(), rec[f"trace/{i}/residual"], **FP32)


@pytest.mark.parametrize("name", ["ps_fused", "ph_fused", "ps_unfused"])
def test_model_fp16_autocast(backend, name):
    """float16 autocast -- the reference's own AMP precision (configs/experiment/hg38/hg38.yaml:20, vep_embeddings.py:352) -- is
    served by the fp32 kernels: logits, loss and gradients equal the fp32 run, the hidden states come back as float16."""
    _, dev = backend
    model, cfg, sd, rec = build_model(name, dev)
    ids, labels = rec["input_ids"].to(dev), rec["labels"].to(dev)
    with torch.autocast(dev.type, dtype=torch.float16):
        out = model(ids, labels=labels, output_hidden_states=True)
        hs = model.caduceus(ids).last_hidden_state
    assert out.logits.dtype == torch.float32 and hs.dtype == torch.float16
    assert all(h.dtype == torch.float16 for h in out.hidden_states)
    torch.testing.assert_close(out.logits.cpu(), rec["logits"], **FP32)
    torch.testing.assert_close(out.loss.cpu(), rec["loss"], **FP32)
    out.loss.backward()
    key = ("caduceus.backbone.layers.0.mixer.submodule.mamba_fwd.x_proj.weight" if cfg["rcps"]
           else "caduceus.backbone.layers.0.mixer.mamba_fwd.x_proj.weight")
    g = model.state_dict(keep_vars=True)[key].grad
    torch.testing.assert_close(g.cpu(), rec["grad/" + key], rtol=2e-3, atol=2e-5 * max(1.0, float(rec["grad/" + key].abs().max())))
    with torch.no_grad():
        ref_h = model.caduceus(ids).last_hidden_state
    torch.testing.assert_close(hs.float().cpu(), ref_h.float().cpu(), rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("name", ["ps_fused", "ph_fused", "ps_fused_res32_odd"])
def test_model_bf16_autocast(backend, name):
    """bf16 compute (autocast, fp32 master weights) against the fp32 reference vectors at the reference's bf16 tolerance."""
    _, dev = backend
    model, cfg, sd, rec = build_model(name, dev)
    ids, labels = rec["input_ids"].to(dev), rec["labels"].to(dev)
    with torch.autocast(dev.type, dtype=torch.bfloat16):
        out = model(ids, labels=labels)
    assert out.logits.dtype == torch.float32
    # two+ layers of bf16 rounding on O(10) logits: judge the error in the relative L2 sense
    rel = float((out.logits.cpu() - rec["logits"]).norm() / rec["logits"].norm())
    assert rel < 3e-2, rel
    assert abs(float(out.loss) - float(rec["loss"])) < 0.05 * max(1.0, float(rec["loss"]))
    out.loss.backward()
    g = model.state_dict(keep_vars=True)["caduceus.backbone.layers.0.mixer.submodule.mamba_fwd.x_proj.weight"
                                         if cfg["rcps"] else "caduceus.backbone.layers.0.mixer.mamba_fwd.x_proj.weight"].grad
    ref = rec["grad/caduceus.backbone.layers.0.mixer.submodule.mamba_fwd.x_proj.weight" if cfg["rcps"]
              else "grad/caduceus.backbone.layers.0.mixer.mamba_fwd.x_proj.weight"]
    cos = F.cosine_similarity(g.float().cpu().flatten(), ref.flatten(), dim=0)
    assert cos > 0.99, float(cos)


def test_inputs_embeds_and_hidden_states(backend):
    _, dev = backend
    model, cfg, sd, rec = build_model("ps_fused", dev)
    ids = rec["input_ids"].to(dev)
    emb = model.get_input_embeddings()(ids)  # (B, L, 2D) reference frame
    ref_emb = om.rcps_embedding(sd["caduceus.backbone.embeddings.word_embeddings.embedding.weight"],
                                sd["caduceus.backbone.embeddings.word_embeddings.complement_map"], rec["input_ids"])
    assert torch.equal(emb.cpu(), ref_emb)
    a = model(ids, output_hidden_states=True)
    b = model(inputs_embeds=emb)
    torch.testing.assert_close(a.logits, b.logits, rtol=0, atol=0)
    assert len(a.hidden_states) == cfg["n_layer"] + 1  # reference quirk: final append only in the fused branch
    torch.testing.assert_close(a.hidden_states[0].cpu(), ref_emb)
    torch.testing.assert_close(a.hidden_states[-1].cpu(), rec["hidden"], **FP32)
    tup = model(ids, labels=rec["labels"].to(dev), return_dict=False)
    assert isinstance(tup, tuple) and tup[0].ndim == 0 and tup[1].shape == a.logits.shape


def test_weighted_cross_entropy_path(backend):
    """`loss_weights` (modeling_caduceus.py:286-294, 484-486): weighted CE over the non-ignored targets, and its gradients."""
    _, dev = backend
    model, cfg, sd, rec = build_model("ps_fused", dev)
    ids, labels = rec["input_ids"].to(dev), rec["labels"].to(dev)
    g = torch.Generator().manual_seed(7)
    lw = torch.rand(labels.shape, generator=g) + 0.1
    out = model(ids, labels=labels, loss_weights=lw.to(dev))
    ref = om.masked_lm_forward(sd, rec["input_ids"], cfg)
    ref_loss = om.weighted_cross_entropy(ref["logits"], rec["labels"], lw, ignore_index=4)
    torch.testing.assert_close(out.loss.cpu(), ref_loss, **FP32)
    out.loss.backward()
    # gradient of the weighted loss w.r.t. the tied embedding, against autograd through the oracle
    key = "caduceus.backbone.embeddings.word_embeddings.embedding.weight"
    sd2 = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    sd2["lm_head.lm_head.weight"] = sd2[key]
    r2 = om.masked_lm_forward(sd2, rec["input_ids"], cfg)
    om.weighted_cross_entropy(r2["logits"], rec["labels"], lw, ignore_index=4).backward()
    got = model.state_dict(keep_vars=True)[key].grad.cpu()
    want = sd2[key].grad
    torch.testing.assert_close(got, want, rtol=6e-4, atol=2e-3 * max(1.0, float(want.abs().max())))


def test_zero_hidden_rows_gate_gradient(backend):
    """Zero rows of `inputs_embeds` make the in_proj gate exactly 0 for every channel of those tokens -- the case in which
    out / z cannot recover y.  Through the production (shared-gate) mixer path the gradient w.r.t. the embeddings must
    still match autograd through the oracle."""
    _, dev = backend
    model, cfg, sd, rec = build_model("ps_fused", dev)
    ids = rec["input_ids"]
    emb = om.rcps_embedding(sd["caduceus.backbone.embeddings.word_embeddings.embedding.weight"],
                            sd["caduceus.backbone.embeddings.word_embeddings.complement_map"], ids).clone()
    emb[:, [0, 5, 17, emb.shape[1] - 1]] = 0.0
    w = torch.randn(emb.shape[0], emb.shape[1], cfg["d_model"] * 2, generator=torch.Generator().manual_seed(1))
    x = emb.clone().to(dev).requires_grad_(True)
    h = model.caduceus(inputs_embeds=x).last_hidden_state
    (h * w.to(dev)).sum().backward()
    xr = emb.clone().requires_grad_(True)
    href, _ = om.backbone_forward(sd, None, cfg, inputs_embeds=xr)
    (href * w).sum().backward()
    torch.testing.assert_close(h.detach().cpu(), href.detach(), **FP32)
    scale = max(1.0, float(xr.grad.abs().max()))
    torch.testing.assert_close(x.grad.cpu(), xr.grad, rtol=6e-4, atol=2e-3 * scale)


def test_training_step_gradients_repeat_bit_for_bit(backend):
    """The weight gradients that used to be summed with fp32 atomics in arrival order (embedding, add + norm, conv1d) are folded from
    per-workgroup slots in a fixed order: the same inputs give bit-identical gradients (Caduceus-PS, batch 1, bf16 as in bench.py)."""
    kind, dev = backend
    import bench
    L = 4096 if kind == "hip" else 512
    torch.manual_seed(2222)
    model = CaduceusForMaskedLM(bench.make_config(64, 2)).to(dev).train()
    ids, labels = bench.synthetic_batch(torch.Generator().manual_seed(7), 1, L, dev)
    grads = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        with torch.autocast(dev.type, dtype=torch.bfloat16):
            out = model(ids, labels=labels)
        out.loss.backward()
        grads.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 0
    differ = [n for n in grads[0] if not torch.equal(grads[0][n], grads[1][n])]
    assert not differ, differ
