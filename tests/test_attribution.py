"""caduceus_amd.attribute through the model, on the golden variants ps_fused, ph_fused and ps_fused_unidir (d_model 32, 2 layers, ids
(2, 64)) in fp32.

Reference: autograd through oracle.oracle_model.backbone_forward(inputs_embeds=...) with the head restated here (the masked-LM
log-probability, a callable on the hidden state, the classifier's pooling + score), and the gradient of the reference-frame embedding
(B, L, D | 2 D) projected on the embedding table in fp64:
  d score / d onehot[b,l,v] = <g[b,l,:D], E[v]> + <g[b,l,D:], flip(E[comp v])>     (oracle_model.rcps_embedding's layout)
Tolerance: the project's own for exactly this quantity -- the gradient w.r.t. the embedding output against autograd through the oracle,
tests/test_model_parity.py::test_zero_hidden_rows_gate_gradient: rtol 6e-4, atol 2e-3 max(1, max |ref|).  bf16 is held to the hand route
of the parent commit (inputs_embeds.requires_grad_(), the ordinary full backward, a torch product with E) at test_model_parity.py's BF16
dict, scaled the same way.
"""
import pytest
import torch

from caduceus_amd import CaduceusForMaskedLM, MaskedTarget, attribute, mixer, ops
from oracle import oracle_model as om
from test_model_parity import BF16, build_model
from test_pooled_finetune import classifiers

ALLOWED = [7, 8, 9, 10]  # A, C, G, T of the golden vocabulary; 7 <-> 10, 8 <-> 9 under the complement map
MASK_ID = 3
VARIANTS = ["ps_fused", "ph_fused", "ps_fused_unidir"]
METHODS = ["gradient", "grad_x_input", "integrated"]
STEPS = 4


def close(got, ref, what, rtol=6e-4, atol=2e-3):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = max(1.0, float(ref.abs().max()))
    print(f"[attribution] {what}: max |got - ref| = {float((got - ref).abs().max()):.3e}, max |ref| = {float(ref.abs().max()):.3e}")
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol * scale, msg=lambda m: f"{what}: {m}")


def _table(sd, cfg):
    """(E (V, D) fp64, comp (V) | None) of the golden state dict."""
    if cfg["rcps"]:
        return (sd["caduceus.backbone.embeddings.word_embeddings.embedding.weight"].double(),
                sd["caduceus.backbone.embeddings.word_embeddings.complement_map"])
    return sd["caduceus.backbone.embeddings.word_embeddings.weight"].double(), None


def _oracle_embed(sd, cfg, ids):
    if cfg["rcps"]:
        return om.rcps_embedding(sd["caduceus.backbone.embeddings.word_embeddings.embedding.weight"],
                                 sd["caduceus.backbone.embeddings.word_embeddings.complement_map"], ids)
    return sd["caduceus.backbone.embeddings.word_embeddings.weight"][ids]


def _project(g, E, comp):
    """Reference-frame embedding gradient (B, L, D | 2 D) -> d score / d onehot (B, L, V), fp64."""
    D = E.shape[1]
    out = g[..., :D].double() @ E.t()
    if comp is not None:
        out = out + g[..., D:].double() @ E[comp].flip(-1).t()
    return out


def _finish(full, ids, method, centre=True):
    """What attribute returns, from d score / d onehot (B, L, V) over the whole vocabulary."""
    c = full[..., ALLOWED]
    if centre:
        c = c - c.mean(-1, keepdim=True)
    if method == "gradient":
        return c
    col = torch.full((full.shape[-1],), -1, dtype=torch.int64)
    col[ALLOWED] = torch.arange(len(ALLOWED))
    k = col[ids]
    return torch.where(k >= 0, c.gather(-1, k.clamp_min(0).unsqueeze(-1))[..., 0], torch.zeros_like(c[..., 0]))


def oracle_attribution(sd, cfg, ids, score, method, centre=True):
    """The reference for attribute(...): score maps the oracle's final hidden state (B, L, D | 2 D) to (B,) scores."""
    E, comp = _table(sd, cfg)
    x = _oracle_embed(sd, cfg, ids).detach()

    def grad_at(point):
        point = point.clone().requires_grad_(True)
        hidden, _ = om.backbone_forward(sd, None, cfg, inputs_embeds=point)
        return torch.autograd.grad(score(hidden).sum(), [point])[0]

    if method != "integrated":
        return _finish(_project(grad_at(x), E, comp), ids, method, centre)
    base = E[ALLOWED].mean(0)
    x0 = (base if comp is None else torch.cat([base, E[comp[ALLOWED]].mean(0).flip(-1)])).float()
    g = sum(grad_at(x0 + (k + 0.5) / STEPS * (x - x0)).double() for k in range(STEPS)) / STEPS
    return _finish(_project(g, E, comp), ids, "grad_x_input")


def _masked_case(ids):
    """One masked position per row, an allowed token to score and another as the reference allele."""
    B, Lq = ids.shape
    pos = torch.tensor([5, Lq - 3])[:B]
    return pos, torch.tensor([7, 9])[:B], torch.tensor([8, 10])[:B]


def _masked_score(sd, cfg, pos, tok, ref):
    def score(hidden):
        rows = torch.arange(hidden.shape[0])
        logp = torch.log_softmax(om.lm_head(sd, hidden, cfg).float()[rows, pos][:, ALLOWED], -1)
        col = {v: k for k, v in enumerate(ALLOWED)}
        s = logp[rows, torch.tensor([col[int(t)] for t in tok])]
        return s if ref is None else s - logp[rows, torch.tensor([col[int(t)] for t in ref])]
    return score


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("with_ref", [False, True], ids=["logp", "llr"])
@pytest.mark.parametrize("name", VARIANTS)
def test_masked_target_against_the_oracle(backend, name, with_ref, method):
    _, dev = backend
    model, cfg, sd, rec = build_model(name, dev)
    ids = rec["input_ids"]
    pos, tok, ref = _masked_case(ids)
    ref = ref if with_ref else None
    masked = ids.clone()
    masked[torch.arange(ids.shape[0]), pos] = MASK_ID
    keep = ids.clone()
    got = attribute(model, ids.to(dev), MaskedTarget(pos, tok, ref, mask_token_id=MASK_ID), allowed_token_ids=ALLOWED, method=method,
                    steps=STEPS)
    assert torch.equal(ids, keep) and got.dtype == torch.float32
    assert got.shape == ((*ids.shape, len(ALLOWED)) if method == "gradient" else tuple(ids.shape))
    want = oracle_attribution(sd, cfg, masked, _masked_score(sd, cfg, pos, tok, ref), method)
    close(got, want, f"{name} masked {method}")
    if method != "gradient":  # the masked position holds no base
        assert bool((got.cpu()[torch.arange(ids.shape[0]), pos] == 0.0).all())


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", VARIANTS)
def test_callable_target_against_the_oracle(backend, name, method):
    _, dev = backend
    model, cfg, sd, rec = build_model(name, dev)
    ids = rec["input_ids"]
    w = torch.randn(rec["hidden"].shape, generator=torch.Generator().manual_seed(1))
    wd = w.to(dev)
    centre = method != "gradient"  # (the un-centred gradient once: d score / d onehot as it is)
    for m in (model, model.caduceus):  # the masked LM and the bare Caduceus
        got = attribute(m, ids.to(dev), lambda h: (h * wd).sum((1, 2)), allowed_token_ids=ALLOWED, method=method, centre=centre, steps=STEPS)
        want = oracle_attribution(sd, cfg, ids, lambda h: (h * w).sum((1, 2)), method, centre)
        close(got, want, f"{name} callable {method} {type(m).__name__}")


def _classifier_score(clf, cfg, cls):
    """The classifier's head on the oracle's hidden state: pool each strand over the sequence, score both, average."""
    W = clf.score.weight.detach().cpu()
    pool = (lambda t: t.mean(1)) if clf.pooling_strategy == "mean" else (lambda t: t.max(1).values)

    def score(hidden):
        D = cfg["d_model"]
        logits = pool(hidden[..., :D]) @ W.t()
        if cfg["rcps"]:
            logits = (logits + pool(hidden[..., D:].flip(-1)) @ W.t()) / 2
        return logits.gather(1, cls[:, None])[:, 0]
    return score


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("fused", [False, True], ids=["unfused-pool", "fused_pool_train"])
@pytest.mark.parametrize("pooling", ["mean", "max"])
@pytest.mark.parametrize("name", VARIANTS)
def test_class_target_against_the_oracle(backend, name, pooling, fused, method):
    _, dev = backend
    clf = classifiers(name, pooling, False, dev)[int(fused)]
    cfg, sd, rec = __import__("conftest").load_golden_model(name)
    ids = rec["input_ids"]
    cls = torch.tensor([2, 0])
    calls = []
    inner = ops.pool_head_grad
    ops.pool_head_grad = lambda *a, **k: calls.append(1) or inner(*a, **k)
    try:
        got = attribute(clf, ids.to(dev), cls, allowed_token_ids=ALLOWED, method=method, steps=STEPS)
    finally:
        ops.pool_head_grad = inner
    assert bool(calls) == fused, "fused_pool_train decides whether the score goes through ops.pool_head_grad"
    want = oracle_attribution(sd, cfg, ids, _classifier_score(clf, cfg, cls), method)
    close(got, want, f"{name} class {pooling} {method}")
    if method == "grad_x_input":  # an int names the same class for every row
        one = attribute(clf, ids.to(dev), 2, allowed_token_ids=ALLOWED)
        assert torch.equal(one[0], got[0])


def test_conjoined_classifier(backend):
    """Post-hoc conjoining: the score is the mean of the two inputs' logits, so each input's attribution is half the plain model's."""
    _, dev = backend
    plain = classifiers("ph_fused", "mean", False, dev)[0]
    conj = classifiers("ph_fused", "mean", True, dev)[0]
    rec = __import__("conftest").load_golden_model("ph_fused")[2]
    a = rec["input_ids"]
    b = torch.randint(7, 11, a.shape, generator=torch.Generator().manual_seed(6))
    got = attribute(conj, torch.stack([a, b], -1).to(dev), 1, allowed_token_ids=ALLOWED, method="gradient")
    assert got.shape == (*a.shape, len(ALLOWED), 2)
    for k, x in enumerate((a, b)):
        close(got[..., k], 0.5 * attribute(plain, x.to(dev), 1, allowed_token_ids=ALLOWED, method="gradient"), f"conjoined input {k}")
    with pytest.raises(ValueError, match=r"\(B, L, 2\)"):
        attribute(conj, a.to(dev), 1, allowed_token_ids=ALLOWED)


def _hand_route(model, ids, wd):
    """The route of the parent commit: inputs_embeds.requires_grad_(), the ordinary full backward, a torch product with E."""
    emb = model.get_input_embeddings()(ids).detach().requires_grad_(True)  # (B, L, 2 D), reference frame
    h = model.caduceus(inputs_embeds=emb).last_hidden_state
    (h.float() * wd).sum().backward()
    we = model.get_input_embeddings()
    E, comp = we.weight.detach().float(), we.complement_map
    D = E.shape[1]
    g = emb.grad.float()
    full = g[..., :D] @ E.t() + g[..., D:] @ E[comp].flip(-1).t()
    c = full[..., ALLOWED]
    return c - c.mean(-1, keepdim=True)


def test_bf16_against_the_hand_route(backend):
    _, dev = backend
    model, cfg, sd, rec = build_model("ps_fused", dev)
    ids = rec["input_ids"].to(dev)
    wd = torch.randn(rec["hidden"].shape, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.autocast(dev.type, dtype=torch.bfloat16):
        got = attribute(model, ids, lambda h: (h.float() * wd).sum((1, 2)), allowed_token_ids=ALLOWED, method="gradient")
        want = _hand_route(model, ids, wd)
    model.zero_grad(set_to_none=True)
    print(f"[attribution] bf16: attribute and the hand route are bit-identical: {torch.equal(got, want)}")
    close(got, want, "bf16 gradient vs the hand route", rtol=BF16["rtol"], atol=BF16["atol"])


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_no_side_effects(backend, bf16):
    """No parameter's .grad, requires_grad or version, and no module's training flag, changes."""
    _, dev = backend
    model, cfg, sd, rec = build_model("ps_fused", dev)
    ids = rec["input_ids"].to(dev)
    frozen = next(p for n, p in model.named_parameters() if n.endswith("norm_f.weight"))
    frozen.requires_grad_(False)
    before = {n: (p.requires_grad, p._version) for n, p in model.named_parameters()}
    for training, method in ((True, "integrated"), (False, "gradient")):
        model.train(training)
        modes = {n: m.training for n, m in model.named_modules()}
        with torch.autocast(dev.type, dtype=torch.bfloat16, enabled=bf16):
            attribute(model, ids, MaskedTarget(*_masked_case(ids), mask_token_id=MASK_ID), allowed_token_ids=ALLOWED, method=method, steps=2)
        assert modes == {n: m.training for n, m in model.named_modules()}
    assert all(p.grad is None for p in model.parameters())
    assert before == {n: (p.requires_grad, p._version) for n, p in model.named_parameters()} and not frozen.requires_grad
    assert not mixer.input_grad_only_enabled() and torch.is_grad_enabled()


def test_a_training_step_after_attribute_is_the_step_without_it(backend):
    """Loss and every gradient of a training step taken after attribute equal, bit for bit, those of a step taken without the call.  At
    the configuration in which the project's gradients repeat bit for bit at all -- Caduceus-PS, batch 1, bf16, the model and batch of
    tests/test_model_parity.py::test_training_step_gradients_repeat_bit_for_bit: with more rows per channel the scans' small parameter
    sums (A_log, D, dt_proj.bias) are accumulated in arrival order on the device and two steps WITHOUT any call in between already differ
    in their last bits."""
    import bench
    kind, dev = backend
    Lq = 4096 if kind == "hip" else 512
    steps = []
    for call in (True, False):
        torch.manual_seed(2222)
        model = CaduceusForMaskedLM(bench.make_config(64, 2)).to(dev).train()
        ids, labels = bench.synthetic_batch(torch.Generator().manual_seed(7), 1, Lq, dev)
        with torch.autocast(dev.type, dtype=torch.bfloat16):
            if call:
                attribute(model, ids, MaskedTarget(torch.tensor([Lq // 2]), torch.tensor([8]), mask_token_id=MASK_ID),
                          allowed_token_ids=ALLOWED, method="integrated", steps=2)
            out = model(ids, labels=labels)
        out.loss.backward()
        steps.append((out.loss.detach(), {n: p.grad for n, p in model.named_parameters() if p.grad is not None}))
    (la, ga), (lb, gb) = steps
    assert torch.equal(la, lb) and ga.keys() == gb.keys() and len(ga) > 10
    assert not [n for n in ga if not torch.equal(ga[n], gb[n])]


WGRAD_OPS = ("proj_wx_wgrad", "proj_wgrad_only", "wgrad_cm_tm", "fold_f32")


def test_the_weight_gradient_products_are_skipped(backend, monkeypatch):
    """d_model 256 in bf16: the ordinary backward runs the weight-gradient products and the fold launch (counted first); with all four
    made to raise, attribute still runs -- under mixer.input_grad_only() the backward never reaches them."""
    import bench
    _, dev = backend
    torch.manual_seed(11)
    model = CaduceusForMaskedLM(bench.make_config(256, 1)).to(dev).train()
    ids, labels = bench.synthetic_batch(torch.Generator().manual_seed(7), 1, 256, dev)
    counts = dict.fromkeys(WGRAD_OPS, 0)

    def counting(name, inner):
        def fn(*a, **k):
            counts[name] += 1
            return inner(*a, **k)
        return fn
    with monkeypatch.context() as mp:
        for name in WGRAD_OPS:
            mp.setattr(ops, name, counting(name, getattr(ops, name)))
        with torch.autocast(dev.type, dtype=torch.bfloat16):
            model(ids, labels=labels).loss.backward()
    print(f"[attribution] weight-gradient calls of one ordinary backward: {counts}")
    assert sum(counts.values()) >= 1 and all(p.grad is not None for p in model.parameters())
    model.zero_grad(set_to_none=True)
    target = MaskedTarget(torch.tensor([100]), torch.tensor([8]), mask_token_id=MASK_ID)
    with torch.autocast(dev.type, dtype=torch.bfloat16):
        want = attribute(model, ids, target, allowed_token_ids=ALLOWED)
    with monkeypatch.context() as mp:
        def boom(*a, **k):
            raise AssertionError("a weight-gradient product under input_grad_only")
        for name in WGRAD_OPS:
            mp.setattr(ops, name, boom)
        with torch.autocast(dev.type, dtype=torch.bfloat16):
            got = attribute(model, ids, target, allowed_token_ids=ALLOWED)
    assert torch.equal(got, want) and bool((got != 0).any()) and bool(torch.isfinite(got).all())
    assert all(p.grad is None for p in model.parameters())


def test_reverse_complement_property(backend):
    """RCPS: attribute(RC ids) is attribute(ids) flipped along L with its columns permuted by the complement map (the target moved to the
    mirrored position and complemented with it)."""
    _, dev = backend
    model, cfg, sd, rec = build_model("ps_fused", dev)
    ids = rec["input_ids"]
    comp = sd["caduceus.backbone.embeddings.word_embeddings.complement_map"]
    Lq = ids.shape[1]
    pos, tok, ref = _masked_case(ids)
    rc_ids = comp[ids.flip(-1)]
    perm = torch.tensor([ALLOWED.index(int(comp[a])) for a in ALLOWED])  # column of comp a
    for method in METHODS:
        a = attribute(model, ids.to(dev), MaskedTarget(pos, tok, ref, mask_token_id=MASK_ID), allowed_token_ids=ALLOWED, method=method,
                      steps=2).cpu()
        b = attribute(model, rc_ids.to(dev), MaskedTarget(Lq - 1 - pos, comp[tok], comp[ref], mask_token_id=MASK_ID),
                      allowed_token_ids=ALLOWED, method=method, steps=2).cpu()
        back = b.flip(1)[..., perm] if method == "gradient" else b.flip(1)
        print(f"[attribution] RC {method}: bit-exact: {torch.equal(back, a)}")
        close(back, a, f"RC property {method}")


def test_errors(backend):
    _, dev = backend
    model, cfg, sd, rec = build_model("ps_fused", dev)
    ids = rec["input_ids"].to(dev)
    t = MaskedTarget(*_masked_case(ids), mask_token_id=MASK_ID)
    with pytest.raises(ValueError, match="closed under the complement map"):
        attribute(model, ids, t, allowed_token_ids=[7, 8, 9], method="integrated")
    attribute(model, ids, t, allowed_token_ids=[7, 8, 9], method="gradient")  # (only the baseline needs the closure)
    with pytest.raises(ValueError, match="centre=False"):
        attribute(model, ids, t, allowed_token_ids=ALLOWED, method="integrated", centre=False)
    with pytest.raises(ValueError, match="method"):
        attribute(model, ids, t, allowed_token_ids=ALLOWED, method="saliency")
    with pytest.raises(ValueError, match="allowed_token_ids"):
        attribute(model, ids, t, allowed_token_ids=[7, 16])
    with pytest.raises(TypeError, match="CaduceusForSequenceClassification"):
        attribute(model, ids, 1, allowed_token_ids=ALLOWED)
    with pytest.raises(TypeError, match="CaduceusForMaskedLM"):
        attribute(model.caduceus, ids, t, allowed_token_ids=ALLOWED)
    with pytest.raises(TypeError, match="class index"):
        attribute(model, ids, "promoter", allowed_token_ids=ALLOWED)
    with pytest.raises(ValueError, match="one per row"):
        attribute(model, ids, lambda h: h.sum(), allowed_token_ids=ALLOWED)
    clf = classifiers("ps_fused", "mean", False, dev)[0]
    with pytest.raises(TypeError, match="CaduceusForMaskedLM"):
        attribute(clf, ids, t, allowed_token_ids=ALLOWED)
    with pytest.raises(ValueError, match="target must lie"):
        attribute(clf, ids, 3, allowed_token_ids=ALLOWED)
    # a head with bias, and a vocabulary above 16: AttribUnsupported, a ValueError like the scoring functions' ScoreUnsupported
    model.lm_head.lm_head.bias = torch.nn.Parameter(torch.zeros(model.lm_head.lm_head.weight.shape[0], device=dev))
    with pytest.raises(ops.AttribUnsupported, match="bias-free LM head"):
        attribute(model, ids, t, allowed_token_ids=ALLOWED)
    from caduceus_amd import CaduceusConfig
    big = CaduceusForMaskedLM(CaduceusConfig(**{**cfg, "vocab_size": 24, "complement_map": {i: i for i in range(24)}})).to(dev)
    with pytest.raises(ops.AttribUnsupported, match=r"vocab_size 24 \(vocab_size <= 16\)"):
        attribute(big, ids, t, allowed_token_ids=ALLOWED)
