"""Fine-tuning through the pool head (CaduceusForSequenceClassification(fused_pool=True, fused_pool_train=True), ops.pool_head_grad,
pooled_embeddings(grad=True)) on the fp32 golden weights: loss and every parameter's gradient against the un-fused route (ops.add_norm,
the pooling in torch, autograd) on the same weights, for every pooling strategy; that training and evaluation now run the same head;
and, on the GPU, that the head's forward under grad keeps nothing of size L alive.

Bound.  Both routes are fp32 implementations of the same function, so they are held to each other at the project's fp32
implementation-parity bound: 6e-4 absolute / 2e-3 relative, and also at tests/test_model_parity.py's spelling of it (rtol 6e-4, atol
2e-3 x max(1, |g|max)); a gradient passes only if it passes both.  "max" sends a channel's gradient to one row on either route -- the lowest
row of the maximum -- and the two routes' rows differ by at most a last bit of a statistic, so a tie between two DISTINCT rows that the
routes would break differently needs two rows equal to within that bit: not at these sizes in fp32.
"""
import pytest
import torch

from caduceus_amd import CaduceusConfig, CaduceusForSequenceClassification, ops, pooled_embeddings
from conftest import load_golden_model
from test_pooled_embeddings import LQ, input_ids
from test_scoring import _golden

F32, BF = torch.float32, torch.bfloat16
CASES = [("ps_fused", False), ("ph_unfused", False), ("ph_fused", True)]


def close(got, want, what):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    torch.testing.assert_close(got, want, rtol=2e-3, atol=6e-4, msg=lambda m: f"{what}: {m}")
    torch.testing.assert_close(got, want, rtol=6e-4, atol=2e-3 * max(1.0, float(want.abs().max())), msg=lambda m: f"{what}: {m}")


def classifiers(name, pooling, conjoin, dev):
    cfg, sd, _ = load_golden_model(name)
    config = CaduceusConfig(**cfg, num_labels=3)
    torch.manual_seed(2)
    plain = CaduceusForSequenceClassification(config, pooling_strategy=pooling, conjoin_train=conjoin)
    plain.caduceus.load_state_dict({k[len("caduceus."):]: v for k, v in sd.items() if k.startswith("caduceus.")}, strict=True)
    fused = CaduceusForSequenceClassification(config, pooling_strategy=pooling, conjoin_train=conjoin, fused_pool=True, fused_pool_train=True)
    fused.load_state_dict(plain.state_dict(), strict=True)
    return plain.to(dev).train(), fused.to(dev).train()


@pytest.mark.parametrize("name,conjoin", CASES, ids=[c[0] + ("-conjoin" if c[1] else "") for c in CASES])
@pytest.mark.parametrize("pooling", ["mean", "max", "first", "last"])
def test_finetune_step_through_the_pool_head(backend, pooling, name, conjoin):
    _, dev = backend
    plain, fused = classifiers(name, pooling, conjoin, dev)
    ids = input_ids(2, LQ, dev, seed=5)
    if conjoin:
        ids = torch.stack([ids, input_ids(2, LQ, dev, seed=6)], -1)
    labels = torch.tensor([2, 0], device=dev)
    seen = []
    inner = ops.pool_head_grad

    def spy(*a, **k):
        seen.append(torch.is_grad_enabled())
        return inner(*a, **k)
    ops.pool_head_grad = spy
    try:
        a = plain(ids, labels=labels)
        b = fused(ids, labels=labels)
    finally:
        ops.pool_head_grad = inner
    assert seen == [True], "the fused model did not train through the pool head"
    close(b.logits, a.logits, "logits")
    close(b.loss, a.loss, "loss")
    a.loss.backward()
    b.loss.backward()
    pa, pb = dict(plain.named_parameters()), dict(fused.named_parameters())
    assert pa.keys() == pb.keys()
    checked = 0
    for k, p in pa.items():
        assert (p.grad is None) == (pb[k].grad is None), k
        if p.grad is not None:
            close(pb[k].grad, p.grad, k)
            checked += 1
    assert checked > 10 and all(p.grad is not None for k, p in pb.items() if "norm_f" in k)
    # one SGD step, then evaluation: the trained model's eval logits are those of the inference-only head on the same weights
    with torch.no_grad():
        for p in fused.parameters():
            if p.grad is not None:
                p -= 0.1 * p.grad
    fused.eval()
    infer = CaduceusForSequenceClassification(fused.config, pooling_strategy=pooling, conjoin_train=conjoin, fused_pool=True)
    infer.load_state_dict(fused.state_dict(), strict=True)
    infer = infer.to(dev).eval()
    with torch.no_grad():
        assert torch.equal(fused(ids).logits, infer(ids).logits)
    assert fused(ids, output_hidden_states=True).hidden_states is not None  # asked for hidden states: the route that has them


def test_fused_pool_alone_keeps_todays_route_under_grad(backend):
    _, dev = backend
    plain, _ = classifiers("ps_fused", "mean", False, dev)
    only = CaduceusForSequenceClassification(plain.config, pooling_strategy="mean", fused_pool=True)
    only.load_state_dict(plain.state_dict(), strict=True)
    only = only.to(dev).train()
    ids = input_ids(2, LQ, dev, seed=5)
    calls = []
    inner = ops.pool_head_grad
    ops.pool_head_grad = lambda *a, **k: calls.append(1) or inner(*a, **k)
    try:
        assert torch.equal(only(ids).logits, plain(ids).logits)
    finally:
        ops.pool_head_grad = inner
    assert not calls and not only.fused_pool_train


@pytest.mark.parametrize("name", ["ps_fused", "ph_unfused"])
def test_pooled_embeddings_backpropagate(backend, name):
    """pooled_embeddings(grad=True): same values as the default, and a gradient that reaches the embedding weights and equals the
    un-fused route's within the bound; the default still runs under no_grad."""
    _, dev = backend
    model, _ = _golden(name, dev)
    model.train()
    ids = input_ids(2, LQ, dev, seed=8)
    emb = next(p for k, p in model.named_parameters() if "word_embeddings" in k)
    for pooling, kw in (("mean", {}), ("window", dict(centre=torch.tensor([3, LQ - 2], device=dev), window_tokens=6))):
        plain = pooled_embeddings(model, ids, pooling, **kw)
        assert not plain.requires_grad
        out = pooled_embeddings(model, ids, pooling, grad=True, **kw)
        assert out.requires_grad and torch.equal(out.detach(), plain)
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(4)).to(dev)
        model.zero_grad()
        (out * g).sum().backward()
        got = emb.grad.clone()
        assert bool((got != 0).any())
        if pooling == "mean":  # the same function through the written activation: model.caduceus(ids), mean over positions
            model.zero_grad()
            h = model.caduceus(ids, return_dict=False)  # (B, L, D) or (B, L, 2 D) with the second strand's channels after the first's
            m = h.float().mean(1)
            ref = m if out.dim() == 2 else torch.stack([m[:, :out.shape[1]], m[:, out.shape[1]:].flip(-1)], -1)
            close(out, ref, "embeddings")
            (ref * g).sum().backward()
            close(got, emb.grad, "d(embedding weights)")


@pytest.mark.gpu
def test_pool_head_grad_forward_keeps_nothing_of_size_L():
    """S = 2, B = 1, L = 4096, D = 64 in bf16 with an fp32 residual, under grad: what the forward allocates on top of its inputs -- out,
    the partials of at most 256 pieces (32 k floats), the fp32 copies of weight and bias -- stays below x.numel() bytes, which is less
    than any tensor of size L (a bf16 y alone would be twice that)."""
    from caduceus_amd import _lib
    _lib.use_library_for_testing(None)
    dev = torch.device("cuda:0")
    S, B, Lq, D = 2, 1, 4096, 64
    g = torch.Generator().manual_seed(1)
    x = torch.randn(S, B, Lq, D, generator=g).to(BF).to(dev).requires_grad_(True)
    res = torch.randn(S, B, Lq, D, generator=g).to(dev).requires_grad_(True)
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(dev).requires_grad_(True)
    for mode in ("mean", "max"):
        ops.pool_head_grad(x, res, w, None, 1e-5, True, BF, mode).sum().backward()  # warm-up: workspaces, caches
        x.grad = res.grad = w.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = ops.pool_head_grad(x, res, w, None, 1e-5, True, BF, mode)
        torch.cuda.synchronize()
        grown, held = torch.cuda.max_memory_allocated() - base, torch.cuda.memory_allocated() - base
        print(f"[pool_head_grad {mode}] forward peak over the inputs {grown} B, held {held} B, x.numel() = {x.numel()}")
        assert out.requires_grad and held <= grown < x.numel(), (mode, grown, held, x.numel())
        del out
