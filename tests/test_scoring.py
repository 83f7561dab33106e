"""caduceus_amd.scoring: sequence_logprobs against the fp64 restatement of the causal stack (one piece and in chunks through the cache)
and against what generate returned; masked_logprobs and variant_llr on golden RCPS, bi-directional and causal weights against the
model's own logits; the caller's ids stay; refusals; and, on the GPU, that no (B, L, V) tensor is allocated.

Bounds: FACTOR and FP32_BOUND of tests/test_mamba_step.py for the stacks (relative error norms against fp64; the 16-bit paths at most
FACTOR times as far from fp64 as log_softmax of the model's own logits).  For the golden models both routes start from the same final
hidden state, so they differ by at most the sum of the two kernels' fp64 bounds (tests/test_score_head.py): the score head's
e_lse + e_z[v] + u |logp|, and e_z[v] + E for an exact log_softmax of logits that carry e_z."""
import pytest
import torch

from caduceus_amd import CaduceusConfig, CaduceusForMaskedLM, generate, masked_logprobs, ops, sequence_logprobs, variant_llr
from caduceus_amd.generation import _logit_mask
from conftest import load_golden_model
from test_decode_stack import _cfg, _model, _scope, _stack_ref64
from test_mamba_step import FACTOR, FP32_BOUND
from test_score_head import score_reference

BASES = (7, 8, 9, 10)
MASK_ID = 3
L = 14
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _norm_err(got, ref):
    return float((got.detach().double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300))


def _next_logp(logits, ids, mask):
    """log softmax(logits + mask) of (B, L, V) gathered at the next ids: (B, L - 1) fp64."""
    lp = torch.log_softmax(logits.double().cpu() + (0 if mask is None else mask.double().cpu()), -1)
    return lp[:, :-1].gather(2, ids.cpu()[:, 1:, None])[..., 0]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("d_model", [64, 40])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_sequence_logprobs_against_fp64(backend, dtype, d_model, B):
    """One piece and chunk_len in {1, 4, 5, L}, each held to both bounds; chunked against one piece is printed, not asserted."""
    _, dev = backend
    _, model = _model(dev, d_model, head_std=0.5)
    torch.manual_seed(2)
    ids = torch.randint(7, 11, (B, L), device=dev)
    mask = _logit_mask(BASES, 16, dev)
    ref = _next_logp(_stack_ref64(model, ids)[0], ids, mask)
    with _scope(dev, dtype):
        own = _next_logp(model(ids).logits, ids, mask)
        got = {c: sequence_logprobs(model, ids, allowed_token_ids=BASES, chunk_len=c) for c in (None, 1, 4, 5, L)}
    e_own = _norm_err(own, ref)
    for c, lp in got.items():
        assert lp.shape == (B, L - 1) and lp.dtype == torch.float32
        e = _norm_err(lp, ref)
        print(f"sequence_logprobs vs fp64 [{dtype}, D={d_model}, B={B}, chunk_len={c}]: {e:.3e}   log_softmax(model logits): {e_own:.3e}   "
              f"equal to one piece bit for bit: {torch.equal(lp, got[None])}")
        if dtype == torch.float32:
            assert e <= FP32_BOUND, (c, e)
        else:
            assert e <= FACTOR * e_own, (c, e, e_own)


def test_sequence_logprobs_options(backend):
    """The default normalisation is the whole padded vocabulary; ignore_index defaults to config.pad_token_id and scores 0.0; a next
    token outside the allowed set scores -inf."""
    _, dev = backend
    _, model = _model(dev, head_std=0.5)
    torch.manual_seed(3)
    ids = torch.randint(7, 11, (2, L), device=dev)
    ids[0, 5], ids[1, 9] = 4, 11  # a pad and an N
    ref = _stack_ref64(model, ids)[0]
    full = sequence_logprobs(model, ids)
    want = _next_logp(ref, ids, None)
    want[0, 4] = 0.0
    assert full[0, 4].item() == 0.0 and _norm_err(full, want) <= FP32_BOUND
    lp = sequence_logprobs(model, ids, allowed_token_ids=BASES, ignore_index=-100, chunk_len=4)
    assert lp[0, 4].item() == float("-inf") and lp[1, 8].item() == float("-inf")
    assert int(torch.isinf(lp).sum()) == 2


@pytest.mark.parametrize("seed", [0, 1])
def test_sequence_logprobs_score_what_generate_produced(backend, seed):
    """fp32: the summed score of the generated tokens equals the sum of log softmax(returned logits + mask)[sampled id].  Each route is
    within FP32_BOUND of fp64 per token and the per-token log-probabilities are O(1): T tokens, T times the bound."""
    _, dev = backend
    _, model = _model(dev, seed=seed, head_std=0.5)
    L0, T, B = 5, 9, 3
    torch.manual_seed(4)
    prompt = torch.randint(7, 11, (B, L0), device=dev)
    ids, logits = generate(model, prompt, T, return_logits=True, seed=17 + seed, top_k=0, allowed_token_ids=BASES)
    mask = _logit_mask(BASES, 16, "cpu").double()
    want = sum(torch.log_softmax(lg.double().cpu() + mask, -1).gather(1, ids[:, L0 + t, None].cpu())[:, 0] for t, lg in enumerate(logits))
    got = sequence_logprobs(model, ids, allowed_token_ids=BASES)[:, L0 - 1:].double().cpu().sum(1)
    print(f"sum over {T} generated tokens: scored {got.tolist()}  from generate's logits {want.tolist()}")
    assert bool(torch.isfinite(got).all()) and bool(((got - want).abs() <= FP32_BOUND * T).all()), (got, want)


# ---- golden weights ----------------------------------------------------------------------------------------------------------------------
def _golden(name, dev):
    cfg, sd, rec = load_golden_model(name)
    head, emb = (("lm_head.lm_head.weight", "caduceus.backbone.embeddings.word_embeddings.embedding.weight")
                 if cfg["rcps"] else ("lm_head.weight", "caduceus.backbone.embeddings.word_embeddings.weight"))
    config = CaduceusConfig(**cfg, tie_word_embeddings=bool(torch.equal(sd[head], sd[emb])), pad_token_id=4)
    model = CaduceusForMaskedLM(config)
    model.load_state_dict(sd, strict=True)
    return model.to(dev).eval(), rec["input_ids"].to(dev)


def _two_kernel_bound(model, masked, pos, mask):
    """(fp64 log-probabilities (B, P, V), bound (B, P, V)) from the final hidden state of `masked`: the score head's tolerance plus that of
    an exact log_softmax of the forward's logits (e_z[v] + E)."""
    B, Lq = masked.shape
    with torch.no_grad():
        hidden = model.caduceus.backbone.forward_tframe(masked)
    S, D = hidden.shape[0], hidden.shape[-1]
    W = model.lm_head.weight.detach().float().cpu()
    comp = model.lm_head.complement_map.cpu() if model.config.rcps else None
    rows = (pos.cpu() + torch.arange(B)[:, None] * Lq).reshape(-1)
    h = hidden.reshape(S, B * Lq, D).cpu()
    ref = score_reference(h, W, comp, rows, None, None if mask is None else mask.cpu(), 4)
    lp, tol = ref["logp_all"]
    bound = torch.where(torch.isfinite(lp), tol + ref["e_z"] + ref["E"][:, None], tol)
    return lp.reshape(B, -1, W.shape[0]), bound.reshape(B, -1, W.shape[0])


@pytest.mark.parametrize("allowed", [None, BASES], ids=["all-ids", "bases"])
@pytest.mark.parametrize("name", ["ps_fused", "ph_fused", "ps_fused_unidir"])
def test_masked_logprobs_equal_the_models_logits(backend, name, allowed):
    _, dev = backend
    model, ids = _golden(name, dev)
    B, Lq = ids.shape
    V = model.config.vocab_size
    g = torch.Generator().manual_seed(len(name))
    pos = torch.stack([torch.randperm(Lq, generator=g)[:3] for _ in range(B)])
    pos[0, 0], pos[-1, -1] = 0, Lq - 1
    before = ids.clone()
    got = masked_logprobs(model, ids, pos.to(dev), mask_token_id=MASK_ID, allowed_token_ids=allowed)
    assert torch.equal(ids, before), "the caller's ids were written"
    assert got.shape == (B, 3, V) and got.dtype == torch.float32
    masked = ids.clone().scatter_(1, pos.to(dev), MASK_ID)
    mask = _logit_mask(allowed, V, dev)
    with torch.no_grad():
        logits = model(masked).logits
    z = logits.gather(1, pos.to(dev)[:, :, None].expand(B, 3, V)).double().cpu()
    want = torch.log_softmax(z + (0 if mask is None else mask.double().cpu()), -1)
    lp64, bound = _two_kernel_bound(model, masked, pos, mask)
    g_ = got.double().cpu()
    assert torch.equal(torch.isinf(g_), torch.isinf(want)) and bool((g_[torch.isinf(g_)] < 0).all())
    fin = torch.isfinite(want)
    ratio = ((g_ - want).abs()[fin] / bound[fin]).max()
    print(f"masked_logprobs vs log_softmax(model logits) [{name}, {allowed}]: worst |diff| / bound = {float(ratio):.3f}; "
          f"vs fp64 of the hidden state / bound = {float(((g_ - lp64).abs()[fin] / bound[fin]).max()):.3f}")
    assert float(ratio) <= 1.0
    if allowed is not None:
        assert bool(((torch.exp(g_).sum(-1) - 1).abs() < 1e-5).all())
    # the same positions as a host-held list
    again = masked_logprobs(model, ids, pos.tolist(), mask_token_id=MASK_ID, allowed_token_ids=allowed)
    assert torch.equal(again, got)


def _variant_pair(ids, g):
    """ref = ids with bases only; alt differs at one position per row (the centre in row 0)."""
    B, Lq = ids.shape
    ref = torch.randint(7, 11, (B, Lq), generator=g)
    alt = ref.clone()
    p = torch.randint(0, Lq, (B,), generator=g)
    p[0] = Lq // 2
    for b in range(B):
        alt[b, p[b]] = 7 + (ref[b, p[b]] - 7 + 1 + b % 3) % 4
    return ref, alt, p


@pytest.mark.parametrize("name", ["ps_fused", "ph_fused", "ps_fused_unidir"])
def test_variant_llr(backend, name):
    _, dev = backend
    model, ids = _golden(name, dev)
    ref, alt, p = _variant_pair(ids.cpu(), torch.Generator().manual_seed(11))
    B = ref.shape[0]
    llr = variant_llr(model, ref.to(dev), alt.to(dev), mask_token_id=MASK_ID, allowed_token_ids=BASES)
    assert llr.shape == (B,) and llr.dtype == torch.float32 and bool(torch.isfinite(llr).all())
    lp = masked_logprobs(model, ref.to(dev), p[:, None].to(dev), mask_token_id=MASK_ID, allowed_token_ids=BASES)[:, 0].cpu()
    ar = torch.arange(B)
    assert torch.equal(llr.cpu(), lp[ar, alt[ar, p]] - lp[ar, ref[ar, p]])
    assert torch.equal(variant_llr(model, ref, alt, mask_token_id=MASK_ID, allowed_token_ids=BASES).cpu(), llr.cpu())  # host-held ids
    if not model.config.rcps:
        return
    # RCPS: the reverse-complemented pair scores the same, within the two calls' bounds at the two bases
    comp = model.lm_head.complement_map.cpu()
    rc = lambda x: comp[x.flip(1)]
    llr_rc = variant_llr(model, rc(ref).to(dev), rc(alt).to(dev), mask_token_id=MASK_ID, allowed_token_ids=BASES)
    mask = _logit_mask(BASES, model.config.vocab_size, dev)
    Lq = ref.shape[1]
    tol = torch.zeros(B, dtype=torch.float64)
    for r, a, q in ((ref, alt, p), (rc(ref), rc(alt), Lq - 1 - p)):
        masked = r.clone().scatter_(1, q[:, None], MASK_ID).to(dev)
        _, bound = _two_kernel_bound(model, masked, q[:, None], mask)
        tol += bound[ar, 0, a[ar, q]] + bound[ar, 0, r[ar, q]]
    d = (llr_rc.double().cpu() - llr.double().cpu()).abs()
    print(f"variant_llr, pair vs reverse complement [{name}]: worst |diff| / bound = {float((d / tol).max()):.3f}, equal bits: "
          f"{torch.equal(llr_rc, llr)}")
    assert bool((d <= tol).all()), (d, tol)


def test_scoring_refusals(backend):
    _, dev = backend
    _, causal = _model(dev)
    ids = torch.randint(7, 11, (2, L), device=dev)
    for over in (dict(bidirectional=True), dict(rcps=True, complement_map={i: i for i in range(12)})):
        other = CaduceusForMaskedLM(CaduceusConfig(**_cfg(**over), pad_token_id=4)).to(dev).eval()
        with pytest.raises(NotImplementedError, match="masked_logprobs"):
            sequence_logprobs(other, ids)
        assert masked_logprobs(other, ids, [[1], [2]], mask_token_id=MASK_ID).shape == (2, 1, 16)
    with pytest.raises(ValueError, match="allowed_token_ids is empty"):
        sequence_logprobs(causal, ids, allowed_token_ids=())
    with pytest.raises(ValueError, match="allowed_token_ids is empty"):
        masked_logprobs(causal, ids, [[1], [2]], mask_token_id=MASK_ID, allowed_token_ids=[])
    with pytest.raises(ValueError, match="must lie in"):
        sequence_logprobs(causal, ids, allowed_token_ids=(7, 16))
    with pytest.raises(ValueError, match="chunk_len"):
        sequence_logprobs(causal, ids, chunk_len=0)
    for bad in ([[0], [L]], [[-1], [0]]):
        with pytest.raises(ValueError, match="positions must lie in"):
            masked_logprobs(causal, ids, bad, mask_token_id=MASK_ID)
    with pytest.raises(ValueError, match="mask_token_id"):
        masked_logprobs(causal, ids, [[0], [1]], mask_token_id=16)
    with pytest.raises(ValueError, match=r"input_ids must lie in \[0, 16\)"):
        sequence_logprobs(causal, ids.cpu() + 9)
    ref = ids.cpu()
    same, two = ref.clone(), ref.clone()
    two[1, 2], two[1, 7] = 7 + (two[1, 2] - 6) % 4, 7 + (two[1, 7] - 6) % 4
    one = ref.clone()
    one[:, 3] = 7 + (one[:, 3] - 6) % 4
    two[0] = one[0]
    with pytest.raises(ValueError, match="exactly one position"):
        variant_llr(causal, ref, same, mask_token_id=MASK_ID)
    with pytest.raises(ValueError, match=r"rows \[1\] differ at \[2\]"):
        variant_llr(causal, ref, two, mask_token_id=MASK_ID)
    # ids already on the device are not read back: such a row scores NaN
    if dev.type != "cpu":
        llr = variant_llr(causal, ref.to(dev), two.to(dev), mask_token_id=MASK_ID)
        assert bool(torch.isfinite(llr[0])) and bool(torch.isnan(llr[1]))
    _, wide = _model(dev, vocab_size=72, tie_word_embeddings=True)
    for call in (lambda: sequence_logprobs(wide, ids), lambda: masked_logprobs(wide, ids, [[0], [1]], mask_token_id=MASK_ID),
                 lambda: variant_llr(wide, ref, one, mask_token_id=MASK_ID)):
        with pytest.raises(ops.ScoreUnsupported, match="vocab_size 72"):
            call()
    _, biased = _model(dev)
    biased.lm_head = torch.nn.Linear(64, 16, bias=True).to(dev)
    with pytest.raises(ops.ScoreUnsupported, match="bias-free"):
        sequence_logprobs(biased, ids)


def test_scoring_is_exported_under_both_package_names():
    import caduceus
    import caduceus_amd
    assert caduceus.scoring is caduceus_amd.scoring and caduceus.variant_llr is caduceus_amd.scoring.variant_llr
    assert {"sequence_logprobs", "masked_logprobs", "variant_llr"} <= set(caduceus_amd.__all__)


@pytest.mark.gpu
def test_masked_logprobs_allocates_no_logits_tensor():
    """P = 3 positions at L = 4096: behind the backbone, masked_logprobs allocates at least B L V 4 bytes less than the same result through
    model(ids).logits, which holds the (B, L, V) fp32 tensor.  (Derived, not measured: the score route's own allocations behind the
    backbone are the row index and (B, P, V) floats; the logits route adds its gather on top of the logits.)  The peak counter is reset as
    the backbone returns -- inside it both routes run the same forward, whose temporaries are far larger than the logits."""
    from caduceus_amd import _lib
    _lib.use_library_for_testing(None)
    dev = torch.device("cuda:0")
    model, _ = _golden("ps_fused", dev)
    B, Lq, V, P = 2, 4096, model.config.vocab_size, 3
    ids = torch.randint(7, 11, (B, Lq), device=dev)
    pos = torch.tensor([[0, 100, Lq - 1], [5, 2048, 4000]], device=dev)
    backbone = model.caduceus.backbone
    inner = backbone.forward_tframe
    mark = {}

    def marked(*a, **k):
        out = inner(*a, **k)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        mark["base"] = torch.cuda.memory_allocated()
        return out
    backbone.forward_tframe = marked
    try:
        def peak(fn):
            out = fn()
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated() - mark["base"], out

        def through_logits():
            with torch.no_grad():
                masked = ids.clone().scatter_(1, pos, MASK_ID)
                z = model(masked).logits.gather(1, pos[:, :, None].expand(B, P, V))
                return torch.log_softmax(z, -1)
        peak(lambda: masked_logprobs(model, ids, pos, mask_token_id=MASK_ID))  # (warm-up: workspaces, caches)
        peak(through_logits)
        p_score, a = peak(lambda: masked_logprobs(model, ids, pos, mask_token_id=MASK_ID))
        p_logits, b = peak(through_logits)
    finally:
        del backbone.forward_tframe
    print(f"peak allocation behind the backbone: masked_logprobs {p_score} B, through .logits {p_logits} B; B L V 4 = {B * Lq * V * 4} B")
    assert p_logits - p_score >= B * Lq * V * 4, (p_logits, p_score)
    assert float((a - b).abs().max()) < 1e-3
