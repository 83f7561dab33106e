"""The whole decode token in one library call (generation.DecodeStack, cad_decode_token) against an fp64 restatement of the stack and
against today's decode_step on the same inputs: logits at every step and both cache states of every layer after the last one; a row
does not depend on its batch; the public generate paths; no allocation per step; refusals.

Bounds (tests/test_mamba_step.py): the fused token at most FACTOR = 1.5 times as far from fp64 as decode_step, and under 6e-4 in fp32.
Bit-identity with decode_step is NOT asserted: the fused token sums a row in cad_add_norm_fwd's order, but the compiler fuses
multiply-adds of the two translations differently, so on gfx950 a row statistic can differ in its last bit (the host emulator, which
does not fuse, gives equal bits).  The test prints whether the logits were equal."""
import pytest
import torch
import torch.nn.functional as F

from caduceus_amd import CaduceusConfig, CaduceusForMaskedLM
from caduceus_amd.generation import DecodeStack, DecodeUnsupported, InferenceParams, decode_step, generate
from caduceus_amd.mamba import fp16_kernels
from conftest import load_golden_model
from test_mamba_step import FACTOR, FP32_BOUND, _ref64

L0, T = 5, 9
# (d_model, d_state, d_conv, rms_norm)
MODELS = [(64, 16, 4, True), (64, 5, 2, False), (40, 16, 2, True), (40, 5, 4, False)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _cfg(d_model=64, d_state=16, d_conv=4, rms=True, **over):
    cfg, _, _ = load_golden_model("ps_fused_unidir")
    cfg = {**cfg, "d_model": d_model, "n_layer": 3, "rms_norm": rms, "rcps": False, "bidirectional": False, "complement_map": None,
           "ssm_cfg": {**cfg["ssm_cfg"], "d_state": d_state, "d_conv": d_conv}}
    return {**cfg, **over}


def _model(dev, d_model=64, d_state=16, d_conv=4, rms=True, seed=0, head_std=None, **over):
    """head_std: an untied head drawn from N(0, head_std^2).  (With the tied head the embedding of the last token dominates the
    residual stream and the model repeats it: fine for error norms, useless where the generated ids are what is compared.)"""
    if head_std is not None:
        over = {**over, "tie_word_embeddings": False}
    cfg = _cfg(d_model, d_state, d_conv, rms, **over)
    torch.manual_seed(seed)
    model = CaduceusForMaskedLM(CaduceusConfig(**cfg, pad_token_id=4))
    with torch.no_grad():  # logits of ~1: an argmax means something; norm parameters off their initial 1 / 0
        model.get_input_embeddings().weight.normal_(std=0.5)
        if head_std is not None:
            assert model.lm_head.weight is not model.get_input_embeddings().weight
            model.lm_head.weight.normal_(std=head_std)
        for n, p in model.named_parameters():
            if "norm" in n:
                p.add_(0.2 * torch.randn_like(p))
    assert model.config.vocab_size == over.get("vocab_size", 16)  # 12 padded to a multiple of 8
    return cfg, model.to(dev).eval()


def _scope(dev, dtype):
    class _S:
        def __enter__(self):
            self.a = torch.autocast(dev.type, dtype=dtype if dtype != torch.float32 else torch.bfloat16, enabled=dtype != torch.float32)
            self.f = fp16_kernels(dtype == torch.float16)
            self.g = torch.no_grad()
            self.g.__enter__(), self.a.__enter__(), self.f.__enter__()

        def __exit__(self, *e):
            self.f.__exit__(*e), self.a.__exit__(*e), self.g.__exit__(*e)
    return _S()


def _stack_ref64(model, seq):
    """fp64 restatement of the causal stack, token by token from empty states: logits (B, L, V) and, per layer, the conv / ssm states
    after the last token."""
    bb = model.caduceus.backbone
    d = lambda p: None if p is None else p.detach().double().cpu()
    hidden = d(bb.embeddings.word_embeddings.weight)[seq.cpu()]
    residual = None

    def norm(x, mod):
        w, b = d(mod.weight), d(getattr(mod, "bias", None))
        if isinstance(mod, torch.nn.LayerNorm):
            return F.layer_norm(x, x.shape[-1:], w, b, mod.eps)
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + mod.eps) * w
    states = []
    for layer in bb.layers:
        residual = hidden if residual is None else hidden + residual
        hidden, convs, ssms = _ref64(layer.mixer.mamba_fwd, norm(residual, layer.norm))
        states.append((convs[-1], ssms[-1]))
    hn = norm(hidden + residual, bb.norm_f)
    return hn @ d(model.lm_head.weight).t(), states


def _err(got, ref):
    return float((got.detach().double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300))


def _run_fused(model, seq, B_cache=None, **step_kw):
    """prefill of seq[:, :L0], then one step per further token of seq (teacher forced): logits (B, T + 1, V) and the stack."""
    stack = DecodeStack(model, B_cache or seq.shape[0])
    logits = [stack.prefill(seq[:, :L0]).clone()]
    for t in range(L0, seq.shape[1]):
        logits.append(stack.step(seq[:, t], **step_kw)[1].clone())
    return torch.stack(logits, 1), stack


def _run_steps(model, seq):
    ip = InferenceParams(max_seqlen=seq.shape[1], max_batch_size=seq.shape[0])
    logits = [decode_step(model, seq[:, :L0], ip)]
    for t in range(L0, seq.shape[1]):
        logits.append(decode_step(model, seq[:, t:t + 1], ip))
    return torch.stack(logits, 1), ip


@pytest.mark.parametrize("B", [1, 3, 9])
@pytest.mark.parametrize("d_model,d_state,d_conv,rms", MODELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_fused_token_against_fp64_and_decode_step(backend, dtype, d_model, d_state, d_conv, rms, B):
    _, dev = backend
    _, model = _model(dev, d_model, d_state, d_conv, rms)
    torch.manual_seed(1)
    seq = torch.randint(7, 11, (B, L0 + T), device=dev)
    ref_logits, ref_states = _stack_ref64(model, seq)
    ref_logits = ref_logits[:, L0 - 1:]
    with _scope(dev, dtype):
        got, stack = _run_fused(model, seq)
        old, ip = _run_steps(model, seq)
    assert got.dtype == torch.float32 and got.shape == (B, T + 1, 16) and stack.act == dtype
    assert stack.inference_params.seqlen_offset == L0 + T
    e_new, e_old = _err(got, ref_logits), _err(old, ref_logits)
    print(f"logits vs fp64 [{dtype}, D={d_model}, N={d_state}, K={d_conv}, rms={rms}, B={B}]: fused {e_new:.3e}  decode_step {e_old:.3e}")
    assert e_new <= FACTOR * e_old, (e_new, e_old)
    if dtype == torch.float32:
        assert e_new <= FP32_BOUND, e_new
    for i, (rc, rs) in enumerate(ref_states):
        conv, ssm = stack.inference_params.key_value_memory_dict[i]
        conv0, ssm0 = ip.key_value_memory_dict[i]
        assert conv.dtype == dtype and ssm.dtype == torch.float32
        ec, ec0, es, es0 = _err(conv[:B], rc), _err(conv0[:B], rc), _err(ssm[:B], rs), _err(ssm0[:B], rs)
        print(f"  layer {i}: conv_state fused {ec:.3e} decode_step {ec0:.3e}   ssm_state fused {es:.3e} decode_step {es0:.3e}")
        assert ec <= FACTOR * ec0 and es <= FACTOR * es0, (i, ec, ec0, es, es0)
        if dtype == torch.float32:
            assert ec <= FP32_BOUND and es <= FP32_BOUND, (i, ec, es)
    print(f"  logits equal to decode_step's bit for bit: {torch.equal(got, old)}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d_model,d_state,d_conv,rms", MODELS)
def test_rows_are_independent(backend, dtype, d_model, d_state, d_conv, rms):
    """Row r of a B = 9 call equals the same row run alone at B = 1 with row_offset = r: logits and sampled ids, bit for bit."""
    _, dev = backend
    _, model = _model(dev, d_model, d_state, d_conv, rms)
    torch.manual_seed(2)
    seq = torch.randint(7, 11, (9, L0 + T), device=dev)
    kw = dict(top_k=0, top_p=0.9, temperature=0.8, seed=1234, allowed_token_ids=(7, 8, 9, 10, 11))
    with _scope(dev, dtype):
        stack = DecodeStack(model, 9)
        stack.prefill(seq[:, :L0], **kw)
        ids, logits, us = [stack.next_ids.clone()], [], [stack.uniforms.clone()]
        for t in range(L0, L0 + T):
            i, l = stack.step(seq[:, t], **kw)
            ids.append(i.clone()), logits.append(l.clone()), us.append(stack.uniforms.clone())
        one = DecodeStack(model, 1)
        for r in range(9):
            one.prefill(seq[r:r + 1, :L0], row_offset=r, **kw)
            assert torch.equal(one.next_ids, ids[0][r:r + 1]) and torch.equal(one.uniforms, us[0][r:r + 1])
            for k, t in enumerate(range(L0, L0 + T)):
                i, l = one.step(seq[r:r + 1, t], row_offset=r, **kw)
                assert torch.equal(l, logits[k][r:r + 1]), (r, t)
                assert torch.equal(i, ids[k + 1][r:r + 1]) and torch.equal(one.uniforms, us[k + 1][r:r + 1]), (r, t)
    all_ids = torch.stack(ids, 1)
    assert int(all_ids.min()) >= 7 and int(all_ids.max()) <= 11
    assert len(set(torch.stack(us, 1).flatten().tolist())) == 9 * (T + 1)  # every (row, position) its own uniform


# Weights for the tests that compare generated ids: an untied head, and per model a seed at which the greedy continuation of every row
# changes its token and no argmax margin of the fp32 logits is small (both asserted below, not assumed).
ID_MODELS = [(m, seed) for m, seed in zip(MODELS, (11, 5, 7, 9))]
ID_MODEL_IDS = [f"D{m[0]}-N{m[1]}-K{m[2]}-{'rms' if m[3] else 'ln'}" for m in MODELS]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("m,seed", ID_MODELS, ids=ID_MODEL_IDS)
def test_greedy_generate_fused_equals_the_loop(backend, dtype, m, seed):
    """generate(..., fused=True) returns the ids of generate(...); no argmax margin of the fp32 logits is below 1e-3, and the ids are not
    a repeat of one token (a step fed a stale id, or written to the wrong position, changes them)."""
    _, dev = backend
    _, model = _model(dev, *m, seed=seed, head_std=0.5)
    torch.manual_seed(4)
    prompt = torch.randint(7, 11, (3, L0)).to(dev)  # (drawn on the host: the seeds were chosen for these prompts)
    with _scope(dev, torch.float32):
        ref_ids, ref_logits = generate(model, prompt, T, return_logits=True)
    top2 = torch.stack(ref_logits, 1).topk(2, dim=-1).values
    margin = float((top2[..., 0] - top2[..., 1]).min())
    print(f"smallest argmax margin of the fp32 logits: {margin:.3e}; new ids {ref_ids[:, L0:].tolist()}")
    assert margin >= 1e-3, margin
    with _scope(dev, dtype):
        ids0, logits0 = generate(model, prompt, T, return_logits=True)
        ids1, logits1 = generate(model, prompt, T, return_logits=True, fused=True)
        ids2 = generate(model, prompt, T, fused=False)
    for row in ids0[:, L0:].tolist():
        assert len(set(row)) >= 3 and any(a != b for a, b in zip(row, row[1:])), row
    assert ids1.shape == (3, L0 + T) and ids1.dtype == prompt.dtype and torch.equal(ids1[:, :L0], prompt)
    assert torch.equal(ids1, ids0) and torch.equal(ids2, ids0)
    assert len(logits1) == T and all(torch.equal(l.argmax(-1), ids1[:, L0 + t]) for t, l in enumerate(logits1))


@pytest.mark.parametrize("B", [3, 9])
@pytest.mark.parametrize("m,seed", ID_MODELS, ids=ID_MODEL_IDS)
def test_sampled_generate_fused_equals_the_loop(backend, m, seed, B):
    """fp32, one seed: generate(..., fused=True) samples the ids the decode_step loop with the sampler as its own launch (fused=False)
    samples -- the prefill's token at position L0 and step t's at L0 + t carry the loop's uniforms, and each step consumes the id the
    step before it sampled.  (The two paths' logits differ by rounding; a uniform within that of a CDF edge would flip an id: ~1e-6
    per token.)"""
    _, dev = backend
    _, model = _model(dev, *m, seed=seed, head_std=0.5)
    torch.manual_seed(7)
    prompt = torch.randint(7, 11, (B, L0)).to(dev)
    kw = dict(top_k=0, top_p=0.95, temperature=2.0, seed=99, allowed_token_ids=(7, 8, 9, 10))
    with _scope(dev, torch.float32):
        ids_f, logits_f = generate(model, prompt, T, return_logits=True, fused=True, **kw)
        ids_l, logits_l = generate(model, prompt, T, return_logits=True, fused=False, **kw)
        greedy = generate(model, prompt, T, fused=True, allowed_token_ids=(7, 8, 9, 10))
    print(f"sampled new ids {ids_f[:, L0:].tolist()}")
    assert torch.equal(ids_f, ids_l)
    for row in ids_f[:, L0:].tolist():
        assert 7 <= min(row) and max(row) <= 10 and len(set(row)) >= 2, row
    assert not torch.equal(ids_f, greedy)  # (the uniforms were used)
    for a, b in zip(logits_f, logits_l):  # the same trajectory: each path within FP32_BOUND of fp64, so within twice that of the other
        assert _err(a, b.double().cpu()) <= 2 * FP32_BOUND


def test_eos_rows_keep_emitting_eos_and_sampling_is_keyed_by_the_seed(backend):
    _, dev = backend
    _, model = _model(dev, seed=5)
    torch.manual_seed(6)
    prompt = torch.randint(7, 11, (9, L0), device=dev)
    kw = dict(top_k=0, temperature=20.0, allowed_token_ids=(7, 8, 9, 10))  # (flat enough for every base to appear)
    a = generate(model, prompt, 24, seed=11, **kw)
    b = generate(model, prompt, 24, seed=11, **kw)
    c = generate(model, prompt, 24, seed=12, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    new = a[:, L0:]
    assert int(new.min()) >= 7 and int(new.max()) <= 10 and len(new.unique()) > 1
    e = generate(model, prompt, 24, seed=11, eos_token_id=8, **kw)[:, L0:]
    for row_e, row_a in zip(e.tolist(), new.tolist()):
        if 8 in row_a:
            k = row_a.index(8)
            assert row_e[:k + 1] == row_a[:k + 1] and all(v == 8 for v in row_e[k:])
        else:
            assert row_e == row_a
    assert any(8 in r for r in new.tolist())
    torch.manual_seed(0)
    d = generate(model, prompt, 8, top_k=4)  # seed=None: drawn from torch's default generator
    torch.manual_seed(0)
    assert torch.equal(d, generate(model, prompt, 8, top_k=4))


def test_logit_masks_kept_by_the_stack_are_bounded(backend):
    _, dev = backend
    _, model = _model(dev)
    stack = DecodeStack(model, 2)
    stack.prefill(torch.randint(7, 11, (2, L0), device=dev))
    for k in range(2 * DecodeStack.MAX_MASKS):
        allowed = (7, 8 + k % 3, k % 7, 11 + k % 5)
        ids, _ = stack.step(top_k=0, seed=k, allowed_token_ids=allowed)
        assert set(ids.tolist()) <= set(allowed)
        assert len(stack._masks) <= DecodeStack.MAX_MASKS


@pytest.mark.gpu
def test_steps_do_not_allocate():
    dev = torch.device("cuda:0")
    _, model = _model(dev)
    prompt = torch.randint(7, 11, (3, L0), device=dev)
    stack = DecodeStack(model, 3)
    stack.prefill(prompt, top_k=4, seed=1)
    stack.step(top_k=4, seed=1, allowed_token_ids=(7, 8, 9, 10))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for _ in range(50):
        stack.step(top_k=4, seed=1, allowed_token_ids=(7, 8, 9, 10))
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert stack.inference_params.seqlen_offset == L0 + 51 and bool(torch.isfinite(stack.step()[1]).all())


@pytest.mark.parametrize("over", [dict(bidirectional=True), dict(rcps=True, complement_map={i: i for i in range(12)}),
                                  dict(bidirectional=True, rcps=True, complement_map={i: i for i in range(12)})],
                         ids=["bidirectional", "rcps", "caduceus_ps"])
def test_stacks_without_a_stepwise_form_are_refused(over):
    cfg = _cfg(**over)
    model = CaduceusForMaskedLM(CaduceusConfig(**cfg, pad_token_id=4)).eval()
    with pytest.raises(NotImplementedError, match="right-to-left direction has no step-wise form"):
        DecodeStack(model, 2)
    with pytest.raises(NotImplementedError, match="right-to-left direction has no step-wise form"):
        generate(model, torch.randint(7, 11, (2, 4)), 3, fused=True)


def test_unsupported_heads_and_replaced_parameters_are_refused(backend):
    _, dev = backend
    _, model = _model(dev)
    stack = DecodeStack(model, 2)
    prompt = torch.randint(7, 11, (2, L0), device=dev)
    stack.prefill(prompt)
    with pytest.raises(ValueError, match="holds 2 rows"):
        stack.prefill(torch.randint(7, 11, (3, L0), device=dev))
    m0 = model.caduceus.backbone.layers[1].mixer.mamba_fwd
    m0.x_proj.weight = torch.nn.Parameter(m0.x_proj.weight.detach().clone())
    with pytest.raises(RuntimeError, match=r"1\.W_x was replaced.*needs a new DecodeStack"):
        stack.prefill(prompt)
    DecodeStack(model, 2).prefill(prompt)  # a new stack picks the new tensor up
    _, biased = _model(dev)
    biased.lm_head = torch.nn.Linear(64, 16, bias=True).to(dev)
    with pytest.raises(DecodeUnsupported, match="bias-free"):
        DecodeStack(biased, 2)
    with pytest.raises(ValueError):
        generate(biased, prompt, 2, fused=True)
    _, wide = _model(dev, vocab_size=72, tie_word_embeddings=True)
    assert wide.config.vocab_size == 72
    with pytest.raises(DecodeUnsupported, match="vocab_size 72"):
        DecodeStack(wide, 2)
    # such a model keeps the loop and samples through ops.sample_tokens' restatement in torch ops
    ids = generate(wide, prompt, 4, top_k=5, seed=3, allowed_token_ids=(7, 8, 9, 10, 70))
    assert ids.shape == (2, L0 + 4) and set(ids[:, L0:].flatten().tolist()) <= {7, 8, 9, 10, 70}
    assert torch.equal(ids, generate(wide, prompt, 4, top_k=5, seed=3, allowed_token_ids=(7, 8, 9, 10, 70), fused=False))
    half = _model(dev)[1].to(torch.bfloat16)
    with pytest.raises(DecodeUnsupported, match="float32 master"):
        DecodeStack(half, 2)
