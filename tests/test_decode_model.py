"""Step-wise decoding at model level: a causal stack (bidirectional=False, rcps=False) through prefill + decode_step and through
generate against the fp64 oracle model, by the rule of test_mamba_step.py (the cache path at most 1.5 times as far from fp64 as the
one-piece forward in bf16; both under the project's 6e-4 in fp32); bi-directional and RCPS stacks keep raising; the paths without
`inference_params` compute what they computed before (recorded logits, bit for bit)."""
import os

import numpy as np
import pytest
import torch

from caduceus_amd import CaduceusConfig, CaduceusForMaskedLM
from caduceus_amd.generation import InferenceParams, decode_step, generate
from conftest import GOLDEN, load_golden_model
from oracle import oracle_model as om
from test_mamba_step import FACTOR, FP32_BOUND

COMP = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 10, 8: 9, 9: 8, 10: 7, 11: 11}


def _cfg(**over):
    cfg, _, _ = load_golden_model("ps_fused_unidir")
    return {**cfg, "d_model": 64, "n_layer": 2, **over}


def _causal_model(dev, fused, seed=0):
    cfg = _cfg(rcps=False, bidirectional=False, complement_map=None, fused_add_norm=fused)
    torch.manual_seed(seed)
    model = CaduceusForMaskedLM(CaduceusConfig(**cfg, pad_token_id=4))
    with torch.no_grad():  # (the default initialisation leaves logits of ~1e-2: spread them so that an argmax means something)
        model.get_input_embeddings().weight.normal_(std=0.5)
    return cfg, model.to(dev).eval()


def _err(got, ref):
    return float((got.double().cpu() - ref.double()).norm() / ref.double().norm())


@pytest.mark.parametrize("fused", [True, False], ids=["fused_add_norm", "unfused"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_causal_stack_three_ways(backend, dtype, fused):
    """Logits of a 24-token sequence (an 8-token prefix and its greedy continuation): one forward; a prefill of 8 and 16 decode_steps
    in a cache of 4 rows; generate's own path from the same prefix.  Each against the fp64 oracle model, the one-piece forward's own
    error being the yardstick."""
    _, dev = backend
    cfg, model = _causal_model(dev, fused)
    B, L0, T = 3, 8, 16
    torch.manual_seed(1)
    prefix = torch.randint(7, 11, (B, L0), device=dev)
    scope = torch.autocast(dev.type, dtype=torch.bfloat16, enabled=dtype == torch.bfloat16)
    with torch.no_grad(), scope:
        seq, gen_logits = generate(model, prefix, T, return_logits=True)
        assert seq.shape == (B, L0 + T) and torch.equal(seq[:, :L0], prefix)
        one = model(seq).logits
        ip = InferenceParams(max_seqlen=L0 + T, max_batch_size=4)
        stepped = [decode_step(model, seq[:, :L0], ip)]
        assert ip.seqlen_offset == L0
        for t in range(L0, L0 + T):
            stepped.append(decode_step(model, seq[:, t:t + 1], ip))
        assert ip.seqlen_offset == L0 + T and sorted(ip.key_value_memory_dict) == [0, 1]
        assert all(c.shape[0] == 4 and s.shape[0] == 4 and s.dtype == torch.float32 for c, s in ip.key_value_memory_dict.values())
    stepped = torch.stack(stepped, 1)        # positions L0 - 1 .. L0 + T - 1
    gen_logits = torch.stack(gen_logits, 1)  # positions L0 - 1 .. L0 + T - 2
    assert stepped.dtype == torch.float32 and stepped.shape == (B, T + 1, one.shape[-1])
    sd64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}
    ref = om.masked_lm_forward(sd64, seq.cpu(), cfg)["logits"]
    e_one = _err(one[:, L0 - 1:], ref[:, L0 - 1:])
    e_step = _err(stepped, ref[:, L0 - 1:])
    e_gen = _err(gen_logits, ref[:, L0 - 1:-1])
    e_one_gen = _err(one[:, L0 - 1:-1], ref[:, L0 - 1:-1])
    print(f"logits vs fp64 oracle [{dtype}, fused={fused}]: one piece {e_one:.3e}  prefill + steps {e_step:.3e}  generate {e_gen:.3e}")
    if dtype == torch.float32:
        assert max(e_one, e_step, e_gen) <= FP32_BOUND, (e_one, e_step, e_gen)
    else:
        assert e_step <= FACTOR * e_one and e_gen <= FACTOR * e_one_gen, (e_one, e_step, e_gen, e_one_gen)
    assert torch.equal(gen_logits, stepped[:, :-1])  # the same launches on the same operands


def test_generate_starts_at_the_forward_s_argmax(backend):
    """generate returns (B, L0 + max_new_tokens) ids that begin with the prompt; the first new token is the argmax of the one-piece
    forward's logits at the prompt's last position."""
    _, dev = backend
    _, model = _causal_model(dev, True, seed=2)
    torch.manual_seed(3)
    prompt = torch.randint(7, 11, (3, 7), device=dev)
    with torch.no_grad():
        ids = generate(model, prompt, 5)
        last = model(prompt).logits[:, -1]
    assert ids.shape == (3, 12) and ids.dtype == prompt.dtype and torch.equal(ids[:, :7], prompt)
    top2 = last.topk(2, dim=-1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-3 * float(last.abs().max())  # no near-tie decides this test
    assert torch.equal(ids[:, 7], last.argmax(-1))


@pytest.mark.parametrize("over", [dict(bidirectional=True, rcps=False, complement_map=None), dict(bidirectional=False, rcps=True),
                                  dict(bidirectional=True, rcps=True)], ids=["bidirectional", "rcps", "caduceus_ps"])
def test_stacks_with_a_right_to_left_direction_keep_raising(over):
    """Every entry to the cache raises NotImplementedError and names the reason; no kernel is reached (no backend needed)."""
    model = CaduceusForMaskedLM(CaduceusConfig(**_cfg(**over), pad_token_id=4)).eval()
    backbone = model.caduceus.backbone
    ids = torch.randint(7, 11, (2, 4))
    ip = InferenceParams(max_seqlen=8, max_batch_size=2)
    why = "right-to-left direction has no step-wise form"
    with pytest.raises(NotImplementedError, match=why):
        backbone(ids, inference_params=ip)
    with pytest.raises(NotImplementedError, match=why):
        backbone.allocate_inference_cache(2, 8)
    with pytest.raises(NotImplementedError, match=why):
        decode_step(model, ids, ip)
    layer = backbone.layers[0]
    with pytest.raises(NotImplementedError, match=why):
        layer.allocate_inference_cache(2, 8)
    width = 64 * (2 if over["rcps"] else 1)
    with pytest.raises(NotImplementedError, match=why):
        layer(torch.zeros(2, 4, width), None, inference_params=ip)
    with pytest.raises(NotImplementedError, match=why):
        layer.mixer(torch.zeros(2, 4, width), inference_params=ip)
    assert ip.key_value_memory_dict == {} and ip.seqlen_offset == 0


def test_causal_cache_surface(backend):
    """allocate_inference_cache of the model, a block and a mixer: upstream's shapes, {layer_idx: states} at model level."""
    _, dev = backend
    _, model = _causal_model(dev, True)
    backbone = model.caduceus.backbone
    cache = backbone.allocate_inference_cache(3, 32, dtype=torch.bfloat16)
    assert sorted(cache) == [0, 1]
    for conv, ssm in cache.values():
        assert conv.shape == (3, 128, 4) and conv.dtype == torch.bfloat16 and ssm.shape == (3, 128, 16) and ssm.dtype == torch.float32
        assert conv.device.type == dev.type and not conv.any() and not ssm.any()
    conv, ssm = backbone.layers[1].allocate_inference_cache(2, 32)
    assert conv.shape == (2, 128, 4) and conv.dtype == torch.float32 and ssm.shape == (2, 128, 16)
    # the backbone's forward takes the cache as its trailing argument and returns what the one-piece forward returns, position by position
    ids = torch.randint(7, 11, (2, 6), device=dev)
    ip = InferenceParams(max_seqlen=8, max_batch_size=2)
    with torch.no_grad():
        full, _ = backbone(ids)
        head, hs = backbone(ids[:, :5], None, False, ip)
        ip.seqlen_offset += 5
        tail, _ = backbone(ids[:, 5:], inference_params=ip)
    assert hs == [] and head.shape == (2, 5, 64) and tail.shape == (2, 1, 64)
    assert float((torch.cat([head, tail], 1) - full).abs().max()) <= FP32_BOUND * float(full.abs().max())


def test_paths_without_a_cache_compute_what_they_did(backend):
    """The ps_fused_unidir golden variant (uni-directional mixers under RCPS) with inference_params=None: logits bit-identical to
    those recorded on this backend before the cache existed (tests/golden/decode_untouched_unidir_<backend>.npy).  Guards the
    refactored paths (Mamba.forward, Block.forward, the LM-head call); passes before and after."""
    name, dev = backend
    cfg, sd, rec = load_golden_model("ps_fused_unidir")
    model = CaduceusForMaskedLM(CaduceusConfig(**cfg, pad_token_id=4))
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    with torch.no_grad():
        logits = model(rec["input_ids"].to(dev)).logits.cpu()
    assert float((logits - rec["logits"]).abs().max()) < 2e-3  # (the reference's own logits, as __graft_entry__.smoke holds them)
    recorded = torch.from_numpy(np.load(os.path.join(GOLDEN, f"decode_untouched_unidir_{name}.npy")))
    assert torch.equal(logits, recorded)
