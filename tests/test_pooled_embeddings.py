"""caduceus_amd.pooled_embeddings and its consumers on the golden RCPS (ps) and post-hoc (ph) weights, fused and un-fused norm variants,
fp32 and bf16: against float64 pooling of the pre-norm tensors the backbone's layer loop returns (the bounds of tests/test_pool_head.py,
whose header derives them), against today's route through model.caduceus(ids) (whose normed rows are cad_add_norm_fwd's, within tol_y
of the same float64 rows: that bound plus the pooled tol_y), reverse-complement equivariance, the VEP and classification consumers, and,
on the GPU, that nothing is read back and that the final (S, B, L, D) activation is never allocated.

Frames: an RCPS result (B, D, 2) is the t-frame's (2, B, D) with strand 1 pooled in its own position order -- "first" and "last"
exchange roles there and a window centre c becomes L - 1 - c."""
import pytest
import torch

from caduceus_amd import (CaduceusForSequenceClassification, DNAEmbeddingModelCaduceus, CaduceusConfig, ops, pooled_embeddings, vep)
from conftest import load_golden_model
from test_norm_head_fp64 import F32, gam, hold
from test_pool_head import pool_reference, rows_reference, window_index
from test_scoring import _golden

BF = torch.bfloat16
NAMES = ["ps_fused", "ps_unfused", "ph_fused", "ph_unfused"]
LQ = 45
POOLINGS = [("mean", {}), ("max", {}), ("first", {}), ("last", {}), ("window", dict(window_tokens=6))]
CENTRES = [0, LQ - 1, 20]


def model_of(name, dev, dtype):
    model, _ = _golden(name, dev)
    return model.to(dtype) if dtype != F32 else model


def input_ids(B, Lq, dev, seed=0):
    return torch.randint(7, 11, (B, Lq), generator=torch.Generator().manual_seed(seed)).to(dev)


def tframe_request(pooling, S, B, Lq, centre, kw):
    """(mode, centre (S, B), half) in the t-frame for a pooling named in the forward frame (restated here, not imported)."""
    if pooling in ("mean", "max"):
        return pooling, None, 0
    if pooling == "window":
        c, half = centre.cpu(), kw["window_tokens"] // 2
    else:
        c, half = torch.full((B,), 0 if pooling == "first" else Lq - 1, dtype=torch.int64), 0
    return "window", torch.stack([c, Lq - 1 - c][:S], 0), half


def pooled_tol_y(tol_y, mode, centre, half):
    """What a perturbation of every row by tol_y moves the pooled value by."""
    if mode == "max":
        return tol_y.max(2).values
    if mode == "window":
        S, B, Lq, D = tol_y.shape
        tol_y = tol_y.gather(2, window_index(centre, half, Lq).unsqueeze(-1).expand(S, B, 2 * half + 1, D))
    return tol_y.mean(2)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_pooled_embeddings_against_fp64_and_todays_route(backend, name, dtype):
    bname, dev = backend
    model = model_of(name, dev, dtype)
    backbone = model.caduceus.backbone
    B = 3
    ids = input_ids(B, LQ, dev)
    centre = torch.tensor(CENTRES, device=dev)
    with torch.no_grad():
        hidden, residual, act = backbone.layers_tframe(ids)
        w, b, eps, is_rms = backbone._final_norm_params()
        # the split left forward_tframe's bits alone: it is the helper plus ops.add_norm
        want, _ = ops.add_norm(hidden, residual, w, b, eps, is_rms, False, act)
        assert torch.equal(backbone.forward_tframe(ids), want) and act == dtype
        today = model.caduceus(ids, return_dict=False).double().cpu()  # (B, L, D | 2 D)
    S, D = hidden.shape[0], hidden.shape[-1]
    assert S == (2 if model.config.rcps else 1) and today.shape[-1] == S * D
    if S == 2:  # DNAEmbeddingModelCaduceus' frame, then back to t-frame rows: strand 1 un-flipped in channels, positions reversed twice
        emb = DNAEmbeddingModelCaduceus(model.config)
        emb.caduceus = model.caduceus
        with torch.no_grad():
            stacked = emb(ids)[0].double().cpu()  # (B, L, D, 2)
        assert torch.equal(stacked[..., 1], today[..., D:].flip(1, 2))
        today_t = torch.stack([stacked[..., 0], stacked[..., 1].flip(1)], 0)
    else:
        today_t = today.unsqueeze(0)
    y, tol_y = rows_reference(hidden.cpu(), None if residual is None else residual.cpu(), w.detach().float().cpu(),
                              None if b is None else b.detach().float().cpu(), is_rms, act, eps)
    for pooling, kw in POOLINGS:
        args = dict(kw, centre=centre) if pooling == "window" else kw
        out = pooled_embeddings(model, ids, pooling, **args)
        assert out.dtype == F32 and out.shape == ((B, D, 2) if S == 2 else (B, D))
        out_t = out.permute(2, 0, 1) if S == 2 else out.unsqueeze(0)
        mode, cen, half = tframe_request(pooling, S, B, LQ, centre, kw)
        ref, tol = pool_reference(y, tol_y, mode, cen, half)
        hold(bname, f"embed-{pooling}", out_t, ref, tol, F32)
        ref2, _ = pool_reference(today_t, torch.zeros_like(today_t), mode, cen, half)
        hold(bname, f"embed-today-{pooling}", out_t, ref2, tol + pooled_tol_y(tol_y, mode, cen, half), F32)
    for m in (model.caduceus, model):
        assert torch.equal(pooled_embeddings(m, ids, "mean"), pooled_embeddings(model, ids, "mean"))
    with pytest.raises(TypeError):
        pooled_embeddings(backbone, ids, "mean")
    with pytest.raises(NotImplementedError):
        pooled_embeddings(model, ids, "median")
    with pytest.raises(ops.PoolUnsupported):
        pooled_embeddings(model, ids, "window", centre=centre, window_tokens=5)
    with pytest.raises(ValueError):
        pooled_embeddings(model, ids, "mean", window_tokens=4)


def test_rcps_result_is_rc_equivariant_bit_for_bit(backend):
    """Reverse-complemented input exchanges [..., 0] and [..., 1] (fp32), for the same pooling and the same centres: both channels are
    in the forward frame.  In the t-frame the exchanged strand's rows arrive in the opposite order, which the head's sums do not see."""
    _, dev = backend
    model, _ = _golden("ps_fused", dev)
    ids = input_ids(2, LQ, dev, seed=3)
    comp = torch.tensor([model.config.complement_map[i] for i in range(model.config.vocab_size)], device=dev)
    rc = comp[ids.flip(-1)]
    centre = torch.tensor([4, LQ - 2], device=dev)
    for pooling, kw in POOLINGS:
        args = dict(kw, centre=centre) if pooling == "window" else kw
        a, b = pooled_embeddings(model, ids, pooling, **args), pooled_embeddings(model, rc, pooling, **args)
        assert torch.equal(a[..., 0], b[..., 1]) and torch.equal(a[..., 1], b[..., 0]), pooling
        assert not torch.equal(a[..., 0], a[..., 1])


@pytest.mark.parametrize("name", ["ps_fused", "ph_fused"])
def test_embed_variants_fused_against_unfused(backend, name):
    """Window 1536 at L 2048, variants at 0, L - 1 and L // 2.  The fused route is held to the fp64 window mean of the fp64 rows with
    the pool head's bound.  Today's route pools cad_add_norm_fwd's rows (within tol_y of the same fp64 rows) with an fp32 mean of n terms
    -- n - 1 additions in whatever order and one division: the same bound.  So the two routes lie within twice the bound of each other.
    (Today's hidden states are formed once, from the layer loop's outputs, and handed to embed_variants as its backbone: forward_tframe
    is that add_norm, bit for bit -- test_pooled_embeddings_against_fp64_and_todays_route.)"""
    from caduceus_amd import engine
    bname, dev = backend
    model, _ = _golden(name, dev)
    rcps = bool(model.config.rcps)
    backbone = model.caduceus.backbone
    Lq, B = 2048, 3
    g = torch.Generator().manual_seed(8)
    batch = {k: torch.randint(7, 11, (B, Lq), generator=g).to(dev) for k in ("ref_input_ids", "alt_input_ids", "ref_rc_input_ids",
                                                                              "alt_rc_input_ids")}
    v = torch.tensor([0, Lq - 1, Lq // 2])
    batch["variant_idx"] = v.to(dev)
    order = ["alt_input_ids", "ref_input_ids"] + ([] if rcps else ["alt_rc_input_ids", "ref_rc_input_ids"])
    stacked = torch.cat([batch[k] for k in order], 0)
    with torch.no_grad():
        hidden, residual, act = backbone.layers_tframe(stacked)
        w, b, eps, is_rms = backbone._final_norm_params()
        today = engine.from_tframe(ops.add_norm(hidden, residual, w, b, eps, is_rms, False, act)[0])
    seen = []
    plain = vep.embed_variants(lambda ids: (seen.append(ids), today)[1], batch, rcps, autocast_dtype=None)
    assert len(seen) == 1 and torch.equal(seen[0], stacked)
    fused = vep.embed_variants(model, batch, rcps, autocast_dtype=None, fused=True)
    y, tol_y = rows_reference(hidden.cpu(), None if residual is None else residual.cpu(), w.detach().float().cpu(),
                              None if b is None else b.detach().float().cpu(), is_rms, act, eps)
    half = vep.WINDOW_SIZE_BP // 2
    cen = torch.stack([torch.cat([v, v]), Lq - 1 - torch.cat([v, v])], 0) if rcps else torch.cat([v, v, Lq - 1 - v, Lq - 1 - v]).unsqueeze(0)
    ref, tol = pool_reference(y, tol_y, "window", cen, half)  # t-frame (S, NB, D)
    if rcps:
        parts = {"concat_avg_ws": [(ref[0, B:], tol[0, B:]), (ref[0, :B], tol[0, :B])],
                 "rc_concat_avg_ws": [(ref[1, B:], tol[1, B:]), (ref[1, :B], tol[1, :B])]}
    else:
        parts = {"concat_avg_ws": [(ref[0, B:2 * B], tol[0, B:2 * B]), (ref[0, :B], tol[0, :B])],
                 "rc_concat_avg_ws": [(ref[0, 3 * B:], tol[0, 3 * B:]), (ref[0, 2 * B:3 * B], tol[0, 2 * B:3 * B])]}
    for k, pair in parts.items():
        r, t = torch.cat([p[0] for p in pair], -1), torch.cat([p[1] for p in pair], -1)
        assert fused[k].shape == plain[k].shape == r.shape and fused[k].dtype == F32
        hold(bname, f"vep-fused-{k}", fused[k], r, t, F32)
        hold(bname, f"vep-fused-vs-plain-{k}", fused[k], plain[k].double().cpu(), 2 * t, F32)
    with pytest.raises(TypeError):
        vep.embed_variants(lambda ids: today, batch, rcps, autocast_dtype=None, fused=True)
    out = vep.dump_embeddings(model, {k: t.cpu() for k, t in batch.items()}, rcps, batch_size=3, autocast_dtype=None, fused=True)
    assert torch.equal(out["concat_avg_ws"], fused["concat_avg_ws"].cpu())


@pytest.mark.parametrize("conjoin", [False, True], ids=["plain", "conjoin"])
@pytest.mark.parametrize("pooling", ["mean", "max", "first", "last"])
def test_classification_fused_pool_against_unfused(backend, pooling, conjoin):
    """Logits of fused_pool=True against fused_pool=False on the same weights: RCPS (two strands, first <-> last on the second) and
    post-hoc conjoining (one batch of 2 B); with grad enabled the fused model takes today's path, bit for bit."""
    _, dev = backend
    for name in (["ph_fused"] if conjoin else ["ps_fused", "ph_unfused"]):
        cfg, sd, _ = load_golden_model(name)
        config = CaduceusConfig(**cfg, num_labels=3)
        torch.manual_seed(2)
        plain = CaduceusForSequenceClassification(config, pooling_strategy=pooling, conjoin_eval=conjoin)
        plain.caduceus.load_state_dict({k[len("caduceus."):]: v for k, v in sd.items() if k.startswith("caduceus.")}, strict=True)
        fused = CaduceusForSequenceClassification(config, pooling_strategy=pooling, conjoin_eval=conjoin, fused_pool=True)
        fused.load_state_dict(plain.state_dict(), strict=True)
        plain, fused = plain.to(dev).eval(), fused.to(dev).eval()
        ids = input_ids(2, LQ, dev, seed=5)
        if conjoin:
            ids = torch.stack([ids, input_ids(2, LQ, dev, seed=6)], -1)
        with torch.no_grad():
            a, b = plain(ids).logits, fused(ids).logits
            flat = torch.cat([ids[..., 0], ids[..., 1]], 0) if conjoin else ids
            hidden, residual, act = plain.caduceus.backbone.layers_tframe(flat)
            w, nb, eps, is_rms = plain.caduceus.backbone._final_norm_params()
        assert a.shape == b.shape == (2, 3)
        # Both routes pool the same fp64 rows within the pool head's bound `tol` (today's: cad_add_norm_fwd's rows, then an fp32 mean of
        # L terms, an exact max or an exact select), so the pooled vectors lie within 2 tol of each other; the score layer is a K x D
        # fp32 product on either side (g(D + 2) each, relative to sum |W| (|pooled| + tol)); the strand average adds three roundings.
        y, tol_y = rows_reference(hidden.cpu(), None if residual is None else residual.cpu(), w.detach().float().cpu(),
                                  None if nb is None else nb.detach().float().cpu(), is_rms, act, eps)
        S, NB, D = y.shape[0], y.shape[1], y.shape[-1]
        mode, cen, half = tframe_request(pooling, S, NB, LQ, None, {})
        ref, tol = pool_reference(y, tol_y, mode, cen, half)
        Wabs = plain.score.weight.detach().double().abs().cpu()
        per = (2 * tol + 2 * gam(D + 2) * (ref.abs() + tol)) @ Wabs.t()  # (S, NB, K)
        per = per.reshape(-1, 2, 3).sum(0) / 2  # the two strands (RCPS) or the two inputs (conjoin: rows B apart), or one
        if S == 1 and not conjoin:
            per = 2 * per
        hold("emu" if dev.type == "cpu" else "hip", f"classify-{pooling}", b, a.double().cpu(), per + gam(3) * a.double().abs().cpu(), F32)
        assert torch.equal(fused(ids).logits, plain(ids).logits)  # grad mode on: today's path
        assert fused(ids, output_hidden_states=True).hidden_states is not None


@pytest.mark.gpu
def test_pooled_embeddings_reads_nothing_back():
    from caduceus_amd import _lib
    _lib.use_library_for_testing(None)
    dev = torch.device("cuda:0")
    for name in ("ps_fused", "ph_fused"):
        model, _ = _golden(name, dev)
        ids = input_ids(2, 256, dev)
        centre = torch.tensor([3, 250], device=dev)
        want = [pooled_embeddings(model, ids, p, **(dict(kw, centre=centre) if p == "window" else kw)) for p, kw in POOLINGS]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = [pooled_embeddings(model, ids, p, **(dict(kw, centre=centre) if p == "window" else kw)) for p, kw in POOLINGS]
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
def test_pooled_embeddings_never_allocates_the_final_activation():
    """L = 4096: behind the layer loop the pooled route's peak lies below the route through model.caduceus(ids) by at least the bytes of
    the final (S, B, L, D) activation (that route also holds the fp32 residual copy, rstd and the strand concatenation; the pooled route
    holds the partials and (S, B, D)).  The peak counter is reset as the layer loop returns -- both routes run the same loop."""
    from caduceus_amd import _lib
    _lib.use_library_for_testing(None)
    dev = torch.device("cuda:0")
    model, _ = _golden("ps_fused", dev)
    backbone = model.caduceus.backbone
    B, Lq = 2, 4096
    ids = input_ids(B, Lq, dev)
    inner = backbone.layers_tframe
    mark = {}

    def marked(*a, **k):
        out = inner(*a, **k)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        mark["base"] = torch.cuda.memory_allocated()
        return out
    backbone.layers_tframe = marked
    try:
        def peak(fn):
            out = fn()
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated() - mark["base"], out

        def through_hidden():
            with torch.no_grad():
                return model.caduceus(ids, return_dict=False).mean(1)
        peak(lambda: pooled_embeddings(model, ids, "mean"))  # (warm-up: workspaces, caches)
        peak(through_hidden)
        p_pool, a = peak(lambda: pooled_embeddings(model, ids, "mean"))
        p_hidden, b = peak(through_hidden)
    finally:
        del backbone.layers_tframe
    D = model.config.d_model
    final = 2 * B * Lq * D * 4  # fp32 golden weights: the (S, B, L, D) normed activation
    print(f"[pool-memory] behind the layer loop: pooled {p_pool} B, through hidden {p_hidden} B, final activation {final} B")
    assert p_hidden - p_pool >= final, (p_pool, p_hidden, final)
    torch.testing.assert_close(torch.cat([a[..., 0], a[..., 1].flip(-1)], -1), b, rtol=1e-4, atol=1e-5)
