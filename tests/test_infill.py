"""caduceus_amd.infilling.infill on the golden RCPS, bi-directional and causal weights: the shape of its result; steps = 1 greedy against
masked_logprobs; steps = 4 against four manual rounds of forward_tframe, ops.lm_head_unmask and the commit rule restated here in plain
python on host lists (both orders, both schedules, one sampled setting), with the open counts after every round; reverse-complement
equivariance of the RCPS model; refusals; and, on the GPU, that nothing is read back.

Everything here is an identity (element for element, or bit for bit where floats are compared): the kernels underneath are held to
float64 in tests/test_unmask_head.py's references.  Three rows of L = 32 with 15, 0 and 5 open positions."""
import math

import pytest
import torch

from caduceus_amd import infill, masked_logprobs, ops
from caduceus_amd.generation import _logit_mask
from test_scoring import _golden

BASES = (7, 8, 9, 10)
MASK_ID = 3
LQ = 32
NAMES = ["ps_fused", "ph_fused", "ps_fused_unidir"]
KW = dict(mask_token_id=MASK_ID, allowed_token_ids=BASES)
SAMPLED = dict(top_k=0, temperature=0.8, seed=11)


def masked_input(seed=0):
    """(3, LQ) bases with MASK_ID at 15 positions of row 0 (the first and the last among them), none of row 1, 5 of row 2."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(7, 11, (3, LQ), generator=g)
    p0 = torch.randperm(LQ - 2, generator=g)[:13] + 1
    ids[0, p0], ids[0, 0], ids[0, LQ - 1] = MASK_ID, MASK_ID, MASK_ID
    ids[2, torch.tensor([2, 3, 4, 20, LQ - 1])] = MASK_ID
    assert (ids == MASK_ID).sum(1).tolist() == [15, 0, 5]
    return ids


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def padded_positions(is_open):
    """(B, P) positions for masked_logprobs: a row's open positions, padded by repeats (a row without any: position 0)."""
    rows = [r.nonzero().flatten().tolist() for r in is_open.cpu()]
    P = max(1, max(len(r) for r in rows))
    return rows, torch.tensor([(r + [r[-1] if r else 0] * P)[:P] for r in rows])


@pytest.mark.parametrize("name", NAMES)
def test_infill_result(backend, name):
    _, dev = backend
    model, _ = _golden(name, dev)
    ids = masked_input().to(dev)
    before = ids.clone()
    was_open = ids == MASK_ID
    got = []
    for kw in (dict(steps=2), dict(steps=3, **SAMPLED), dict(steps=2, order="left_to_right", schedule="linear", top_k=2, top_p=0.9, seed=5)):
        out, lp = infill(model, ids, return_logprobs=True, **KW, **kw)
        assert torch.equal(ids, before), "the caller's ids were written"
        assert out.shape == ids.shape and out.dtype == torch.int64 and lp.shape == ids.shape and lp.dtype == torch.float32
        assert not bool((out == MASK_ID).any())
        assert set(out[was_open].tolist()) <= set(BASES)
        assert torch.equal(out[~was_open], ids[~was_open]) and bool((bits(lp)[(~was_open).cpu()] == 0).all())
        assert bool(torch.isfinite(lp).all()) and bool((lp[was_open] < 0).all())
        got.append(out)
    assert torch.equal(infill(model, ids, steps=3, **KW, **SAMPLED), got[1]), "the same seed gave other ids"
    # a host-held tensor is taken too, and a row does not depend on its batch: row 2 alone at row_offset 2
    assert torch.equal(infill(model, ids.cpu(), steps=2, **KW), got[0])
    assert torch.equal(infill(model, ids[2:], steps=3, row_offset=2, **KW, **SAMPLED), got[1][2:])


@pytest.mark.parametrize("name", NAMES)
def test_one_greedy_step_takes_the_most_probable_base(backend, name):
    """steps = 1, top_k = 1: the id at every filled position has the largest of masked_logprobs' entries there, bit for bit (a form that
    holds under exact ties), and the returned log-probability is that entry."""
    _, dev = backend
    model, _ = _golden(name, dev)
    ids = masked_input(1).to(dev)
    out, lp = infill(model, ids, steps=1, return_logprobs=True, **KW)
    rows, pos = padded_positions(ids == MASK_ID)
    ref = masked_logprobs(model, ids, pos, **KW).cpu()  # (B, P, V)
    out, lp = out.cpu(), lp.cpu()
    n = 0
    for b, r in enumerate(rows):
        for k, p in enumerate(r):
            assert bits(ref[b, k, out[b, p]]) == bits(ref[b, k].max()), (b, p)
            assert bits(lp[b, p]) == bits(ref[b, k, out[b, p]]), (b, p)
            n += 1
    assert n == 20


def f_restated(schedule, r, steps):
    if r == steps - 1:
        return 0.0
    return math.cos(math.pi / 2 * (r + 1) / steps) if schedule == "cosine" else 1 - (r + 1) / steps


@pytest.mark.parametrize("order,schedule,sampling", [("confidence", "cosine", {}), ("left_to_right", "linear", {}),
                                                     ("confidence", "linear", SAMPLED), ("left_to_right", "cosine", SAMPLED)],
                         ids=["conf-cos", "l2r-lin", "conf-lin-sampled", "l2r-cos-sampled"])
@pytest.mark.parametrize("name", NAMES)
def test_four_steps_equal_four_manual_rounds(backend, name, order, schedule, sampling):
    _, dev = backend
    model, _ = _golden(name, dev)
    steps = 4
    ids = masked_input(2).to(dev)
    out, lp = infill(model, ids, steps=steps, order=order, schedule=schedule, return_logprobs=True, **KW, **sampling)
    w = model.lm_head.weight
    comp = model.lm_head.complement_map if model.config.rcps else None
    mask = _logit_mask(BASES, w.shape[0], dev)
    cur = ids.clone()
    n0 = (cur == MASK_ID).sum(1).tolist()
    assert n0 == [15, 0, 5]
    prev = list(n0)
    want_lp = torch.zeros(ids.shape)
    for r in range(steps):
        with model._precision_scope(), torch.no_grad():
            hidden = model.caduceus.backbone.forward_tframe(cur)
            ids_r, conf_r = ops.lm_head_unmask(hidden, w, comp, cur, mask_token_id=MASK_ID, position=r << 32, logit_mask=mask,
                                               **{"seed": 0, **sampling})
        ids_r, conf_r, host = ids_r.cpu(), conf_r.cpu(), cur.cpu()
        for b in range(ids.shape[0]):
            open_b = [p for p in range(LQ) if host[b, p] == MASK_ID]
            assert len(open_b) == prev[b]
            stay = min(prev[b], math.floor(n0[b] * f_restated(schedule, r, steps)))
            ranked = sorted(open_b, key=lambda p: (-float(conf_r[b, p]), p)) if order == "confidence" else open_b
            for p in ranked[:len(open_b) - stay]:
                host[b, p], want_lp[b, p] = ids_r[b, p], conf_r[b, p]
            prev[b] = stay
        cur = host.to(dev)
        assert (cur == MASK_ID).sum(1).tolist() == prev, (r, prev)
    print(f"[infill] {name} {order} {schedule} {sampling}: open after the rounds ends at {prev}")
    assert prev == [0, 0, 0]
    assert torch.equal(out.cpu(), cur.cpu()) and torch.equal(bits(lp), bits(want_lp))


def test_open_counts_of_the_schedules():
    """floor(n0 f(r)) for n0 = 15 and 5 at steps = 4, worked by hand: cosine 0.9239, 0.7071, 0.3827, 0; linear 0.75, 0.5, 0.25, 0."""
    from caduceus_amd.infilling import open_fraction
    for schedule, want15, want5 in (("cosine", [13, 10, 5, 0], [4, 3, 1, 0]), ("linear", [11, 7, 3, 0], [3, 2, 1, 0])):
        f = [open_fraction(schedule, r, 4) for r in range(4)]
        assert f == [f_restated(schedule, r, 4) for r in range(4)] and f[-1] == 0.0
        assert [math.floor(15 * x) for x in f] == want15 and [math.floor(5 * x) for x in f] == want5
    assert open_fraction("cosine", 0, 1) == 0.0 and open_fraction("linear", 0, 1) == 0.0


@pytest.mark.parametrize("name", ["ps_fused", "ps_fused_unidir"])
def test_reverse_complement_equivariance(backend, name):
    """RCPS, steps = 1, top_k = 1: infilling the reverse complement (the mirrored positions masked) gives the reverse complement of the
    infill.  A position whose two largest allowed log-probabilities are equal bit for bit would be exempt (the lowest-id tie rule is not
    equivariant); the input is chosen so that there is none, and that is asserted."""
    _, dev = backend
    model, _ = _golden(name, dev)
    comp = model.lm_head.complement_map.to(dev)
    assert int(comp[MASK_ID]) == MASK_ID
    rc = lambda x: comp[x.flip(1)]
    ids = masked_input(3).to(dev)
    rows, pos = padded_positions(ids == MASK_ID)
    lp = masked_logprobs(model, ids, pos, **KW).cpu()
    top2 = lp.topk(2, dim=-1).values
    tied = sum(int(bits(top2[b, k, 0]) == bits(top2[b, k, 1])) for b, r in enumerate(rows) for k in range(len(r)))
    assert tied == 0, "the input has an exact tie at the top: choose another seed"
    out = infill(model, ids, steps=1, **KW)
    out_rc = infill(model, rc(ids), steps=1, **KW)
    assert torch.equal(out_rc, rc(out))


def test_infill_refusals(backend):
    _, dev = backend
    model, _ = _golden("ph_fused", dev)
    ids = masked_input().to(dev)
    with pytest.raises(ValueError, match="must not hold mask_token_id"):
        infill(model, ids, mask_token_id=MASK_ID, allowed_token_ids=(3, 7, 8))
    with pytest.raises(ValueError, match="allowed_token_ids"):
        infill(model, ids, mask_token_id=MASK_ID, allowed_token_ids=None)
    with pytest.raises(ValueError, match="allowed_token_ids is empty"):
        infill(model, ids, mask_token_id=MASK_ID, allowed_token_ids=())
    with pytest.raises(ValueError, match="steps"):
        infill(model, ids, steps=0, **KW)
    with pytest.raises(ValueError, match="order"):
        infill(model, ids, order="random", **KW)
    with pytest.raises(ValueError, match="schedule"):
        infill(model, ids, schedule="sqrt", **KW)
    with pytest.raises(ValueError, match="top_k"):
        infill(model, ids, top_k=-1, **KW)
    with pytest.raises(ValueError, match="mask_token_id"):
        infill(model, ids, mask_token_id=16, allowed_token_ids=BASES)
    model.lm_head = torch.nn.Linear(32, 16, bias=True).to(dev)
    with pytest.raises(ops.ScoreUnsupported, match="bias-free"):
        infill(model, ids, **KW)


def test_infill_is_exported_under_both_package_names():
    import caduceus
    import caduceus_amd
    assert caduceus.infilling is caduceus_amd.infilling and caduceus.infill is caduceus_amd.infilling.infill
    assert "infill" in caduceus_amd.__all__


@pytest.mark.gpu
def test_infill_reads_nothing_back():
    """A whole infill (sampled, four rounds) with torch's synchronisation check set to raise: no nonzero(), no .item(), no blocking
    copy anywhere in it.  A first call outside the check takes what happens once per process; ids and result stay on the device."""
    from caduceus_amd import _lib
    _lib.use_library_for_testing(None)
    dev = torch.device("cuda:0")
    model, _ = _golden("ps_fused", dev)
    ids = masked_input(4).to(dev)
    want = infill(model, ids, steps=4, **KW, **SAMPLED)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, lp = infill(model, ids, steps=4, return_logprobs=True, **KW, **SAMPLED)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out, want) and not bool((out == MASK_ID).any())
