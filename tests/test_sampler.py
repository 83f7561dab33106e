"""The token sampler (cad_sample_tokens, ops.sample_tokens) against an fp64 numpy restatement of its rules (include/caduceus_hip.h),
fed the kernel's own uniforms; the uniforms against an integer restatement of Philox4x32-10; sampled frequencies against the
distribution; the ctypes mirrors of the new argument records against the header; generate's argument validation.

A row is left out of the id comparison only where fp64 itself sits within 1e-5 of a decision: u against a CDF edge, or a top-p
cumulative against 1 - top_p.  At most 1 % of the rows of a cell may be left out (the seed below: at most 0.4 %)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from caduceus_amd import CaduceusConfig, CaduceusForMaskedLM, _lib, ops
from caduceus_amd.generation import generate
from conftest import ROOT, load_golden_model

NEAR = 1e-5


# ---- restatements ---------------------------------------------------------------------------------------------------
def sample_ref(logits, mask, top_k, top_p, temperature, u):
    """(ids (B), near (B) bool) in fp64.  near: a decision of this row lies within NEAR of its boundary."""
    x = logits.astype(np.float64)
    if mask is not None:
        x = x + mask.astype(np.float64)
    B, V = x.shape
    ar = np.broadcast_to(np.arange(V), (B, V))
    order = np.lexsort((ar, -x), axis=-1)  # logit descending, ties: the lower id first
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, ar, -1)
    near = np.zeros(B, dtype=bool)
    if top_k == 1:
        return order[:, 0], near
    keep_n = V if top_k == 0 or top_k > V else top_k
    keep = rank < keep_n
    if temperature != 1.0:
        x = x / temperature
    with np.errstate(invalid="ignore"):
        mx = np.where(keep, x, -np.inf).max(-1, keepdims=True)
        e = np.nan_to_num(np.where(keep, np.exp(x - mx), 0.0), nan=0.0)
    if 0.0 < top_p < 1.0:
        p_sorted = np.take_along_axis(e / e.sum(-1, keepdims=True), order, -1)
        cum = np.take_along_axis(np.cumsum(p_sorted[:, ::-1], -1)[:, ::-1], rank, -1)  # this entry and everything ranked behind it
        cand = keep & (rank != 0)
        near |= (cand & (np.abs(cum - (1.0 - top_p)) < NEAR)).any(-1)
        e = np.where(cand & (cum <= 1.0 - top_p), 0.0, e)
    live = e > 0
    cdf = np.cumsum(e, -1) / e.sum(-1, keepdims=True)
    near |= (live & (np.abs(cdf - u[:, None]) < NEAR)).any(-1)
    hit = live & (cdf > u[:, None])
    first = np.where(hit.any(-1), hit.argmax(-1), V - 1 - live[:, ::-1].argmax(-1))
    return first, near


def philox_u(seed, r, position):
    """Philox4x32-10 (Salmon et al. 2011), key = seed, counter = (r, position); first output word, top 24 bits."""
    ctr = [r & 0xFFFFFFFF, r >> 32 & 0xFFFFFFFF, position & 0xFFFFFFFF, position >> 32 & 0xFFFFFFFF]
    key = [seed & 0xFFFFFFFF, seed >> 32 & 0xFFFFFFFF]
    for _ in range(10):
        a, b = 0xD2511F53 * ctr[0], 0xCD9E8D57 * ctr[2]
        ctr = [(b >> 32) ^ ctr[1] ^ key[0], b & 0xFFFFFFFF, (a >> 32) ^ ctr[3] ^ key[1], a & 0xFFFFFFFF]
        key = [(key[0] + 0x9E3779B9) & 0xFFFFFFFF, (key[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return np.float32((ctr[0] >> 8) / 16777216.0)


def _logits(B, V, seed):
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((B, V))).astype(np.float32)
    for r in range(0, B, 16):  # exact ties: at the top, at a top-k cut, among small entries
        k = (r // 16) % 3
        srt = np.argsort(-x[r])
        if k == 0:
            x[r, srt[1 % V]] = x[r, srt[0]]
        elif k == 1:
            x[r, srt[3 % V]] = x[r, srt[2 % V]]
        else:
            x[r, srt[-1]] = x[r, srt[-2]]
    return x


GRID = [(k, p, t) for k in (0, 1, 3, "V") for p in (0.0, 0.5, 0.9) for t in (1.0, 0.7)]


# ---- not GPU ----------------------------------------------------------------------------------------------------------
def test_restatement_on_hand_worked_cases():
    lp = np.log(np.array([[0.1, 0.2, 0.3, 0.4]]))
    one = lambda x, k, p, t, u: int(sample_ref(np.asarray(x, dtype=np.float64).reshape(1, -1), None, k, p, t, np.array([u]))[0][0])
    # top-p: ascending cumulative 0.1, 0.3, 0.6, 1.0; threshold 0.35 removes ids 0 and 1, survivors 3/7 and 4/7
    assert one(lp, 0, 0.65, 1.0, 0.42) == 2 and one(lp, 0, 0.65, 1.0, 0.43) == 3 and one(lp, 0, 0.65, 1.0, 0.0) == 2
    # threshold 0.25 removes id 0 only: CDF 2/9, 5/9, 1
    assert one(lp, 0, 0.75, 1.0, 0.2) == 1 and one(lp, 0, 0.75, 1.0, 0.5) == 2 and one(lp, 0, 0.75, 1.0, 0.99) == 3
    # the boundary itself is reported: cumulative 0.3 against 1 - 0.7
    assert bool(sample_ref(lp, None, 0, 0.7, 1.0, np.array([0.9]))[1][0])
    assert not bool(sample_ref(lp, None, 0, 0.65, 1.0, np.array([0.9]))[1][0])
    # the most probable entry survives any top_p; among equals the lowest id
    assert one([0.0, 10.0], 0, 1e-6, 1.0, 0.999) == 1
    assert one([1.0, 1.0, 1.0], 0, 0.01, 1.0, 0.999) == 0
    # ties: argmax to the lowest id; at a top-k cut the lower ids are kept
    assert one([3.0, 5.0, 5.0, 1.0], 1, 0.0, 1.0, 0.7) == 1
    assert [one([5.0, 5.0, 5.0, 1.0], 2, 0.0, 1.0, u) for u in (0.0, 0.49, 0.51, 0.999)] == [0, 0, 1, 1]
    # top_k >= V keeps all, like 0
    for u in (0.05, 0.25, 0.55, 0.95):
        assert one(lp, 4, 0.0, 1.0, u) == one(lp, 9, 0.0, 1.0, u) == one(lp, 0, 0.0, 1.0, u) == int(np.searchsorted([0.1, 0.3, 0.6, 1.0], u, "right"))
    # temperature -> 0: the argmax whatever u; temperature 2 flattens: sqrt weights
    assert all(one([1.0, 2.0, 1.5], 0, 0.0, 1e-3, u) == 1 for u in (0.0, 0.5, 0.999999))
    w = np.sqrt([0.1, 0.2, 0.3, 0.4])
    edges = np.cumsum(w) / w.sum()
    assert all(one(lp, 0, 0.0, 2.0, u) == int(np.searchsorted(edges, u, "right")) for u in (0.1, 0.3, 0.5, 0.7, 0.9))
    # a mask of -inf removes an id before anything else
    m = np.array([0.0, 0.0, 0.0, -np.inf])
    assert int(sample_ref(lp, m, 1, 0.0, 1.0, np.array([0.5]))[0][0]) == 2
    assert int(sample_ref(lp, m, 0, 0.0, 1.0, np.array([0.999]))[0][0]) == 2


def test_restatement_alone_leaves_out_at_most_one_percent():
    """The cells of the GPU test, with the generator's uniforms: the rows the comparison may leave out, per cell."""
    worst = 0.0
    for V in (4, 16, 64):
        x = _logits(512, V, 100 + V)
        u = np.array([philox_u(77, r, 3) for r in range(512)], dtype=np.float64)
        for k, p, t in GRID:
            _, near = sample_ref(x, None, V if k == "V" else k, p, t, u)
            worst = max(worst, float(near.mean()))
    print(f"largest share of rows near a boundary: {worst:.4f}")
    assert worst <= 0.01


def test_philox_known_answer_and_host_copy():
    # Random123's known-answer vector for philox4x32-10: counter 0, key 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
    assert philox_u(0, 0, 0) == np.float32((0x6627E8D5 >> 8) / 16777216.0)
    for seed, r, pos in [(0, 0, 0), (1, 2, 3), (2 ** 63 + 5, 2 ** 40 + 1, 2 ** 33), (2 ** 64 - 1, 2 ** 31, 2 ** 31 - 1)]:
        assert np.float32(ops.philox_uniform(seed, r, pos)) == philox_u(seed, r, pos)


def _struct_fields(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "caduceus_hip.h")).read(), flags=re.S)
    body = re.search(r"struct %s \{(.*?)\};" % name, txt, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = decl.split(",")
            fields.append(names[0].split()[-1].lstrip("*"))
            fields += [n.strip().lstrip("*") for n in names[1:]]
    return fields


def test_argument_records_mirror_the_header(tmp_path):
    mirror = {"cad_sampler_args": _lib.SamplerArgs, "cad_decode_layer": _lib.DecodeLayer, "cad_decode_args": _lib.DecodeArgs}
    for name, cls in mirror.items():
        assert [f[0] for f in cls._fields_] == _struct_fields(name), name
    src = tmp_path / "sz.c"
    probes = "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in mirror)
    probes += 'printf("sampler_off %zu\\n", offsetof(cad_decode_args, sampler));printf("B_off %zu\\n", offsetof(cad_decode_args, B));'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "caduceus_hip.h"\nint main(){' + probes + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for name, cls in mirror.items():
        assert int(got[name]) == ctypes.sizeof(cls), name
    assert int(got["sampler_off"]) == _lib.DecodeArgs.sampler.offset and int(got["B_off"]) == _lib.DecodeArgs.B.offset


def test_generate_validates_its_sampling_arguments():
    """Raised before any kernel is reached (no backend needed)."""
    cfg, _, _ = load_golden_model("ps_fused_unidir")
    cfg = {**cfg, "rcps": False, "bidirectional": False, "complement_map": None}
    model = CaduceusForMaskedLM(CaduceusConfig(**cfg, pad_token_id=4)).eval()
    ids = torch.randint(7, 11, (2, 4))
    for bad in (dict(top_p=-0.1), dict(top_p=1.5), dict(temperature=0.0), dict(temperature=-1.0), dict(top_k=-1), dict(top_k=2.5)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            generate(model, ids, 3, **bad)
    with pytest.raises(ValueError, match="allowed_token_ids is empty"):
        generate(model, ids, 3, allowed_token_ids=[])
    for bad in ([7, 16], [-1, 8]):
        with pytest.raises(ValueError, match=r"allowed_token_ids must lie in \[0, 16\)"):
            generate(model, ids, 3, allowed_token_ids=bad)
    with pytest.raises(ValueError, match="eos_token_id"):
        generate(model, ids, 3, eos_token_id=16)
    for bad in (dict(top_p=2.0), dict(temperature=0.0)):
        with pytest.raises(ValueError):
            ops.sample_tokens(torch.zeros(2, 4), **bad)


# ---- kernel (host emulator here, gfx950 on the GPU) -------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [4, 16, 64])
def test_kernel_against_the_restatement(backend, V):
    _, dev = backend
    B = 512
    x = _logits(B, V, 100 + V)
    xt = torch.from_numpy(x).to(dev)
    for k, p, t in GRID:
        top_k = V if k == "V" else k
        ids, u = ops.sample_tokens(xt, top_k, p, t, seed=77, position=3, return_u=True)
        assert ids.dtype == torch.int64 and ids.shape == (B,) and u.dtype == torch.float32
        u = u.cpu().numpy()
        assert np.array_equal(u, np.array([philox_u(77, r, 3) for r in range(B)], dtype=np.float32))
        ref, near = sample_ref(x, None, top_k, p, t, u.astype(np.float64))
        ids = ids.cpu().numpy()
        assert 0 <= ids.min() and ids.max() < V
        assert near.mean() <= 0.01, (V, k, p, t, near.mean())
        bad = np.flatnonzero((ids != ref) & ~near)
        assert bad.size == 0, (V, k, p, t, bad[:8], ids[bad[:8]], ref[bad[:8]])


def test_ids_outside_the_allowed_set_never_appear(backend):
    _, dev = backend
    V, B = 16, 512
    x = _logits(B, V, 5)
    x[:, 7:12] -= 6.0  # the allowed ids are the unlikely ones
    xt = torch.from_numpy(x).to(dev)
    allowed = [7, 8, 9, 10, 11]
    mask = torch.full((V,), float("-inf"))
    mask[allowed] = 0.0
    m = mask.numpy()
    mask = mask.to(dev)
    for k, p, t in GRID:
        ids, u = ops.sample_tokens(xt, k if k != "V" else V, p, t, seed=5, position=9, logit_mask=mask, return_u=True)
        ids = ids.cpu().numpy()
        assert set(ids.tolist()) <= set(allowed), (k, p, t)
        ref, near = sample_ref(x, m, k if k != "V" else V, p, t, u.cpu().numpy().astype(np.float64))
        assert np.array_equal(ids[~near], ref[~near]), (k, p, t)


def test_uniforms_depend_on_seed_row_and_position_only(backend):
    _, dev = backend
    x = torch.zeros(9, 16, device=dev)
    u = lambda B, **kw: ops.sample_tokens(x[:B], 0, return_u=True, **kw)[1].cpu().numpy()
    whole = u(9, seed=2 ** 40 + 3, position=17)
    assert np.array_equal(whole, np.array([philox_u(2 ** 40 + 3, r, 17) for r in range(9)], dtype=np.float32))
    for r in (8, 0, 5):  # other batches, another call order
        assert np.array_equal(u(1, seed=2 ** 40 + 3, position=17, row_offset=r), whole[r:r + 1])
    assert np.array_equal(u(4, seed=2 ** 40 + 3, position=17, row_offset=5), whole[5:])
    assert np.array_equal(u(2, seed=2 ** 40 + 3, position=17, row_offset=2 ** 33),
                          np.array([philox_u(2 ** 40 + 3, 2 ** 33 + r, 17) for r in range(2)], dtype=np.float32))
    pos = np.concatenate([u(9, seed=2 ** 40 + 3, position=q) for q in range(16, 48)])
    assert len(set(pos.tolist())) == pos.size and 0.0 <= pos.min() and pos.max() < 1.0
    assert not np.array_equal(u(9, seed=2 ** 40 + 4, position=17), whole)


def test_sampled_frequencies(backend):
    """8192 rows of one logit vector (V = 16, allowed: the four bases and N), one step: every id's count within 5 sigma of n p.
    Five ids, two-sided 5 sigma (the normal tail 5.7e-7, the binomial's a little heavier): below 1e-5 per run."""
    _, dev = backend
    n, V = 8192, 16
    rng = np.random.default_rng(11)
    row = (2.0 * rng.standard_normal(V)).astype(np.float32)
    allowed = [7, 8, 9, 10, 11]
    mask = torch.full((V,), float("-inf"))
    mask[allowed] = 0.0
    ids = ops.sample_tokens(torch.from_numpy(np.tile(row, (n, 1))).to(dev), 0, seed=2024, position=1, logit_mask=mask.to(dev)).cpu().numpy()
    e = np.where(np.isin(np.arange(V), allowed), np.exp(row.astype(np.float64) - row[allowed].max()), 0.0)
    p = e / e.sum()
    counts = np.bincount(ids, minlength=V)
    for v in range(V):
        assert abs(counts[v] - n * p[v]) <= 5.0 * np.sqrt(n * p[v] * (1.0 - p[v])), (v, counts[v], n * p[v])


def test_vocabularies_beyond_the_kernel_take_the_same_rules_in_torch(backend):
    """V = 80: the kernel refuses (CAD_ERR_UNSUPPORTED), ops.sample_tokens restates the rules in torch ops; V = 64 through both."""
    _, dev = backend
    lib = _lib.get_lib()
    x = torch.from_numpy(_logits(64, 80, 9)).to(dev)
    out = torch.zeros(64, dtype=torch.int64, device=dev)
    s = ops.sampler_args(top_k=0)
    assert lib.cad_sample_tokens(_lib.ptr(x), 64, 80, ctypes.byref(s), _lib.ptr(out), None, _lib.stream_and_check(x, out)) == 2
    for k, p, t in GRID:
        top_k = 80 if k == "V" else k
        ids, u = ops.sample_tokens(x, top_k, p, t, seed=1, position=2, return_u=True)
        ref, near = sample_ref(x.cpu().numpy(), None, top_k, p, t, u.cpu().numpy().astype(np.float64))
        assert np.array_equal(ids.cpu().numpy()[~near], ref[~near]) and near.mean() <= 0.05
    x64 = x[:, :64].contiguous()
    for k, p, t in GRID:
        top_k = 64 if k == "V" else k
        ids, u = ops.sample_tokens(x64, top_k, p, t, seed=1, position=2, return_u=True)
        ref, near = sample_ref(x64.cpu().numpy(), None, top_k, p, t, u.cpu().numpy().astype(np.float64))
        alt = ops._sample_tokens_torch(x64, top_k, p, t, u)
        assert np.array_equal(alt.cpu().numpy()[~near], ref[~near])
