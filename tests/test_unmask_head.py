"""The unmask head (csrc/unmask.hip, cad_lm_head_unmask) by identity with kernels that are already held to float64, from the same stored
hidden state.  No tolerance and no left-out rows: the references are what the library itself computes for the same bits.

  ids_out   at open rows: ops.sample_tokens on row l of ops.lm_head's logits (cad_lm_head_fwd, tests/test_norm_head_fp64.py; the sampler,
            tests/test_sampler.py), called with position + l and the same row offset, mask and sampler arguments -- element for element
  u_out     that call's uniforms, bit for bit, and test_sampler.philox_u(seed, row_offset + b, position + l)
  conf      at open rows: ops.lm_head_score (tests/test_score_head.py) with the drawn ids as targets and the same mask -- bit for bit
  closed    ids_out == ids_in, conf == 0.0, u_out == 0.0 exactly

Shapes: (B, L) below, at and above one 16-row tile, a ragged last tile, a batch boundary inside a tile; every width class and dtype of
the matrix-core and the one-wave-per-row path; V in {16, 12, 5}; S in {1, 2}; no row open, all, only the last, every other one.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops
from conftest import ROOT
from test_norm_head_fp64 import BF, COMP, F32, HF, TAG, Arena, lm_inputs
from test_sampler import GRID, _struct_fields, philox_u
from test_score_head import COMPS, GENERAL, MFMA, _cu_count, _mask

MASK_ID = 3
SHAPES = [(1, 1), (15, 1), (1, 16), (1, 17), (3, 11)]
PATTERNS = ["none", "all", "last", "alternating"]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def ids_with(R, V, open_rows, g):
    """(R) ids in [0, V) without MASK_ID, then MASK_ID at open_rows (a bool tensor)."""
    ids = torch.randint(0, V, (R,), generator=g)
    ids[ids == MASK_ID] = 0
    ids[open_rows] = MASK_ID
    return ids


def open_pattern(kind, R):
    o = torch.zeros(R, dtype=torch.bool)
    if kind == "all":
        o[:] = True
    elif kind == "last":
        o[R - 1] = True
    elif kind == "alternating":
        o[::2] = True
    return o


def check_case(backend, tag, h, W, comp, ids, B, Lq, allowed, top_k, top_p, temperature, seed, position, row_offset):
    """One call of the unmask head against the three kernels it joins; returns (ids_out, conf, u) on the host."""
    name, dev = backend
    S, R, D = h.shape
    V = W.shape[0]
    assert R == B * Lq
    hd, wd = h.to(dev).reshape(S, B, Lq, D), W.to(dev)
    cd = comp.to(dev) if S == 2 else None
    mask = _mask(V, allowed)
    md = None if mask is None else mask.to(dev)
    idd = ids.to(dev).reshape(B, Lq)
    before = idd.clone()
    kw = dict(top_k=top_k, top_p=top_p, temperature=temperature, seed=seed, row_offset=row_offset, logit_mask=md)
    with torch.no_grad():
        ids_out, conf, u = ops.lm_head_unmask(hd, wd, cd, idd, mask_token_id=MASK_ID, position=position, return_u=True, **kw)
        assert torch.equal(idd, before), "the caller's ids were written"
        assert ids_out.shape == (B, Lq) and ids_out.dtype == torch.int64 and conf.dtype == torch.float32 and u.dtype == torch.float32
        is_open = (idd == MASK_ID).cpu()
        logits = ops.lm_head(hd, wd, cd)[0]  # (B, L, V): cad_lm_head_fwd on the same stored hidden
        want_ids, want_u = torch.zeros(B, Lq, dtype=torch.int64), torch.zeros(B, Lq)
        for l in range(Lq):
            if bool(is_open[:, l].any()):
                a, b = ops.sample_tokens(logits[:, l].contiguous(), position=position + l, return_u=True, **kw)
                want_ids[:, l], want_u[:, l] = a.cpu(), b.cpu()
        want_conf = ops.lm_head_score(hd, wd, cd, targets=ids_out, logit_mask=md).cpu()
    ids_out, conf, u = ids_out.cpu(), conf.cpu(), u.cpu()
    n_open = int(is_open.sum())
    print(f"[unmask] {name} {tag}: {n_open} of {R} rows open, top_k {top_k} top_p {top_p} T {temperature} "
          f"mask {allowed} position {position} row_offset {row_offset}")
    assert torch.equal(ids_out[is_open], want_ids[is_open]), (tag, "ids", ids_out[is_open], want_ids[is_open])
    assert torch.equal(bits(u)[is_open], bits(want_u)[is_open]), (tag, "u against cad_sample_tokens")
    host_u = torch.tensor([[philox_u(seed, row_offset + b, position + l) for l in range(Lq)] for b in range(B)], dtype=torch.float32)
    assert torch.equal(bits(u)[is_open], bits(host_u)[is_open]), (tag, "u against the integer restatement")
    assert torch.equal(bits(conf)[is_open], bits(want_conf)[is_open]), (tag, "conf", conf[is_open], want_conf[is_open])
    if n_open:
        assert bool(torch.isfinite(conf[is_open]).all()) and bool((conf[is_open] <= 0).all()), tag
        if allowed is not None:
            assert set(ids_out[is_open].tolist()) <= set(allowed), tag
    closed = ~is_open
    assert torch.equal(ids_out[closed], ids.reshape(B, Lq)[closed]), (tag, "a closed row's id changed")
    assert bool((bits(conf)[closed] == 0).all()) and bool((bits(u)[closed] == 0).all()), (tag, "a closed row's conf / u is not +0.0")
    return ids_out, conf, u


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("D,dtype", MFMA + GENERAL, ids=[f"D{d}-{TAG[t]}" for d, t in MFMA + GENERAL])
def test_unmask_rows_patterns_sampler_grid(backend, D, dtype, S):
    """Every (B, L) of SHAPES with every open pattern (at (3, 11) in all three vocabularies): 28 calls, which walk test_sampler's GRID of
    24 sampler settings once and a little more; the mask is on in every second pair of calls, the other pairs in the S = 2 test, and
    every second call sits at position (2 << 32) + 5 with row offset 7."""
    lib = L.get_lib()
    assert lib.cad_lm_head_unmask_supported(D, 16, L.dtype_code(dtype)) == 1
    n = 0
    for k, (B, Lq) in enumerate(SHAPES):
        R = B * Lq
        for V in ((16, 12, 5) if (B, Lq) == (3, 11) else ((16, 12, 5)[k % 3],)):
            comp = COMPS[V]
            h, W, _, _ = lm_inputs(S, R, D, V, dtype, 23 * D + R + V + S, comp=comp)
            for pattern in PATTERNS:
                top_k, top_p, temperature = GRID[n % len(GRID)]
                allowed = ([7, 8, 9, 10] if V > 10 else [1, 2, 4]) if ((n >> 1) & 1) ^ (S - 1) else None
                position, row_offset = (((2 << 32) + 5, 7) if n & 1 else (3, 0))
                g = torch.Generator().manual_seed(1000 * D + 10 * R + V + n)
                ids = ids_with(R, V, open_pattern(pattern, R), g)
                check_case(backend, f"D{D}-{TAG[dtype]}-S{S}-B{B}-L{Lq}-V{V}-{pattern}", h, W, comp, ids, B, Lq, allowed,
                           V if top_k == "V" else top_k, top_p, temperature, 77 + n, position, row_offset)
                n += 1
    assert n >= len(GRID)


@pytest.mark.parametrize("tiles", [(0, 2, 17), (0, 16, 17)], ids=["tiles-0-2-17", "tiles-0-16-17"])
@pytest.mark.parametrize("D,dtype,S", [(128, BF, 2), (256, F32, 1), (512, BF, 2)], ids=["D128-bf16-S2", "D256-f32-S1", "D512-bf16-S2"])
def test_unmask_tile_walk_with_skipped_tiles(backend, D, dtype, S, tiles):
    """One CU: 8 waves walk 18 tiles at (B, L) = (1, 275), wave w the tiles w, w + 8, w + 16; the last tile is ragged with 3 rows.
    Open rows only in tiles 0, 2 and 17: every wave but three closes all its tiles from their ids alone, wave 0 computes its first tile
    and skips two, wave 1 skips two and computes the ragged one.  Open rows in tiles 0, 16 and 17: wave 0 computes, skips tile 8, and
    computes again -- the prefetch under tile 0 must fetch tile 16, not the skipped one."""
    Lq = 2 * 8 * 16 + 16 + 3
    h, W, _, _ = lm_inputs(S, Lq, D, 16, dtype, 5 * D + S)
    o = torch.zeros(Lq, dtype=torch.bool)
    for t in tiles:
        o[16 * t:16 * t + 16:1 if t else 3] = True  # (tile 0: every third row, so closed rows sit inside a computed tile too)
    ids = ids_with(Lq, 16, o, torch.Generator().manual_seed(D + S))
    try:
        _cu_count(1)
        check_case(backend, f"walk-D{D}-{tiles}", h, W, COMP, ids, 1, Lq, [7, 8, 9, 10], 0, 0.9, 0.7, 2 ** 40 + 3, 1 << 32, 2 ** 33)
    finally:
        _cu_count(0)


@pytest.mark.parametrize("D,dtype", [(128, BF), (256, F32), (40, HF)], ids=["D128-bf16", "D256-f32", "D40-f16"])
def test_unmask_in_place_and_without_u(backend, D, dtype):
    """Through the C entry point: ids_out == ids_in gives what a separate output gives; u_out NULL writes the other two alike; rows
    beyond `rows` stay untouched."""
    name, dev = backend
    B, Lq, V, S, SENT = 3, 11, 16, 2, -512.0
    R = B * Lq
    h, W, _, _ = lm_inputs(S, R, D, V, dtype, 900 + D)
    ids = ids_with(R, V, open_pattern("alternating", R), torch.Generator().manual_seed(D))
    ref_ids, ref_conf, _ = check_case(backend, f"inplace-D{D}", h, W, COMP, ids, B, Lq, [7, 8, 9, 10], 0, 0.0, 0.8, 11, 5, 1)
    hd, wd, cd, md = h.to(dev), W.to(dev), COMP.to(dev), _mask(V, [7, 8, 9, 10]).to(dev)
    buf = torch.full((R + 5,), 9, dtype=torch.int64, device=dev)
    buf[:R] = ids.to(dev)
    conf = torch.full((R + 5,), SENT, device=dev)
    stream = L.stream_and_check(hd, wd, cd, md, buf, conf)
    s = ops.sampler_args(0, 0.0, 0.8, 11, 1, 5, md)
    a = L.LmUnmaskArgs(L.ptr(hd), L.ptr(wd), L.ptr(cd), L.ptr(buf), L.ptr(buf), L.ptr(conf), None, s, R, Lq, D, V, S, MASK_ID,
                       L.dtype_code(dtype))
    L.check(L.get_lib().cad_lm_head_unmask(C.byref(a), stream), "cad_lm_head_unmask")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert torch.equal(buf[:R].cpu(), ref_ids.reshape(-1)) and torch.equal(bits(conf[:R]), bits(ref_conf.reshape(-1)))
    assert bool((buf[R:] == 9).all()) and bool((conf[R:] == SENT).all()), "rows beyond `rows` were written"


@pytest.mark.parametrize("dtype", [F32, BF, HF], ids=["f32", "bf16", "f16"])
def test_unmask_misaligned_hidden_takes_the_general_path(backend, dtype):
    """hidden one element into its buffer: no 16-byte loads are possible, the launcher takes the one-wave-per-row kernel, as the forward
    and the score head do for such a tensor; the identities hold there too, and the sentinels around the view stay."""
    name, dev = backend
    B, Lq, D, V, S = 2, 19, 128, 16, 2
    h, W, _, _ = lm_inputs(S, B * Lq, D, V, dtype, 950)
    A = Arena(dev, 1)
    hv = A.put(h)
    assert hv.data_ptr() % 16 != 0 and hv.is_contiguous()
    ids = ids_with(B * Lq, V, open_pattern("alternating", B * Lq), torch.Generator().manual_seed(4))
    check_case(backend, f"misaligned-{TAG[dtype]}", hv, W, COMP, ids, B, Lq, None, 3, 0.5, 1.0, 9, 0, 0)
    A.intact()


def test_unmask_refusals(backend):
    name, dev = backend
    B, Lq, D, V = 1, 5, 64, 16
    h, W, _, _ = lm_inputs(2, B * Lq, D, V, F32, 1)
    hd, wd, cd = h.to(dev).reshape(2, B, Lq, D), W.to(dev), COMP.to(dev)
    ids = torch.full((B, Lq), MASK_ID, dtype=torch.int64, device=dev)
    lib = L.get_lib()
    assert lib.cad_lm_head_unmask_supported(64, 17, 0) == 0 and lib.cad_lm_head_unmask_supported(64, 16, 3) == 0
    assert lib.cad_lm_head_unmask_supported(1000, 1, 2) == 1
    assert not ops.lm_head_unmask_supported(64, 16, torch.float64)
    out, conf = torch.zeros(B * Lq, dtype=torch.int64, device=dev), torch.zeros(B * Lq, device=dev)
    stream = L.stream_and_check(hd, wd, cd, ids, out, conf)

    def mk(top_k=1, **kw):
        f = dict(hidden=L.ptr(hd), weight=L.ptr(wd), comp=L.ptr(cd), ids_in=L.ptr(ids), ids_out=L.ptr(out), conf=L.ptr(conf), u_out=None,
                 sampler=ops.sampler_args(), rows=B * Lq, L=Lq, D=D, V=V, n_strands=2, mask_id=MASK_ID, dtype=0)
        f.update(kw)
        a = L.LmUnmaskArgs(**f)
        a.sampler.top_k = top_k
        return a
    assert lib.cad_lm_head_unmask(C.byref(mk()), stream) == 0
    assert lib.cad_lm_head_unmask(C.byref(mk(V=17)), stream) == 2
    assert lib.cad_lm_head_unmask(C.byref(mk(dtype=3)), stream) == 2
    assert lib.cad_lm_head_unmask(C.byref(mk(top_k=-1)), stream) == 1
    for bad in (mk(conf=None), mk(ids_out=None), mk(comp=None), mk(L=2), mk(L=0)):
        assert lib.cad_lm_head_unmask(C.byref(bad), stream) == 1
    with pytest.raises(ops.ScoreUnsupported, match="vocab_size 72"):
        ops.lm_head_unmask(hd, torch.zeros(72, D, device=dev), None, ids, mask_token_id=MASK_ID)
    with pytest.raises(ValueError, match="top_k"):
        ops.lm_head_unmask(hd, wd, cd, ids, mask_token_id=MASK_ID, top_k=-1)
    with pytest.raises(RuntimeError, match="no backward"):
        ops.lm_head_unmask(hd, wd.clone().requires_grad_(True), cd, ids, mask_token_id=MASK_ID)
    with pytest.raises(TypeError, match="int64"):
        ops.lm_head_unmask(hd, wd, cd, ids[:, :4], mask_token_id=MASK_ID)


def test_unmask_struct_matches_the_compiler(tmp_path):
    """cad_lm_unmask_args as a C compiler lays it out equals the ctypes mirror: the field names against the header, sizeof and every
    offset against gcc."""
    fields = [f[0] for f in L.LmUnmaskArgs._fields_]
    assert fields == _struct_fields("cad_lm_unmask_args")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "caduceus_hip.h"\nint main(){printf("%zu\\n", sizeof(cad_lm_unmask_args));' +
                   "".join(f'printf("%zu\\n", offsetof(cad_lm_unmask_args, {f}));' for f in fields) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got[0] == C.sizeof(L.LmUnmaskArgs)
    assert got[1:] == [getattr(L.LmUnmaskArgs, f).offset for f in fields]
