"""Milliseconds per call of the pool head (cad_pool_head) against the composition it replaces behind the backbone's layer loop, on the
same device in the same process: cad_add_norm_fwd writing the normed (S, B, L, D) activation, the fp32 residual copy and rstd, then
engine.from_tframe (strand concatenation with a channel flip) and the caller's pooling in torch -- `.mean(1)`, `.max(1).values`, or
vep's strand split, position / channel flips and window_mean.

Shape: L = 131072 rows per strand, D = 256, S = 2 (RCPS), B = 1, bf16 activations with the fp32 residual stream, RMSNorm; MEAN, MAX
and WINDOW (half = 768, centre L // 2).  Both sides are called with their kernel outputs allocated once (the torch half of the
composition allocates its own temporaries, as it does in use).  HIP events around blocks of `--block` calls, the variants alternating
block by block after `--warmup` calls of each; the figure is the median block over `--blocks`, per call.  Bytes are the algorithm's:
what each route has to read and write, computed from the shapes.  `--forward` adds one forward_tframe of a d_model 256, 16-layer RCPS
model at that length for scale.  Not a test; bench.py is untouched.

    python tools/pool_bench.py [--out profiles/pool_head.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from caduceus_amd import _lib as L  # noqa: E402
from caduceus_amd import engine, vep  # noqa: E402

MODES = {"mean": L.POOL_MEAN, "max": L.POOL_MAX, "window": L.POOL_WINDOW}


def _variants(S, B, Lq, D, half, dev):
    """{name: (callable, bytes moved)} on one set of inputs."""
    lib = L.get_lib()
    g = torch.Generator().manual_seed(S)
    x = torch.randn(S, B, Lq, D, generator=g).to(torch.bfloat16).to(dev)
    res = torch.randn(S, B, Lq, D, generator=g).to(dev)
    w = (1 + 0.2 * torch.randn(D, generator=g)).to(dev)
    centre_b = torch.full((B,), Lq // 2, dtype=torch.int64, device=dev)
    centre = torch.stack([centre_b, Lq - 1 - centre_b][:S], 0).contiguous()
    y = torch.empty(S, B, Lq, D, dtype=torch.bfloat16, device=dev)
    res_out = torch.empty(S, B, Lq, D, device=dev)
    rstd = torch.empty(S * B * Lq, device=dev)
    out = torch.empty(S, B, D, device=dev)
    scratch = torch.empty(max(lib.cad_pool_head_scratch_floats(S, B, Lq, D, m, half if m == L.POOL_WINDOW else 0) for m in MODES.values()),
                          device=dev)
    keep = [x, res, w, centre, y, res_out, rstd, out, scratch]
    stream = L.stream_and_check(x)
    code = L.dtype_code(torch.bfloat16)
    a_norm = L.AddNormArgs(L.ptr(x), L.ptr(res), L.ptr(w), None, L.ptr(y), L.ptr(res_out), L.ptr(rstd), None, B * Lq, S, D, 1e-5, 1, 0, code,
                           code, None, None)
    a_pool = {m: L.PoolHeadArgs(L.ptr(x), L.ptr(res), L.ptr(w), None, L.ptr(centre) if m == "window" else None, L.ptr(out), L.ptr(scratch),
                                B, Lq, half if m == "window" else 0, S, D, 1e-5, 1, code, code, MODES[m]) for m in MODES}

    def head(m):
        def fn():
            L.check(lib.cad_pool_head(C.byref(a_pool[m]), stream), "cad_pool_head")
            return out  # (S, B, D)
        return fn

    def composed(m):
        def fn():
            L.check(lib.cad_add_norm_fwd(C.byref(a_norm), stream), "cad_add_norm_fwd")
            h = engine.from_tframe(y)  # (B, L, S D)
            if m == "mean":
                return h.mean(1)
            if m == "max":
                return h.max(1).values
            if S == 1:
                return vep.window_mean(h, centre_b, 2 * half)
            fwd, rc = h[..., :D], h[..., D:].flip(dims=[1, 2])
            return torch.stack([vep.window_mean(fwd, centre_b, 2 * half), vep.window_mean(rc, centre_b, 2 * half)], -1)
        return fn

    rows = S * B * Lq
    stream_in = rows * D * (2 + 4) + D * 4
    norm_out = rows * D * (2 + 4) + rows * 4
    cat = (2 * rows * D * 2) if S == 2 else 0        # from_tframe: the normed tensor read and written once more
    nwin = S * B * (2 * half + 1)
    pieces = {m: lib.cad_pool_head_pieces(Lq, MODES[m], half if m == "window" else 0) for m in MODES}
    variants = {}
    for m in MODES:
        part = 2 * S * B * pieces[m] * D * 4 + S * B * D * 4
        head_bytes = (stream_in if m != "window" else nwin * D * (2 + 4) + D * 4) + part
        tail = rows * D * 2 if m != "window" else ((2 * rows * D * 2 if S == 2 else 0) + 3 * nwin * D * 2)  # flips, gather, mean
        variants[f"head_{m}"] = (head(m), head_bytes)
        variants[f"composed_{m}"] = (composed(m), stream_in + norm_out + cat + tail + S * B * D * 2)
    # the two routes agree at the sizes that are timed (bf16 rows pooled in bf16 by torch on the composed side)
    for m in MODES:
        got = head(m)().clone()
        want = composed(m)().float()
        want_t = torch.stack([want[..., :D], want[..., D:].flip(-1)], 0) if (S == 2 and m != "window") else \
            (want.permute(2, 0, 1) if S == 2 else want.unsqueeze(0))
        torch.testing.assert_close(got, want_t, rtol=2e-2, atol=2e-2)
    return variants, keep


def _time(variants, blocks, block, warmup):
    for fn, _ in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(blocks):
        for name, (fn, _) in variants.items():  # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(block):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / block)
    return ms


def _forward_ms(Lq, D, dev, reps=5):
    """One forward_tframe of a d_model-256, 16-layer RCPS model in bf16 at this length (random weights): the scale the head sits on."""
    from caduceus_amd import Caduceus, CaduceusConfig
    comp = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 10, 8: 9, 9: 8, 10: 7, 11: 11, 12: 12, 13: 13, 14: 14, 15: 15}
    cfg = CaduceusConfig(d_model=D, n_layer=16, vocab_size=16, rcps=True, bidirectional=True, complement_map=comp, fused_add_norm=True,
                         rms_norm=True, residual_in_fp32=True, ssm_cfg=dict(d_state=16, d_conv=4, expand=2))
    torch.manual_seed(0)
    model = Caduceus(cfg).to(dev).to(torch.bfloat16).eval()
    ids = torch.randint(7, 11, (1, Lq), device=dev)
    ms = []
    with torch.no_grad():
        for i in range(reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            model.backbone.forward_tframe(ids)
            b.record()
            b.synchronize()
            if i >= 2:
                ms.append(a.elapsed_time(b))
    return {"n_layer": 16, "ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--strands", type=int, default=2)
    ap.add_argument("--d-model", type=int, default=256)
    ap.add_argument("--half", type=int, default=768)
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available() and L.is_device_build(), "pool_bench needs the gfx950 library and a GPU"
    version = L.version()
    assert "variant" not in version and "TIMING-BUILD" not in version, f"measure the product build, not {version}"
    dev = torch.device("cuda:0")
    with torch.no_grad():
        variants, keep = _variants(args.strands, args.batch, args.rows, args.d_model, args.half, dev)
        ms = _time(variants, args.blocks, args.block, args.warmup)
    rec = {}
    for name, (_, nbytes) in variants.items():
        med = statistics.median(ms[name])
        rec[name] = {"ms_per_call_median": round(med, 5), "ms_min": round(min(ms[name]), 5), "ms_max": round(max(ms[name]), 5),
                     "algorithm_bytes": nbytes, "gb_per_s": round(nbytes / med / 1e6, 1)}
    for m in MODES:
        rec[f"composed_over_head_{m}"] = round(rec[f"composed_{m}"]["ms_per_call_median"] / rec[f"head_{m}"]["ms_per_call_median"], 2)
    print(json.dumps(rec), flush=True)
    del variants, keep
    result = {"tool": "tools/pool_bench.py", "library": version, "device": torch.cuda.get_device_name(0), "rows_per_strand": args.rows,
              "batch": args.batch, "n_strands": args.strands, "d_model": args.d_model, "half": args.half, "dtype": "bfloat16 x, fp32 residual",
              "timing": f"HIP events around blocks of {args.block} calls, variants alternating, median of {args.blocks} blocks after "
                        f"{args.warmup} warm-up calls each; per call",
              "composition": "cad_add_norm_fwd (y, fp32 residual copy, rstd to memory) + engine.from_tframe + torch mean / max, or vep's "
                             "flips + window_mean",
              "results": rec}
    if args.forward:
        result["forward_tframe"] = _forward_ms(args.rows, args.d_model, dev)
        print(json.dumps(result["forward_tframe"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
