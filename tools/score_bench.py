"""Milliseconds per call of the score head (cad_lm_head_score) against the composition that was possible before it existed
(cad_lm_head_fwd writing (rows, V) fp32 logits, then torch log_softmax and gather), on the same device in the same process.

Shape: rows = 131072, D = 256, V = 16, bf16 hidden, S = 2 (RCPS) and S = 1.  Two modes: every row scored against a target (what
sequence_logprobs does), and 1024 gathered rows with the whole log-probability row written (what masked_logprobs does; the composition
still computes every row's logits, then indexes).  The four bases are the allowed ids in both.  Both sides are called through prepared
argument records with their outputs allocated once, so the host adds the same little to each.  HIP events around blocks of `--block`
calls, the variants alternating block by block after `--warmup` calls of each; the figure is the median block over `--blocks`, per
call.  Bytes are the algorithm's: what each route has to read and write, computed from the shapes.  Not a test; bench.py is untouched.

    python tools/score_bench.py [--out profiles/score_head.json]
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
from caduceus_amd.generation import _logit_mask  # noqa: E402

COMP = [0, 1, 2, 3, 4, 5, 6, 10, 9, 8, 7, 11, 12, 13, 14, 15]


def _variants(S, rows, D, V, n_gather, dev):
    """{name: (callable, bytes moved)} on one set of inputs."""
    lib = L.get_lib()
    g = torch.Generator().manual_seed(S)
    hidden = torch.randn(S, rows, D, generator=g).to(torch.bfloat16).to(dev)
    weight = torch.randn(V, D, generator=g).to(dev)
    comp = torch.tensor(COMP[:V], device=dev) if S == 2 else None
    targets = torch.randint(7, 11, (rows,), generator=g).to(dev)
    idx = torch.randperm(rows, generator=g)[:n_gather].sort().values.to(dev)
    mask = _logit_mask((7, 8, 9, 10), V, dev)
    logp = torch.empty(rows, device=dev)
    logp_g = torch.empty(n_gather, V, device=dev)
    logits = torch.empty(rows, V, device=dev)
    acc = torch.zeros(2, device=dev)
    keep = [hidden, weight, comp, targets, idx, mask, logp, logp_g, logits, acc]
    stream = L.stream_and_check(hidden)
    code = L.dtype_code(torch.bfloat16)
    a_all = L.LmScoreArgs(L.ptr(hidden), L.ptr(weight), L.ptr(comp), None, L.ptr(targets), L.ptr(mask), L.ptr(logp), None, rows, rows, D, V, S,
                          4, code)
    a_gat = L.LmScoreArgs(L.ptr(hidden), L.ptr(weight), L.ptr(comp), L.ptr(idx), None, L.ptr(mask), None, L.ptr(logp_g), rows, n_gather, D, V,
                          S, 4, code)
    a_fwd = L.LmHeadArgs(L.ptr(hidden), L.ptr(weight), L.ptr(comp), None, L.ptr(logits), C.c_void_p(acc.data_ptr()),
                         C.c_void_p(acc.data_ptr() + 4), rows, D, V, S, 4, code, None)

    def score_all():
        L.check(lib.cad_lm_head_score(C.byref(a_all), stream), "cad_lm_head_score")
        return logp

    def score_gathered():
        L.check(lib.cad_lm_head_score(C.byref(a_gat), stream), "cad_lm_head_score")
        return logp_g

    def composed_all():
        L.check(lib.cad_lm_head_fwd(C.byref(a_fwd), stream), "cad_lm_head_fwd")
        return torch.log_softmax(logits + mask, -1).gather(1, targets[:, None])[:, 0]

    def composed_gathered():
        L.check(lib.cad_lm_head_fwd(C.byref(a_fwd), stream), "cad_lm_head_fwd")
        return torch.log_softmax(logits[idx] + mask, -1)

    hb, wb, lg = S * rows * D * 2, V * D * 4, rows * V * 4
    out = {
        "score_all_rows": (score_all, hb + wb + rows * 8 + rows * 4),
        # logits written and read, the masked sum written and read, log_softmax written and read, the gathered column written
        "composed_all_rows": (composed_all, hb + wb + lg + 2 * lg + 2 * lg + rows * 8 + rows * 4),
        "score_gathered": (score_gathered, S * n_gather * D * 2 + wb + n_gather * 8 + n_gather * V * 4),
        "composed_gathered": (composed_gathered, hb + wb + lg + n_gather * (8 + 5 * V * 4)),
    }
    # the two routes agree (the sizes that are timed)
    torch.testing.assert_close(score_all(), composed_all(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(score_gathered(), composed_gathered(), rtol=1e-4, atol=1e-4)
    return out, keep


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--gather", type=int, default=1024)
    ap.add_argument("--d-model", type=int, default=256)
    ap.add_argument("--vocab", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available() and L.is_device_build(), "score_bench needs the gfx950 library and a GPU"
    version = L.version()
    assert "variant" not in version and "TIMING-BUILD" not in version, f"measure the product build, not {version}"
    dev = torch.device("cuda:0")
    rows_out = []
    with torch.no_grad():
        for S in (2, 1):
            variants, keep = _variants(S, args.rows, args.d_model, args.vocab, args.gather, dev)
            ms = _time(variants, args.blocks, args.block, args.warmup)
            rec = {"n_strands": S}
            for name, (_, nbytes) in variants.items():
                med = statistics.median(ms[name])
                rec[name] = {"ms_per_call_median": round(med, 5), "ms_min": round(min(ms[name]), 5), "ms_max": round(max(ms[name]), 5),
                             "algorithm_bytes": nbytes, "gb_per_s": round(nbytes / med / 1e6, 1)}
            rec["composed_over_score_all_rows"] = round(rec["composed_all_rows"]["ms_per_call_median"] / rec["score_all_rows"]["ms_per_call_median"], 2)
            rec["composed_over_score_gathered"] = round(rec["composed_gathered"]["ms_per_call_median"] / rec["score_gathered"]["ms_per_call_median"], 2)
            rows_out.append(rec)
            print(json.dumps(rec), flush=True)
            del variants, keep
    result = {"tool": "tools/score_bench.py", "library": version, "device": torch.cuda.get_device_name(0), "rows": args.rows,
              "gathered_rows": args.gather, "d_model": args.d_model, "vocab_size": args.vocab, "dtype": "bfloat16", "allowed_token_ids": [7, 8, 9, 10],
              "timing": f"HIP events around blocks of {args.block} calls, variants alternating, median of {args.blocks} blocks after "
                        f"{args.warmup} warm-up calls each; per call",
              "composition": "cad_lm_head_fwd (fp32 logits to memory) + torch.log_softmax(logits + mask) + gather / index",
              "results": rows_out}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
