"""Milliseconds per launch of the unmask head (cad_lm_head_unmask) next to the score head writing every row's log-probabilities
(cad_lm_head_score with logp_all) on the same hidden state, and next to the forward it follows in an infill round
(backbone.forward_tframe of the headline model, Caduceus-PS d_model 256, n_layer 16, one sequence of `rows` positions, bf16 autocast).

Shape: rows = 131072, D = 256, S = 2, bf16 hidden, V = 16, the four bases allowed.  The unmask head once with every row open and once
with 15 % of the rows open (Bernoulli per row, seeded), sampled (top_k 0, temperature 0.8) so that the whole sampler runs.  The kernels
are called through prepared argument records with their outputs allocated once.  HIP events around single launches after `--warmup`
launches each, the variants alternating; the figure is the median over `--reps` launches.  Not a test; bench.py is untouched.

    python tools/unmask_bench.py [--out profiles/unmask_head.json] [--no-forward]
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
from caduceus_amd import ops  # noqa: E402
from caduceus_amd.generation import _logit_mask  # noqa: E402

COMP = [0, 1, 2, 3, 4, 5, 6, 10, 9, 8, 7, 11, 12, 13, 14, 15]
MASK_ID = 3


def _median_ms(fns, reps, warmup):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():  # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {k: {"ms_median": round(statistics.median(v), 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--d-model", type=int, default=256)
    ap.add_argument("--n-layer", type=int, default=16)
    ap.add_argument("--open-share", type=float, default=0.15)
    ap.add_argument("--reps", type=int, default=41)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available() and L.is_device_build(), "unmask_bench needs the gfx950 library and a GPU"
    version = L.version()
    assert "variant" not in version and "TIMING-BUILD" not in version, f"measure the product build, not {version}"
    dev = torch.device("cuda:0")
    lib = L.get_lib()
    rows, D, V, S = args.rows, args.d_model, 16, 2
    g = torch.Generator().manual_seed(1)
    hidden = torch.randn(S, rows, D, generator=g).to(torch.bfloat16).to(dev)
    weight = torch.randn(V, D, generator=g).to(dev)
    comp = torch.tensor(COMP, device=dev)
    mask = _logit_mask((7, 8, 9, 10), V, dev)
    bases = torch.randint(7, 11, (rows,), generator=g)
    ids_all = torch.full((rows,), MASK_ID, dtype=torch.int64).to(dev)
    ids_part = torch.where(torch.rand(rows, generator=g) < args.open_share, torch.tensor(MASK_ID), bases).to(dev)
    ids_out, conf = torch.empty(rows, dtype=torch.int64, device=dev), torch.empty(rows, device=dev)
    logp_all = torch.empty(rows, V, device=dev)
    stream = L.stream_and_check(hidden)
    code = L.dtype_code(torch.bfloat16)
    sampler = ops.sampler_args(0, 0.0, 0.8, 11, 0, 0, mask)
    mk = lambda ids: L.LmUnmaskArgs(L.ptr(hidden), L.ptr(weight), L.ptr(comp), L.ptr(ids), L.ptr(ids_out), L.ptr(conf), None, sampler, rows,
                                    rows, D, V, S, MASK_ID, code)
    a_all, a_part = mk(ids_all), mk(ids_part)
    a_score = L.LmScoreArgs(L.ptr(hidden), L.ptr(weight), L.ptr(comp), None, None, L.ptr(mask), None, L.ptr(logp_all), rows, rows, D, V, S, 4,
                            code)
    fns = {
        "unmask_all_open": lambda: L.check(lib.cad_lm_head_unmask(C.byref(a_all), stream), "cad_lm_head_unmask"),
        "unmask_part_open": lambda: L.check(lib.cad_lm_head_unmask(C.byref(a_part), stream), "cad_lm_head_unmask"),
        "score_logp_all": lambda: L.check(lib.cad_lm_head_score(C.byref(a_score), stream), "cad_lm_head_score"),
    }
    with torch.no_grad():
        res = _median_ms(fns, args.reps, args.warmup)
        # the three agree on the rows that are timed: the score of the drawn id is the confidence
        fns["unmask_all_open"]()
        fns["score_logp_all"]()
        assert torch.equal(logp_all.gather(1, ids_out[:, None])[:, 0], conf)
        res["open_rows_part"] = int((ids_part == MASK_ID).sum())
        if not args.no_forward:
            sys.path.insert(0, ROOT)
            from bench import make_config
            from caduceus_amd import CaduceusForMaskedLM
            model = CaduceusForMaskedLM(make_config(args.d_model, args.n_layer)).to(dev).eval()
            seq = ids_part.reshape(1, rows)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                fwd = {"forward_tframe": lambda: model.caduceus.backbone.forward_tframe(seq)}
                res.update(_median_ms(fwd, max(5, args.reps // 4), 2))
    result = {"tool": "tools/unmask_bench.py", "library": version, "device": torch.cuda.get_device_name(0), "rows": rows, "d_model": D,
              "n_strands": S, "vocab_size": V, "dtype": "bfloat16", "allowed_token_ids": [7, 8, 9, 10], "sampler": "top_k 0, temperature 0.8",
              "timing": f"HIP events around single launches, variants alternating, median of {args.reps} after {args.warmup} warm-up launches",
              "results": res}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
