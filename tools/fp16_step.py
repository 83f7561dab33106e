"""Same-box timing of the headline training step (Caduceus-PS, d_model 256, 16 layers, seqlen 131072, batch 1: bench.py's model,
batch and AdamW) three ways in ONE process on one GPU:

    bf16          bf16 autocast (bench.py --dtype bf16)
    fp16          fp16 autocast with the opt-in fp16 kernels (caduceus_amd.fp16_kernels) + torch.amp.GradScaler
    fp16_via_fp32 fp16 autocast without the opt-in: the fp32 kernels serve the request (+ GradScaler)

The modes alternate in blocks of --steps steps for --rounds rounds (same clocks and power state for all three); the median block is
reported.  One extra step per mode runs with the library's HIP-event profiler on, for the per-kernel-family split.

    python tools/fp16_step.py [--rounds 3] [--steps 4] [--out profiles/fp16_step.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import make_config, synthetic_batch  # noqa: E402
from caduceus_amd import CaduceusForMaskedLM, _lib, fp16_kernels  # noqa: E402

MODES = ("bf16", "fp16", "fp16_via_fp32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqlen", type=int, default=131072)
    ap.add_argument("--d-model", type=int, default=256)
    ap.add_argument("--n-layer", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result JSON here")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(2222)
    model = CaduceusForMaskedLM(make_config(args.d_model, args.n_layer)).to(dev).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, betas=(0.9, 0.95), fused=True)
    gen = torch.Generator().manual_seed(2222)
    batches = [synthetic_batch(gen, 1, args.seqlen, dev) for _ in range(4)]
    scalers = {m: torch.amp.GradScaler("cuda", init_scale=2.0 ** 12) for m in ("fp16", "fp16_via_fp32")}

    def step(mode, i):
        ids, labels = batches[i % len(batches)]
        opt.zero_grad(set_to_none=True)
        amp = torch.bfloat16 if mode == "bf16" else torch.float16
        with fp16_kernels(mode == "fp16"), torch.autocast("cuda", dtype=amp):
            loss = model(ids, labels=labels).loss
        if mode == "bf16":
            loss.backward()
            opt.step()
        else:
            sc = scalers[mode]
            sc.scale(loss).backward()
            sc.step(opt)
            sc.update()
        return loss

    blocks = {m: [] for m in MODES}
    peak = {}
    for m in MODES:  # warm-up (and the peak memory of a step of each mode)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for i in range(args.warmup):
            step(m, i)
        torch.cuda.synchronize()
        peak[m] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    for r in range(args.rounds):
        for m in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                loss = step(m, i)
            torch.cuda.synchronize()
            blocks[m].append((time.perf_counter() - t0) * 1e3 / args.steps)
            assert torch.isfinite(loss), (m, float(loss))
    families = {}
    for m in MODES:
        _lib.prof_reset()
        _lib.prof_enable(True)
        step(m, 0)
        torch.cuda.synchronize()
        families[m] = {k: round(ms, 3) for k, (ms, n) in _lib.prof_read().items() if n}
        _lib.prof_enable(False)
    ms = {m: round(statistics.median(v), 2) for m, v in blocks.items()}
    res = {"metric": "train_step_ms", "shape": f"PS d{args.d_model} n{args.n_layer} L{args.seqlen} B1",
           "device": torch.cuda.get_device_name(0), "library": _lib.version(), "step_ms_median": ms,
           "step_ms_blocks": {m: [round(x, 2) for x in v] for m, v in blocks.items()},
           "fp16_over_bf16": round(ms["fp16"] / ms["bf16"], 3), "fp16_over_fp16_via_fp32": round(ms["fp16"] / ms["fp16_via_fp32"], 3),
           "peak_memory_gb": peak, "kernel_family_ms_one_step": families}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
