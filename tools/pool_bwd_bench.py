"""Final norm + pooling, forward + backward, through the pool head (ops.pool_head_grad: cad_pool_head, cad_pool_head_bwd) against the
un-fused route it replaces under grad (ops.add_norm, torch.mean, autograd), in one process on one device: median milliseconds per
forward + backward over `--reps` repetitions after `--warmup`, the backward kernel's own median (cad_pool_head_bwd alone, through the
C entry) with its rate over 12 bytes per element (6 read: bf16 x + fp32 residual; 6 written: bf16 dx + fp32 dres_in), and the peak
memory of either route over its inputs.  Prints one JSON line.

    python tools/pool_bwd_bench.py [--S 2 --B 1 --L 131072 --D 256 --reps 30 --warmup 5]"""
import argparse
import ctypes as C
import json
import statistics

import torch

from caduceus_amd import _lib as L
from caduceus_amd import ops


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    for k, v in (("S", 2), ("B", 1), ("L", 131072), ("D", 256), ("reps", 30), ("warmup", 5)):
        ap.add_argument("--" + k, type=int, default=v)
    o = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(o.S, o.B, o.L, o.D, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    res = torch.randn(o.S, o.B, o.L, o.D, generator=g).to(dev).requires_grad_(True)
    w = (1 + 0.1 * torch.randn(o.D, generator=g)).to(dev).requires_grad_(True)
    go = torch.randn(o.S, o.B, o.D, generator=g).to(dev)

    def fused():
        x.grad = res.grad = w.grad = None
        ops.pool_head_grad(x, res, w, None, 1e-5, True, torch.bfloat16, "mean").backward(go)

    def unfused():
        x.grad = res.grad = w.grad = None
        y, _ = ops.add_norm(x, res, w, None, 1e-5, True, False, torch.bfloat16)
        y.mean(2).float().backward(go)

    def peak(fn):
        fn()
        x.grad = res.grad = w.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    out = {"shape": [o.S, o.B, o.L, o.D], "reps": o.reps, "version": L.version()}
    out["fused_ms"], out["fused_min_ms"] = timed(fused, o.reps, o.warmup)
    out["unfused_ms"], out["unfused_min_ms"] = timed(unfused, o.reps, o.warmup)
    out["fused_over_unfused"] = out["fused_ms"] / out["unfused_ms"]
    out["fused_peak_bytes"], out["unfused_peak_bytes"] = peak(fused), peak(unfused)
    # the backward kernel alone
    lib = L.get_lib()
    xd, rd, wd = x.detach(), res.detach(), w.detach()
    dx, dres, dw = torch.empty_like(xd), torch.empty_like(rd), torch.empty_like(wd)
    scratch = torch.empty(lib.cad_pool_head_bwd_scratch_floats(o.S, o.B, o.L, o.D, L.POOL_MEAN, 0), device=dev)
    stream = L.stream_and_check(xd, rd, wd, go, dx, dres, dw, scratch)
    a = L.PoolHeadBwdArgs(L.ptr(xd), L.ptr(rd), L.ptr(wd), None, None, L.ptr(go), None, L.ptr(dx), L.ptr(dres), L.ptr(dw), None, None,
                          L.ptr(scratch), o.B, o.L, 0, o.S, o.D, 1e-5, 1, L.CAD_BF16, L.CAD_BF16, L.POOL_MEAN)
    ms, mn = timed(lambda: L.check(lib.cad_pool_head_bwd(C.byref(a), stream), "cad_pool_head_bwd"), o.reps, o.warmup)
    out["bwd_kernel_ms"], out["bwd_kernel_min_ms"] = ms, mn
    out["bwd_kernel_TBps_over_12B"] = 12 * xd.numel() / (ms * 1e-3) / 1e12
    print(json.dumps(out))


if __name__ == "__main__":
    main()
