"""Microseconds per decode token per layer: the step kernels (ops.mamba_step, three launches) against the same step composed from the
full-sequence ops (ops.mm, ops.causal_conv1d on a d_conv-long window, ops.selective_scan_stateful at L = 1), on the same device in the
same run.  d_model 256, batch 1 and 8, bf16 and fp32; HIP events around `--steps` steps (default 400, at least 200) after `--warmup`.
The composition is the baseline because nothing else could step before the step kernels existed; its weights are cast once outside the
timed loop and its states are kept in the layouts its ops want, so it is the composition at its best.  Not a test; bench.py is untouched.

    python tools/decode_bench.py [--out profiles/decode_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from caduceus_amd import _lib, engine, ops  # noqa: E402
from caduceus_amd.mamba import Mamba  # noqa: E402


def _time_us(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / steps


def _launches(fn):
    """Device kernels one call of fn launches (the profiler's count), or None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:  # noqa: BLE001
        return None


def _own_step(m, B, act, dev):
    conv, ssm = m.allocate_inference_cache(B, 1, dtype=act)
    h = torch.randn(B, 1, m.d_model, device=dev).to(act)
    return lambda: m.step(h, conv, ssm)


def _composed_step(m, B, act, dev):
    E, N, R, K = m.d_inner, m.d_state, m.dt_rank, m.d_conv
    own = engine._OWN_GEMM_B16
    w_in, w_x, w_dt, w_outT = (m.in_proj.weight.to(act), m.x_proj.weight.to(act), m.dt_proj.weight.to(act),
                               m.out_proj.weight.to(act).t())
    A, Dp, dt_bias = -torch.exp(m.A_log.float()), m.D.float(), m.dt_proj.bias.float()
    conv = torch.zeros(E, B, K, device=dev, dtype=act)   # channel-major, as the conv wants it
    ssm = torch.zeros(E, B, N, device=dev)                # (E, SB, N), as the scan's carries are
    h = torch.randn(B, m.d_model, device=dev).to(act)

    def step():
        xz = ops.mm(w_in, h.t(), own_b16=own)                                   # (2E, B)
        conv.copy_(torch.cat([conv[:, :, 1:], xz[:E].unsqueeze(2)], dim=2))
        xc = ops.causal_conv1d(conv, m.conv1d.weight, m.conv1d.bias, B, 0, 1)[:, :, K - 1:].contiguous()  # (E, B, 1)
        dbc = ops.mm(w_x, xc.view(E, B), own_b16=own)                            # (R + 2N, B)
        delta = ops.mm(w_dt, dbc[:R], own_b16=own)
        y, hT = ops.selective_scan_stateful(xc, delta.view(E, B, 1), A, dbc[R:R + N].view(N, B, 1), dbc[R + N:].view(N, B, 1), Dp,
                                            xz[E:].view(E, B, 1), dt_bias, ssm, B, 0, 1)
        ssm.copy_(hT)
        return ops.mm(y.view(E, B).t(), w_outT, own_b16=own)

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--d-model", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.steps >= 200, "at least 200 timed steps"
    assert torch.cuda.is_available() and _lib.is_device_build(), "decode_bench needs the gfx950 library and a GPU"
    version = _lib.version()
    assert "variant" not in version and "TIMING-BUILD" not in version, f"measure the product build, not {version}"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = Mamba(args.d_model, layer_idx=0).to(dev).eval()
    rows = []
    with torch.no_grad():
        for act in (torch.bfloat16, torch.float32):
            for B in (1, 8):
                own, comp = _own_step(m, B, act, dev), _composed_step(m, B, act, dev)
                rec = {"dtype": str(act).split(".")[1], "batch": B,
                       "own_us_per_token_per_layer": round(_time_us(own, args.steps, args.warmup), 2),
                       "composed_us_per_token_per_layer": round(_time_us(comp, args.steps, args.warmup), 2),
                       "own_launches_per_layer": _launches(own), "composed_launches_per_layer": _launches(comp)}
                rec["composed_over_own"] = round(rec["composed_us_per_token_per_layer"] / rec["own_us_per_token_per_layer"], 2)
                rows.append(rec)
                print(json.dumps(rec), flush=True)
    result = {"tool": "tools/decode_bench.py", "library": version, "device": torch.cuda.get_device_name(0), "d_model": args.d_model,
              "steps": args.steps, "warmup": args.warmup, "own_gemm_b16": bool(engine._OWN_GEMM_B16), "results": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
