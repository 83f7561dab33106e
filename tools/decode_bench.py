"""Microseconds per decode token per layer: the step kernels (ops.mamba_step, three launches) against the same step composed from the
full-sequence ops (ops.mm, ops.causal_conv1d on a d_conv-long window, ops.selective_scan_stateful at L = 1), on the same device in the
same run.  d_model 256, batch 1 and 8, bf16 and fp32; HIP events around `--steps` steps (default 400, at least 200) after `--warmup`.
The composition is the baseline because nothing else could step before the step kernels existed; its weights are cast once outside the
timed loop and its states are kept in the layouts its ops want, so it is the composition at its best.  Not a test; bench.py is untouched.

    python tools/decode_bench.py [--out profiles/decode_bench.json]

--stack: microseconds per GENERATED token of a whole causal model (d_model 256, n_layer 16, vocab 12 padded to 16; bf16 and fp32, batch 1
and 8) through the three public paths, in this process on this device: generate's greedy loop over decode_step, generate(..., fused=True)
greedy, and generate(..., fused=True) sampled (top_k 0, top_p 0.9, temperature 0.8, the four bases allowed).  Wall clock around whole
generate calls of `--steps` new tokens behind a device synchronisation (the host's share is the point), best of three.

    python tools/decode_bench.py --stack [--out profiles/decode_stack_d256.json]
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


def _stack(args, version, dev):
    import time
    from caduceus_amd import CaduceusConfig, CaduceusForMaskedLM
    from caduceus_amd.generation import generate
    torch.manual_seed(0)
    cfg = CaduceusConfig(d_model=args.d_model, n_layer=args.n_layer, vocab_size=12, pad_vocab_size_multiple=8, bidirectional=False,
                         rcps=False, rms_norm=True, fused_add_norm=True, residual_in_fp32=True, pad_token_id=4)
    model = CaduceusForMaskedLM(cfg).to(dev).eval()
    with torch.no_grad():
        model.get_input_embeddings().weight.normal_(std=0.5)
    sampled = dict(top_k=0, top_p=0.9, temperature=0.8, seed=1, allowed_token_ids=(7, 8, 9, 10))
    paths = {"loop_greedy": {}, "fused_greedy": dict(fused=True), "fused_sampled": dict(fused=True, **sampled)}

    def us_per_token(kw, prompt):
        best = None
        for rep in range(4):  # (the first repetition warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate(model, prompt, args.steps, **kw)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e6 / args.steps
            best = dt if rep == 1 else (min(best, dt) if rep > 1 else None)
        return round(best, 2)

    def issue_and_total_us(prompt, tokens=20):
        """Whether the fused token waits for the host or for the device: `tokens` steps (49 launches each at 16 layers, few enough to
        stay inside the launch queue) issued back to back -- the host's time to issue them, and the time until the device has run them."""
        from caduceus_amd.generation import DecodeStack
        stack = DecodeStack(model, prompt.shape[0])
        stack.prefill(prompt)
        best = None
        for rep in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(tokens):
                stack.step()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rep and (best is None or t2 - t0 < best[1]):
                best = (t1 - t0, t2 - t0)
        return round(best[0] * 1e6 / tokens, 2), round(best[1] * 1e6 / tokens, 2)

    rows = []
    for act in (torch.bfloat16, torch.float32):
        for B in (1, 8):
            prompt = torch.randint(7, 11, (B, 8), device=dev)
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=act == torch.bfloat16):
                rec = {"dtype": str(act).split(".")[1], "batch": B}
                for name, kw in paths.items():
                    rec[name + "_us_per_token"] = us_per_token(kw, prompt)
                rec["fused_step_host_issue_us_per_token"], rec["fused_step_issued_and_run_us_per_token"] = issue_and_total_us(prompt)
            rec["loop_over_fused_greedy"] = round(rec["loop_greedy_us_per_token"] / rec["fused_greedy_us_per_token"], 2)
            rec["loop_over_fused_sampled"] = round(rec["loop_greedy_us_per_token"] / rec["fused_sampled_us_per_token"], 2)
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    return {"tool": "tools/decode_bench.py --stack", "library": version, "device": torch.cuda.get_device_name(0), "d_model": args.d_model,
            "n_layer": args.n_layer, "vocab_size": model.config.vocab_size, "new_tokens_per_call": args.steps, "prompt": 8,
            "timing": "wall clock around generate() between device synchronisations, best of 3 after one warm-up call",
            "issue_timing": "fused_step_*: 20 DecodeStack.step() calls issued back to back, best of 5: host time to issue them / time until the device has run them",
            "launches_per_token_fused": 3 * args.n_layer + 1, "sampled": {k: v for k, v in sampled.items()}, "results": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stack", action="store_true", help="whole-model generation paths instead of one layer's step")
    ap.add_argument("--n-layer", type=int, default=16)
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
    if args.stack:
        result = _stack(args, version, dev)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
        print(json.dumps(result))
        return
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
