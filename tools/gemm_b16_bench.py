"""cad_gemm_b16 (strided bf16 MFMA GEMM, csrc/gemm_b16.hip) against torch.mm (hipBLASLt) in the same process on the same GPU, at the generic
engine's products for d_model 256 / L 131072 / two strands (T = 262144 tokens): in_proj, x_proj, dt_proj, out_proj, d(x2d) and the
K-sliced dW_in, on the operand views engine.py and ops._MmB16 hand to the kernel.  The table decides the default of
engine._OWN_GEMM_B16: own >= 0.8 x library throughput on in_proj and out_proj.
usage: python tools/gemm_b16_bench.py [--d-model 256] [--T 262144] [--reps 10] [--out profiles/gemm_b16_bench.txt]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from caduceus_amd import _lib, ops  # noqa: E402


def timeit(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d-model", type=int, default=256)
    ap.add_argument("--T", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    D, T = a.d_model, a.T
    E, R, N = 2 * D, (D + 15) // 16, 16
    g = torch.Generator().manual_seed(0)
    r = lambda *s: (0.5 * torch.randn(*s, generator=g)).to(torch.bfloat16).to(dev)
    x2d, w_in = r(T, D), r(2 * E, D)
    xc, w_x = r(E, T), r(R + 2 * N, E)
    dbc, w_dt = r(R + 2 * N, T), r(E, R)
    y, w_out = r(E, T), r(D, E)
    dxz = r(2 * E, T)
    shapes = {
        "in_proj   W (2E x D) . X^T (D x T)": (lambda f: f(w_in, x2d.t()), 2.0 * 2 * E * D * T),
        "x_proj    W (R+2N x E) . xc (E x T)": (lambda f: f(w_x, xc), 2.0 * (R + 2 * N) * E * T),
        "dt_proj   W (E x R) . dt_lr (R x T)": (lambda f: f(w_dt, dbc[:R]), 2.0 * E * R * T),
        "out_proj  y^T (T x E) . W^T (E x D)": (lambda f: f(y.t(), w_out.t()), 2.0 * D * E * T),
        "d(x2d)    W^T (D x 2E) . dxz (2E x T)": (lambda f: f(w_in.t(), dxz), 2.0 * 2 * E * D * T),
        "dW_in     dxz (2E x T) . X (T x D)  [K = T, sliced]": (lambda f: f(dxz, x2d), 2.0 * 2 * E * D * T),
    }
    lines = [f"# {_lib.version()} | torch {torch.__version__} | {torch.cuda.get_device_name(0)} | d_model {D}, T {T}, bf16, median of {a.reps}",
             f"# {'product':<52} {'library ms':>10} {'own ms':>9} {'library TF/s':>12} {'own TF/s':>9} {'own/library':>11} {'max rel diff':>12}"]
    ratio = {}
    for name, (call, flop) in shapes.items():
        ref = call(torch.mm).float()
        own = call(ops.mm_b16).float()
        err = float((own - ref).abs().max() / ref.abs().max())
        del ref, own
        t_lib, t_own = timeit(lambda: call(torch.mm), a.reps), timeit(lambda: call(ops.mm_b16), a.reps)
        ratio[name.split()[0]] = t_lib / t_own
        lines.append(f"  {name:<52} {t_lib:>10.3f} {t_own:>9.3f} {flop / t_lib / 1e9:>12.1f} {flop / t_own / 1e9:>9.1f} {t_lib / t_own:>11.2f} {err:>12.2e}")
    ok = ratio["in_proj"] >= 0.8 and ratio["out_proj"] >= 0.8
    lines.append(f"# rule: own >= 0.8 x library on in_proj and out_proj -> engine._OWN_GEMM_B16 defaults to {ok}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
