"""Seconds per call of attribute(..., method="grad_x_input") against the route that was possible before it existed
(inputs_embeds.requires_grad_(), the ordinary full backward with every weight gradient, a torch product of the (B, L, 2 D) gradient with
the embedding table), on the same device in the same process.

Model: Caduceus-PS, d_model 256, 16 layers, bf16 autocast, batch 1, L = 131072, a masked-LM target at one position, the four bases
allowed.  The two routes alternate call by call after `--warmup` calls of each; every call ends in a device synchronise inside the host
clock; the figure is the median over `--reps` calls.  Both routes' results are compared at the timed size.  The launch lists are the
library calls (cad_* entry points that launch, host queries left out) of one call of each route, counted by name.
The measurement runs in ONE child process under its own time limit; a child that fails or runs out of time is reported, not retried.

    python tools/attrib_time.py [--out profiles/attrib_time.txt]
"""
import argparse
import collections
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ALLOWED = [7, 8, 9, 10]
MASK_ID = 3
# host queries of the C-ABI (everything else launches)
QUERY_SUFFIX = ("_supported", "_partials", "_slots", "_floats", "_chunk_len", "_entries", "_ints", "_pieces", "_chunk_rows")
QUERY_NAMES = ("cad_version", "cad_status_string", "cad_is_device_build", "cad_stream_probe")


def _is_query(name):
    return name in QUERY_NAMES or (name.endswith(QUERY_SUFFIX) and name != "cad_reduce_partials")


class _Recorder:
    """Stands in for the bound library: every cad_* call is noted, then made."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("cad_"):
            return fn

        def call(*args):
            self._calls.append(name)
            return fn(*args)
        return call


def _launches(fn):
    from caduceus_amd import _lib
    real, calls = _lib.get_lib(), []
    _lib._lib = _Recorder(real, calls)
    try:
        fn()
    finally:
        _lib._lib = real
    return collections.Counter(c for c in calls if not _is_query(c))


def worker(args, dev=None):
    import torch

    import bench
    from caduceus_amd import CaduceusForMaskedLM, MaskedTarget, _lib, attribute
    if dev is None:
        assert torch.cuda.is_available() and _lib.is_device_build(), "attrib_time needs the gfx950 library and a GPU"
        dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    torch.manual_seed(0)
    model = CaduceusForMaskedLM(bench.make_config(args.d_model, args.n_layer)).to(dev).train()
    Lq = args.seq_len
    ids = torch.randint(7, 11, (1, Lq), generator=torch.Generator().manual_seed(1)).to(dev)
    pos, tok = torch.tensor([Lq // 2], device=dev), torch.tensor([8], device=dev)
    target = MaskedTarget(pos, tok, mask_token_id=MASK_ID)
    we = model.get_input_embeddings()
    al = torch.tensor(ALLOWED, device=dev)
    tok_col = ALLOWED.index(8)

    def ours():
        with torch.autocast(dev.type, dtype=torch.bfloat16):
            return attribute(model, ids, target, allowed_token_ids=ALLOWED, method="grad_x_input")

    def hand():
        with torch.autocast(dev.type, dtype=torch.bfloat16):
            masked = ids.clone()
            masked[0, pos] = MASK_ID
            emb = we(masked).detach().requires_grad_(True)                      # (1, L, 2 D), reference frame
            hidden_t = model.caduceus.backbone.forward_tframe(None, emb)          # (2, 1, L, D)
            logits, _ = model.logits_tframe(hidden_t[:, :, pos], None, -100)      # (1, 1, V)
            logp = torch.log_softmax(logits[0, 0].float()[al], -1)
            logp[tok_col].backward()
        model.zero_grad(set_to_none=True)
        E, D = we.weight.detach().float(), we.weight.shape[1]
        g = emb.grad[0].float()
        full = g[:, :D] @ E.t() + g[:, D:] @ E[we.complement_map].flip(-1).t()    # (L, V): the strands recombined
        c = full[:, al]
        c = c - c.mean(-1, keepdim=True)
        col = torch.full((E.shape[0],), -1, dtype=torch.int64, device=dev)
        col[al] = torch.arange(len(ALLOWED), device=dev)
        k = col[masked[0]]
        return torch.where(k >= 0, c.gather(1, k.clamp_min(0)[:, None])[:, 0], torch.zeros_like(c[:, 0]))[None]

    routes = {"attribute": ours, "hand_route": hand}
    outs = {}
    for name, fn in routes.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    sync()
    a, b = outs["attribute"].double(), outs["hand_route"].double()
    rel = float((a - b).norm() / b.norm())
    secs = {k: [] for k in routes}
    for _ in range(args.reps):
        for name, fn in routes.items():  # alternating
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            secs[name].append(time.perf_counter() - t0)
    lists = {name: _launches(fn) for name, fn in routes.items()}
    sync()
    med = {k: statistics.median(v) for k, v in secs.items()}
    lines = [f"tool: tools/attrib_time.py   library: {_lib.version()}   device: {torch.cuda.get_device_name(0) if dev.type == 'cuda' else dev}",
             f"model: Caduceus-PS d_model {args.d_model}, {args.n_layer} layers, bf16 autocast, batch 1, L = {Lq}, masked-LM target, "
             f"allowed ids {ALLOWED}",
             f"timing: host clock around one call ending in a device synchronise, routes alternating, median of {args.reps} calls after "
             f"{args.warmup} warm-up calls each",
             f"results agree at this size: relative L2 difference of grad_x_input {rel:.3e} (bit-identical: {bool(torch.equal(a, b))})"]
    for k in routes:
        lines.append(f"{k}: median {med[k] * 1e3:.2f} ms   min {min(secs[k]) * 1e3:.2f} ms   max {max(secs[k]) * 1e3:.2f} ms   "
                     f"library launches per call {sum(lists[k].values())}")
    lines.append(f"hand_route / attribute = {med['hand_route'] / med['attribute']:.3f}")
    for k in routes:
        lines.append(f"launches of one {k} call: " + ", ".join(f"{n} x{c}" for n, c in sorted(lists[k].items())))
    only = sorted(set(lists["hand_route"]) - set(lists["attribute"]))
    lines.append("launched by the hand route only: " + (", ".join(only) or "none"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d-model", type=int, default=256)
    ap.add_argument("--n-layer", type=int, default=16)
    ap.add_argument("--seq-len", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attrib_time.txt"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"] + [a for a in sys.argv[1:] if a != "--worker"]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"attrib_time: the measurement did not finish within {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
