"""The scan backward's cross-channel sums dB / dC (per-workgroup partial slots + one of three folds) and its sums over positions dA / dD /
d(bias), element by element against an fp64 restatement (oracle.oracle_ops.scan_bwd_sums_f64), at the fold depths of the production
layers (64 and 128 slots) and with bounds derived from how the kernel rounds (check_sum below).  The reference reduces dB / dC over the
channels inside selective_scan_cuda.bwd (mamba_inner_fn reached from /root/reference/caduceus/modeling_caduceus.py:11,128,130).

The C-ABI cases call cad_scan_bwd_multi directly so that the raw slots can be read; each case is folded by every fold that serves it:
cad_reduce_partials_multi, cad_fold_partials_stream (mode CAD_FOLD_ALL), ops.fold_behind_scan with the real scan (the concurrent path of
the training step) and the L-split (ops.scan_bwd_launch, k = 2 and 4).  Negative controls perturb the device's own slots on the host and
show that the bounds reject the perturbation."""
import ctypes as C
import time

import pytest
import torch

from caduceus_amd import _lib as CL
from caduceus_amd import ops
from oracle import oracle_ops

CHUNK = 512
BF16 = dict(rtol=3e-2, atol=5e-2)   # the classes of tests/test_kernels.py
FP32 = dict(rtol=6e-4, atol=2e-3)
U32 = 2.0 ** -24                    # unit roundoff of binary32

# Rounding of the kernel's dB / dC path, per activation dtype (include/caduceus_hip.h, csrc/scan_bwd.hip):
#   channel: bf16 activations (packed slab): every channel's term g dt u / dy h is rounded to bf16 (v_cvt_pk_bf16_f32, nearest even)
#            before the 8-channel sum on the matrix core (fp32 accumulation); fp16 / fp32: the channel terms are summed in fp32
#   slot:    the workgroup's sum is stored as bf16 (bf16 and fp16 activations, nearest even) or fp32
#   dst:     the fold adds the slots in fp32 and rounds once to the activation dtype; fp16 also has an absolute error floor, half its
#            subnormal spacing 2^-24
# A rounding to nearest errs by at most u |value|, u the unit roundoff: 2^-8 for bf16 (8 significant bits), 2^-11 for fp16, 2^-24 for
# fp32.  The bound takes 2 u (a margin of two).
UNITS = {torch.bfloat16: dict(channel=2.0 ** -8, slot=2.0 ** -8, dst=2.0 ** -8, floor=0.0),
         torch.float16: dict(channel=0.0, slot=2.0 ** -8, dst=2.0 ** -11, floor=2.0 ** -25),
         torch.float32: dict(channel=0.0, slot=U32, dst=U32, floor=0.0)}
# kappa: the kernel's own fp32 recurrence against the fp64 one, per channel term relative to |p_e|.  A term is a product of a few
# rounded factors (exp2 of the fp32-rounded dt A log2(e), dt, u, C dy) and of the state (gradient) recurrence, whose error grows by a
# few roundings per step over its memory 1 / (dt |A|): <= 64 steps at these inputs (dt >= 0.02, |A| >= 0.5 where the state lives
# long), <= 8 roundings per step, a factor 2 for the cancellation inside the state sums: 64 * 8 * 2 = 2^10 units of binary32 = 2^-14.
KAPPA = 2.0 ** -14
RESULTS = {}  # case id -> worst err / tol per checked output (printed; -s shows them)


def slot_width(E: int) -> int:
    """Channels per partial slot: the largest channel count that still fits one slot (cad_scan_bwd_partials(E) = ceil(E / W)).
    (ceil(E / cad_scan_bwd_partials(E)) is not it: E = 20 gives 7, the kernel's slots hold 8 + 8 + 4.)"""
    lib = CL.get_lib()
    W = 1
    while lib.cad_scan_bwd_partials(W + 1) == 1:
        W += 1
    assert lib.cad_scan_bwd_partials(E) == -(-E // W)
    return W


def check_sum(what, got, S, Ag, Ae, act, G, case):
    """|got - S| <= 2 u_ch Ae + 2 u_slot Ag + 2 u_dst |S| + (G / 8 + 8) u32 Ag + kappa Ae + floor, element by element.
    S = sum_e p_e (fp64), Ag = sum_g |P_g| (P_g: slot g's channel sum), Ae = sum_e |p_e|.  The fp32 fold adds the slots in groups of 8
    (CAD_FOLD_GROUP) and the group sums left to right: no element passes through more than G / 8 + 8 additions."""
    u = UNITS[act]
    tol = (2 * u["channel"] + KAPPA) * Ae + (2 * u["slot"] + (G // 8 + 8) * U32) * Ag + 2 * u["dst"] * S.abs() + 2 * u["floor"]
    return _report(what, got.double(), S, tol, case)


def check_param(what, got, ref, absum, act, L_row, rows, case):
    """|got - ref| <= kappa' sum|terms| for the fp32 sums over positions (dA, dD, d(bias)).  A lane sums its 8 positions per chunk of its
    channel sequentially over the chunks (L_row / 64 additions), the 64 lanes are folded in 6 steps, the rows and segments arrive by fp32
    atomics: kappa' = kappa + (L_row / 64 + 6 + rows) u32."""
    tol = (KAPPA + (L_row / 64 + 6 + rows) * U32) * absum
    return _report(what, got.double(), ref, tol, case)


def _report(what, got, ref, tol, case):
    got, ref, tol = got.to(ref.device), ref, tol
    err = (got - ref).abs()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
    ratio = torch.where(torch.isnan(got), float("inf"), ratio)
    worst = float(ratio.max())
    RESULTS.setdefault(case, {})[what] = max(worst, RESULTS.get(case, {}).get(what, 0.0))
    if not worst <= 1.0:
        i = int(torch.argmax(torch.nan_to_num(ratio, posinf=1e300)))
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape))
        nbad = int((ratio > 1).sum())
        raise AssertionError(f"{case}: {what}{list(idx)} = {float(got.flatten()[i]):.9g}, fp64 {float(ref.flatten()[i]):.9g}, "
                             f"|err| {float(err.flatten()[i]):.3g} > tol {float(tol.flatten()[i]):.3g} (err/tol {worst:.3g}; "
                             f"{nbad} of {ratio.numel()} elements out of bounds)")
    return worst


def rejected_fraction(got, S, Ag, Ae, act, G, mask=None):
    u = UNITS[act]
    tol = (2 * u["channel"] + KAPPA) * Ae + (2 * u["slot"] + (G // 8 + 8) * U32) * Ag + 2 * u["dst"] * S.abs() + 2 * u["floor"]
    bad = (got.double() - S).abs() > tol
    return float(bad[mask].double().mean()) if mask is not None else float(bad.double().mean())


# ---- inputs, device run ----------------------------------------------------------------------------------------------------------------
def make_inputs(E, SB, L, N, act, nsets, seed, delta_is_dt):
    """CPU fp32 masters holding exactly the act-rounded values the kernel sees.  One gate and one dout for all sets (the shared gate of
    a BiMamba layer: both scans are gated by z and receive the same gradient); a few exact-zero gates (the fix-up worklist)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    q = lambda t: t.to(act).float()
    sets = []
    for _ in range(nsets):
        t = dict(u=q(r(E, SB, L)), A=-(0.5 + 15.5 * torch.rand(E, N, generator=g)), B=q(r(N, SB, L)), C=q(r(N, SB, L)), D=r(E),
                 bias=r(E) - 3.0)
        raw = r(E, SB, L)
        if delta_is_dt:  # dt as the dt_proj epilogue stores it
            t["delta"] = q(torch.nn.functional.softplus(0.5 * raw - 1.0 + t["bias"][:, None, None]))
        else:
            t["delta"] = q(raw)
        sets.append(t)
    z = q(r(E, SB, L))
    z[1, 0, 3] = 0.0
    z[E - 1, SB - 1, L - 1] = 0.0
    z[E // 2, SB // 2, L // 2] = 0.0
    dout = q(r(E, SB, L))
    return sets, z, dout


def run_device(dev, sets, z, dout, split, dirs, act, delta_is_dt, k=1, stream_counters=False):
    """Forward (for `out` and the chunk states) + backward through the C ABI, the way mixer.py builds the launch: set 0 writes the gate
    gradient of both sets (out2 = set 1's output).  Returns (per-set dicts of device outputs, slots, keep-alive)."""
    lib = CL.get_lib()
    nsets = len(sets)
    E, SB, L = sets[0]["u"].shape
    N = sets[0]["A"].shape[1]
    Lk = L // k
    dcode = CL.dtype_code(act)
    on = lambda t, dt=act: t.to(dev).to(dt).contiguous()
    zd, dyd = on(z), on(dout)
    fa = (CL.ScanArgs * nsets)()
    ds = []
    for i, t in enumerate(sets):
        d = dict(u=on(t["u"]), delta=on(t["delta"]), B=on(t["B"]), C=on(t["C"]), A=on(t["A"], torch.float32),
                 D=on(t["D"], torch.float32), bias=on(t["bias"], torch.float32))
        d["out"] = torch.empty_like(d["u"])
        d["state"] = torch.empty((int(lib.cad_scan_state_floats(E, SB * k, Lk, N)),), dtype=torch.float32, device=dev)
        fa[i] = CL.ScanArgs(CL.ptr(d["u"]), CL.ptr(d["delta"]), CL.ptr(d["A"]), CL.ptr(d["B"]), CL.ptr(d["C"]), CL.ptr(d["D"]),
                            CL.ptr(zd), CL.ptr(d["bias"]), CL.ptr(d["out"]), CL.ptr(d["state"]), SB * k, Lk, split * k, E, N,
                            dirs[i][0], dirs[i][1], dcode)
        fa[i].delta_is_dt = int(delta_is_dt)
        ds.append(d)
    stream = CL.stream_and_check(zd, dyd, *[x for d in ds for x in d.values()])
    keep_f, Ps = ops.scan_fwd_launch(lib, fa, nsets, stream, k, [d["A"] for d in ds], dirs, split)
    npart = int(lib.cad_scan_bwd_partials(E))
    dz = torch.empty_like(zd)
    ba = (CL.ScanBwdArgs * nsets)()
    nci = int(lib.cad_scan_bwd_fold_counter_ints(SB * k, Lk))
    counters = torch.zeros((nsets, nci), dtype=torch.int32, device=dev)
    for i, d in enumerate(ds):
        d["du"], d["ddelta"] = torch.empty_like(d["u"]), torch.empty_like(d["u"])
        d["dA"], d["dD"], d["dbias"] = torch.zeros_like(d["A"]), torch.zeros_like(d["D"]), torch.zeros_like(d["bias"])
        d["slots"] = torch.full((2, npart, N, SB, L), float("nan"), dtype=ops.scan_slot_dtype(act), device=dev)
        d["fix_list"], d["fix_cnt"] = ops.gate_fix_buffers(lib, d["u"], N)
        ba[i] = CL.ScanBwdArgs(CL.ptr(d["u"]), CL.ptr(d["delta"]), CL.ptr(d["A"]), CL.ptr(d["B"]), CL.ptr(d["C"]), CL.ptr(d["D"]),
                               CL.ptr(zd), CL.ptr(d["bias"]), CL.ptr(dyd), CL.ptr(d["out"]), CL.ptr(d["state"]), CL.ptr(d["du"]),
                               CL.ptr(d["ddelta"]), CL.ptr(dz) if i == 0 else None, CL.ptr(d["dA"]), CL.ptr(d["slots"][0]),
                               CL.ptr(d["slots"][1]), CL.ptr(d["dD"]), CL.ptr(d["dbias"]), SB * k, Lk, split * k, E, N,
                               dirs[i][0], dirs[i][1], dcode, npart, None, None,
                               CL.ptr(ds[1]["out"]) if (i == 0 and nsets == 2) else None, CL.ptr(d["fix_list"]),
                               CL.ptr(d["fix_cnt"]), CL.ptr(dz))
        ba[i].delta_is_dt = int(delta_is_dt)
        if stream_counters:
            ba[i].fold_counters = CL.ptr(counters[i])
    launch = lambda: ops.scan_bwd_launch(lib, ba, nsets, stream, k, Ps, dirs, split)
    return ds, dz, dict(lib=lib, launch=launch, ba=ba, stream=stream, npart=npart, counters=counters, keep=(keep_f, fa, zd, dyd),
                        SB=SB, L=L, N=N, k=k, split=split, dirs=dirs, act=act)


def fold_args(ds, run, counters, give_ups):
    SB, L, N, k, split, npart = run["SB"], run["L"], run["N"], run["k"], run["split"], run["npart"]
    fa = (CL.FoldArgs * len(ds))()
    for i, d in enumerate(ds):
        fa[i] = CL.FoldArgs(CL.ptr(d["slots"][0]), CL.ptr(d["slots"][1]), CL.ptr(d["dB"]), CL.ptr(d["dC"]), CL.ptr(counters[i]),
                            CL.ptr(give_ups[i]), SB * k, L // k, split * k, N, npart, run["dirs"][i][0], run["dirs"][i][1],
                            CL.dtype_code(run["act"]))
    return fa


def fold(ds, run, how):
    """Folds every set's slots into fresh (NaN-filled) dB / dC with `how`: "reduce" (cad_reduce_partials_multi), "stream"
    (cad_fold_partials_stream, CAD_FOLD_ALL), or "behind" (launches the scan itself: ops.fold_behind_scan)."""
    lib, act, npart, SB, L, N, k = run["lib"], run["act"], run["npart"], run["SB"], run["L"], run["N"], run["k"]
    dev = ds[0]["u"].device
    for d in ds:
        d["dB"] = torch.full((N, SB, L), float("nan"), dtype=act, device=dev)
        d["dC"] = torch.full((N, SB, L), float("nan"), dtype=act, device=dev)
    if how == "reduce":
        jobs = (CL.ReduceJob * 4)()
        for i, d in enumerate(ds):
            jobs[2 * i] = CL.ReduceJob(CL.ptr(d["slots"][0]), CL.ptr(d["dB"]))
            jobs[2 * i + 1] = CL.ReduceJob(CL.ptr(d["slots"][1]), CL.ptr(d["dC"]))
        CL.check(lib.cad_reduce_partials_multi(jobs, 2 * len(ds), npart, N * SB * L, CL.dtype_code(act), run["stream"]), "reduce")
        return None
    give_ups = torch.zeros((len(ds), SB * k, npart), dtype=torch.int32, device=dev)
    if how == "stream":
        nch = (L // k) // CHUNK
        counters = run["counters"].clone()
        counters[:, SB * k * nch] = npart * SB * k  # every scan workgroup placed: nothing to wait for
        fa = fold_args(ds, run, counters, give_ups)
        CL.check(lib.cad_fold_partials_stream(fa, len(ds), 2, run["stream"]), "fold all")
        return None
    assert how == "behind"
    fa = fold_args(ds, run, run["counters"], give_ups)
    old = ops.FOLD_GIVE_UPS
    ops.FOLD_GIVE_UPS = []
    try:
        keep = ops.fold_behind_scan(lib, fa, len(ds), dev, run["launch"], give_ups=give_ups)
        gave_up = int(sum(int(x) for x in ops.FOLD_GIVE_UPS))
    finally:
        ops.FOLD_GIVE_UPS = old
    CL.check(lib.cad_scan_bwd_gate_fix(run["ba"], len(ds), run["stream"]), "gate fix")
    assert int(give_ups.abs().sum()) == 0, "the cleanup pass must clear every give-up record"
    return keep, gave_up


def oracle(sets, z, dout, split, dirs, delta_is_dt, W, want_slots):
    E, SB, L = sets[0]["u"].shape
    out = []
    for i, t in enumerate(sets):
        rev = [dirs[i][0] if r < split else dirs[i][1] for r in range(SB)]
        out.append(oracle_ops.scan_bwd_sums_f64(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], z, t["bias"], dout, rev, W,
                                                delta_is_dt=delta_is_dt, want_slots=want_slots))
    return out


def check_case(case, dev, E, SB, L, N, act, nsets, split, delta_is_dt, folds, ks=(), slots=True, controls=True, seed=5):
    dirs = [(0, 1), (1, 0)][:nsets] if split not in (0, SB) else [(0, 0), (1, 1)][:nsets]
    sets, z, dout = make_inputs(E, SB, L, N, act, nsets, seed, delta_is_dt)
    W = slot_width(E)
    G = -(-E // W)
    t0 = time.perf_counter()
    refs = oracle(sets, z, dout, split, dirs, delta_is_dt, W, slots)
    t_oracle = time.perf_counter() - t0
    to = lambda t: None if t is None else t.to(dev)
    dz_ref = to(sum(r["dz"].double() for r in refs))
    on_dev = [{kk: (tuple(to(x) for x in v) if isinstance(v, tuple) else to(v)) for kk, v in r.items()} for r in refs]
    lib = CL.get_lib()
    streamable = act == torch.bfloat16 and bool(lib.cad_fold_stream_supported(N, G, L, CL.dtype_code(act)))

    def check_outputs(ds, dz, tag, k, with_slots):
        for i, (d, r) in enumerate(zip(ds, on_dev)):
            for name in ("dB", "dC"):
                check_sum(f"{tag} set {i} {name}", d[name], *r[name], act, G, case)
            if with_slots:
                for j, name in enumerate(("dB", "dC")):
                    Pg, PgA = r[f"{name}_slots"]
                    u = UNITS[act]
                    tol = (2 * u["channel"] + KAPPA) * PgA + 2 * u["slot"] * Pg.abs()
                    _report(f"set {i} {name} slot", d["slots"][j], Pg, tol, case)
            rows = SB * k
            for name in ("dA", "dD", "dbias"):
                check_param(f"{tag} set {i} {name}", d[name], *r[name], act, L // k, rows, case)
            cls = FP32 if act == torch.float32 else BF16
            for name in ("du", "ddelta"):
                ref = r[name]
                scale = max(1.0, float(ref.abs().max()))
                torch.testing.assert_close(d[name].float(), ref, rtol=cls["rtol"], atol=cls["atol"] * scale,
                                           msg=lambda m, name=name, i=i: f"{case} {tag} set {i} {name}: {m}")
        scale = max(1.0, float(dz_ref.abs().max()))
        cls = FP32 if act == torch.float32 else BF16
        torch.testing.assert_close(dz.double(), dz_ref, rtol=cls["rtol"], atol=cls["atol"] * scale,
                                   msg=lambda m: f"{case} {tag} dz: {m}")

    # k = 1: the scan once, its slots folded by the kernel behind it and by the stream fold
    ds, dz, run = run_device(dev, sets, z, dout, split, dirs, act, delta_is_dt)
    run["launch"]()
    CL.check(lib.cad_scan_bwd_gate_fix(run["ba"], nsets, run["stream"]), "gate fix")
    for how in folds:
        if how == "stream" and not streamable:
            continue
        if how == "behind":
            continue
        fold(ds, run, how)
        check_outputs(ds, dz, how, 1, slots and how == folds[0])
    if controls:
        negative_controls(case, ds[0], on_dev[0], act, G, L)
    del ds, run
    # the concurrent fold of the training step, next to the real scan
    if "behind" in folds and streamable:
        ds, dz, run = run_device(dev, sets, z, dout, split, dirs, act, delta_is_dt, stream_counters=True)
        _, gave_up = fold(ds, run, "behind")
        check_outputs(ds, dz, "behind", 1, False)
        del ds, run
    # L-split: segments of L / k as rows, folded behind the scan where the stream fold serves the segment length
    for k in ks:
        if L % (k * CHUNK) != 0:
            continue
        seg_stream = streamable and bool(lib.cad_fold_stream_supported(N, G, L // k, CL.dtype_code(act)))
        ds, dz, run = run_device(dev, sets, z, dout, split, dirs, act, delta_is_dt, k=k, stream_counters=seg_stream)
        if seg_stream:
            fold(ds, run, "behind")
        else:
            run["launch"]()
            CL.check(lib.cad_scan_bwd_gate_fix(run["ba"], nsets, run["stream"]), "gate fix")
            fold(ds, run, "reduce")
        check_outputs(ds, dz, f"lsplit k={k}", k, False)
        del ds, run
    print(f"\n{case}: fp64 oracle {t_oracle:.1f} s on {oracle_ops.num_threads()} threads; worst err/tol " + ", ".join(f"{kk} {v:.3f}" for kk, v in sorted(RESULTS[case].items())))


def negative_controls(case, d, r, act, G, L):
    """Perturbations of the device's own slots, folded on the host in fp64 and rounded to the destination dtype like a fold: the bound
    must reject each at a clear fraction of the elements it touches."""
    slots = d["slots"][0].double()  # dB slots of set 0: (G, N, SB, L)
    S, Ag, Ae = r["dB"]
    fold_host = lambda s: s.sum(0).to(act)
    assert rejected_fraction(fold_host(slots), S, Ag, Ae, act, G) == 0.0  # the unperturbed host fold passes
    g = G // 2
    row = torch.zeros_like(S, dtype=torch.bool)
    row[:, 0] = True
    fracs = {}
    dropped = slots.clone()
    dropped[g] = 0
    fracs["slot dropped"] = (rejected_fraction(fold_host(dropped), S, Ag, Ae, act, G), None)
    if L >= 2 * CHUNK:
        shifted = slots.clone()
        shifted[g, :, 0] = torch.roll(slots[g, :, 0], -CHUNK, dims=-1)  # row 0 read at the neighbouring chunk
        fracs["chunk shift"] = (rejected_fraction(fold_host(shifted), S, Ag, Ae, act, G, row), row)
    mirrored = slots.clone()
    mirrored[g, :, 0] = slots[g, :, 0].flip(-1)  # row 0 stored in the wrong direction
    fracs["mirrored"] = (rejected_fraction(fold_host(mirrored), S, Ag, Ae, act, G, row), row)
    RESULTS.setdefault(case, {}).update({f"control {kk} rejected": v for kk, (v, _) in fracs.items()})
    for kk, (v, _) in fracs.items():
        assert v >= MIN_REJECTED, f"{case}: negative control '{kk}' rejected at only {v:.4f} of its elements"


MIN_REJECTED = 0.01  # of the thousands of elements a perturbation touches: dozens or more out of bounds (one fails the test)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
EMU_CASES = [  # id, E, SB, L, N, act, nsets, split, delta_is_dt, folds, ks
    ("bf16 E36 L1104 2 sets", 36, 2, 1104, 16, torch.bfloat16, 2, 1, True, ("reduce",), ()),
    ("fp16 E36 L1037 N8", 36, 2, 1037, 8, torch.float16, 1, 1, False, ("reduce",), ()),
    ("fp32 E20 L1104 2 sets", 20, 2, 1104, 16, torch.float32, 2, 1, False, ("reduce",), ()),
    ("bf16 E64 L1024 streamed", 64, 1, 1024, 16, torch.bfloat16, 1, 1, True, ("reduce", "stream", "behind"), (2,)),
]

GPU_CASES = [
    ("bf16 E512 L4096 2 sets", 512, 2, 4096, 16, torch.bfloat16, 2, 1, True, ("reduce", "stream", "behind"), (2, 4)),
    ("bf16 E1024 L4096 2 sets", 1024, 2, 4096, 16, torch.bfloat16, 2, 1, True, ("reduce", "stream", "behind"), (2, 4)),
    ("bf16 E36 L1104 3 rows", 36, 3, 1104, 16, torch.bfloat16, 2, 2, True, ("reduce",), ()),
    ("bf16 E1024 L1037 N16", 1024, 2, 1037, 16, torch.bfloat16, 2, 1, True, ("reduce",), ()),
    ("fp16 E512 L1104 2 sets", 512, 2, 1104, 16, torch.float16, 2, 1, False, ("reduce",), ()),
    ("fp16 E36 L1037 N8", 36, 2, 1037, 8, torch.float16, 1, 1, False, ("reduce",), ()),
    ("fp32 E512 L4096 2 sets", 512, 2, 4096, 16, torch.float32, 2, 1, False, ("reduce",), (2,)),
    ("fp32 E1024 L1037 N8", 1024, 1, 1037, 8, torch.float32, 1, 1, False, ("reduce",), ()),
]


@pytest.mark.parametrize("spec", EMU_CASES, ids=[c[0] for c in EMU_CASES])
def test_scan_bwd_sums_emulator_and_device(backend, spec):
    name, dev = backend
    case, E, SB, L, N, act, nsets, split, dt_in, folds, ks = spec
    check_case(f"{name} {case}", dev, E, SB, L, N, act, nsets, split, dt_in, folds, ks)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_scan_bwd_sums_production_depths(spec):
    CL.use_library_for_testing(None)
    dev = torch.device("cuda:0")
    case, E, SB, L, N, act, nsets, split, dt_in, folds, ks = spec
    check_case(f"hip {case}", dev, E, SB, L, N, act, nsets, split, dt_in, folds, ks)


TIER_B = [  # the training step's layer scans: configs[2] (E 512, SB 2), depth 128 (E 1024), Caduceus-Ph (SB 1: the automatic L-split)
    ("configs[2] E512 SB2", 512, 2, 2),
    ("E1024 SB2", 1024, 2, 2),
    ("Ph E512 SB1 auto L-split", 512, 1, 2),
]


@pytest.mark.gpu
@pytest.mark.parametrize("spec", TIER_B, ids=[c[0] for c in TIER_B])
def test_scan_bwd_sums_training_shapes(spec):
    """L = 131072, bf16, two sets under the shared gate (one launch, as the mixer runs them), the L-split factor the training step picks (ops.lsplit_factor) and the
    concurrent fold (ops.fold_behind_scan), against the fp64 sums: checks (b) to (d)."""
    CL.use_library_for_testing(None)
    dev = torch.device("cuda:0")
    case, E, SB, nsets = spec
    L, N, act = 131072, 16, torch.bfloat16
    k = ops.lsplit_factor(E, SB, L, nsets)
    if SB == 1:
        assert k == 2, f"Caduceus-Ph's layer scan is expected to take the two-way L-split (got k = {k})"
    lib = CL.get_lib()
    G = int(lib.cad_scan_bwd_partials(E))
    assert lib.cad_fold_stream_supported(N, G, L // k, CL.dtype_code(act)) == 1
    check_case(f"hip {case} L131072 k={k}", dev, E, SB, L, N, act, nsets, 1 if SB > 1 else 0, True, ("behind",),
               (k,) if k > 1 else (), slots=False, controls=False)


# ---- the oracle itself -------------------------------------------------------------------------------------------------------------------
def test_f64_oracle_matches_the_fp32_oracle():
    """scan_bwd_sums_f64 against the fp32 C oracle (cad_oracle_scan_bwd, pinned to the reference's vectors by test_oracle_golden.py) on
    the same inputs, rows in both directions; and its S / Ag / Ae / slot sums consistent with each other."""
    E, SB, L, N = 12, 2, 300, 16
    sets, z, dout = make_inputs(E, SB, L, N, torch.float32, 1, 3, False)
    t = sets[0]
    r = oracle(sets, z, dout, 1, [(0, 1)], False, 8, True)[0]
    for sb, rev in ((0, False), (1, True)):
        f = (lambda x: x.flip(-1)) if rev else (lambda x: x)
        row = lambda x: f(x[:, sb]).unsqueeze(0).contiguous()
        u_, d_, z_, dy_ = map(row, (t["u"], t["delta"], z, dout))
        B_, C_ = row(t["B"]), row(t["C"])
        out = [torch.empty_like(x) for x in (u_, u_, u_)]
        dA, dB, dC = torch.empty_like(t["A"]), torch.empty_like(B_), torch.empty_like(C_)
        dD, db = torch.empty_like(t["D"]), torch.empty_like(t["bias"])
        P = oracle_ops._p
        oracle_ops.lib().cad_oracle_scan_bwd(P(u_), P(d_), P(t["A"]), P(B_), P(C_), P(t["D"]), P(z_), P(t["bias"]), P(dy_),
                                             P(out[0]), P(out[1]), P(dA), P(dB), P(dC), P(dD), P(out[2]), P(db), C.c_int64(1),
                                             C.c_int64(E), C.c_int64(L), C.c_int64(N))
        back = lambda x: f(x[0])
        for name, got, want in (("du", back(out[0]), r["du"][:, sb]), ("ddelta", back(out[1]), r["ddelta"][:, sb]),
                                ("dz", back(out[2]), r["dz"][:, sb]), ("dB", back(dB), r["dB"][0][:, sb]),
                                ("dC", back(dC), r["dC"][0][:, sb])):
            torch.testing.assert_close(got.double(), want.double(), rtol=1e-4, atol=1e-4 * float(want.abs().max()), msg=name)
    S, Ag, Ae = r["dB"]
    Pg, PgA = r["dB_slots"]
    torch.testing.assert_close(Pg.sum(0), S, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(Pg.abs().sum(0), Ag, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(PgA.sum(0), Ae, rtol=1e-12, atol=1e-12)
    assert bool((S.abs() <= Ag * (1 + 1e-12)).all()) and bool((Ag <= Ae * (1 + 1e-12)).all())
    for name in ("dA", "dD", "dbias"):
        s, a = r[name]
        assert bool((s.abs() <= a * (1 + 1e-12)).all()), name
