"""Hand-scheduled forward/backward of one weight-tied BiMamba mixer over both RCPS strands (the production path:
`bidirectional=True, bidirectional_strategy="add", bidirectional_weight_tie=True, bias=False`).

engine.py composes the same computation from per-op autograd Functions (kept for every other configuration and as the
readable specification).  Scheduling the backward by hand removes what generic autograd cannot know
(profiles/r01_step_and_scan_v3_summary.txt: ~40 ms of copies / adds / duplicate GEMMs per 382 ms step):
  * with a tied out_proj, d(y_f) == d(y_r): ONE GEMM, written channel-major directly (no transposing copies);
  * the two scans share the gate z and the upstream gradient: set f's backward kernel writes the gate gradient of both straight into
    the dxz buffer (cad_scan_bwd_args.out2);
  * weight gradients (reductions over all T tokens with tiny outputs) are fp32 partial tiles of the own kernels, summed by one fold
    launch at the end of the backward;
  * the conv forward / backward of both parameter sets run as one launch each (x read once, dx = dx_f + dx_r written once); dB/dC partial sums are reduced straight into the rows of
    the x_proj gradient operand; du is folded into the x_proj backward GEMM (addmm).
BiMambaMixerFn.forward / backward read as the schedule; every step of it is one module-level stage function (_in_proj ... _dW_in_partials)
that owns its dispatch chain: the own kernel if it serves the shape, else the next kernel, else the GEMM library through torch.
All kernels are the C-ABI entry points of include/caduceus_hip.h.  At the benchmarked shapes (bf16, d_model 256 / 512) EVERY product runs
on the library's own MFMA kernels (csrc/gemm.hip and its headers proj_wstat.h / proj_ring.h / gemm_stream.h, gemm_fp8.hip): in_proj, x_proj, dt_proj (+ bias + softplus), out_proj, d(y), d(dt_lr) +
dW_dt (one pass, cad_proj_wx_wgrad), dW_x, d(xc), d(x2d), dW_in and dW_out; fp32 takes cad_gemm_f32, and only bf16 / fp16 shapes that no
own kernel serves reach hipBLASLt through torch.
Scan launches with fewer workgroups than the GPU has CUs are L-split (ops.lsplit_factor).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
from collections import namedtuple

import torch

from . import _lib as L
from . import ops

# the seven parameters of one parameter set (f, r), in the order BiMambaMixerFn.apply takes them
SetParams = namedtuple("SetParams", "conv_w conv_b W_x W_dt dt_bias A_log D")
# what one parameter set saves for the backward (fp32: A = -exp(A_log), D, dt_bias, conv_w (E, K), conv_b; compute dtype: the rest)
SetSaved = namedtuple("SetSaved", "xc delta A dbc D dt_bias conv_w conv_b w_x w_dt state A_log")
# outputs of one set's scan backward: dBC = the (2, npart, N, SB, L) partial slots of dB / dC; dA, dD, dbias are accumulated (zeroed)
SetWork = namedtuple("SetWork", "du ddelta dA dD dbias dBC npart")
# the non-tensor context of a backward: pdtypes = SetParams of dtypes (None: no such parameter) per set, delta_is_dt per set
Meta = namedtuple("Meta", "SB Lq split pdtypes conv_w_shapes win_dt wout_dt delta_is_dt k")
# prepare_step_cache's per-layer record: compute-dtype weights and their transposes (w_x, w_dt, A and their transposes: one per set)
StepCache = namedtuple("StepCache", "versions w_in w_out w_x w_dt A w_inT w_outT w_xT w_dtT w_out2 w_in_fp8")
_DIRS = ((0, 1), (1, 0))  # (rev_lo, rev_hi) of set f and set r: which of the two strand row groups a set scans reversed


def _flatten(records):
    return [t for r in records for t in r]


def _unflatten(cls, flat, n):
    """The inverse of _flatten for n records of namedtuple cls at the head of flat -> (records, what follows them)."""
    w = len(cls._fields)
    return [cls(*flat[j * w:(j + 1) * w]) for j in range(n)], flat[n * w:]


def _conv_fwd2(x, params, split, dirs):
    """Both parameter sets' causal conv + SiLU of the same x in one launch (x is read once).  params: [(wf, bf)] * 2."""
    E, SB, Lq = x.shape
    n = len(params)
    args = (L.Conv1dArgs * n)()
    outs = []
    for i, (wf, bf) in enumerate(params):
        out = torch.empty_like(x)
        stream = L.stream_and_check(x, wf, bf, out)
        args[i] = L.Conv1dArgs(L.ptr(x), L.ptr(wf), L.ptr(bf), L.ptr(out), SB, Lq, split, E, wf.shape[1], dirs[i][0],
                               dirs[i][1], L.dtype_code(x.dtype))
        outs.append(out)
    L.check(L.get_lib().cad_conv1d_fwd_multi(args, n, stream), "cad_conv1d_fwd_multi")
    return outs


def _zeros_f32(spec, device):
    """{name: zero tensor} for spec = {name: (shape, torch.float32 | torch.int32)}, carved out of ONE fp32 allocation (one fill kernel
    instead of one per tensor: the accumulated per-channel gradients of a layer are ten tiny tensors; zero bits are zero counters)."""
    sizes = [int(torch.Size(s).numel()) for s, _ in spec.values()]
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + (n + 3) // 4 * 4)  # 16-byte aligned views
    flat = torch.zeros((offs[-1],), dtype=torch.float32, device=device)
    return {name: flat[o:o + n].view(dt).view(s) for o, n, (name, (s, dt)) in zip(offs, sizes, spec.items())}


def _conv_bwd2(x, params, douts, dx, split, dirs, bufs=None):
    """dx = sum over both parameter sets of their input gradients (written once), dw / dbias per set.
    bufs: optional pre-zeroed fp32 (dw, db) per set."""
    E, SB, Lq = x.shape
    n = len(params)
    args = (L.Conv1dBwdArgs * n)()
    res, slots = [], []
    for i, (wf, bf) in enumerate(params):
        if bufs is not None:
            dw, db = bufs[i]
        else:
            dw = torch.zeros_like(wf)
            db = None if bf is None else torch.zeros_like(bf)
        stream = L.stream_and_check(x, wf, bf, douts[i], dx, dw, db)
        args[i] = L.Conv1dBwdArgs(L.ptr(x), L.ptr(wf), L.ptr(bf), L.ptr(douts[i]), L.ptr(dx), L.ptr(dw), L.ptr(db), SB, Lq,
                                  split, E, wf.shape[1], dirs[i][0], dirs[i][1], L.dtype_code(x.dtype), 0)
        # per-workgroup slots of dw / dbias, folded by the library in a fixed order (ops.wgrad_slots): the same gradient every run
        ns = L.get_lib().cad_conv1d_bwd_slots(C.byref(args[i]))
        ws, bs = ops.wgrad_slots(ns, dw.numel(), x.device, zero=False), (None if db is None else ops.wgrad_slots(ns, E, x.device, zero=False))
        res.append((dw, db))
        slots.append((ws, bs))
    wptr = (C.c_void_p * n)(*[ws.data_ptr() for ws, _ in slots])
    bptr = (C.c_void_p * n)(*[0 if bs is None else bs.data_ptr() for _, bs in slots])
    L.check(L.get_lib().cad_conv1d_bwd_multi_slotted(args, n, wptr, bptr, stream), "cad_conv1d_bwd_multi_slotted")
    return res


def _kchunks(T: int) -> int:
    """Number of K-chunks for the weight-gradient GEMMs (reduction over all T tokens, tiny outputs).  hipBLASLt does not
    split K by itself for these shapes (0.6 ms at 0.65 TB/s); as a strided-batch GEMM over 64 chunks plus an fp32 sum of
    the partial products the same gradient takes 0.1-0.2 ms (tools/gemm_bench.py), with the same rounding error."""
    n = 64
    while n > 1 and (T % n != 0 or T // n < 1024):
        n //= 2
    return n


def _wgrad_cm_cm(a_cm: torch.Tensor, b_cm: torch.Tensor) -> torch.Tensor:
    """a (M, T) @ b (N, T)^T with both operands channel-major (T contiguous) -> (M, N) fp32."""
    M, T = a_cm.shape
    if a_cm.dtype in (torch.float32, torch.float16):  # the own fp32 matrix-core kernel cuts K itself (ops.mm_f32; fp16: exact widening)
        return ops.mm_f32(a_cm.float(), b_cm.float().t())
    n = _kchunks(T)
    if b_cm.shape[0] <= 16 and n >= 64 and T % 16 == 0:
        n = 16  # thin products (dW_dt): fewer, deeper chunks (tools/wgrad_sweep.py: 48 vs 55 us at T = 262144)
    if n == 1:
        return ops.mm(a_cm, b_cm.t()).float()
    Kc = T // n
    # (sum with fp32 accumulation straight from the bf16 partial products: no separate up-cast launch)
    return torch.sum(ops.bmm(a_cm.view(M, n, Kc).permute(1, 0, 2), b_cm.view(-1, n, Kc).permute(1, 2, 0)), dim=0,
                     dtype=torch.float32)


def _own_wgrad_chunked_ok(X: torch.Tensor, M: int) -> bool:
    """Reductions over ALL tokens with K = d_inner > 512 rows (d_model 512: configs[4]): the own weight-gradient kernel takes 512 rows of
    X per launch, so X is cut into row blocks -- the rows of dW are independent."""
    K, T = X.shape
    return K > 512 and K % 512 == 0 and ops.proj_wgrad_only_supported(X, M, 512, T)


def _own_wgrad_chunked(X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    """dW (M, K) fp32 = Y (M, T) @ X (K, T)^T with fp32 accumulation over all tokens (cad_proj_wx_wgrad's weight-gradient stage), K in
    blocks of 512 rows.  Replaces the K-split library bmm whose bf16-rounded partial products cost 3-4 % relative error on
    dW_x of a d_model 512 layer (found by tests/test_configs.py::test_config4_one_layer_d512_L262144_every_gradient_vs_oracle)."""
    K = X.shape[0]
    return torch.cat([ops.proj_wgrad_only(X[h:h + 512], Y) for h in range(0, K, 512)], dim=1)


def _wgrad_cm_tm(a_cm: torch.Tensor, b_tm: torch.Tensor) -> torch.Tensor:
    """a (M, T) channel-major @ b (T, N) token-major -> (M, N) fp32."""
    M, T = a_cm.shape
    if _OWN_GEMM:
        own = ops.wgrad_cm_tm(a_cm, b_tm)
        if own is not None:
            return own
    if a_cm.dtype in (torch.float32, torch.float16):
        return ops.mm_f32(a_cm.float(), b_tm.float())
    n = _kchunks(T)
    if n == 1:
        return ops.mm(a_cm, b_tm).float()
    Kc = T // n
    return torch.sum(ops.bmm(a_cm.view(M, n, Kc).permute(1, 0, 2), b_tm.view(n, Kc, -1)), dim=0, dtype=torch.float32)


# Test and A/B handles, not options: tests/test_proj.py, tests/test_fold_stream.py and tools/layer_bench.py --ab set them in-process to
# reach the branch behind the own kernel (the real path of shapes the own kernels refuse); only the defaults run on the device.
# d(dt_lr) and dW_dt from one pass over d(delta) (cad_proj_wx_wgrad); False: the two-kernel path
_FUSED_WGRAD = True
# dW_x = d(dbc) . xc^T on the weight-gradient stage of the same kernel (W == NULL) instead of the GEMM library + a partial sum
_OWN_DWX = True
# out_proj forward on the own token-major-output MFMA kernel (cad_proj_xTw); False: hipBLASLt on [y_f ; y_r]
_OWN_OUT_PROJ = True
# d(x2d), dW_in and dW_out -- the products whose two operands both stream -- on the own tiled MFMA kernel (cad_gemm_stream: fp32
# accumulation over ALL tokens for the weight gradients); False: torch.mm / K-split bmm (hipBLASLt).  At d_model 512 (configs[4]: two
# 256-column tiles, the strided operand is walked twice) the library products are 0.5 ms per layer faster (31.75 vs 32.28 ms per layer,
# 535.2 vs 538.2 ms per step: profiles/r05_gemm_stream_d512.txt), i.e. 0.6 % of a step is the price of a configs[4] step without a
# library GEMM and with fp32-accumulated weight gradients
_OWN_GEMM = True
# in_proj, out_proj and d(y) at d_model 512 on the same tiled kernel (cad_gemm_stream, column tiles fastest) instead of the W-stationary
# cad_proj_wxT, which streams the token operand once per 128-row block of W (16 times at M = 2048); False: cad_proj_wxT / the library
_STREAM_PROJ_D512 = True
# the fp32 partial tiles of a layer's weight gradients (dW_in, dW_out: K slices of cad_gemm_stream; dW_x, dW_dt: per-workgroup slots of
# cad_proj_wx_wgrad) summed by ONE own launch at the end of the backward (cad_fold_f32_multi) instead of four torch reductions + an add;
# False: torch.sum per tensor
_GLUE_FOLD = True
# BASELINE configs[4]: in_proj on the fp8 (OCP e4m3) matrix cores (csrc/gemm_fp8.hip); set CADUCEUS_AMD_FP8_PROJ=1 or call
# set_fp8_in_proj(True).  Forward only: the backward keeps the bf16 activations it saves today.
_FP8_IN_PROJ = os.environ.get("CADUCEUS_AMD_FP8_PROJ", "0") == "1"
# the dB / dC partial slots folded by cad_fold_partials_stream on a second stream WHILE the scan backward runs (the scan is bound by VALU
# issue, the fold by memory latency: 0.39 ms per layer of fold kernel leave the critical path); CADUCEUS_AMD_STREAM_FOLD=0: the fold
# kernel behind the scan (cad_reduce_partials_multi) -- same summation order, bit-identical gradients
_STREAM_FOLD = os.environ.get("CADUCEUS_AMD_STREAM_FOLD", "1") != "0"
_STREAM_FOLD_MIN_CHUNKS = 16  # rows shorter than this many 512-position chunks keep the fold kernel behind the scan (see _scan_bwd)


# test hook (tests/test_configs.py): a list here receives, per backward call, the operands of the x_proj weight gradient of both
# parameter sets as the kernels saw them -- {"ddbc": [d(dt_lr ; B ; C) (R + 2N, T)] * 2, "xc": [conv output (E, T)] * 2} (clones)
CAPTURE_XPROJ_OPERANDS = None


_grad_scope = threading.local()


@contextlib.contextmanager
def input_grad_only(enabled: bool = True):
    """While active (thread-local), a BiMambaMixerFn forward records that its backward owes only d(x2d): the gradient of the layer's
    input, for attributions (caduceus_amd.attribution) -- no weight-gradient product, no slot sums, no fold launch, no parameter casts;
    every parameter receives None.  It is the forward that decides: parameters normally require grad, so ctx.needs_input_grad cannot.
    The kernels that produce small parameter sums as a by-product (scan dA / dD / dbias, conv dw) run as they are; their sums are dropped."""
    prev = getattr(_grad_scope, "input_only", False)
    _grad_scope.input_only = bool(enabled)
    try:
        yield
    finally:
        _grad_scope.input_only = prev


def input_grad_only_enabled() -> bool:
    return bool(getattr(_grad_scope, "input_only", False))


def set_fp8_in_proj(on: bool) -> None:
    global _FP8_IN_PROJ
    _FP8_IN_PROJ = bool(on)
    ops.FP8_ACTIVATIONS = _FP8_IN_PROJ


ops.FP8_ACTIVATIONS = _FP8_IN_PROJ


def prepare_step_cache(pairs, act: torch.dtype) -> None:
    """Compute-dtype copies of every layer's projection weights and A = -exp(A_log), for ALL layers at once with
    multi-tensor (foreach) launches -- instead of ten tiny cast / exp / neg kernels per layer per step
    (profiles/r02_step_trace.txt: ~1000 sub-5-us launches per step).  pairs: [(mamba_fwd, mamba_rev)] of the layers that run
    BiMambaMixerFn.  The copies are attached to mamba_fwd (a StepCache) together with the parameter versions they were made from;
    BiMambaMixerFn.forward uses them only while those versions are current."""
    if not pairs:
        return
    src, dst, alog, owners = [], [], [], []
    # the compute-dtype copies of one kind of weight (in / out / x / dt) of ALL layers are slices of one stacked buffer, so that the
    # backward's transposed operands (W_out^T, W_x^T, W_dt^T) come from ONE batched transpose per kind and step instead of five
    # strided copy launches per layer (a multi-tensor copy from transposed views falls back to one launch per tensor)
    kinds = ("in", "out", "x", "dt")
    plist = [{"in": [mf.in_proj.weight], "out": [mf.out_proj.weight], "x": [mf.x_proj.weight, mr.x_proj.weight],
              "dt": [mf.dt_proj.weight, mr.dt_proj.weight]} for mf, mr in pairs]
    stacked = {}
    for kd in kinds:
        shapes = {tuple(p.shape) for pl in plist for p in pl[kd]}
        n = sum(len(pl[kd]) for pl in plist)
        if len(shapes) == 1:
            stacked[kd] = torch.empty((n,) + next(iter(shapes)), dtype=act, device=plist[0][kd][0].device)
    cursor = {kd: 0 for kd in kinds}

    def alloc(kd, p):
        if kd in stacked:
            v = stacked[kd][cursor[kd]]
            cursor[kd] += 1
            return v
        return torch.empty(p.shape, dtype=act, device=p.device)

    order = ("in", "out", "x", "dt", "x", "dt")  # w_in, w_out, w_x_f, w_dt_f, w_x_r, w_dt_r: the order the stacked buffers are filled in
    for (mf, mr), pl in zip(pairs, plist):
        ps = [pl["in"][0], pl["out"][0], pl["x"][0], pl["dt"][0], pl["x"][1], pl["dt"][1]]
        out = [alloc(kd, p) for kd, p in zip(order, ps)]
        src += [p.detach() for p in ps]
        dst += out
        alog += [mf.A_log.detach().float(), mr.A_log.detach().float()]
        owners.append((mf, ps + [mf.A_log, mr.A_log], out))
    torch._foreach_copy_(dst, src)
    # (W_in^T is prepared when one of its two consumers -- the streamed in_proj, d(x2d) -- will ask for it)
    need_in_T = "in" in stacked and (_dx2d_is_streamed() or _in_proj_is_streamed(stacked["in"].shape[2], act))
    trans = {kd: stacked[kd].transpose(1, 2).contiguous() for kd in ("out", "x", "dt") + (("in",) if need_in_T else ()) if kd in stacked}
    cursor = {kd: 0 for kd in kinds}

    def transposed(kd, w):
        if kd in trans:
            v = trans[kd][cursor[kd]]
            cursor[kd] += 1
            return v
        return w.t().contiguous()

    wTs = []
    for mf, ps, (w_in, w_out, w_x_f, w_dt_f, w_x_r, w_dt_r) in owners:  # (transposes in the order of the stacked buffers, W_in^T last)
        w_outT, w_x_fT, w_dt_fT, w_x_rT, w_dt_rT = [transposed(kd, w) for kd, w in zip(order[1:], (w_out, w_x_f, w_dt_f, w_x_r, w_dt_r))]
        wTs.append(dict(w_outT=w_outT, w_xT=(w_x_fT, w_x_rT), w_dtT=(w_dt_fT, w_dt_rT), w_inT=transposed("in", w_in) if need_in_T else None))
    negA = torch._foreach_exp(alog)
    torch._foreach_neg_(negA)
    for (mf, ps, (w_in, w_out, w_x_f, w_dt_f, w_x_r, w_dt_r)), wT, A_f, A_r in zip(owners, wTs, negA[0::2], negA[1::2]):
        # d_model 512: out_proj streams [y_f ; y_r] against [W_out, W_out] (K = 2 E) -- built once per step, not per layer call
        w_out2 = torch.cat([w_out, w_out], 1) if _out_proj_is_streamed(w_out.shape[0]) else None
        w_in_fp8 = None
        if _FP8_IN_PROJ and act == torch.bfloat16 and ops.fp8_proj_supported(w_in, w_in.shape[1]):
            w_in_fp8 = ops.quant_weight_fp8(mf.in_proj.weight)  # from the fp32 master weight, once per step
        mf._cad_step_cache = StepCache(versions=[(id(p), p._version) for p in ps], w_in=w_in, w_out=w_out, w_x=(w_x_f, w_x_r),
                                       w_dt=(w_dt_f, w_dt_r), A=(A_f, A_r), w_out2=w_out2, w_in_fp8=w_in_fp8, **wT)


def _cached(mf, params):
    c = getattr(mf, "_cad_step_cache", None)
    if c is None or c.versions != [(id(p), p._version) for p in params]:
        return None
    return c


def _transposed(cache, field, w, i=None):
    """W^T from the step cache (field of StepCache, set i of a per-set field), or -- no step cache (eval, or the parameters changed
    since prepare_step_cache), or a transpose it did not prepare -- made here."""
    wT = None if cache is None else getattr(cache, field)
    if wT is not None and i is not None:
        wT = wT[i]
    return w.t().contiguous() if wT is None else wT


# ---- forward stages --------------------------------------------------------------------------------------------------------------
def _in_proj_is_streamed(Dm: int, act) -> bool:  # d_model 512: both operands streamed through the tiled kernel, which takes W_in^T
    return _STREAM_PROJ_D512 and Dm > 256 and act == torch.bfloat16


def _in_proj(x2d, W_in, w_in, cache, fp8_act):
    """xz (2E, T) channel-major = W_in x2d^T."""
    T, Dm = x2d.shape
    if _FP8_IN_PROJ and x2d.dtype == torch.bfloat16 and ops.fp8_proj_supported(x2d, Dm):
        # fp8 matrix cores: per-token e4m3 activations x per-row e4m3 weights, fp32 accumulation, bf16 channel-major output
        wq, sw = cache.w_in_fp8 if (cache and cache.w_in_fp8 is not None) else ops.quant_weight_fp8(W_in)
        # e4m3 activations + per-token scales: written by the add + norm kernel that produced x2d (fp8_act), else quantised here
        xq, sx = (fp8_act[0].view(T, Dm), fp8_act[1]) if fp8_act is not None else ops.quant_rows_fp8(x2d)
        return ops.proj_wxT_fp8(wq, sw, xq, sx)
    xz = None
    if _in_proj_is_streamed(Dm, x2d.dtype):
        # A = tokens, B = W_in^T, channel-major result (None if the shape is not served)
        xz = ops.gemm_out_t(x2d, _transposed(cache, "w_inT", w_in))
    if xz is None and ops.proj_supported(x2d, Dm):  # bf16: the W-stationary MFMA kernel (csrc/proj_wstat.h) writes channel-major directly
        xz = ops.proj_wxT(w_in, x2d)
    if xz is None:
        xz = ops.mm(w_in, x2d.t())  # fp32: cad_gemm_f32; a bf16 shape no own kernel serves: the library
    return xz


def _x_proj(w_x, xc):
    """[dt_lr ; B ; C] (R + 2N, T) = W_x xc, xc (E, T) channel-major."""
    (M, E), T = w_x.shape, xc.shape[1]
    if ops.proj_wx_supported(xc, E, T, M=M):  # thin-M / deep-K MFMA kernel: xc read once, W_x in LDS
        return ops.proj_wx(w_x, xc)
    if E % 128 == 0 and ops.proj_wx_supported(xc, E // 2, T, M=M):
        # d_inner 1024 (configs[4]): 64 rows x 1024 of W_x do not fit LDS next to the X ring -- two K halves.  The first half is
        # STORED in bf16 and widened again as the addend of the second, so dt_lr / B / C see two roundings (first half, then the
        # sum), not one fp32 accumulation over K; xc is still read once
        dbc = ops.proj_wx(w_x[:, :E // 2], xc[:E // 2])
        return ops.proj_wx(w_x[:, E // 2:], xc[E // 2:], out=dbc, acc=dbc)
    return ops.mm(w_x, xc)


def _dt_proj(w_dt, dt_lr, dt_bias):
    """(delta (E, T), delta_is_dt): delta = softplus(W_dt dt_lr + dt_bias) from the own kernel, which the scans then take as it is
    (delta_is_dt) -- delta_bias + softplus in the epilogue of an HBM-bound kernel with idle VALU instead of the scan prologues; from the
    library plain W_dt dt_lr, and the scans add the bias and apply the softplus."""
    R, T = dt_lr.shape
    if ops.proj_wx_supported(dt_lr, R, T):  # thin-K MFMA kernel (transposing LDS reads), csrc/proj_wstat.h
        return ops.proj_wx(w_dt, dt_lr, softplus_bias=dt_bias), True
    return ops.mm(w_dt, dt_lr), False


def _scan_fwd(sets, z, ycat, delta_is_dt, split, k):
    """Both parameter sets in one scan launch, y of set i into rows [i E, (i + 1) E) of ycat; k > 1: every row cut into k segments along
    L (ops.lsplit_factor) when the launch would otherwise leave CUs idle (Caduceus-Ph at batch 1).  Returns (sets with their chunk
    states, the segments' decay products the backward needs again)."""
    lib = L.get_lib()
    E, SB, Lq = z.shape
    args = (L.ScanArgs * 2)()
    with_state = []
    for i, (s, out) in enumerate(zip(sets, ycat.view(2, E, SB, Lq))):
        N = s.A.shape[1]
        R = s.dbc.shape[0] - 2 * N
        state = torch.empty((lib.cad_scan_state_floats(E, SB * k, Lq // k, N),), dtype=torch.float32, device=z.device)
        Bm, Cm = s.dbc[R:R + N], s.dbc[R + N:]
        args[i], stream = ops.scan_fwd_args(E, SB, Lq, N, split, _DIRS[i], z.dtype, k=k, delta_is_dt=delta_is_dt[i], u=s.xc, delta=s.delta,
                                            A=s.A, Bm=Bm, Cm=Cm, D=s.D, z=z, delta_bias=s.dt_bias, out=out, chunk_state=state)
        with_state.append(s._replace(state=state))
    _keep, seg_P = ops.scan_fwd_launch(lib, args, 2, stream, k, [s.A for s in sets], _DIRS, split)
    return with_state, seg_P


def _out_proj_is_streamed(Dm: int) -> bool:  # d_model 512: W_out is too deep for cad_proj_xTw's resident fragments
    return _STREAM_PROJ_D512 and Dm > 256


def _out_proj(w_out, ycat, cache):
    """out (T, D) token-major = W_out (y_f + y_r), ycat = [y_f ; y_r] (2E, T): the out_proj is tied."""
    Dm, E = w_out.shape
    T = ycat.shape[1]
    if _OWN_OUT_PROJ and ops.proj_xTw_supported(ycat, Dm, E, T):
        # both panels through one set of resident W_out fragments, token-major output (cad_proj_xTw)
        return ops.proj_xTw(w_out, ycat[:E], ycat[E:])
    # both operands streamed (cad_gemm_stream), [y_f ; y_r] against [W_out, W_out] with K = 2 E; plain products for anything the kernel
    # does not serve
    out2d = None
    if _STREAM_PROJ_D512 and ycat.dtype == torch.bfloat16:
        w_out2 = cache.w_out2 if cache else None
        out2d = ops.proj_xTw_stream(w_out2 if w_out2 is not None else torch.cat([w_out, w_out], 1), ycat)
    if out2d is None:
        out2d = ops.mm(ycat.t(), torch.cat([w_out, w_out], 1).t())
    return out2d


# ---- backward stages -------------------------------------------------------------------------------------------------------------
def _d_y(dout2d, w_out, cache):
    """d(y_f) == d(y_r) (E, T) channel-major = W_out^T dout^T: with a tied out_proj the two are the same tensor."""
    Dm = dout2d.shape[1]
    dy = None
    if _STREAM_PROJ_D512 and Dm > 256 and dout2d.dtype == torch.bfloat16:
        dy = ops.gemm_out_t(dout2d, w_out)  # (T, D) @ W_out (D, E) -> (E, T): the weight as it lies is the row-major B operand
    if dy is None and ops.proj_supported(dout2d, Dm):
        dy = ops.proj_wxT(_transposed(cache, "w_outT", w_out), dout2d)
    if dy is None:
        dy = ops.mm(w_out.t(), dout2d.t())
    return dy


def _dW_out(ycat, dout2d, glue):
    """dW_out (D, E) fp32 from [y_f ; y_r] (2E, T): both halves multiply the same tied weight."""
    E, Dm = ycat.shape[0] // 2, dout2d.shape[1]
    part = ops.wgrad_cm_tm(ycat, dout2d, return_partials=True) if (_GLUE_FOLD and _OWN_GEMM) else None  # (slices, 2E, D)
    if part is None:
        dW_cat = _wgrad_cm_tm(ycat, dout2d)
        return (dW_cat[:E] + dW_cat[E:]).t()
    # the fold adds the two halves (second level) as it sums the slices
    dW_out_ED = torch.empty((E, Dm), dtype=torch.float32, device=ycat.device)
    glue.append((part, dW_out_ED, E * Dm, part.shape[0], 2 * E * Dm, 2, E * Dm))
    return dW_out_ED.t()


def _scan_bwd(sets, xz, ycat, dy, seg_P, meta):
    """The scan backward of both sets in one launch, the fold of its dB / dC partial slots into rows [R:] of each set's x_proj gradient
    operand, and the exact gate gradient at lost gates.  Returns (dxz with its [dz] half written, per-set SetWork, per-set d(dbc)
    with rows [R:] written, the zeroed conv dw / db buffers per set)."""
    lib = L.get_lib()
    SB, Lq, split, k, act, dev = meta.SB, meta.Lq, meta.split, meta.k, xz.dtype, xz.device
    E = xz.shape[0] // 2
    z = xz[E:]
    dxz = torch.empty_like(xz)  # [dx ; dz]: the gate z is shared, set f's kernel writes the gradient of both gates (out2 = y_r)
    spec = {}
    for i, s in enumerate(sets):  # per set: dA, dD, ddelta_bias (scan), dw, db (conv): accumulated by the kernels -> zeroed
        spec.update({("dA", i): (s.A.shape, torch.float32), ("dD", i): (s.D.shape, torch.float32),
                     ("dbias", i): (s.dt_bias.shape, torch.float32), ("conv_dw", i): (s.conv_w.shape, torch.float32),
                     ("conv_db", i): (s.conv_b.shape if s.conv_b is not None else (0,), torch.float32)})
    spec.update({("fix_cnt", i): ((1,), torch.int32) for i in range(2)})  # worklist counters of the exact z == 0 gate gradient
    N = sets[0].A.shape[1]
    npart = lib.cad_scan_bwd_partials(E)
    nch = max(1, (Lq // k) // int(lib.cad_scan_bwd_chunk_len()))
    # (the fold follows the scan chunk by chunk with one workgroup per CU: it pays for long rows -- many chunks per (row, slice) item,
    # few items per workgroup; short rows in large batches (configs[1]: 2 chunks, 64 items per workgroup) keep the streaming fold
    # kernel behind the scan: 4.18 vs 4.83 ms per layer, profiles/r06_ab_stream_fold.txt)
    stream_fold = (_STREAM_FOLD and sets[1].A.shape[1] == N and ops.fold_stream_supported(N, npart, Lq // k, act)
                   and nch >= _STREAM_FOLD_MIN_CHUNKS and npart * SB * k * 2 <= 4 * ops._cu_count()
                   and ops.fold_side_available(dev))
    if stream_fold:  # arrival counters (set, row, chunk) and give-up records (set, row, slice) of the concurrent fold
        nci = (int(lib.cad_scan_bwd_fold_counter_ints(SB * k, Lq // k)) + 3) // 4 * 4  # chunk arrivals + started count + CU marks
        spec.update({"fold_counters": ((2, nci), torch.int32), "give_ups": ((2, SB * k, npart), torch.int32)})
    zero = _zeros_f32(spec, dev)
    n_fix = lib.cad_scan_gate_fix_entries(E, SB, Lq)
    fix_list = [torch.empty((n_fix,), dtype=torch.int64, device=dev) for _ in range(2)]
    args = (L.ScanBwdArgs * 2)()
    work = []
    for i, (s, y) in enumerate(zip(sets, ycat.view(2, E, SB, Lq))):
        N = s.A.shape[1]
        R = s.dbc.shape[0] - 2 * N
        np_i = lib.cad_scan_bwd_partials(E)  # (asked once per set on top of `npart`: the pinned schedule keeps the three queries)
        w = SetWork(torch.empty_like(s.xc), torch.empty_like(s.xc), zero["dA", i], zero["dD", i], zero["dbias", i],
                    torch.empty((2, np_i, N, SB, Lq), dtype=ops.scan_slot_dtype(act), device=dev), np_i)
        dz = dxz[E:] if i == 0 else None
        Bm, Cm = s.dbc[R:R + N], s.dbc[R + N:]
        args[i], stream = ops.scan_bwd_args(E, SB, Lq, N, split, _DIRS[i], act, w.npart, k=k, delta_is_dt=meta.delta_is_dt[i], u=s.xc,
                                            delta=s.delta, A=s.A, Bm=Bm, Cm=Cm, D=s.D, z=z, delta_bias=s.dt_bias, dout=dy, out=y,
                                            chunk_state=s.state, du=w.du, ddelta=w.ddelta, dz=dz, dA=w.dA, dB=w.dBC[0], dC=w.dBC[1],
                                            dD=w.dD, ddelta_bias=w.dbias, out2=ycat[E:] if i == 0 else None, gate_fix_list=fix_list[i],
                                            gate_fix_count=zero["fix_cnt", i], gate_fix_dz=dxz[E:],
                                            fold_counters=zero["fold_counters"][i] if stream_fold else None)
        work.append(w)
    ddbcs = [torch.empty_like(s.dbc) for s in sets]
    rows = []  # per set: (dB slots, dC slots, dB rows of d(dbc), dC rows of d(dbc))
    for s, w, ddbc in zip(sets, work, ddbcs):
        N = s.A.shape[1]
        R = s.dbc.shape[0] - 2 * N
        rows.append((*map(L.ptr, w.dBC), L.ptr(ddbc[R:R + N]), L.ptr(ddbc[R + N:])))
    launch_scan = lambda: ops.scan_bwd_launch(lib, args, 2, stream, k, seg_P, _DIRS, split)
    if stream_fold:
        # ... chunk by chunk on a second stream while the scan still runs (cad_fold_partials_stream): the side stream follows the scan launch
        fargs = (L.FoldArgs * 2)()
        for i, (s, w) in enumerate(zip(sets, work)):
            fargs[i] = L.FoldArgs(*rows[i], L.ptr(zero["fold_counters"][i]), L.ptr(zero["give_ups"][i]), SB * k, Lq // k, split * k,
                                  s.A.shape[1], w.npart, *_DIRS[i], L.dtype_code(act))
        _keep = ops.fold_behind_scan(lib, fargs, 2, dev, launch_scan, give_ups=zero["give_ups"])
    else:
        _keep = launch_scan()
    # the gate fix runs behind the scan: a no-op unless some gate is lost (z == 0; fp16: |z| <= 2^-15)
    L.check(lib.cad_scan_bwd_gate_fix(args, 2, stream), "cad_scan_bwd_gate_fix")
    if not stream_fold:
        # ... by one launch behind the scan (four folds: cad_reduce_partials_multi)
        jobs = (L.ReduceJob * 4)(*[L.ReduceJob(src, dst) for dB_s, dC_s, dB, dC in rows for src, dst in ((dB_s, dB), (dC_s, dC))])
        assert work[0].npart == work[1].npart and sets[0].A.shape[1] == sets[1].A.shape[1], "one fold launch: both sets share depth and d_state"
        L.check(lib.cad_reduce_partials_multi(jobs, 4, work[0].npart, sets[0].A.shape[1] * SB * Lq, L.dtype_code(act), stream),
                "cad_reduce_partials_multi")
    return dxz, work, ddbcs, [(zero["conv_dw", i], zero["conv_db", i] if s.conv_b is not None else None) for i, s in enumerate(sets)]


def _d_dt_lr(s, w, ddbc, i, cache, slots, want_dW=True):
    """d(dt_lr) = W_dt^T d(delta) into rows [:R] of d(dbc) (rows [R:] hold the folded dB / dC: the gradient of [dt_lr ; B ; C] is
    assembled in place), and dW_dt (E, R) fp32 -- or None: left in slots["dt"][i] for the fold of the weight-gradient partials.
    want_dW=False (input_grad_only): the plain product alone, and None."""
    (E, T), R = s.xc.shape, s.w_dt.shape[1]
    ddelta, dt_lr, out = w.ddelta, s.dbc[:R], ddbc[:R]
    if want_dW and _FUSED_WGRAD and ops.proj_wx_wgrad_supported(ddelta, R, E, T):
        # d(dt_lr) and dW_dt = d(delta) dt_lr^T from ONE pass over d(delta) (cad_proj_wx_wgrad)
        if "dt" not in slots:
            slots["dt"] = ops.wgrad_partials(T, E, R, ddelta.device, nsets=2)
        ops.proj_wx_wgrad(_transposed(cache, "w_dtT", s.w_dt, i), ddelta, dt_lr, out=out, part=slots["dt"][i])
        return None
    if ops.proj_wx_supported(ddelta, E, T, M=R):
        ops.proj_wx(_transposed(cache, "w_dtT", s.w_dt, i), ddelta, out=out)
    else:
        ops.mm(s.w_dt.t(), ddelta, out=out)
    if not want_dW:
        return None
    if _OWN_DWX and _own_wgrad_chunked_ok(ddelta, R):
        return _own_wgrad_chunked(ddelta, dt_lr).t()
    return _wgrad_cm_cm(ddelta, dt_lr)


def _dW_x(s, ddbc, i, slots):
    """dW_x (R + 2N, E) fp32 = d(dbc) xc^T -- or None: left in slots["x"][i] for the fold of the weight-gradient partials."""
    xc, (E, T), M = s.xc, s.xc.shape, ddbc.shape[0]
    if _OWN_DWX and ops.proj_wgrad_only_supported(xc, M, E, T):
        if "x" not in slots:
            slots["x"] = ops.wgrad_partials(T, E, M, xc.device, nsets=2)
        ops.proj_wgrad_only(xc, ddbc, part=slots["x"][i])
        return None
    if _OWN_DWX and _own_wgrad_chunked_ok(xc, M):
        return _own_wgrad_chunked(xc, ddbc)
    return _wgrad_cm_cm(ddbc, xc)


def _d_xc(s, du, ddbc, i, cache):
    """d(xc) = du + W_x^T . d(dbc), in place in du (no copy of the 268 MB addend)."""
    M, T = ddbc.shape
    if ops.proj_wx_supported(du, M, T):
        ops.proj_wx(_transposed(cache, "w_xT", s.w_x, i), ddbc, out=du, acc=du)
    elif du.dtype == torch.float32:
        ops.mm_f32(s.w_x.t(), ddbc, out=du, addend=du)
    elif du.dtype == torch.float16:  # (shapes the fp16 MFMA kernel does not serve: the fp32 kernel on the exact widening)
        du.copy_(ops.mm_f32(s.w_x.t().float(), ddbc.float(), addend=du.float()))
    else:
        du.addmm_(s.w_x.t(), ddbc)


def _dx2d_is_streamed() -> bool:
    return _OWN_GEMM


def _d_x2d(dxz, w_in, cache):
    """d(x2d) (T, D) token-major = dxz^T W_in (d_model 256: one 256-row tile, dxz read once; d_model 512: profiles/r05_gemm_stream_d512.txt)."""
    dx2d = ops.proj_xTw_stream(_transposed(cache, "w_inT", w_in), dxz) if _dx2d_is_streamed() else None
    return ops.mm(dxz.t(), w_in) if dx2d is None else dx2d


def _dW_in_partials(dxz, x2d, glue):
    """dW_in (2E, D) fp32 as a job of the fold of the weight-gradient partials, or None where its partial tiles are not served."""
    part = ops.wgrad_cm_tm(dxz, x2d, return_partials=True) if (_GLUE_FOLD and _OWN_GEMM) else None
    if part is None:
        return None
    dW_in = torch.empty((dxz.shape[0], x2d.shape[1]), dtype=torch.float32, device=x2d.device)
    glue.append((part, dW_in, dW_in.numel(), part.shape[0], dW_in.numel(), 1, 0))
    return dW_in


def _wgrad_slot_sums(slots, glue):
    """{"dt" / "x": (2, K, M) fp32 sums over the partial slots (2, P, K, M) of both sets} (fixed order) -- with _GLUE_FOLD as jobs of the
    fold launch.  The slots hold (K, M); they are summed as they lie (a reduction over a permuted view runs at a quarter of the rate)."""
    if not _GLUE_FOLD:
        return {name: wg.sum(dim=1) for name, wg in slots.items()}
    sums = {}
    for name in ("dt", "x"):
        if name in slots:
            _, P, K, M = slots[name].shape
            sums[name] = torch.empty((2, K, M), dtype=torch.float32, device=slots[name].device)
            glue += [(src, dst, K * M, P, K * M, 1, 0) for src, dst in zip(slots[name], sums[name])]
    return sums


def _backward_input_only(dout2d, xz, w_in, w_out, ycat, sets, seg_P, meta, cache):
    """d(x2d) alone (input_grad_only): the stages d(x2d) depends on, in the full backward's order -- d(y), the scan backward with its
    dB / dC fold, d(dt_lr), d(xc), the conv backward, d(x2d).  No weight-gradient product, slot, slot sum or fold launch."""
    E = xz.shape[0] // 2
    T = dout2d.shape[0]
    dy = _d_y(dout2d, w_out, cache)
    dxz, work, ddbcs, conv_bufs = _scan_bwd(sets, xz, ycat, dy, seg_P, meta)
    for i, (s, w, ddbc) in enumerate(zip(sets, work, ddbcs)):
        _d_dt_lr(s, w, ddbc, i, cache, None, want_dW=False)
        _d_xc(s, w.du, ddbc, i, cache)
    _conv_bwd2(xz[:E], [(s.conv_w, s.conv_b) for s in sets], [w.du for w in work], dxz[:E], meta.split, _DIRS, bufs=conv_bufs)
    return _d_x2d(dxz.view(2 * E, T), w_in, cache)


class BiMambaMixerFn(torch.autograd.Function):
    """out (T, D) = out_proj(scan_f + scan_r) for normed input x2d (T, D), T = S*B*L rows in t-frame order.

    Tensor arguments: x2d, W_in (2E, D), W_out (D, E), then per parameter set (f, r):
    conv_w (E,1,K), conv_b (E), W_x (R+2N, E), W_dt (E, R), dt_bias (E), A_log (E, N), D (E)."""

    @staticmethod
    def forward(ctx, x2d, SB, Lq, split, cache, fp8_act, W_in, W_out, *ps):
        act = x2d.dtype
        T = x2d.shape[0]
        E = W_in.shape[0] // 2
        params, _ = _unflatten(SetParams, ps, 2)
        if cache is not None and cache.w_in.dtype != act:
            cache = None
        w_in = cache.w_in if cache else W_in.to(act)
        w_out = cache.w_out if cache else W_out.to(act)
        xz = _in_proj(x2d, W_in, w_in, cache, fp8_act).view(2 * E, SB, Lq)
        x, z = xz[:E], xz[E:]
        cparams = [(p.conv_w.float().reshape(E, -1).contiguous(), None if p.conv_b is None else p.conv_b.float().contiguous())
                   for p in params]
        xcs = [xc.view(E, T) for xc in _conv_fwd2(x, cparams, split, _DIRS)]  # (from here on activations are (channels, T) views)
        sets, delta_is_dt = [], []
        for i, (p, xc, (conv_w, conv_b)) in enumerate(zip(params, xcs, cparams)):
            w_x, w_dt = (cache.w_x[i], cache.w_dt[i]) if cache else (p.W_x.to(act), p.W_dt.to(act))
            dbc = _x_proj(w_x, xc)
            dt_bias = p.dt_bias.float().contiguous()
            delta, fused = _dt_proj(w_dt, dbc[:w_dt.shape[1]], dt_bias)
            A = cache.A[i] if cache else -torch.exp(p.A_log.float())
            sets.append(SetSaved(xc, delta, A, dbc, p.D.float().contiguous(), dt_bias, conv_w, conv_b, w_x, w_dt, None, p.A_log))
            delta_is_dt.append(fused)
        k = ops.lsplit_factor(E, SB, Lq, 2)
        ycat = torch.empty((2 * E, SB, Lq), dtype=act, device=x2d.device)  # [y_f ; y_r]: one out_proj GEMM with K = 2E
        sets, seg_P = _scan_fwd(sets, z, ycat, delta_is_dt, split, k)
        out2d = _out_proj(w_out, ycat.view(2 * E, T), cache)
        ctx.cache = cache  # (not saved tensors: plain per-step copies owned by the cache)
        ctx.input_grad_only = input_grad_only_enabled()
        ctx.save_for_backward(x2d, xz, w_in, w_out, ycat, *_flatten(sets), *seg_P)
        ctx.meta = Meta(SB, Lq, split, [SetParams(*(None if t is None else t.dtype for t in p)) for p in params],
                        [p.conv_w.shape for p in params], W_in.dtype, W_out.dtype, tuple(delta_is_dt), k)
        return out2d

    @staticmethod
    def backward(ctx, dout2d):
        x2d, xz, w_in, w_out, ycat, *rest = ctx.saved_tensors
        sets, seg_P = _unflatten(SetSaved, rest, 2)
        meta, cache = ctx.meta, ctx.cache
        T = x2d.shape[0]
        E = xz.shape[0] // 2
        dout2d = dout2d.contiguous()
        if ctx.input_grad_only:
            return (_backward_input_only(dout2d, xz, w_in, w_out, ycat, sets, seg_P, meta, cache),) + (None,) * (7 + 2 * len(SetParams._fields))
        glue = []  # (src, dst, n, nparts, stride, nparts2, stride2) jobs of the one fp32 fold launch at the end (_GLUE_FOLD)
        slots = {}  # "dt" / "x": fp32 partial slots of the own weight-gradient kernels, both sets (allocated by the first set that uses them)
        dy = _d_y(dout2d, w_out, cache)
        dW_out = _dW_out(ycat.view(2 * E, T), dout2d, glue)
        dxz, work, ddbcs, conv_bufs = _scan_bwd(sets, xz, ycat, dy, seg_P, meta)
        part = []
        for i, (s, w, ddbc) in enumerate(zip(sets, work, ddbcs)):
            dW_dt = _d_dt_lr(s, w, ddbc, i, cache, slots)
            dW_x = _dW_x(s, ddbc, i, slots)
            _d_xc(s, w.du, ddbc, i, cache)
            part.append((dW_x, dW_dt, w.dA * s.A))  # A = -exp(A_log)  =>  dA/dA_log = A
        if CAPTURE_XPROJ_OPERANDS is not None:
            CAPTURE_XPROJ_OPERANDS.append({"ddbc": [d.clone() for d in ddbcs], "xc": [s.xc.clone() for s in sets]})
        conv_g = _conv_bwd2(xz[:E], [(s.conv_w, s.conv_b) for s in sets], [w.du for w in work], dxz[:E], meta.split, _DIRS,
                            bufs=conv_bufs)
        sums = _wgrad_slot_sums(slots, glue)
        # d(x2d) and dW_in first: the fold launch below reads dW_in's partial tiles
        dx2d = _d_x2d(dxz.view(2 * E, T), w_in, cache)
        dW_in = _dW_in_partials(dxz.view(2 * E, T), x2d, glue)
        if glue:
            ops.fold_f32(glue)
        if "x" in sums:
            sums["x"] = sums["x"].transpose(1, 2).contiguous()  # (the small (2, K, M) result is transposed, not the slots)
        grads = []
        for i, (dt, (dwc, dbc_conv), (dW_x, dW_dt, dA_log), w) in enumerate(zip(meta.pdtypes, conv_g, part, work)):
            dW_x = sums["x"][i] if dW_x is None else dW_x
            dW_dt = sums["dt"][i] if dW_dt is None else dW_dt
            grads += SetParams(conv_w=dwc.reshape(meta.conv_w_shapes[i]).to(dt.conv_w),
                               conv_b=None if dbc_conv is None else dbc_conv.to(dt.conv_b), W_x=dW_x.to(dt.W_x), W_dt=dW_dt.to(dt.W_dt),
                               dt_bias=w.dbias.to(dt.dt_bias), A_log=dA_log.to(dt.A_log), D=w.dD.to(dt.D))
        if dW_in is None:
            dW_in = _wgrad_cm_tm(dxz.view(2 * E, T), x2d)
        return (dx2d, None, None, None, None, None, dW_in.to(meta.win_dt), dW_out.to(meta.wout_dt), *grads)


def can_use(mamba_fwd, mamba_rev, strategy) -> bool:
    """The hand-scheduled path covers the released-model configuration; everything else goes through engine.py."""
    if mamba_rev is None or (strategy or "add") != "add":
        return False
    tied = (mamba_rev.in_proj.weight is mamba_fwd.in_proj.weight and mamba_rev.out_proj.weight is mamba_fwd.out_proj.weight)
    no_bias = mamba_fwd.in_proj.bias is None and mamba_fwd.out_proj.bias is None
    same = mamba_fwd.d_state == mamba_rev.d_state and mamba_fwd.dt_rank == mamba_rev.dt_rank
    return bool(tied and no_bias and same)


def bimamba_mixer(hn: torch.Tensor, mamba_fwd, mamba_rev, split: int) -> torch.Tensor:
    S, B, Lq, Dm = hn.shape
    ps = _flatten(SetParams(m.conv1d.weight, m.conv1d.bias, m.x_proj.weight, m.dt_proj.weight, m.dt_proj.bias, m.A_log, m.D)
                  for m in (mamba_fwd, mamba_rev))
    cache = _cached(mamba_fwd, [mamba_fwd.in_proj.weight, mamba_fwd.out_proj.weight, mamba_fwd.x_proj.weight,
                                mamba_fwd.dt_proj.weight, mamba_rev.x_proj.weight, mamba_rev.dt_proj.weight,
                                mamba_fwd.A_log, mamba_rev.A_log])
    fp8_act = ops.fp8_operand_of(hn) if _FP8_IN_PROJ else None  # (ops.add_norm(want_fp8=True) attaches it; stale copies are refused)
    out = BiMambaMixerFn.apply(hn.reshape(S * B * Lq, Dm), S * B, Lq, split, cache, fp8_act, mamba_fwd.in_proj.weight,
                               mamba_fwd.out_proj.weight, *ps)
    return out.view(S, B, Lq, Dm)
