"""Autograd-aware Python entry points over the C-ABI kernels (include/caduceus_hip.h).

Each function mirrors one interface the reference reaches through its third-party native dependencies
(mamba_ssm `selective_scan_fn` / `causal_conv1d_fn` / `rms_norm_fn`; call sites cited in the header), but in the
flip-free "t-frame" / channel-major layouts described in DESIGN.md.  PyTorch is used here only as the owner of device
memory, streams and the autograd graph; all arithmetic of these ops happens in the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Tuple

import torch

from . import _lib as L


def _zeros_like_f32(t, shape=None):
    return torch.zeros(t.shape if shape is None else shape, dtype=torch.float32, device=t.device)


# ------------------------------------------------------------------------------------------------------------------
# embedding
# ------------------------------------------------------------------------------------------------------------------
class _Embed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, weight, comp, n_strands, out_dtype):
        ids = ids.contiguous()
        w = weight.contiguous()
        B, Lq = ids.shape
        V, D = w.shape
        out = torch.empty((n_strands, B, Lq, D), dtype=out_dtype, device=w.device)
        stream = L.stream_and_check(ids, w, comp, out)
        a = L.EmbedArgs(L.ptr(ids), L.ptr(comp), L.ptr(w), L.ptr(out), B, Lq, D, V, n_strands, L.dtype_code(w.dtype),
                        L.dtype_code(out_dtype))
        L.check(L.get_lib().cad_embed_fwd(C.byref(a), stream), "cad_embed_fwd")
        ctx.save_for_backward(ids, comp)
        ctx.meta = (V, D, n_strands, w.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        ids, comp = ctx.saved_tensors
        V, D, n_strands, wdt = ctx.meta
        dout = dout.contiguous()
        dw = torch.zeros((V, D), dtype=torch.float32, device=dout.device)
        if V * D * 4 > 64 * 1024:
            # the kernel keeps the whole (V, D) gradient in LDS (DNA vocabularies: 16 x D); larger vocabularies
            # (CaduceusConfig's default vocab_size is 50277) scatter-add through the allocator-owning framework instead
            flat = ids.reshape(-1)
            dw.index_add_(0, flat, dout[0].reshape(-1, D).float())
            if n_strands == 2:
                dw.index_add_(0, comp[flat], dout[1].reshape(-1, D).float())
            return None, dw.to(wdt), None, None, None
        stream = L.stream_and_check(ids, comp, dout, dw)
        B, Lq = ids.shape
        a = L.EmbedBwdArgs(L.ptr(ids), L.ptr(comp), L.ptr(dout), L.ptr(dw), B, Lq, D, V, n_strands,
                           L.dtype_code(dout.dtype))
        slots = wgrad_slots(L.get_lib().cad_embed_bwd_slots(C.byref(a)), V * D, dout.device)
        L.check(L.get_lib().cad_embed_bwd_slotted(C.byref(a), L.ptr(slots), stream), "cad_embed_bwd_slotted")
        return None, dw.to(wdt), None, None, None


def wgrad_slots(n_slots: int, n: int, device, zero: bool = True) -> torch.Tensor:
    """fp32 (n_slots, n): one slot per workgroup of a backward kernel for its share of a weight gradient (the cad_*_bwd_slotted
    entry points), folded by the library in a fixed order instead of fp32 atomics in arrival order, so that the gradient -- and every
    training step after it -- is the same in every run.  zero=False: for the kernels whose every workgroup stores its whole slot (conv1d,
    add + norm) -- no fill launch; the embedding's scalar kernel runs fewer workgroups than it has slots and keeps the fill."""
    if n_slots < 1:
        raise RuntimeError("caduceus_amd: a backward kernel reported no workgroups")
    return (torch.zeros if zero else torch.empty)((n_slots, n), dtype=torch.float32, device=device)


def embed(ids: torch.Tensor, weight: torch.Tensor, comp: Optional[torch.Tensor], n_strands: int,
          out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(B, L) int64 ids -> (n_strands, B, L, D) t-frame embedding.  RCPSEmbedding (modeling_rcps.py:46-67)."""
    if ids.dtype != torch.int64:
        ids = ids.long()
    if n_strands == 2 and comp is None:
        raise AssertionError("Complement map must be provided for RCPS.")  # modeling_caduceus.py:350
    return _Embed.apply(ids, weight, comp, n_strands, out_dtype)


# ------------------------------------------------------------------------------------------------------------------
# fused add + norm
# ------------------------------------------------------------------------------------------------------------------
# set by mixer.set_fp8_in_proj: add_norm also emits the e4m3 copy of the normed activations (cad_add_norm_args.y_fp8 / y_scale)
FP8_ACTIVATIONS = False


class _AddNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps, is_rms, swap_flip, y_dtype, want_fp8=False):
        x = x.contiguous()
        S, D = x.shape[0], x.shape[-1]
        rows = x.numel() // (S * D)
        w = weight.float().contiguous()
        b = None if bias is None else bias.float().contiguous()
        res = None if residual is None else residual.contiguous()
        if res is not None and res.dtype != torch.float32:
            raise TypeError("caduceus_amd keeps the residual stream in fp32")
        y = torch.empty(x.shape, dtype=y_dtype, device=x.device)
        res_out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        rstd = torch.empty((S * rows,), dtype=torch.float32, device=x.device)
        mean = None if is_rms else torch.empty((S * rows,), dtype=torch.float32, device=x.device)
        yq = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_fp8 else None
        ys = torch.empty((S * rows,), dtype=torch.float32, device=x.device) if want_fp8 else None
        stream = L.stream_and_check(x, res, w, b, y, res_out, rstd, mean, yq, ys)
        a = L.AddNormArgs(L.ptr(x), L.ptr(res), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(res_out), L.ptr(rstd), L.ptr(mean),
                          rows, S, D, float(eps), int(is_rms), int(swap_flip), L.dtype_code(x.dtype),
                          L.dtype_code(y_dtype), L.ptr(yq), L.ptr(ys))
        L.check(L.get_lib().cad_add_norm_fwd(C.byref(a), stream), "cad_add_norm_fwd")
        ctx.save_for_backward(res_out, rstd, mean, w)
        ctx.meta = (rows, S, D, is_rms, swap_flip, x.dtype, y_dtype, residual is not None, bias is not None,
                    weight.dtype)
        if want_fp8:
            ctx.mark_non_differentiable(yq, ys)
            return y, res_out, yq, ys
        return y, res_out

    @staticmethod
    def backward(ctx, dy, dres_out, *_unused):
        res_out, rstd, mean, w = ctx.saved_tensors
        rows, S, D, is_rms, swap_flip, x_dtype, y_dtype, has_res, has_bias, wdt = ctx.meta
        dy = dy.contiguous()
        dres_out = None if dres_out is None else dres_out.contiguous()
        dx = torch.empty(res_out.shape, dtype=x_dtype, device=dy.device)
        dres_in = torch.empty(res_out.shape, dtype=torch.float32, device=dy.device) if has_res else None
        # (dw / db are WRITTEN by the fold of the slots, the slots by their workgroups: nothing here needs a fill launch)
        dw = torch.empty((D,), dtype=torch.float32, device=dy.device)
        db = torch.empty((D,), dtype=torch.float32, device=dy.device) if has_bias else None
        stream = L.stream_and_check(dy, dres_out, res_out, rstd, mean, w, dx, dres_in, dw, db)
        a = L.AddNormBwdArgs(L.ptr(dy), L.ptr(dres_out), L.ptr(res_out), L.ptr(rstd), L.ptr(mean), L.ptr(w), L.ptr(dx),
                             L.ptr(dres_in), L.ptr(dw), L.ptr(db), rows, S, D, int(is_rms), int(swap_flip),
                             L.dtype_code(x_dtype), L.dtype_code(y_dtype))
        n = L.get_lib().cad_add_norm_bwd_slots(C.byref(a))
        ws, bs = wgrad_slots(n, D, dy.device, zero=False), (None if db is None else wgrad_slots(n, D, dy.device, zero=False))
        L.check(L.get_lib().cad_add_norm_bwd_slotted(C.byref(a), L.ptr(ws), L.ptr(bs), stream), "cad_add_norm_bwd_slotted")
        return dx, dres_in, dw.to(wdt), (None if db is None else db.to(wdt)), None, None, None, None, None


def add_norm(x: torch.Tensor, residual: Optional[torch.Tensor], weight: torch.Tensor, bias: Optional[torch.Tensor],
             eps: float, is_rms: bool, swap_flip: bool, y_dtype: torch.dtype, want_fp8: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """x: (S, ..., D) t-frame.  Returns (normed in y_dtype, fp32 residual stream) -- rms_norm_fn(prenorm=True) for both
    strands at once, with the reference's fused-path strand swap as an index map when `swap_flip`.
    want_fp8: the caller feeds `normed` to mixer.bimamba_mixer, whose in_proj runs on the fp8 matrix cores (configs[4]) -- only those
    call sites ask for the e4m3 epilogue (the final norm_f, the un-fused wrapper and the sequence-parallel path never consume it)."""
    if swap_flip and x.shape[0] != 2:
        raise ValueError("swap_flip needs two strands")
    D = int(x.shape[-1])
    if want_fp8 and FP8_ACTIVATIONS and y_dtype == torch.bfloat16 and D % 4 == 0 and D <= 512 and _fp8_epilogue_aligned(x, residual) and \
            bool(L.get_lib().cad_proj_fp8_supported(D)):
        # its e4m3 operand (+ per-token scales) is written by this kernel's epilogue and travels with the tensor, together with what
        # identifies the contents it was made from (fp8_operand_of checks version, storage and shape before the mixer trusts it)
        y, res, yq, ys = _AddNorm.apply(x, residual, weight, bias, eps, is_rms, swap_flip, y_dtype, True)
        y._cad_fp8 = (yq, ys, y._version, y.data_ptr(), tuple(y.shape))
        return y, res
    return _AddNorm.apply(x, residual, weight, bias, eps, is_rms, swap_flip, y_dtype)


def _fp8_epilogue_aligned(x, residual) -> bool:
    """cad_add_norm_fwd writes the e4m3 copy from its 16-byte vector instantiation only (addnorm.hip: CAD_ERR_UNSUPPORTED otherwise):
    mirror that here, so that an input the scalar kernel serves keeps working with the fp8 projection switched on."""
    ok = x.is_contiguous() and x.data_ptr() % 16 == 0 and (x.shape[-1] * x.element_size()) % 16 == 0
    if residual is not None:
        ok = ok and residual.data_ptr() % 16 == 0
    return ok


def fp8_operand_of(y: torch.Tensor):
    """(e4m3 copy, per-token scales) attached by add_norm(want_fp8=True), or None unless `y` still is the tensor they were made from:
    same storage, same shape, and not written since (an in-place op between the norm and the mixer bumps the version counter)."""
    rec = getattr(y, "_cad_fp8", None)
    if rec is None or not y.is_contiguous():
        return None
    yq, ys, ver, ptr, shape = rec
    if y._version != ver or y.data_ptr() != ptr or tuple(y.shape) != shape:
        return None
    return yq, ys


# ------------------------------------------------------------------------------------------------------------------
# causal conv1d
# ------------------------------------------------------------------------------------------------------------------
class _Conv1d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, split, rev_lo, rev_hi):
        x = x.contiguous()
        E, SB, Lq = x.shape
        wf = w.float().reshape(E, -1).contiguous()
        bf = None if bias is None else bias.float().contiguous()
        out = torch.empty_like(x)
        stream = L.stream_and_check(x, wf, bf, out)
        a = L.Conv1dArgs(L.ptr(x), L.ptr(wf), L.ptr(bf), L.ptr(out), SB, Lq, split, E, wf.shape[1], rev_lo, rev_hi,
                         L.dtype_code(x.dtype))
        L.check(L.get_lib().cad_conv1d_fwd(C.byref(a), stream), "cad_conv1d_fwd")
        ctx.save_for_backward(x, wf, bf)
        ctx.meta = (split, rev_lo, rev_hi, w.shape, w.dtype, bias is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, wf, bf = ctx.saved_tensors
        split, rev_lo, rev_hi, wshape, wdt, has_bias = ctx.meta
        E, SB, Lq = x.shape
        dout = dout.contiguous()
        dx = torch.empty_like(x)
        dw = torch.empty_like(wf)  # (written by the fold of the slots)
        db = torch.empty((E,), dtype=torch.float32, device=x.device) if has_bias else None
        stream = L.stream_and_check(x, wf, bf, dout, dx, dw, db)
        a = L.Conv1dBwdArgs(L.ptr(x), L.ptr(wf), L.ptr(bf), L.ptr(dout), L.ptr(dx), L.ptr(dw), L.ptr(db), SB, Lq, split,
                            E, wf.shape[1], rev_lo, rev_hi, L.dtype_code(x.dtype), 0)
        n = L.get_lib().cad_conv1d_bwd_slots(C.byref(a))
        ws, bs = wgrad_slots(n, dw.numel(), x.device, zero=False), (None if db is None else wgrad_slots(n, E, x.device, zero=False))
        L.check(L.get_lib().cad_conv1d_bwd_multi_slotted(C.byref(a), 1, (C.c_void_p * 1)(ws.data_ptr()),
                                                         (C.c_void_p * 1)(0 if bs is None else bs.data_ptr()), stream),
                "cad_conv1d_bwd_multi_slotted")
        return dx, dw.reshape(wshape).to(wdt), (None if db is None else db.to(wdt)), None, None, None


def causal_conv1d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], split: int, rev_lo: int,
                  rev_hi: int) -> torch.Tensor:
    """x: (E, SB, L) channel-major.  Depthwise causal conv + SiLU in each row's own direction."""
    return _Conv1d.apply(x, w, bias, int(split), int(rev_lo), int(rev_hi))


# ------------------------------------------------------------------------------------------------------------------
# selective scan
# ------------------------------------------------------------------------------------------------------------------
# Every caller of the scan kernels (the autograd functions below, seqpar._ScanSeqPar, the mixer's _scan_fwd / _scan_bwd) fills
# cad_scan_args / cad_scan_bwd_args through scan_fwd_args / scan_bwd_args: tensors by field name, absent fields NULL, the L-split
# reshaping applied in that one place.  The autograd functions also share their backward: scan_bwd_sets (outputs + structs),
# fold_dBC and scan_bwd_grads (parameter-dtype casts, dz over the sets); each keeps its own launches.
# ---- L-split (two-pass) scans on one GPU --------------------------------------------------------------------------------
# A scan launch has ceil(E / 8) * rows * sets workgroups -- 256 for Caduceus-PS at batch 1, i.e. one per CU, but only 128 for
# Caduceus-Ph or a uni-directional model at batch 1.  When fewer than ~one workgroup per CU exist,
# every row is cut into k segments along L, presented to the SAME kernels as rows (E, SB * k, L / k) of the same buffers:
#   pass 1 (cheap kernel modes `map_only` / `carry_only`): each segment's affine state map from a zero entry state,
#   composition of the k maps per row in the row's own direction (a few element-wise launches on (E, SB * k, N) tensors),
#   pass 2 (the full kernels) from the true entry states (h0 / dhT of the scan C-ABI).
# The same carries and composition chain segments ACROSS ranks in caduceus_amd/seqpar.py.
_CU_COUNT = {}


def _cu_count() -> int:
    """Compute units of the CURRENT device (256 on MI355X), queried once per device; 256 without a device (host emulator).  The
    library's launchers size their grids with the same number (csrc/api.hip: cad_cu_count)."""
    if not torch.cuda.is_available():
        return 256
    dev = torch.cuda.current_device()
    if dev not in _CU_COUNT:
        _CU_COUNT[dev] = int(torch.cuda.get_device_properties(dev).multi_processor_count)
    return _CU_COUNT[dev]


def lsplit_factor(E: int, SB: int, Lq: int, nsets: int) -> int:
    env = os.environ.get("CADUCEUS_AMD_LSPLIT", "")
    chunk = int(L.get_lib().cad_scan_chunk_len())
    if env:  # forced (tests, A/B runs): segments only have to be whole forward chunks
        k = max(1, int(env))
        return k if Lq % (k * chunk) == 0 else 1
    ok = lambda k: Lq % (k * chunk) == 0 and Lq // k >= 8 * chunk
    wgs = ((E + 7) // 8) * SB * nsets
    k = 1
    while wgs * 2 * k <= _cu_count() and ok(2 * k):
        k *= 2
    return k


def compose_segments(P, S, k: int, split: int, rev_lo: int, rev_hi: int, towards_end: bool):
    """P, S: (E, SB * k, N) maps  v -> P * v + S  of the k segments of every row (segment q of row r is row r * k + q).
    Returns the value ENTERING every segment when the chain starts from zero at the row's logical start
    (towards_end=False: forward states) or at its logical end (towards_end=True: state gradients)."""
    E, SBk, N = S.shape
    SB = SBk // k
    P4, S4 = P.view(E, SB, k, N), S.view(E, SB, k, N)
    out = torch.zeros_like(S4)
    for rows, rev in ((slice(0, split), rev_lo), (slice(split, SB), rev_hi)):
        if rows.start >= rows.stop:
            continue
        ascending = (rev == 0) != towards_end
        order = list(range(k)) if ascending else list(range(k - 1, -1, -1))
        v = None
        for j, q in enumerate(order):
            if v is not None:
                out[:, rows, q] = v
            if j + 1 < k:
                v = S4[:, rows, q] if v is None else P4[:, rows, q] * v + S4[:, rows, q]
    return out.view(E, SBk, N)


def scan_fwd_launch(lib, args, nsets: int, stream, k: int, As, dirs, split: int):
    """cad_scan_fwd_multi on argument structs that already describe the k-way reshaped problem (SB * k rows of L / k).
    k > 1: runs pass 1 (map_only), composes the entry states and points args[i].h0 at them.  Returns (keep-alive tensors,
    [P_i]) -- P_i = exp(A * sum_dt) per segment, which the backward needs again."""
    keep, Ps = [], []
    if k > 1:
        E, SBk, N = args[0].E, args[0].SB, args[0].N
        dev = As[0].device
        p1 = (L.ScanArgs * nsets)()
        hTs, sdts = [], []
        for i in range(nsets):
            C.memmove(C.byref(p1[i]), C.byref(args[i]), C.sizeof(L.ScanArgs))
            hT = torch.empty((E, SBk, N), dtype=torch.float32, device=dev)
            sdt = torch.empty((E, SBk), dtype=torch.float32, device=dev)
            p1[i].map_only, p1[i].out, p1[i].chunk_state, p1[i].z = 1, None, None, None
            p1[i].h0, p1[i].hT, p1[i].sum_dt = None, L.ptr(hT), L.ptr(sdt)
            hTs.append(hT), sdts.append(sdt)
        L.check(lib.cad_scan_fwd_multi(p1, nsets, stream), "cad_scan_fwd_multi (map pass)")
        for i in range(nsets):
            P = torch.exp(As[i].unsqueeze(1) * sdts[i].unsqueeze(-1))
            h0 = compose_segments(P, hTs[i], k, split, dirs[i][0], dirs[i][1], towards_end=False).contiguous()
            args[i].h0 = L.ptr(h0)
            keep.append(h0)
            Ps.append(P)
    L.check(lib.cad_scan_fwd_multi(args, nsets, stream), "cad_scan_fwd_multi")
    return keep, Ps


def scan_bwd_launch(lib, args, nsets: int, stream, k: int, Ps, dirs, split: int):
    """cad_scan_bwd_multi on k-way reshaped argument structs; k > 1: pass 1 (carry_only) + composition of the state
    gradients entering every segment (args[i].dhT)."""
    keep = []
    if k > 1:
        E, SBk, N = args[0].E, args[0].SB, args[0].N
        dev = Ps[0].device
        p1 = (L.ScanBwdArgs * nsets)()
        gs = []
        for i in range(nsets):
            C.memmove(C.byref(p1[i]), C.byref(args[i]), C.sizeof(L.ScanBwdArgs))
            g = torch.empty((E, SBk, N), dtype=torch.float32, device=dev)
            p1[i].carry_only, p1[i].dhT, p1[i].dh0 = 1, None, L.ptr(g)
            p1[i].dz, p1[i].out2, p1[i].gate_fix_list, p1[i].gate_fix_count = None, None, None, None
            p1[i].fold_counters = None  # (the carry pass writes no slots)
            gs.append(g)
        L.check(lib.cad_scan_bwd_multi(p1, nsets, stream), "cad_scan_bwd_multi (carry pass)")
        for i in range(nsets):
            dhT = compose_segments(Ps[i], gs[i], k, split, dirs[i][0], dirs[i][1], towards_end=True).contiguous()
            args[i].dhT = L.ptr(dhT)
            keep.append(dhT)
    L.check(lib.cad_scan_bwd_multi(args, nsets, stream), "cad_scan_bwd_multi")
    return keep


# ---- the dB / dC fold behind the running scan backward (cad_fold_partials_stream) ----------------------------------------------------
_FOLD_SIDE = {}  # device index -> (side stream, "inputs ready" event, "fold done" event)


def fold_stream_supported(N: int, npart: int, Lq: int, dtype) -> bool:
    return bool(L.get_lib().cad_fold_stream_supported(int(N), int(npart), int(Lq), L.dtype_code(dtype)))


def _fold_side(device):
    """(side stream, event, event) whose kernels really run NEXT TO the current stream's, or None.  HIP serves all streams from a few
    hardware queues: a second stream that shares the current stream's queue runs its kernels behind it (measured under torchrun + RCCL:
    the process group's stream shifted the assignment, the fold ran after every scan, +8 ms per step).  So candidates are probed once
    per (device, current stream) with cad_stream_probe -- one wave waiting up to 2 ms on one stream for a flag set from the other --
    and the first stream that overlaps is kept; with none, the caller keeps the fold kernel behind the scan."""
    main = torch.cuda.current_stream(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), main.cuda_stream)
    if key not in _FOLD_SIDE:
        lib = L.get_lib()
        found = None
        buf = torch.zeros((16, 2), dtype=torch.int32, device=device)
        for i in range(8):
            cand = torch.cuda.Stream(device)
            cand.wait_stream(main)  # (the zero fill above)
            L.check(lib.cad_stream_probe(C.c_void_p(main.cuda_stream), C.c_void_p(cand.cuda_stream), L.ptr(buf[i, 0:1]),
                                         L.ptr(buf[i, 1:2]), 2000), "cad_stream_probe")
            main.wait_stream(cand)
            if int(buf[i, 1].item()) == 1:  # (one host synchronisation per candidate, once per process)
                found = cand
                break
        _FOLD_SIDE[key] = None if found is None else (found, torch.cuda.Event(), torch.cuda.Event())
        if os.environ.get("CADUCEUS_AMD_VERBOSE"):
            print(f"caduceus_amd: concurrent fold stream for {key}: {'candidate %d' % i if found is not None else 'none (fold kernel behind the scan)'}")
    return _FOLD_SIDE[key]


def fold_side_available(device) -> bool:
    return (not L.is_device_build()) or _fold_side(device) is not None


FOLD_GIVE_UPS = None  # a list: every device launch appends the number of give-up records (a device scalar) of its concurrent pass


def _count_give_ups(give_ups):
    """Diagnostics (tests, tools): the slices the concurrent pass left to the cleanup.  The records are int32 (chunk + 1) and are
    counted as such: read as fp32 they are denormals, which a flush-to-zero count would miss."""
    if FOLD_GIVE_UPS is not None and give_ups is not None:
        assert give_ups.dtype == torch.int32
        FOLD_GIVE_UPS.append(torch.count_nonzero(give_ups))


def fold_behind_scan(lib, fold_args, nsets: int, device, launch_scan, give_ups=None):
    """launch_scan() enqueues cad_scan_bwd_multi (with fold_counters set) on the current stream; the fold is enqueued on a second stream
    right behind it so that the two kernels run side by side (the fold's workgroups -- 48 VGPRs, 8 KB of LDS -- fit on the CUs next to
    the scan's), the current stream then waits for the fold and runs the cleanup pass (a no-op unless the fold gave up waiting, i.e.
    the two kernels were NOT co-scheduled).  The host emulator has no streams: the same three launches in order."""
    if not L.is_device_build():
        out = launch_scan()
        L.check(lib.cad_fold_partials_stream(fold_args, nsets, 0, None), "cad_fold_partials_stream (concurrent)")
        _count_give_ups(give_ups)
        L.check(lib.cad_fold_partials_stream(fold_args, nsets, 1, None), "cad_fold_partials_stream (cleanup)")
        return out
    side, ev_ready, ev_done = _fold_side(device)
    main = torch.cuda.current_stream(device)
    ev_ready.record(main)  # counters zeroed, slots and destination rows allocated (and their previous users finished) before the fold starts
    out = launch_scan()
    side.wait_event(ev_ready)
    L.check(lib.cad_fold_partials_stream(fold_args, nsets, 0, C.c_void_p(side.cuda_stream)), "cad_fold_partials_stream (concurrent)")
    ev_done.record(side)
    main.wait_event(ev_done)
    _count_give_ups(give_ups)
    L.check(lib.cad_fold_partials_stream(fold_args, nsets, 1, C.c_void_p(main.cuda_stream)), "cad_fold_partials_stream (cleanup)")
    return out


def gate_fix_buffers(lib, u, N):
    """Worklist (int64 slots) + zeroed counter (int32) for the exact gate gradient at lost gates (cad_scan_bwd_gate_fix): z == 0 and
    |z| < 2^-100; in fp16 every |z| <= 2^-15 (~1 % of the chunks of N(0, 1) gates)."""
    E, SB, Lq = u.shape
    lst = torch.empty((lib.cad_scan_gate_fix_entries(E, SB, Lq),), dtype=torch.int64, device=u.device)
    cnt = torch.zeros((1,), dtype=torch.int32, device=u.device)
    return lst, cnt


_SCAN_PTRS = {cls: frozenset(f for f, t in cls._fields_ if t is C.c_void_p) for cls in (L.ScanArgs, L.ScanBwdArgs)}


def _scan_struct(cls, E, SB, Lq, N, split, dirs, act, k, ints, tensors):
    if not tensors.keys() <= _SCAN_PTRS[cls]:  # (ctypes would take a misspelt field as a plain attribute)
        raise TypeError(f"{cls.__name__} has no pointer field {sorted(tensors.keys() - _SCAN_PTRS[cls])}")
    stream = L.stream_and_check(*tensors.values())
    return cls(SB=SB * k, L=Lq // k, split=split * k, E=E, N=N, rev_lo=dirs[0], rev_hi=dirs[1], dtype=L.dtype_code(act), **ints,
               **{f: L.ptr(t) for f, t in tensors.items()}), stream


def scan_fwd_args(E, SB, Lq, N, split, dirs, act, *, k=1, delta_is_dt=False, **tensors):
    """(cad_scan_args, launch stream) of one parameter set: rows (E, SB, Lq) of dtype `act`, dirs = (rev_lo, rev_hi), every row cut into
    k segments along L.  tensors: the struct's pointer fields by name (u=, delta=, ..., h0=, hT=, sum_dt=); None or absent stays NULL."""
    return _scan_struct(L.ScanArgs, E, SB, Lq, N, split, dirs, act, k, dict(delta_is_dt=int(bool(delta_is_dt))), tensors)


def scan_bwd_args(E, SB, Lq, N, split, dirs, act, n_partials, *, k=1, delta_is_dt=False, **tensors):
    """(cad_scan_bwd_args, launch stream), as scan_fwd_args; n_partials: the depth of the dB / dC slots (cad_scan_bwd_partials)."""
    return _scan_struct(L.ScanBwdArgs, E, SB, Lq, N, split, dirs, act, k,
                        dict(n_partials=n_partials, delta_is_dt=int(bool(delta_is_dt))), tensors)


def scan_inputs(z, tensors):
    """(contiguous z, [(u, delta, A, Bm, Cm, D, delta_bias)] as the kernels take them: contiguous, parameters in fp32)."""
    z = None if z is None else z.contiguous()
    sets = []
    for i in range(0, len(tensors), 7):
        u, delta, A, Bm, Cm, D, bias = tensors[i:i + 7]
        if delta.dtype != u.dtype or Bm.dtype != u.dtype or Cm.dtype != u.dtype or (z is not None and z.dtype != u.dtype):
            raise TypeError("selective_scan: u, delta, B, C, z must share one dtype")
        sets.append((u.contiguous(), delta.contiguous(), A.float().contiguous(), Bm.contiguous(), Cm.contiguous(),
                     D.float().contiguous(), bias.float().contiguous()))
    return z, sets


def scan_param_dtypes(tensors):
    return [(tensors[i + 2].dtype, tensors[i + 5].dtype, tensors[i + 6].dtype) for i in range(0, len(tensors), 7)]


def scan_bwd_sets(lib, sets, z, douts, split, dirs, *, k=1, delta_is_dt=False, npart=None, dhTs=None, dh0=False, gate_fix):
    """Argument structs of the scan backward with freshly allocated outputs.  sets[i]: (u, delta, A, Bm, Cm, D, delta_bias, chunk_state,
    out) as the forward saved them.  npart: the slot depth where the caller has asked for it already; gate_fix: the exact-gate worklist
    (used with a gate only), or None.  Returns (struct array, per set ({field: output}, dB / dC slots), stream)."""
    args, res = (L.ScanBwdArgs * len(sets))(), []
    for i, (u, delta, A, Bm, Cm, D, bias, state, fout) in enumerate(sets):
        (E, SB, Lq), N = u.shape, A.shape[1]
        np_i = lib.cad_scan_bwd_partials(E) if npart is None else npart  # one partial-sum slot per workgroup (written, not accumulated)
        dBC = torch.empty((2, np_i, N, SB, Lq), dtype=scan_slot_dtype(u.dtype), device=u.device)
        o = dict(du=torch.empty_like(u), ddelta=torch.empty_like(u), dz=None if z is None else torch.empty_like(u),
                 dA=torch.zeros_like(A), dB=dBC[0], dC=dBC[1], dD=torch.zeros_like(D), ddelta_bias=torch.zeros_like(bias))
        if dh0:
            o["dh0"] = torch.empty((E, SB, N), dtype=torch.float32, device=u.device)
        if gate_fix is not None and z is not None:
            o["gate_fix_list"], o["gate_fix_count"] = gate_fix(lib, u, N)
            o["gate_fix_dz"] = o["dz"]
        args[i], stream = scan_bwd_args(E, SB, Lq, N, split, dirs[i], u.dtype, np_i, k=k, delta_is_dt=delta_is_dt, u=u, delta=delta,
                                        A=A, Bm=Bm, Cm=Cm, D=D, z=z, delta_bias=bias, dout=douts[i], out=fout, chunk_state=state,
                                        dhT=dhTs[i] if dhTs else None, **o)
        res.append((o, dBC))
    return args, res, stream


def fold_dBC(dBC, act, stream):
    """(dB, dC) (N, SB, L) in `act` from the (2, npart, N, SB, L) partial slots of one set: one fold launch each."""
    npart, n = dBC.shape[1], dBC[0, 0].numel()
    dB, dC = (torch.empty(dBC.shape[2:], dtype=act, device=dBC.device) for _ in range(2))
    for src, dst in ((dBC[0], dB), (dBC[1], dC)):
        L.check(L.get_lib().cad_reduce_partials(L.ptr(src), npart, n, L.ptr(dst), L.dtype_code(act), stream), "cad_reduce_partials")
    return dB, dC


def scan_bwd_grads(res, pdt, stream, dz_in_place=True):
    """([du, ddelta, dA, dB, dC, dD, ddelta_bias] per set, parameter gradients in the parameters' dtypes pdt[i]; dz summed over the sets
    that share the gate, or None)."""
    grads, dz_tot = [], None
    for (o, dBC), (Adt, Ddt, bdt) in zip(res, pdt):
        dB, dC = fold_dBC(dBC, o["du"].dtype, stream)
        grads.append([o["du"], o["ddelta"], o["dA"].to(Adt), dB, dC, o["dD"].to(Ddt), o["ddelta_bias"].to(bdt)])
        if o["dz"] is not None:
            dz_tot = o["dz"] if dz_tot is None else (dz_tot.add_(o["dz"]) if dz_in_place else dz_tot + o["dz"])
    return grads, dz_tot


class _ScanMulti(torch.autograd.Function):
    """1 or 2 parameter sets (same shapes, shared gate z) in one launch.  Tensor args per set:
    u, delta, A, Bm, Cm, D, delta_bias."""

    @staticmethod
    def forward(ctx, z, split, dirs, delta_is_dt, *tensors):
        lib = L.get_lib()
        z, sets = scan_inputs(z, tensors)
        nsets = len(sets)
        args, saved = (L.ScanArgs * nsets)(), []
        for i, (u, delta, A, Bm, Cm, D, bias) in enumerate(sets):
            (E, SB, Lq), N = u.shape, A.shape[1]
            k = lsplit_factor(E, SB, Lq, nsets)  # same shapes in every set -> same k
            out = torch.empty_like(u)
            state = (torch.empty((lib.cad_scan_state_floats(E, SB * k, Lq // k, N),), dtype=torch.float32, device=u.device)
                     if any(ctx.needs_input_grad) else None)
            args[i], stream = scan_fwd_args(E, SB, Lq, N, split, dirs[i], u.dtype, k=k, delta_is_dt=delta_is_dt, u=u, delta=delta, A=A,
                                            Bm=Bm, Cm=Cm, D=D, z=z, delta_bias=bias, out=out, chunk_state=state)
            saved += [*sets[i], state, out]
        _keep, Ps = scan_fwd_launch(lib, args, nsets, stream, k, [s[2] for s in sets], dirs, split)
        ctx.save_for_backward(z, *saved, *Ps)
        ctx.meta = (split, dirs, nsets, scan_param_dtypes(tensors), delta_is_dt, k)
        return tuple(saved[8::9])

    @staticmethod
    def backward(ctx, *douts):
        z, *flat = ctx.saved_tensors
        split, dirs, nsets, pdt, delta_is_dt, k = ctx.meta
        lib = L.get_lib()
        douts = [d.contiguous() for d in douts]
        args, res, stream = scan_bwd_sets(lib, [flat[9 * i:9 * i + 9] for i in range(nsets)], z, douts, split, dirs, k=k,
                                          delta_is_dt=delta_is_dt, gate_fix=gate_fix_buffers)
        _keep = scan_bwd_launch(lib, args, nsets, stream, k, flat[9 * nsets:], dirs, split)
        if z is not None:  # exact gate gradient at lost gates (z == 0: rare, the launch is a no-op otherwise; fp16: |z| <= 2^-15)
            L.check(lib.cad_scan_bwd_gate_fix(args, nsets, stream), "cad_scan_bwd_gate_fix")
        grads, dz = scan_bwd_grads(res, pdt, stream)
        return (dz, None, None, None, *[g for set_grads in grads for g in set_grads])


def selective_scan_multi(sets, z, split: int, dirs, delta_is_dt: bool = False):
    """sets: list of (u, delta, A, Bm, Cm, D, delta_bias) with u, delta: (E, SB, L); A: (E, N) (= -exp(A_log));
    Bm, Cm: (N, SB, L); D, delta_bias: (E).  z: shared gate (E, SB, L) or None.  dirs: [(rev_lo, rev_hi)] per set.
    mamba_ssm `selective_scan_fn(..., delta_softplus=True)` for each set, each row in its own direction.
    delta_is_dt: `delta` already holds dt = softplus(delta_raw + delta_bias) (proj_wx(..., softplus_bias=)); its gradient is
    still the one w.r.t. delta_raw, and delta_bias still receives its gradient."""
    flat = [t for s_ in sets for t in s_]
    return _ScanMulti.apply(z, int(split), tuple((int(a), int(b)) for a, b in dirs), bool(delta_is_dt), *flat)


def selective_scan(u, delta, A, Bm, Cm, D, z, delta_bias, split: int, rev_lo: int, rev_hi: int) -> torch.Tensor:
    """Single parameter set (see selective_scan_multi)."""
    return selective_scan_multi([(u, delta, A, Bm, Cm, D, delta_bias)], z, split, [(rev_lo, rev_hi)])[0]


class _ScanStateful(torch.autograd.Function):
    """One parameter set over a row SEGMENT: (u, delta, A, Bm, Cm, D, z, delta_bias, h0) -> (out, hT).  h0 / hT are the
    (E, SB, N) fp32 states entering / leaving the segment along each row's direction; both are differentiable, so
    consecutive segments chain through plain autograd (chunk-pipelined scans over sequences that do not fit at once, and
    the building block of caduceus_amd/seqpar.py).  The one-set case of _ScanMulti's path, on the single-set entry points."""

    @staticmethod
    def forward(ctx, u, delta, A, Bm, Cm, D, z, bias, h0, split, rev_lo, rev_hi):
        lib = L.get_lib()
        z, (inputs,) = scan_inputs(z, (u, delta, A, Bm, Cm, D, bias))
        u, delta, Af, Bm, Cm, Df, bf = inputs
        (E, SB, Lq), N = u.shape, Af.shape[1]
        h0f = None if h0 is None else h0.float().contiguous()
        out = torch.empty_like(u)
        hT = torch.empty((E, SB, N), dtype=torch.float32, device=u.device)
        state = torch.empty((lib.cad_scan_state_floats(E, SB, Lq, N),), dtype=torch.float32, device=u.device)
        a, stream = scan_fwd_args(E, SB, Lq, N, split, (rev_lo, rev_hi), u.dtype, u=u, delta=delta, A=Af, Bm=Bm, Cm=Cm, D=Df, z=z,
                                  delta_bias=bf, out=out, chunk_state=state, h0=h0f, hT=hT)
        L.check(lib.cad_scan_fwd(C.byref(a), stream), "cad_scan_fwd")
        ctx.save_for_backward(z, *inputs, state, out)
        ctx.meta = (split, (rev_lo, rev_hi), scan_param_dtypes((u, delta, A, Bm, Cm, D, bias)), h0 is not None)
        return out, hT

    @staticmethod
    def backward(ctx, dout, dhT):
        lib = L.get_lib()
        z, *saved = ctx.saved_tensors
        split, dirs, pdt, has_h0 = ctx.meta
        dout = torch.zeros_like(saved[0]) if dout is None else dout.contiguous()
        dhT = None if dhT is None else dhT.float().contiguous()
        args, res, stream = scan_bwd_sets(lib, [saved], z, [dout], split, [dirs], dhTs=[dhT], dh0=True, gate_fix=gate_fix_buffers)
        L.check(lib.cad_scan_bwd(args, stream), "cad_scan_bwd")
        if z is not None:
            L.check(lib.cad_scan_bwd_gate_fix(args, 1, stream), "cad_scan_bwd_gate_fix")
        ((du, ddelta, dA, dB, dC, dD, dbias),), dz = scan_bwd_grads(res, pdt, stream)
        return (du, ddelta, dA, dB, dC, dD, dz, dbias, res[0][0]["dh0"] if has_h0 else None, None, None, None)


def selective_scan_stateful(u, delta, A, Bm, Cm, D, z, delta_bias, h0, split: int, rev_lo: int, rev_hi: int):
    """Segment scan with state carries: returns (out, hT).  See _ScanStateful."""
    return _ScanStateful.apply(u, delta, A, Bm, Cm, D, z, delta_bias, h0, int(split), int(rev_lo), int(rev_hi))


# ------------------------------------------------------------------------------------------------------------------
# LM head (+ masked cross entropy)
# ------------------------------------------------------------------------------------------------------------------
class _LmHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, weight, comp, labels, ignore_index, own_b16=False):
        hidden = hidden.contiguous()
        S, D = hidden.shape[0], hidden.shape[-1]
        rows = hidden.numel() // (S * D)
        w = weight.float().contiguous()
        V = w.shape[0]
        logits = torch.empty(hidden.shape[1:-1] + (V,), dtype=torch.float32, device=hidden.device)
        lab = None if labels is None else labels.reshape(-1).long().contiguous()
        acc = torch.zeros((2,), dtype=torch.float32, device=hidden.device)
        # deterministic loss: per-workgroup partial sums folded in a fixed order (no fp32 atomics)
        parts = (torch.empty((L.get_lib().cad_lm_head_partials(rows),), dtype=torch.float32, device=hidden.device)
                 if labels is not None else None)
        stream = L.stream_and_check(hidden, w, comp, lab, logits, acc, parts)
        a = L.LmHeadArgs(L.ptr(hidden), L.ptr(w), L.ptr(comp), L.ptr(lab), L.ptr(logits), C.c_void_p(acc.data_ptr()),
                         C.c_void_p(acc.data_ptr() + 4), rows, D, V, S, int(ignore_index), L.dtype_code(hidden.dtype),
                         L.ptr(parts))
        L.check(L.get_lib().cad_lm_head_fwd(C.byref(a), stream), "cad_lm_head_fwd")
        loss = acc[0] / acc[1] if labels is not None else acc[0]
        ctx.save_for_backward(hidden, w, comp, lab, logits, acc)
        ctx.meta = (ignore_index, weight.dtype, labels is not None, bool(own_b16))
        # an output nobody differentiated reaches backward as None instead of a zero-filled (rows, V) fp32 tensor the kernel would
        # allocate and read (training uses the loss alone)
        ctx.set_materialize_grads(False)
        return logits, loss

    @staticmethod
    def backward(ctx, dlogits, dloss):
        hidden, w, comp, lab, logits, acc = ctx.saved_tensors
        ignore_index, wdt, has_labels, own = ctx.meta
        S, D = hidden.shape[0], hidden.shape[-1]
        V = w.shape[0]
        lib = L.get_lib()
        use_loss = has_labels and dloss is not None
        # channel block of the kernel: the whole row (d_model 128 / 256) or 256 channels of a wider head (d_model 512: two launches,
        # the channels are independent in both products)
        DB = D if lib.cad_lm_head_bwd_supported(int(D), int(V)) else (256 if D % 256 == 0 and lib.cad_lm_head_bwd_supported(256, int(V)) else 0)
        if (use_loss or dlogits is not None) and hidden.dtype in (torch.float32, torch.bfloat16, torch.float16) and DB and \
                hidden.data_ptr() % 16 == 0:  # (kernel: 16-byte vector accesses)
            # on the matrix cores: softmax gradient, d hidden of both strands, dW partial slots (cad_lm_head_bwd)
            rows = hidden.numel() // (S * D)
            dh = torch.empty_like(hidden)
            parts = torch.empty((lib.cad_lm_head_bwd_partials(rows), V, D), dtype=torch.float32, device=hidden.device)
            coef = (dloss.float() / acc[1]).reshape(1) if use_loss else None
            dlg = None if dlogits is None else dlogits.reshape(-1, V).float().contiguous()
            stream = L.stream_and_check(hidden, w, comp, lab if use_loss else None, logits, dlg, coef, dh, parts)
            for c0 in range(0, D, DB):
                es = hidden.element_size()
                a = L.LmHeadBwdArgs(hidden.data_ptr() + c0 * es, w.data_ptr() + c0 * 4, L.ptr(comp), L.ptr(lab) if use_loss else None,
                                    L.ptr(logits), L.ptr(dlg), L.ptr(coef), dh.data_ptr() + c0 * es, parts.data_ptr() + c0 * 4, rows, DB, V, S,
                                    int(ignore_index), L.dtype_code(hidden.dtype), 0 if DB == D else D)
                L.check(lib.cad_lm_head_bwd(C.byref(a), stream), "cad_lm_head_bwd")
            return dh, parts.sum(dim=0).to(wdt), None, None, None, None
        # (other shapes: torch ops)
        # d loss / d logits = (softmax - onehot) * valid / count, assembled WITHOUT boolean-mask indexing: `sm[rows[valid], lab[valid]]`
        # goes through nonzero(), i.e. a device-to-host copy in the middle of the backward -- the launch queue ran dry behind it
        # (~0.4 ms of idle gaps per step in the kernel trace)
        g = None if dlogits is None else dlogits.reshape(-1, V).float()
        if has_labels and dloss is not None:
            valid = ((lab != ignore_index) & (lab >= 0) & (lab < V)).to(torch.float32).unsqueeze(1)  # as the forward counts
            sm = torch.softmax(logits.reshape(-1, V), dim=-1)
            sm.scatter_add_(1, lab.clamp(0, V - 1).unsqueeze(1), -valid)  # rows that do not count add -0 somewhere
            # rows that do not count get an exact 0, not 0 * coefficient: with every label ignored the coefficient is 1 / 0, and
            # F.cross_entropy (like cad_lm_head_bwd) then returns zero gradients beside its NaN loss
            sm.mul_(dloss / acc[1]).masked_fill_(valid == 0, 0.0)
            g = sm if g is None else g + sm
        if g is None:
            g = torch.zeros((logits.numel() // V, V), dtype=torch.float32, device=hidden.device)
        gt = g.to(hidden.dtype)
        h = hidden.reshape(S, -1, D)
        dh = torch.empty_like(h)
        wt = w.to(hidden.dtype)
        dh[0] = mm(gt, wt, own_b16=own)
        dw = mm(gt.t(), h[0], own_b16=own).float()
        if S == 2:
            dh[1] = mm(gt, wt[comp], own_b16=own)
            d2 = mm(gt.t(), h[1], own_b16=own).float()
            dw.index_add_(0, comp, d2)
        return dh.reshape(hidden.shape), dw.to(wdt), None, None, None, None


def lm_head(hidden: torch.Tensor, weight: torch.Tensor, comp: Optional[torch.Tensor],
            labels: Optional[torch.Tensor] = None, ignore_index: int = -100, own_b16: bool = False):
    """hidden: (S, B, L, D) t-frame -> (fp32 logits (B, L, V), loss or None).  RCPSLMHead + cross_entropy.
    own_b16: the backward's torch-op branch (shapes cad_lm_head_bwd does not take) multiplies bf16 on cad_gemm_b16, not the library."""
    logits, loss = _LmHead.apply(hidden, weight, comp, labels, ignore_index, own_b16)
    return logits, (loss if labels is not None else None)


class ScoreUnsupported(ValueError):
    """The head lies outside what cad_lm_head_score serves (a bias-free head with vocab_size <= 16 on fp32 / bf16 / fp16 hidden)."""


def lm_head_score_supported(D: int, V: int, act: torch.dtype) -> bool:
    if act not in (torch.float32, torch.bfloat16, torch.float16):
        return False
    return bool(L.get_lib().cad_lm_head_score_supported(int(D), int(V), L.dtype_code(act)))


def lm_head_score(hidden_t: torch.Tensor, weight: torch.Tensor, comp: Optional[torch.Tensor], targets: Optional[torch.Tensor] = None,
                  row_index: Optional[torch.Tensor] = None, logit_mask: Optional[torch.Tensor] = None, want_all: bool = False,
                  ignore_index: int = -100):
    """Log-probabilities from the final t-frame hidden state (S, ..., D) in one launch (cad_lm_head_score); no logits tensor exists.
    row_index: int64 rows of the flattened (rows, D) hidden to score (any shape, any order, repeats allowed); None scores every row.
    targets: int64, one per scored row -> logp = log softmax(z + logit_mask)[target], 0.0 where the target is ignore_index or outside
    [0, V), -inf where it is masked.  want_all -> logp_all (..., V).  logit_mask: (V) fp32 of 0 / -inf (generation._logit_mask).
    Returns logp, logp_all, or (logp, logp_all) when both are asked for, shaped like row_index (or like hidden's row dimensions).
    No autograd: tensors that require grad are refused while grad mode is on.  A head the kernel does not serve raises ScoreUnsupported."""
    if targets is None and not want_all:
        raise ValueError("lm_head_score: give targets, want_all=True, or both")
    if torch.is_grad_enabled() and (hidden_t.requires_grad or weight.requires_grad):
        raise RuntimeError("lm_head_score has no backward: call it under torch.no_grad() (or detach its inputs); the differentiable head "
                           "is ops.lm_head")
    S, D = hidden_t.shape[0], hidden_t.shape[-1]
    V = weight.shape[0]
    if weight.dim() != 2 or weight.shape[1] != D:
        raise ValueError(f"lm_head_score: weight must be (V, {D}), got {tuple(weight.shape)}")
    if not lm_head_score_supported(D, V, hidden_t.dtype):
        raise ScoreUnsupported(f"lm_head_score: cad_lm_head_score does not serve d_model {D}, vocab_size {V} in {hidden_t.dtype} "
                               "(vocab_size <= 16; float32, bfloat16 or float16 hidden); score such a head from model(ids).logits")
    if S not in (1, 2) or (S == 2 and comp is None):
        raise ValueError("lm_head_score: hidden is (1, ..., D), or (2, ..., D) with a complement map")
    hidden = hidden_t.detach().contiguous()
    rows = hidden.numel() // (S * D)
    w = weight.detach().float().contiguous()
    dev = hidden.device
    if row_index is not None:
        if row_index.dtype != torch.int64:
            raise TypeError("lm_head_score: row_index is int64")
        if row_index.device.type == "cpu" and row_index.numel() and (int(row_index.min()) < 0 or int(row_index.max()) >= rows):
            raise ValueError(f"lm_head_score: row_index must lie in [0, {rows})")
        shape = tuple(row_index.shape)
        ridx = row_index.reshape(-1).contiguous()
    else:
        shape, ridx = tuple(hidden.shape[1:-1]), None
    n = math.prod(shape)
    if n == 0 or rows == 0:
        raise ValueError("lm_head_score: nothing to score")
    tg = None
    if targets is not None:
        if targets.numel() != n:
            raise ValueError(f"lm_head_score: {n} rows are scored, targets holds {targets.numel()}")
        tg = targets.reshape(-1).long().contiguous()
    if logit_mask is not None:
        if logit_mask.dtype != torch.float32 or logit_mask.numel() != V:
            raise TypeError("lm_head_score: logit_mask holds V float32 values (0 or -inf)")
        logit_mask = logit_mask.contiguous()
        if logit_mask.device.type == "cpu" and not bool((logit_mask == 0).any()):
            raise ValueError("lm_head_score: logit_mask allows no id")
    logp = torch.empty(shape, dtype=torch.float32, device=dev) if tg is not None else None
    logp_all = torch.empty(shape + (V,), dtype=torch.float32, device=dev) if want_all else None
    stream = L.stream_and_check(hidden, w, comp if S == 2 else None, ridx, tg, logit_mask, logp, logp_all)
    a = L.LmScoreArgs(L.ptr(hidden), L.ptr(w), L.ptr(comp) if S == 2 else None, L.ptr(ridx), L.ptr(tg), L.ptr(logit_mask), L.ptr(logp),
                      L.ptr(logp_all), rows, n, D, V, S, int(ignore_index), L.dtype_code(hidden.dtype))
    L.check(L.get_lib().cad_lm_head_score(C.byref(a), stream), "cad_lm_head_score")
    if logp is None:
        return logp_all
    return (logp, logp_all) if want_all else logp


class AttribUnsupported(ValueError):
    """The embedding lies outside what cad_embed_attrib serves (vocab_size <= 16 on an fp32 / bf16 / fp16 gradient)."""


def embed_attrib_supported(D: int, V: int, act: torch.dtype) -> bool:
    if act not in (torch.float32, torch.bfloat16, torch.float16):
        return False
    return bool(L.get_lib().cad_embed_attrib_supported(int(D), int(V), L.dtype_code(act)))


def embed_attrib(dh_t: torch.Tensor, weight: torch.Tensor, comp: Optional[torch.Tensor], ids: torch.Tensor, allowed: torch.Tensor,
                 centre: bool = True, want_grad: bool = True, want_gxi: bool = True):
    """Nucleotide attributions from the gradient dh_t (S, ..., D) of a score w.r.t. the t-frame embedding output, in one launch
    (cad_embed_attrib): g[v] = <dh0, E[v]> + <dh1, E[comp v]> is the gradient w.r.t. the one-hot input, the LM head's logit row with the
    embedding table `weight` (V, D) as the weight.  allowed: int64, ascending and unique, A ids in [0, V).  centre: the mean of g over
    the allowed ids is subtracted.  want_grad -> grad (..., A) fp32, columns in the order of `allowed`; want_gxi -> gxi (...) fp32, the
    (centred) value at the row's own id `ids`, exactly 0.0 where that id is not allowed.  Returns grad, gxi, or (grad, gxi).
    No autograd: the inputs are detached.  An embedding the kernel does not serve raises AttribUnsupported."""
    if not (want_grad or want_gxi):
        raise ValueError("embed_attrib: ask for grad, gxi, or both")
    S, D = dh_t.shape[0], dh_t.shape[-1]
    V = weight.shape[0]
    if weight.dim() != 2 or weight.shape[1] != D:
        raise ValueError(f"embed_attrib: weight must be (V, {D}), got {tuple(weight.shape)}")
    if not embed_attrib_supported(D, V, dh_t.dtype):
        raise AttribUnsupported(f"embed_attrib: cad_embed_attrib does not serve d_model {D}, vocab_size {V} in {dh_t.dtype} "
                                "(vocab_size <= 16; float32, bfloat16 or float16 gradient)")
    if S not in (1, 2) or (S == 2 and comp is None):
        raise ValueError("embed_attrib: dh is (1, ..., D), or (2, ..., D) with a complement map")
    dh = dh_t.detach().contiguous()
    shape = tuple(dh.shape[1:-1])
    rows = math.prod(shape)
    if rows == 0:
        raise ValueError("embed_attrib: nothing to attribute")
    if ids.dtype != torch.int64 or ids.numel() != rows:
        raise TypeError(f"embed_attrib: ids holds {rows} int64 values, one per row")
    if allowed.dtype != torch.int64 or allowed.dim() != 1 or not 1 <= allowed.numel() <= V:
        raise TypeError(f"embed_attrib: allowed holds 1 .. {V} int64 ids")
    if allowed.device.type == "cpu":  # what the host holds is checked on the host
        al = allowed.tolist()
        if al != sorted(set(al)) or al[0] < 0 or al[-1] >= V:
            raise ValueError(f"embed_attrib: allowed must be ascending, unique and lie in [0, {V})")
    A = allowed.numel()
    w = weight.detach().float().contiguous()
    ids = ids.reshape(-1).contiguous()
    allowed = allowed.contiguous()
    dev = dh.device
    grad = torch.empty(shape + (A,), dtype=torch.float32, device=dev) if want_grad else None
    gxi = torch.empty(shape, dtype=torch.float32, device=dev) if want_gxi else None
    cmap = comp if S == 2 else None
    stream = L.stream_and_check(dh, w, cmap, ids, allowed, grad, gxi)
    a = L.EmbedAttribArgs(L.ptr(dh), L.ptr(w), L.ptr(cmap), L.ptr(ids), L.ptr(allowed), L.ptr(grad), L.ptr(gxi), rows, D, V, S, A,
                          int(bool(centre)), L.dtype_code(dh.dtype))
    L.check(L.get_lib().cad_embed_attrib(C.byref(a), stream), "cad_embed_attrib")
    if grad is None:
        return gxi
    return (grad, gxi) if want_gxi else grad


def lm_head_unmask_supported(D: int, V: int, act: torch.dtype) -> bool:
    if act not in (torch.float32, torch.bfloat16, torch.float16):
        return False
    return bool(L.get_lib().cad_lm_head_unmask_supported(int(D), int(V), L.dtype_code(act)))


def lm_head_unmask(hidden_t: torch.Tensor, weight: torch.Tensor, comp: Optional[torch.Tensor], ids: torch.Tensor, *, mask_token_id: int,
                   top_k: int = 1, top_p: float = 0.0, temperature: float = 1.0, seed: int = 0, row_offset: int = 0, position: int = 0,
                   logit_mask: Optional[torch.Tensor] = None, return_u: bool = False):
    """One round of iterative unmasking from the final t-frame hidden state (S, B, L, D) in one launch (cad_lm_head_unmask); neither
    logits nor log-probabilities per id exist.  ids (B, L) int64: where it equals mask_token_id the position is open and gets the id the
    sampler draws from its logit row (sample_tokens' rules; the uniform keyed by (seed, row_offset + b, position + l)) and, as conf, the
    model's own log-probability of that id over the ids logit_mask allows (lm_head_score's number: temperature, top_k and top_p not
    applied); every other position keeps its id and gets conf 0.0.  Returns (ids_out (B, L) int64, conf (B, L) fp32[, u (B, L) fp32]);
    ids is left as it is.  No autograd, as lm_head_score.  A head the kernel does not serve raises ScoreUnsupported."""
    check_sampling(top_k, top_p, temperature)
    if torch.is_grad_enabled() and (hidden_t.requires_grad or weight.requires_grad):
        raise RuntimeError("lm_head_unmask has no backward: call it under torch.no_grad() (or detach its inputs)")
    if hidden_t.dim() != 4:
        raise ValueError(f"lm_head_unmask: hidden is (S, B, L, D), got {tuple(hidden_t.shape)}")
    S, B, Lq, D = hidden_t.shape
    V = weight.shape[0]
    if weight.dim() != 2 or weight.shape[1] != D:
        raise ValueError(f"lm_head_unmask: weight must be (V, {D}), got {tuple(weight.shape)}")
    if not lm_head_unmask_supported(D, V, hidden_t.dtype):
        raise ScoreUnsupported(f"lm_head_unmask: cad_lm_head_unmask does not serve d_model {D}, vocab_size {V} in {hidden_t.dtype} "
                               "(vocab_size <= 16; float32, bfloat16 or float16 hidden)")
    if S not in (1, 2) or (S == 2 and comp is None):
        raise ValueError("lm_head_unmask: hidden is (1, B, L, D), or (2, B, L, D) with a complement map")
    if ids.dtype != torch.int64 or tuple(ids.shape) != (B, Lq):
        raise TypeError(f"lm_head_unmask: ids is ({B}, {Lq}) int64")
    if B * Lq == 0:
        raise ValueError("lm_head_unmask: nothing to unmask")
    if logit_mask is not None:
        if logit_mask.dtype != torch.float32 or logit_mask.numel() != V:
            raise TypeError("lm_head_unmask: logit_mask holds V float32 values (0 or -inf)")
        logit_mask = logit_mask.contiguous()
        if logit_mask.device.type == "cpu" and not bool((logit_mask == 0).any()):
            raise ValueError("lm_head_unmask: logit_mask allows no id")
    hidden = hidden_t.detach().contiguous()
    w = weight.detach().float().contiguous()
    ids = ids.contiguous()
    dev = hidden.device
    ids_out = torch.empty((B, Lq), dtype=torch.int64, device=dev)
    conf = torch.empty((B, Lq), dtype=torch.float32, device=dev)
    u = torch.empty((B, Lq), dtype=torch.float32, device=dev) if return_u else None
    cmap = comp if S == 2 else None
    stream = L.stream_and_check(hidden, w, cmap, ids, logit_mask, ids_out, conf, u)
    a = L.LmUnmaskArgs(L.ptr(hidden), L.ptr(w), L.ptr(cmap), L.ptr(ids), L.ptr(ids_out), L.ptr(conf), L.ptr(u),
                       sampler_args(top_k, top_p, temperature, seed, row_offset, position, logit_mask), B * Lq, Lq, D, V, S,
                       int(mask_token_id), L.dtype_code(hidden.dtype))
    L.check(L.get_lib().cad_lm_head_unmask(C.byref(a), stream), "cad_lm_head_unmask")
    return (ids_out, conf, u) if return_u else (ids_out, conf)


class PoolUnsupported(ValueError):
    """The pooling lies outside what cad_pool_head serves (d_model <= 1024; float32, bfloat16 or float16 activations; half < 2^22)."""


POOL_MODES = {"mean": L.POOL_MEAN, "max": L.POOL_MAX, "window": L.POOL_WINDOW}
_POOL_PAIRS = ((torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16),
               (torch.float32, torch.float16), (torch.float16, torch.float16))


def pool_head_supported(D: int, x_dtype: torch.dtype, y_dtype: torch.dtype, mode: str = "mean", half: int = 0) -> bool:
    if (x_dtype, y_dtype) not in _POOL_PAIRS or mode not in POOL_MODES:
        return False
    return bool(L.get_lib().cad_pool_head_supported(int(D), L.dtype_code(x_dtype), L.dtype_code(y_dtype), POOL_MODES[mode], int(half)))


def _pool_head_checked(who, x, residual, weight, bias, y_dtype, mode, centre, half):
    """The argument checks pool_head and pool_head_grad share -> (S, B, L, D, half)."""
    if x.dim() != 4:
        raise ValueError(f"{who}: x is (S, B, L, D), got {tuple(x.shape)}")
    S, B, Lq, D = x.shape
    if S not in (1, 2) or B * Lq * D == 0:
        raise ValueError(f"{who}: x is (1 | 2, B, L, D) with at least one row, got {tuple(x.shape)}")
    if weight is None and bias is not None:
        raise ValueError(f"{who}: a bias without a weight")
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None and tuple(t.shape) != (D,):
            raise ValueError(f"{who}: {name} must be ({D},), got {tuple(t.shape)}")
    if residual is not None:
        if residual.dtype != torch.float32:
            raise TypeError("caduceus_amd keeps the residual stream in fp32")
        if residual.shape != x.shape:
            raise ValueError(f"{who}: residual must be {tuple(x.shape)}, got {tuple(residual.shape)}")
    half = int(half)
    if mode == "window":
        if centre is None or centre.dtype != torch.int64 or tuple(centre.shape) != (S, B):
            raise TypeError(f"{who}: window pooling takes centre ({S}, {B}) int64")
        if half < 0:
            raise ValueError(f"{who}: half >= 0")
    elif centre is not None or half != 0:
        raise ValueError(f"{who}: centre and half belong to mode 'window', not {mode!r}")
    if not pool_head_supported(D, x.dtype, y_dtype, mode, half):
        raise PoolUnsupported(f"{who}: cad_pool_head does not serve d_model {D}, x {x.dtype} -> y {y_dtype}, mode {mode!r}, half {half} "
                              "(d_model <= 1024; the type pairs of add_norm; half < 2^22)")
    return S, B, Lq, D, half


def _pool_head_fwd(x, res, w, b, cen, eps, is_rms, y_dtype, code, half):
    """cad_pool_head on detached, contiguous operands (w / b fp32) -> out (S, B, D) fp32."""
    S, B, Lq, D = x.shape
    lib = L.get_lib()
    out = torch.empty((S, B, D), dtype=torch.float32, device=x.device)
    scratch = torch.empty((lib.cad_pool_head_scratch_floats(S, B, Lq, D, code, half),), dtype=torch.float32, device=x.device)
    stream = L.stream_and_check(x, res, w, b, cen, out, scratch)
    a = L.PoolHeadArgs(L.ptr(x), L.ptr(res), L.ptr(w), L.ptr(b), L.ptr(cen), L.ptr(out), L.ptr(scratch), B, Lq, half, S, D, float(eps),
                       int(is_rms), L.dtype_code(x.dtype), L.dtype_code(y_dtype), code)
    L.check(lib.cad_pool_head(C.byref(a), stream), "cad_pool_head")
    return out


def pool_head(x: torch.Tensor, residual: Optional[torch.Tensor], weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
              eps: float, is_rms: bool, y_dtype: torch.dtype, mode: str, centre: Optional[torch.Tensor] = None,
              half: int = 0) -> torch.Tensor:
    """Final add + norm and pooling over the sequence in one pass (cad_pool_head): x (S, B, L, D) is the last layer's t-frame output,
    residual its fp32 residual stream or None; the normed rows are add_norm's (swap_flip off, rounded to y_dtype) and are never written.
    mode "mean" / "max" pool all L rows; "window" averages rows clamp(centre[s, b] + k, 0, L - 1), k = -half .. half (the edge row
    repeats; any int64 centre; half = 0 gathers one row).  weight None: no norm, the rows of x (+ residual) are pooled as they are.
    Returns (S, B, D) fp32.  No autograd: tensors that require grad are refused while grad mode is on (pool_head_grad is the
    differentiable form).  Arguments the kernel does not serve raise PoolUnsupported."""
    if mode not in POOL_MODES:
        raise ValueError(f"pool_head: mode is one of {sorted(POOL_MODES)}, got {mode!r}")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, residual, weight, bias)):
        raise RuntimeError("pool_head has no backward: call it under torch.no_grad() (or detach its inputs); the differentiable route is "
                           "ops.add_norm followed by the pooling in torch")
    S, B, Lq, D, half = _pool_head_checked("pool_head", x, residual, weight, bias, y_dtype, mode, centre, half)
    x = x.detach().contiguous()
    res = None if residual is None else residual.detach().contiguous()
    w = None if weight is None else weight.detach().float().contiguous()
    b = None if bias is None else bias.detach().float().contiguous()
    cen = centre.contiguous() if mode == "window" else None
    return _pool_head_fwd(x, res, w, b, cen, eps, is_rms, y_dtype, POOL_MODES[mode], half)


class _PoolHead(torch.autograd.Function):
    """cad_pool_head with cad_pool_head_bwd behind it.  Saved: the inputs, and `out` for MAX (the rows its gradient goes to are found
    from it in the backward); no statistic, y or dy of size L exists in either direction."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, centre, eps, is_rms, y_dtype, code, half):
        xc = x.detach().contiguous()
        res = None if residual is None else residual.detach().contiguous()
        w = None if weight is None else weight.detach().float().contiguous()
        b = None if bias is None else bias.detach().float().contiguous()
        out = _pool_head_fwd(xc, res, w, b, centre, eps, is_rms, y_dtype, code, half)
        ctx.save_for_backward(xc, res, weight, bias, centre, out if code == L.POOL_MAX else None)
        ctx.cfg = (float(eps), int(is_rms), y_dtype, code, half)
        return out

    @staticmethod
    def backward(ctx, g):
        x, res, weight, bias, cen, out = ctx.saved_tensors
        eps, is_rms, y_dtype, code, half = ctx.cfg
        S, B, Lq, D = x.shape
        lib = L.get_lib()
        dev = x.device
        w = None if weight is None else weight.detach().float().contiguous()
        b = None if bias is None else bias.detach().float().contiguous()
        g = g.detach().float().contiguous()
        need_w = weight is not None and ctx.needs_input_grad[2]
        need_b = bias is not None and ctx.needs_input_grad[3]
        dx = torch.empty_like(x)
        dres = None if res is None else torch.empty_like(res)
        dw = torch.empty((D,), dtype=torch.float32, device=dev) if need_w else None
        db = torch.empty((D,), dtype=torch.float32, device=dev) if need_b else None
        is_max = code == L.POOL_MAX
        rows = torch.empty((S, B, D), dtype=torch.int64, device=dev) if is_max else None
        scratch = None
        if is_max or need_w or need_b:
            scratch = torch.empty((lib.cad_pool_head_bwd_scratch_floats(S, B, Lq, D, code, half),), dtype=torch.float32, device=dev)
        stream = L.stream_and_check(x, res, w, b, cen, g, out, dx, dres, dw, db, rows, scratch)
        a = L.PoolHeadBwdArgs(L.ptr(x), L.ptr(res), L.ptr(w), L.ptr(b), L.ptr(cen), L.ptr(g), L.ptr(out), L.ptr(dx), L.ptr(dres), L.ptr(dw),
                              L.ptr(db), L.ptr(rows), L.ptr(scratch), B, Lq, half, S, D, eps, is_rms, L.dtype_code(x.dtype),
                              L.dtype_code(y_dtype), code)
        L.check(lib.cad_pool_head_bwd(C.byref(a), stream), "cad_pool_head_bwd")
        return (dx if ctx.needs_input_grad[0] else None, dres if ctx.needs_input_grad[1] else None,
                dw.to(weight.dtype) if need_w else None, db.to(bias.dtype) if need_b else None, None, None, None, None, None, None)


def pool_head_grad(x: torch.Tensor, residual: Optional[torch.Tensor], weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                   eps: float, is_rms: bool, y_dtype: torch.dtype, mode: str, centre: Optional[torch.Tensor] = None,
                   half: int = 0) -> torch.Tensor:
    """pool_head with a backward (cad_pool_head_bwd): the same arguments and checks, the same cad_pool_head call -- so the same bits --
    and gradients for x, residual, weight and bias.  Only the inputs are saved (and `out` for "max"): the backward recomputes each row's
    add and statistics and writes dx (x's dtype) and d(residual) (fp32) in one pass; the rounding of the normed rows to y_dtype is
    straight-through, as in add_norm; "max" sends a channel's gradient to the lowest row that attains the maximum, as torch.max does.
    d(weight) / d(bias) come back in the parameters' dtype, run-to-run identical."""
    if mode not in POOL_MODES:
        raise ValueError(f"pool_head_grad: mode is one of {sorted(POOL_MODES)}, got {mode!r}")
    S, B, Lq, D, half = _pool_head_checked("pool_head_grad", x, residual, weight, bias, y_dtype, mode, centre, half)
    cen = centre.contiguous() if mode == "window" else None
    return _PoolHead.apply(x, residual, weight, bias, cen, eps, is_rms, y_dtype, POOL_MODES[mode], half)


# ------------------------------------------------------------------------------------------------------------------
# dense projections on the matrix cores (raw ops, no autograd: caduceus_amd/mixer.py schedules their gradients by hand)
# ------------------------------------------------------------------------------------------------------------------
def mm_f32(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (M, N) fp32 = [addend +] a (M, K) @ b (K, N) on the fp32 matrix core (cad_gemm_f32) -- torch.mm / torch.addmm for the fp32 path
    without a library GEMM.  a / b: 2-D fp32 views with ONE unit stride each (plain or transposed, any row pitch: the channel-major and
    token-major views of the mixer are taken as they are); out: any 2-D fp32 view (default: a new contiguous tensor); addend: out's
    strides (or out itself).  A product with a small result and a long reduction (a weight gradient over all tokens: 1024 x 256 from
    K = 262144) is cut into K slices -- one launch, fp32 partial tiles, one fp32 sum -- for the same two reasons as on the bf16 path:
    16 output tiles cannot fill 256 CUs, and 64 partial sums of 4096 terms round better than one chain of 262144.  The batched form is
    bmm_f32."""
    if a.dim() != 2 or b.dim() != 2:
        raise ValueError("mm_f32: 2-D operands")
    M, K = a.shape
    N = b.shape[1]
    n = _f32_kslices(M, N, K) if b.shape[0] == K else 1  # (a shape mismatch is reported by _gemm_f32)
    if n > 1:
        return _mm_kslices("gemm_f32", torch.float32, torch.float32, a, b, n, out, addend)
    return _gemm_f32(a.unsqueeze(0), b.unsqueeze(0), None if out is None else out.unsqueeze(0),
                     None if addend is None else addend.unsqueeze(0))[0]


def _mm_kslices(name, in_dtype, out_dtype, a, b, n, out, addend):
    """The K-slice branch of mm_f32 / mm_b16: the n slices in ONE batched launch with fp32 partial tiles, summed in fp32 in slice order
    (fold_f32; torch.sum where M * N is no multiple of 4), the addend added in fp32, ONE rounding to out_dtype (the type of `out`)."""
    M, K = a.shape
    N = b.shape[1]
    Kc = K // n
    part = _gemm_strided(name, in_dtype, torch.float32, a.unflatten(1, (n, Kc)).permute(1, 0, 2), b.unflatten(0, (n, Kc)),
                         None, None)  # (n, M, N) fp32
    res = torch.empty((M, N), dtype=torch.float32, device=a.device)
    if (M * N) % 4 == 0:
        fold_f32([(part, res, M * N, n, M * N, 1, 0)])
    else:
        torch.sum(part, dim=0, out=res)
    if addend is not None:
        res = res + addend.float()
    if out is None:
        return res.to(out_dtype)
    out.copy_(res)
    return out


def _f32_kslices(M: int, N: int, K: int) -> int:
    """K slices of an fp32 product (1: none), chosen with the launcher's two tile configurations in mind (csrc/gemm_f32.hip): a result of
    at least eight 128 x 128 tiles is cut until two such tiles per CU exist (slices of >= 1024 terms) and runs on the large
    configuration; a smaller one is cut until its 64 x 64 tiles fill the chip (slices of >= 256 terms)."""
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    if M > 64 and N > 64 and t128 >= 8:
        tiles, want, least = t128, 2 * _cu_count(), 1024
    else:
        tiles, want, least = ((M + 63) // 64) * ((N + 63) // 64), _cu_count(), 256
    n = 1
    while tiles * n < want and n < 64 and K % (2 * n) == 0 and K // (2 * n) >= least:
        n *= 2
    return n


def bmm_f32(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (n, M, N) fp32 = a (n, M, K) @ b (n, K, N), one launch (cad_gemm_f32, blockIdx.z = batch); a / b: 3-D fp32 views, one unit
    stride among the two inner dimensions of each."""
    return _gemm_f32(a, b, out, None)


def _gemm_f32(a, b, out, addend):
    return _gemm_strided("gemm_f32", torch.float32, torch.float32, a, b, out, addend)


def _gemm_strided(name, in_dtype, out_dtype, a, b, out, addend):
    """The launch of cad_gemm_f32 (fp32 operands) and cad_gemm_b16 (bf16 operands; bf16 result, or out_dtype fp32: its out_f32 form): one
    argument struct, one stride normalisation."""
    if a.dtype != in_dtype or b.dtype != in_dtype or a.dim() != 3 or b.dim() != 3:
        raise ValueError(f"{name}: {in_dtype} operands, (n, M, K) @ (n, K, N)")
    n, M, K = a.shape
    N = b.shape[2]
    if b.shape[0] != n or b.shape[1] != K:
        raise ValueError(f"{name}: shapes {tuple(a.shape)} @ {tuple(b.shape)}")

    def strides(t):
        """(row, column) element strides the kernel needs: one of them 1.  The stride of a size-1 dimension is never used: report it as
        the unit one when the other is not; a matrix with two non-unit strides is copied."""
        rs, cs = t.stride(1), t.stride(2)
        if t.shape[1] == 1 and cs != 1:
            rs = 1
        elif t.shape[2] == 1 and rs != 1:
            cs = 1
        if rs != 1 and cs != 1:
            t = t.contiguous()
            rs, cs = t.stride(1), t.stride(2)
            if cs != 1:  # (n, M, 1) contiguous: strides (M, 1, 1) -- cannot happen; kept as a guard
                raise ValueError(f"{name}: operand without a unit stride")
        return t, rs, cs

    a, a_rs, a_cs = strides(a)
    b, b_rs, b_cs = strides(b)
    if out is None:
        out = torch.empty((n, M, N), dtype=out_dtype, device=a.device)
    if out.dtype != out_dtype or tuple(out.shape) != (n, M, N):
        raise ValueError(f"{name}: out must be {out_dtype} (n, M, N)")
    if addend is not None and (addend.dtype != out_dtype or addend.shape != out.shape or addend.stride() != out.stride()):
        raise ValueError(f"{name}: addend must have out's dtype, shape and strides")
    if M == 0 or N == 0:
        return out
    if K == 0:
        if addend is None:
            out.zero_()
        elif addend.data_ptr() != out.data_ptr():
            out.copy_(addend)
        return out
    stream = L.stream_and_check(a, b, out, addend, contiguous=False)
    bs = lambda t: t.stride(0) if n > 1 else 0
    args = L.GemmF32Args(L.ptr(a), L.ptr(b), L.ptr(out), None if addend is None else L.ptr(addend), M, N, K,
                         a_rs, a_cs, b_rs, b_cs, max(out.stride(1), 1), max(out.stride(2), 1), n, bs(a), bs(b), bs(out))
    if in_dtype == torch.float32:
        L.check(L.get_lib().cad_gemm_f32(C.byref(args), stream), "cad_gemm_f32")
    else:
        L.check(L.get_lib().cad_gemm_b16(C.byref(args), int(out_dtype == torch.float32), stream), "cad_gemm_b16")
    return out


class _MmF32(torch.autograd.Function):
    """a @ b (+ addend) in fp32 on cad_gemm_f32, differentiable: da = g @ b^T, db = a^T @ g through the same kernel (transposed views)."""

    @staticmethod
    def forward(ctx, a, b, addend):
        ctx.save_for_backward(a, b)
        return mm_f32(a, b, addend=addend)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = mm_f32(g, b.t()) if ctx.needs_input_grad[0] else None
        db = mm_f32(a.t(), g) if ctx.needs_input_grad[1] else None
        return da, db, (g if ctx.needs_input_grad[2] else None)


def _own_f32(*ts) -> bool:
    return all(t.dtype == torch.float32 for t in ts)


def _f16(*ts) -> bool:
    return all(t.dtype == torch.float16 for t in ts)


class _MmF16(torch.autograd.Function):
    """a @ b (+ addend) of fp16 operands on cad_gemm_f32: exact widening, fp32 accumulation, ONE rounding of the fp16 result --
    the fp16 products that no fp16 MFMA kernel serves (small / ragged shapes, the generic engine).  Gradients the same way."""

    @staticmethod
    def forward(ctx, a, b, addend):
        ctx.save_for_backward(a, b)
        return mm_f32(a.float(), b.float(), addend=None if addend is None else addend.float()).to(torch.float16)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g32 = g.float()
        da = mm_f32(g32, b.float().t()).to(a.dtype) if ctx.needs_input_grad[0] else None
        db = mm_f32(a.float().t(), g32).to(b.dtype) if ctx.needs_input_grad[1] else None
        return da, db, (g if ctx.needs_input_grad[2] else None)


def mm_b16(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (M, N) bf16 = [addend +] a (M, K) @ b (K, N) of bf16 operands on cad_gemm_b16 (csrc/gemm_b16.hip): fp32 accumulation, the sum
    (plus the widened addend) rounded ONCE to bf16.  Views as for mm_f32: one unit stride per operand, any pitch, any 2-D bf16 view as
    out.  A product with a small result and a long reduction (an engine weight gradient with K = S * B * L tokens) is cut into K slices
    by mm_f32's rule: ONE batched launch with fp32 partial tiles (the kernel's out_f32 form), summed by fold_f32, rounded once."""
    if a.dim() != 2 or b.dim() != 2:
        raise ValueError("mm_b16: 2-D operands")
    M, K = a.shape
    N = b.shape[1]
    n = _f32_kslices(M, N, K) if b.shape[0] == K else 1  # (a shape mismatch is reported by _gemm_strided)
    if n > 1:
        return _mm_kslices("gemm_b16", torch.bfloat16, torch.bfloat16, a, b, n, out, addend)
    return _gemm_strided("gemm_b16", torch.bfloat16, torch.bfloat16, a.unsqueeze(0), b.unsqueeze(0), None if out is None else out.unsqueeze(0),
                         None if addend is None else addend.unsqueeze(0))[0]


def bmm_b16(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, out_f32: bool = False) -> torch.Tensor:
    """out (n, M, N) = a (n, M, K) @ b (n, K, N) of bf16 operands, one launch (cad_gemm_b16, blockIdx.z = batch); out_f32: the fp32 sums
    instead of their bf16 rounding."""
    return _gemm_strided("gemm_b16", torch.bfloat16, torch.float32 if out_f32 else torch.bfloat16, a, b, out, None)


class _MmB16(torch.autograd.Function):
    """a @ b (+ addend) of bf16 operands on cad_gemm_b16, differentiable: da = g @ b^T, db = a^T @ g through the same kernel (transposed
    views; a weight gradient over all tokens takes mm_b16's K slices)."""

    @staticmethod
    def forward(ctx, a, b, addend):
        ctx.save_for_backward(a, b)
        return mm_b16(a, b, addend=None if addend is None else addend.contiguous())

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = mm_b16(g, b.t()) if ctx.needs_input_grad[0] else None
        db = mm_b16(a.t(), g) if ctx.needs_input_grad[1] else None
        return da, db, (g if ctx.needs_input_grad[2] else None)


def _b16(*ts) -> bool:
    return all(t.dtype == torch.bfloat16 for t in ts)


def mm(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, own_b16: bool = False) -> torch.Tensor:
    """torch.mm for the call sites that have no dedicated kernel: fp32 operands take the own fp32 matrix-core kernel (cad_gemm_f32;
    differentiable), fp16 operands the same kernel on their exact fp32 widening (fp16 result), bf16 shapes the MFMA projection kernels
    do not serve the library -- or, for a call site that asks for it (own_b16: the generic engine, the LM-head fallbacks), the own bf16
    kernel (cad_gemm_b16; differentiable)."""
    if _own_f32(a, b):
        if out is not None:
            return mm_f32(a, b, out=out)
        return _MmF32.apply(a, b, None)
    if _f16(a, b):
        if out is not None:
            return out.copy_(mm_f32(a.float(), b.float()))
        return _MmF16.apply(a, b, None)
    if own_b16 and _b16(a, b):
        if out is not None:
            return mm_b16(a, b, out=out)
        return _MmB16.apply(a, b, None)
    return torch.mm(a, b) if out is None else torch.mm(a, b, out=out)


def addmm(acc: torch.Tensor, a: torch.Tensor, b: torch.Tensor, own_b16: bool = False) -> torch.Tensor:
    """acc + a @ b (torch.addmm), fp32 / fp16 on the own kernel; bf16 on the library, or (own_b16, as for mm) on cad_gemm_b16 with the
    addend inside the one rounding."""
    if _own_f32(acc, a, b):
        return _MmF32.apply(a, b, acc)
    if _f16(acc, a, b):
        return _MmF16.apply(a, b, acc)
    if own_b16 and _b16(acc, a, b):
        return _MmB16.apply(a, b, acc)
    return torch.addmm(acc, a, b)


def bmm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """torch.bmm (no autograd use in this package), fp32 on the own kernel; fp16 operands: the same kernel on their fp32 widening,
    fp32 result (the callers sum the batch in fp32)."""
    if _own_f32(a, b):
        return bmm_f32(a, b)
    if _f16(a, b):
        return bmm_f32(a.float(), b.float())
    return torch.bmm(a, b)


# ------------------------------------------------------------------------------------------------------------------
# the 16-bit (bf16 / fp16) MFMA projections: csrc/gemm.hip, gemm_f16.hip and their headers proj_wstat.h, proj_ring.h
# ------------------------------------------------------------------------------------------------------------------
# 16-bit element types of the MFMA projection kernels: each cad_proj_* / cad_gemm_stream entry point has an fp16 sibling
_MFMA_DTYPES = (torch.bfloat16, torch.float16)


def _proj_fn(name: str, dtype: torch.dtype):
    """The bf16 entry point `name` or its fp16 sibling `name`_f16 (same argument struct)."""
    return getattr(L.get_lib(), name + "_f16" if dtype == torch.float16 else name)


def scan_slot_dtype(act: torch.dtype) -> torch.dtype:
    """Element type of the scan backward's dB / dC partial slots: the activation dtype, except bf16 slots for fp16 activations (sums of
    loss-scaled gradients keep fp32's range; include/caduceus_hip.h, cad_scan_bwd)."""
    return torch.bfloat16 if act == torch.float16 else act


def proj_supported(t: torch.Tensor, K: int) -> bool:
    """The MFMA projection kernels take bf16 / fp16 operands with a supported reduction length.  (K = 512, d_model 512: stand-alone and cold the
    library GEMM is 18-25 % faster than the W-stationary kernel, inside the training step it is not -- 558.9 vs 555.9 ms per step;
    profiles/r04_proj_d512.txt.  The own kernel stays.)"""
    return t.dtype in _MFMA_DTYPES and bool(L.get_lib().cad_proj_supported(int(K)))


def proj_wxT(W: torch.Tensor, X: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (M, T) channel-major = W (M, K) @ X (T, K)^T, bf16 (fp16) in / fp32 accumulate / bf16 (fp16) out (cad_proj_wxT[_f16])."""
    M, K = W.shape
    T = X.shape[0]
    if X.shape[1] != K or W.stride(1) != 1 or X.stride(1) != 1:
        raise ValueError("proj_wxT: W (M, K) and X (T, K) with unit inner stride")
    _same_mfma_dtype(W, X, out)
    if out is None:
        out = torch.empty((M, T), dtype=X.dtype, device=X.device)
    stream = L.stream_and_check(W, X, out, contiguous=False)
    a = L.ProjArgs(L.ptr(W), L.ptr(X), L.ptr(out), T, M, K, W.stride(0), X.stride(0), out.stride(0), None, 0)
    L.check(_proj_fn("cad_proj_wxT", X.dtype)(C.byref(a), stream), "cad_proj_wxT")
    return out


def _same_mfma_dtype(*ts) -> None:
    """The 16-bit MFMA kernels read every operand in ONE element type (bf16 or fp16): a mixed call would reinterpret bits."""
    dts = {t.dtype for t in ts if t is not None}
    if len(dts) != 1 or not dts <= set(_MFMA_DTYPES):
        raise TypeError(f"caduceus_amd projection kernels take bf16 or fp16 operands of one dtype, got {sorted(map(str, dts))}")


def proj_wx_supported(t: torch.Tensor, K: int, T: int, M: Optional[int] = None) -> bool:
    """thin K (K <= 64, any M, optional addend), or -- when M is given -- thin M / deep K (M <= 64, K % 64 == 0, no addend)"""
    if t.dtype not in _MFMA_DTYPES:
        return False
    lib = L.get_lib()
    if lib.cad_proj_wx_supported(int(K), int(T)):
        return True
    return M is not None and bool(lib.cad_proj_wx_thin_supported(int(M), int(K), int(T)))


def proj_wx(W: torch.Tensor, X: torch.Tensor, out: Optional[torch.Tensor] = None,
            acc: Optional[torch.Tensor] = None, softplus_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (M, T) = W (M, K) @ X (K, T) [+ acc (M, T)], all channel-major bf16, thin K (cad_proj_wx).  `acc` may be `out`
    itself (in-place accumulate).  softplus_bias (M) fp32: out = softplus(W @ X + bias) evaluated in fp32 (thin K only)."""
    M, K = W.shape
    T = X.shape[1]
    if X.shape[0] != K or W.stride(1) != 1 or X.stride(1) != 1:
        raise ValueError("proj_wx: W (M, K) and X (K, T) with unit inner stride")
    _same_mfma_dtype(W, X, out, acc)
    if out is None:
        out = torch.empty((M, T), dtype=X.dtype, device=X.device)
    stream = L.stream_and_check(W, X, out, acc, softplus_bias, contiguous=False)
    if softplus_bias is not None and (softplus_bias.dtype != torch.float32 or softplus_bias.numel() != M or
                                      not softplus_bias.is_contiguous()):
        raise ValueError("proj_wx: softplus_bias must be a contiguous fp32 vector of M elements")
    a = L.ProjArgs(L.ptr(W), L.ptr(X), L.ptr(out), T, M, K, W.stride(0), X.stride(0), out.stride(0), L.ptr(acc),
                   0 if acc is None else acc.stride(0), L.ptr(softplus_bias), 0 if softplus_bias is None else 1)
    L.check(_proj_fn("cad_proj_wx", X.dtype)(C.byref(a), stream), "cad_proj_wx")
    return out


def proj_xTw_supported(X: torch.Tensor, M: int, K: int, T: int) -> bool:
    return X.dtype in _MFMA_DTYPES and bool(L.get_lib().cad_proj_xTw_supported(int(M), int(K), int(T)))


def proj_xTw(W: torch.Tensor, X: torch.Tensor, X2: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (T, M) token-major = X (K, T)^T @ W (M, K)^T [+ X2 (K, T)^T @ W^T], X / X2 channel-major bf16 (cad_proj_xTw): out_proj on the
    sum of the two directions' scan outputs through ONE set of resident weight fragments, fp32 accumulation over both panels."""
    M, K = W.shape
    T = X.shape[1]
    _same_mfma_dtype(W, X, X2, out)
    if out is None:
        out = torch.empty((T, M), dtype=X.dtype, device=X.device)
    stream = L.stream_and_check(W, X, X2, out, contiguous=False)
    assert W.stride(1) == 1 and X.stride(1) == 1 and out.stride(1) == 1 and (X2 is None or (X2.stride() == X.stride() and X2.shape == X.shape))
    a = L.ProjTmArgs(L.ptr(W), L.ptr(X), L.ptr(X2), L.ptr(out), T, M, K, W.stride(0), X.stride(0), out.stride(0))
    L.check(_proj_fn("cad_proj_xTw", X.dtype)(C.byref(a), stream), "cad_proj_xTw")
    return out


def proj_wx_wgrad_supported(X: torch.Tensor, M: int, K: int, T: int) -> bool:
    return X.dtype in _MFMA_DTYPES and bool(L.get_lib().cad_proj_wx_wgrad_supported(int(M), int(K), int(T)))


def wgrad_partials(T: int, K: int, M: int, device, nsets: int = 1) -> torch.Tensor:
    """(nsets, P, K, M) fp32 partial slots of cad_proj_wx_wgrad, one (K, M) slot per workgroup: a caller with several parameter sets
    hands each launch its own [i] and folds all of them with ONE sum over dim 1 afterwards."""
    return torch.empty((nsets, L.get_lib().cad_proj_wx_wgrad_partials(T), K, M), dtype=torch.float32, device=device)


def proj_wx_wgrad(W: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, out: Optional[torch.Tensor] = None,
                  part: Optional[torch.Tensor] = None):
    """(out (M, T) = W (M, K) @ X (K, T),  dW (K, M) fp32 = X (K, T) @ Y (M, T)^T) from ONE pass over X (cad_proj_wx_wgrad):
    d(dt_lr) = W_dt^T d(delta) together with dW_dt = d(delta) dt_lr^T.  All operands channel-major bf16.
    part: a (P, K, M) slice of wgrad_partials() -- then the partial slots are left un-summed (returns (out, None))."""
    M, K = W.shape
    T = X.shape[1]
    if X.shape[0] != K or Y.shape != (M, T) or W.stride(1) != 1 or X.stride(1) != 1 or Y.stride(1) != 1:
        raise ValueError("proj_wx_wgrad: W (M, K), X (K, T), Y (M, T) with unit inner stride")
    _same_mfma_dtype(W, X, Y, out)
    if out is None:
        out = torch.empty((M, T), dtype=X.dtype, device=X.device)
    own = part is None
    if own:
        part = wgrad_partials(T, K, M, X.device)[0]
    stream = L.stream_and_check(W, X, Y, out, part, contiguous=False)
    a = L.ProjArgs(L.ptr(W), L.ptr(X), L.ptr(out), T, M, K, W.stride(0), X.stride(0), out.stride(0), None, 0, None, 0,
                   L.ptr(Y), Y.stride(0), L.ptr(part))
    L.check(_proj_fn("cad_proj_wx_wgrad", X.dtype)(C.byref(a), stream), "cad_proj_wx_wgrad")
    return out, (part.sum(dim=0) if own else None)


def proj_wgrad_only_supported(X: torch.Tensor, M: int, K: int, T: int) -> bool:
    return X.dtype in _MFMA_DTYPES and bool(L.get_lib().cad_proj_wgrad_only_supported(int(M), int(K), int(T)))


def proj_wgrad_only(X: torch.Tensor, Y: torch.Tensor, part: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """dW (M, K) fp32 = Y (M, T) @ X (K, T)^T, both channel-major bf16, M <= 64: the weight-gradient stage of cad_proj_wx_wgrad
    alone (W == NULL) -- dW_x = d(dbc) . xc^T of the x_proj backward.  part: as for proj_wx_wgrad (slots hold the (K, M) transpose)."""
    K, T = X.shape
    M = Y.shape[0]
    if Y.shape[1] != T or X.stride(1) != 1 or Y.stride(1) != 1:
        raise ValueError("proj_wgrad_only: X (K, T), Y (M, T) with unit inner stride")
    _same_mfma_dtype(X, Y)
    own = part is None
    if own:
        part = wgrad_partials(T, K, M, X.device)[0]
    stream = L.stream_and_check(X, Y, part, contiguous=False)
    a = L.ProjArgs(None, L.ptr(X), None, T, M, K, 0, X.stride(0), 0, None, 0, None, 0, L.ptr(Y), Y.stride(0), L.ptr(part))
    L.check(_proj_fn("cad_proj_wx_wgrad", X.dtype)(C.byref(a), stream), "cad_proj_wx_wgrad")
    return part.sum(dim=0).t().contiguous() if own else None


# ------------------------------------------------------------------------------------------------------------------
# the streamed tiled GEMM (csrc/gemm_stream.h) and the fp32 folds of partial tiles (csrc/fold_f32.hip)
# ------------------------------------------------------------------------------------------------------------------
GEMM_PARTIALS, GEMM_OUT_T_BF16 = 0, 1


def gemm_stream_slices(R: int, Cc: int, K: int) -> int:
    """K slices of a weight gradient: as many as fill the GPU with one 256 x 256 tile per workgroup (cad_gemm_stream), 0 = unsupported."""
    if R % 256 or Cc % 256 or R < 256 or Cc < 256:
        return 0
    n = max(1, _cu_count() // ((R // 256) * (Cc // 256)))
    while n > 1 and (K % (32 * n) != 0):
        n -= 1
    return n if K % (32 * n) == 0 else 0


def fold_f32(jobs) -> None:
    """cad_fold_f32_multi: jobs = [(src, dst, n, nparts, stride, nparts2, stride2)], src / dst fp32 tensors (src addressed from its data
    pointer: dst[i] = sum_{j < nparts2, k < nparts} src[j * stride2 + k * stride + i]) -- every sum in ONE launch."""
    arr = (L.FoldF32Job * len(jobs))()
    tensors = []
    for q, (src, dst, n, nparts, stride, nparts2, stride2) in enumerate(jobs):
        if src.dtype != torch.float32 or dst.dtype != torch.float32 or not dst.is_contiguous() or dst.numel() != n:
            raise ValueError("fold_f32: fp32 tensors, dst contiguous with n elements")
        arr[q] = L.FoldF32Job(L.ptr(src), L.ptr(dst), n, stride, stride2, nparts, nparts2)
        tensors += [src, dst]
    stream = L.stream_and_check(*tensors, contiguous=False)
    L.check(L.get_lib().cad_fold_f32_multi(arr, len(jobs), stream), "cad_fold_f32_multi")


def wgrad_cm_tm(a_cm: torch.Tensor, b_tm: torch.Tensor, return_partials: bool = False) -> Optional[torch.Tensor]:
    """(M, N) fp32 = a (M, T) channel-major @ b (T, N) token-major, bf16 operands, fp32 accumulation over ALL tokens (cad_gemm_stream,
    CAD_GEMM_PARTIALS: one fp32 tile per K slice, summed here): dW_in and dW_out of the mixer.  None if the shape is not served.
    return_partials: the (slices, M, N) partial tiles as they are (the caller folds them, e.g. with fold_f32 next to other sums)."""
    M, T = a_cm.shape
    N = b_tm.shape[1]
    if a_cm.dtype not in _MFMA_DTYPES or b_tm.dtype != a_cm.dtype or a_cm.stride(1) != 1 or b_tm.stride(1) != 1:
        return None
    if a_cm.stride(0) % 8 or b_tm.stride(0) % 8 or a_cm.data_ptr() % 16 or b_tm.data_ptr() % 16:
        return None
    n = gemm_stream_slices(M, N, T)
    if n == 0 or not L.get_lib().cad_gemm_stream_supported(M, N, T, n):
        return None
    part = torch.empty((n, M, N), dtype=torch.float32, device=a_cm.device)
    stream = L.stream_and_check(a_cm, b_tm, part, contiguous=False)
    a = L.GemmStreamArgs(L.ptr(a_cm), L.ptr(b_tm), L.ptr(part), M, N, T, a_cm.stride(0), b_tm.stride(0), 0, n, GEMM_PARTIALS)
    L.check(_proj_fn("cad_gemm_stream", a_cm.dtype)(C.byref(a), stream), "cad_gemm_stream")
    if return_partials:
        return part
    return part[0] if n == 1 else part.sum(0)


def gemm_out_t(A: torch.Tensor, B: torch.Tensor, col_fastest: bool = True) -> Optional[torch.Tensor]:
    """out (C, R) bf16 = (A (R, K) @ B (K, C))^T, both operands row-major bf16 and streamed, fp32 accumulation (cad_gemm_stream,
    CAD_GEMM_OUT_T_BF16).  With A = token-major activations (T, d_model) and B = W^T (d_model, M) this is a projection with channel-major
    output (M, T): the in_proj and d(y) of the mixer at d_model 512 (configs[4]), where it replaces the W-stationary cad_proj_wxT
    (which streams X once per 128-row block of W).  col_fastest: neighbouring workgroups share an A tile.  None if the shape is not served."""
    return proj_xTw_stream(A, B, col_fastest=col_fastest)


def proj_xTw_stream(Wt: torch.Tensor, X: torch.Tensor, col_fastest: bool = False) -> Optional[torch.Tensor]:
    """out (T, M) token-major bf16 = X (K, T)^T @ Wt (M, K)^T with X channel-major and BOTH operands streamed (cad_gemm_stream,
    CAD_GEMM_OUT_T_BF16): d(x2d) = dxz^T W_in with Wt = W_in^T (D, 2E), K = 2E too deep for resident weight fragments.  None if the
    shape is not served."""
    M, K = Wt.shape
    T = X.shape[1]
    if X.dtype not in _MFMA_DTYPES or Wt.dtype != X.dtype or Wt.stride(1) != 1 or X.stride(1) != 1:
        return None
    if Wt.stride(0) % 8 or X.stride(0) % 8 or Wt.data_ptr() % 16 or X.data_ptr() % 16:
        return None
    if not L.get_lib().cad_gemm_stream_supported(M, T, K, 1):
        return None
    out = torch.empty((T, M), dtype=X.dtype, device=X.device)
    stream = L.stream_and_check(Wt, X, out, contiguous=False)
    a = L.GemmStreamArgs(L.ptr(Wt), L.ptr(X), L.ptr(out), M, T, K, Wt.stride(0), X.stride(0), out.stride(0), 1, GEMM_OUT_T_BF16,
                         int(bool(col_fastest)))
    L.check(_proj_fn("cad_gemm_stream", X.dtype)(C.byref(a), stream), "cad_gemm_stream")
    return out


# ------------------------------------------------------------------------------------------------------------------
# fp8 (OCP e4m3) in_proj: BASELINE configs[4] "fp8 MFMA projections"
# ------------------------------------------------------------------------------------------------------------------
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def fp8_proj_supported(t: torch.Tensor, K: int) -> bool:
    return t.dtype in (torch.bfloat16, torch.float32) and bool(L.get_lib().cad_proj_fp8_supported(int(K)))


def quant_rows_fp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x (T, K) fp32 / bf16 -> (q (T, K) e4m3 bytes as uint8, scale (T) fp32) with x ~ q * scale[:, None]: one scale per token
    (cad_quant_rows_fp8), so a token's quantisation does not depend on its position."""
    T, K = x.shape
    if x.stride(1) != 1:
        raise ValueError("quant_rows_fp8: unit inner stride")
    q = torch.empty((T, K), dtype=torch.uint8, device=x.device)
    scale = torch.empty((T,), dtype=torch.float32, device=x.device)
    stream = L.stream_and_check(x, q, scale, contiguous=False)
    a = L.QuantFp8Args(L.ptr(x), L.ptr(q), L.ptr(scale), T, K, x.stride(0), q.stride(0), L.dtype_code(x.dtype))
    L.check(L.get_lib().cad_quant_rows_fp8(C.byref(a), stream), "cad_quant_rows_fp8")
    return q, scale


def quant_weight_fp8(W: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """W (M, K) -> (e4m3 bytes as uint8, per-row scale (M) fp32).  Weights change once per optimizer step: plain torch ops."""
    w = W.detach().float()
    s = (w.abs().amax(dim=1) / FP8_MAX).clamp_min(1e-30)
    q = (w / s[:, None]).clamp_(-FP8_MAX, FP8_MAX).to(FP8).view(torch.uint8)
    return q.contiguous(), s.contiguous()


def proj_wxT_fp8(Wq: torch.Tensor, sw: torch.Tensor, Xq: torch.Tensor, sx: torch.Tensor,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (M, T) channel-major bf16 = (Wq (M, K) @ Xq (T, K)^T) * sw[:, None] * sx[None, :] on the fp8 matrix cores
    (cad_proj_wxT_fp8); Wq / Xq: e4m3 bytes (uint8 tensors), sw / sx: fp32 scales."""
    M, K = Wq.shape
    T = Xq.shape[0]
    if Xq.shape[1] != K or Wq.dtype != torch.uint8 or Xq.dtype != torch.uint8 or Wq.stride(1) != 1 or Xq.stride(1) != 1:
        raise ValueError("proj_wxT_fp8: Wq (M, K), Xq (T, K) uint8 (e4m3 bytes) with unit inner stride")
    if sw.dtype != torch.float32 or sx.dtype != torch.float32 or sw.numel() != M or sx.numel() != T:
        raise ValueError("proj_wxT_fp8: sw (M), sx (T) fp32")
    if out is None:
        out = torch.empty((M, T), dtype=torch.bfloat16, device=Xq.device)
    stream = L.stream_and_check(Wq, Xq, sw, sx, out, contiguous=False)
    a = L.ProjFp8Args(L.ptr(Wq), L.ptr(Xq), L.ptr(sw), L.ptr(sx), L.ptr(out), T, M, K, Wq.stride(0), Xq.stride(0),
                      out.stride(0))
    L.check(L.get_lib().cad_proj_wxT_fp8(C.byref(a), stream), "cad_proj_wxT_fp8")
    return out


# ------------------------------------------------------------------------------------------------------------------
# one decode token of a left-to-right Mamba parameter set (inference only: no autograd)
# ------------------------------------------------------------------------------------------------------------------
def mamba_step_supported(D: int, E: int, N: int, R: int, K: int, act: torch.dtype) -> bool:
    return bool(L.get_lib().cad_mamba_step_supported(D, E, N, R, K, L.dtype_code(act)))


def mamba_step_scratch(B: int, E: int, N: int, R: int, device) -> torch.Tensor:
    """The fp32 scratch buffer mamba_step needs for B rows; the caller holds it across steps (the library never allocates)."""
    return torch.empty((int(L.get_lib().cad_mamba_step_scratch_floats(B, E, N, R)),), dtype=torch.float32, device=device)


def mamba_step(h: torch.Tensor, conv_state: torch.Tensor, ssm_state: torch.Tensor, W_in: torch.Tensor, b_in: Optional[torch.Tensor],
               conv_w: torch.Tensor, conv_b: Optional[torch.Tensor], W_x: torch.Tensor, W_dt: torch.Tensor, dt_bias: torch.Tensor,
               A_log: torch.Tensor, D: torch.Tensor, W_out: torch.Tensor, b_out: Optional[torch.Tensor], scratch: torch.Tensor,
               act: Optional[torch.dtype] = None) -> torch.Tensor:
    """out (B, D) = one token of mamba_ssm `Mamba.step` for h (B, D) in `act` (default: h's dtype), three launches (cad_mamba_step).
    conv_state (>= B, E, K) in `act` and ssm_state (>= B, E, N) fp32 are updated IN PLACE in their rows [0, B).  Parameters are the
    fp32 master tensors (conv_w: (E, K) or (E, 1, K)); scratch: mamba_step_scratch(B, ...) or larger.  Inference only: nothing here is
    recorded for autograd.  A shape the kernels do not serve raises (CAD_ERR_UNSUPPORTED); there is no other path."""
    act = h.dtype if act is None else act
    if h.dim() != 2 or h.dtype != act or conv_state.dtype != act or ssm_state.dtype != torch.float32:
        raise TypeError(f"mamba_step: h (B, D) and conv_state in {act}, ssm_state in float32 "
                        f"(got {h.dtype}, {conv_state.dtype}, {ssm_state.dtype})")
    B, Dm = h.shape
    E, R = W_dt.shape
    K = conv_state.shape[2]
    N = ssm_state.shape[2]
    params = [W_in, b_in, conv_w, conv_b, W_x, W_dt, dt_bias, A_log, D, W_out, b_out]
    if any(p is not None and p.dtype != torch.float32 for p in params):
        raise TypeError("mamba_step: parameters are the fp32 master tensors")
    params = [None if p is None else p.detach() for p in params]
    W_in, b_in, conv_w, conv_b, W_x, W_dt, dt_bias, A_log, D, W_out, b_out = params
    conv_w = conv_w.reshape(E, -1)
    shapes_ok = (tuple(W_in.shape) == (2 * E, Dm) and tuple(conv_w.shape) == (E, K) and tuple(W_x.shape) == (R + 2 * N, E)
                 and tuple(A_log.shape) == (E, N) and tuple(W_out.shape) == (Dm, E) and dt_bias.numel() == E and D.numel() == E
                 and (b_in is None or b_in.numel() == 2 * E) and (conv_b is None or conv_b.numel() == E)
                 and (b_out is None or b_out.numel() == Dm) and tuple(conv_state.shape[1:]) == (E, K)
                 and tuple(ssm_state.shape[1:]) == (E, N) and conv_state.shape[0] >= B and ssm_state.shape[0] >= B and B >= 1)
    if not shapes_ok:
        raise ValueError("mamba_step: operand shapes do not describe one Mamba parameter set")
    lib = L.get_lib()
    if scratch.dtype != torch.float32 or scratch.numel() < lib.cad_mamba_step_scratch_floats(B, E, N, R):
        raise ValueError("mamba_step: scratch must hold cad_mamba_step_scratch_floats(B, E, N, R) float32 values")
    out = torch.empty((B, Dm), dtype=act, device=h.device)
    stream = L.stream_and_check(h, conv_state, ssm_state, W_in, b_in, conv_w, conv_b, W_x, W_dt, dt_bias, A_log, D, W_out, b_out, scratch,
                                out)
    a = L.MambaStepArgs(L.ptr(h), L.ptr(out), L.ptr(conv_state), L.ptr(ssm_state), L.ptr(W_in), L.ptr(b_in), L.ptr(conv_w), L.ptr(conv_b),
                        L.ptr(W_x), L.ptr(W_dt), L.ptr(dt_bias), L.ptr(A_log), L.ptr(D), L.ptr(W_out), L.ptr(b_out), L.ptr(scratch), B, Dm,
                        E, N, R, K, L.dtype_code(act))
    L.check(lib.cad_mamba_step(C.byref(a), stream), "cad_mamba_step")
    return out


# ------------------------------------------------------------------------------------------------------------------
# token sampler and the whole decode token of a causal stack (cad_sample_tokens / cad_decode_token)
# ------------------------------------------------------------------------------------------------------------------
SAMPLER_VMAX = 64


def philox_uniform(seed: int, r: int, position: int) -> float:
    """The uniform in [0, 1) the kernels draw for (seed, r = row_offset + row, position): the first word of Philox4x32-10 with key
    (seed low, seed high) and counter (r low, r high, position low, position high), its top 24 bits.  Plain integers on the host."""
    m32 = 0xFFFFFFFF
    c = [r & m32, (r >> 32) & m32, position & m32, (position >> 32) & m32]
    k0, k1 = seed & m32, (seed >> 32) & m32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & m32, (p0 >> 32) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & m32, (k1 + 0xBB67AE85) & m32
    return (c[0] >> 8) * 2.0 ** -24


def check_sampling(top_k: int, top_p: float, temperature: float):
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k must be a non-negative integer (0 keeps every token), got {top_k}")
    if not 0.0 <= top_p <= 1.0:
        raise ValueError(f"top_p must lie in [0, 1], got {top_p}")
    if not temperature > 0.0:
        raise ValueError(f"temperature must be positive, got {temperature}")


def sampler_args(top_k=1, top_p=0.0, temperature=1.0, seed=0, row_offset=0, position=0, logit_mask=None) -> L.SamplerArgs:
    check_sampling(top_k, top_p, temperature)
    return L.SamplerArgs(L.ptr(logit_mask), int(seed) & 0xFFFFFFFFFFFFFFFF, int(row_offset), int(position), int(top_k), float(top_p),
                         float(temperature))


def _sample_tokens_torch(x, top_k, top_p, temperature, u):
    """cad_sample_tokens' rules (include/caduceus_hip.h) in torch ops, for vocabularies beyond the kernel's 64 ids."""
    B, V = x.shape
    ar = torch.arange(V, device=x.device).expand(B, V)
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices  # ties: the lower id first
    rank = torch.empty_like(order).scatter_(1, order, ar)
    if top_k == 1:
        return order[:, 0]
    keep_n = V if top_k == 0 or top_k > V else top_k
    keep = rank < keep_n
    if temperature != 1.0:
        x = x / temperature
    mx = torch.where(keep, x, torch.full_like(x, float("-inf"))).amax(-1, keepdim=True)
    e = torch.where(keep, torch.exp(x - mx), torch.zeros_like(x)).nan_to_num(nan=0.0)
    if 0.0 < top_p < 1.0:
        p_sorted = (e / e.sum(-1, keepdim=True)).gather(1, order)
        cum = p_sorted.flip(-1).cumsum(-1).flip(-1).gather(1, rank)  # this entry and everything ranked behind it
        drop = keep & (rank != 0) & (cum <= 1.0 - top_p)
        keep, e = keep & ~drop, torch.where(drop, torch.zeros_like(e), e)
    cdf = e.cumsum(-1)
    live = keep & (e > 0)
    first = torch.where(live & (cdf > u[:, None] * cdf[:, -1:]), ar, torch.full_like(ar, V)).amin(-1)
    last = torch.where(live, ar, torch.full_like(ar, -1)).amax(-1)
    return torch.where(first < V, first, torch.where(last >= 0, last, order[:, 0]))


def sample_tokens(logits: torch.Tensor, top_k: int = 1, top_p: float = 0.0, temperature: float = 1.0, seed: int = 0, row_offset: int = 0,
                  position: int = 0, logit_mask: Optional[torch.Tensor] = None, return_u: bool = False):
    """ids (B) int64 sampled from logits (B, V) fp32 by the rules of cad_sample_tokens (mamba_ssm's `sample`: logit_mask (V) of 0 / -inf,
    top_k, temperature, top_p, inverse CDF at the uniform keyed by (seed, row_offset + row, position)).  V <= 64 runs the kernel, one
    launch; a larger vocabulary the same rules in torch ops.  return_u: also the uniforms (B) fp32 the rows consumed."""
    check_sampling(top_k, top_p, temperature)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise TypeError("sample_tokens: logits (B, V) float32")
    B, V = logits.shape
    if logit_mask is not None and (logit_mask.dtype != torch.float32 or logit_mask.numel() != V):
        raise TypeError("sample_tokens: logit_mask holds V float32 values (0 or -inf)")
    logits = logits.contiguous()
    if V > SAMPLER_VMAX:
        u = torch.tensor([philox_uniform(int(seed) & 0xFFFFFFFFFFFFFFFF, row_offset + b, position) for b in range(B)], dtype=torch.float32,
                         device=logits.device)
        ids = _sample_tokens_torch(logits if logit_mask is None else logits + logit_mask, int(top_k), float(top_p), float(temperature), u)
        return (ids, u) if return_u else ids
    ids = torch.empty((B,), dtype=torch.int64, device=logits.device)
    u = torch.empty((B,), dtype=torch.float32, device=logits.device) if return_u else None
    stream = L.stream_and_check(logits, logit_mask, ids, u)
    s = sampler_args(top_k, top_p, temperature, seed, row_offset, position, logit_mask)
    L.check(L.get_lib().cad_sample_tokens(L.ptr(logits), B, V, C.byref(s), L.ptr(ids), L.ptr(u), stream), "cad_sample_tokens")
    return (ids, u) if return_u else ids


def decode_supported(D: int, E: int, N: int, R: int, K: int, V: int, act: torch.dtype) -> bool:
    return bool(L.get_lib().cad_decode_supported(D, E, N, R, K, V, L.dtype_code(act)))


def decode_scratch(B: int, D: int, E: int, device) -> torch.Tensor:
    """The fp32 scratch of decode_token for B rows; the caller holds it across tokens (the library never allocates)."""
    return torch.empty((int(L.get_lib().cad_decode_scratch_floats(B, D, E)),), dtype=torch.float32, device=device)


def decode_token(args: "L.DecodeArgs", stream) -> None:
    """One generated token of a causal stack: cad_decode_token on a prepared argument record (generation.DecodeStack builds it once and
    keeps every tensor it points to alive).  3 n_layer + 1 launches on `stream`, nothing allocated, nothing read back."""
    L.check(L.get_lib().cad_decode_token(C.byref(args), stream), "cad_decode_token")
