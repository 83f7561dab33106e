"""The schedule of the hand-scheduled BiMamba mixer (caduceus_amd/mixer.py), pinned: every C-ABI call (`cad_*`: the launches and the host
queries that steer the dispatch chains) of one layer, forward + backward, in order, against literal lists.  The lists were recorded at the
commit BEFORE mixer.py was cut into stage functions, so they hold that refactor to its parent's schedule; a change of the schedule (a
fusion, a reordered launch) edits its list deliberately."""
import pytest
import torch

from caduceus_amd import _lib, mixer, ops
from caduceus_amd.mamba import Mamba

# The dispatch decisions are host-side predicates of shape and dtype (the library's *_supported queries), the same in the emulator and the
# device build: one list per case serves both backends.  Only the layer with the concurrent fold has a list per backend, because the two
# backends run it at different shapes (see the test); the device's once-per-process search for a side stream is kept out of the record.
SCHEDULE = {
    "a_d256_bf16": """
    cad_proj_supported cad_proj_wxT cad_conv1d_fwd_multi cad_proj_wx_supported cad_proj_wx_thin_supported cad_proj_wx cad_proj_wx_supported
    cad_proj_wx cad_proj_wx_supported cad_proj_wx_thin_supported cad_proj_wx cad_proj_wx_supported cad_proj_wx cad_scan_chunk_len
    cad_scan_state_floats cad_scan_state_floats cad_scan_fwd_multi cad_proj_xTw_supported cad_proj_xTw cad_proj_supported cad_proj_wxT
    cad_gemm_stream_supported cad_gemm_stream cad_scan_bwd_partials cad_scan_bwd_chunk_len cad_fold_stream_supported cad_scan_gate_fix_entries
    cad_scan_bwd_partials cad_scan_bwd_partials cad_scan_bwd_multi cad_scan_bwd_gate_fix cad_reduce_partials_multi cad_proj_wx_wgrad_supported
    cad_proj_wx_wgrad_partials cad_proj_wx_wgrad cad_proj_wgrad_only_supported cad_proj_wx_wgrad_partials cad_proj_wx_wgrad
    cad_proj_wx_supported cad_proj_wx cad_proj_wx_wgrad_supported cad_proj_wx_wgrad cad_proj_wgrad_only_supported cad_proj_wx_wgrad
    cad_proj_wx_supported cad_proj_wx cad_conv1d_bwd_slots cad_conv1d_bwd_slots cad_conv1d_bwd_multi_slotted cad_gemm_stream_supported
    cad_gemm_stream cad_gemm_stream_supported cad_gemm_stream cad_fold_f32_multi""",
    "c_d512_bf16": """
    cad_gemm_stream_supported cad_gemm_stream cad_conv1d_fwd_multi cad_proj_wx_supported cad_proj_wx_thin_supported cad_proj_wx_supported
    cad_proj_wx_thin_supported cad_proj_wx cad_proj_wx cad_proj_wx_supported cad_proj_wx cad_proj_wx_supported cad_proj_wx_thin_supported
    cad_proj_wx_supported cad_proj_wx_thin_supported cad_proj_wx cad_proj_wx cad_proj_wx_supported cad_proj_wx cad_scan_chunk_len
    cad_scan_state_floats cad_scan_state_floats cad_scan_fwd_multi cad_proj_xTw_supported cad_gemm_stream_supported cad_gemm_stream
    cad_gemm_stream_supported cad_gemm_stream cad_gemm_stream_supported cad_gemm_stream cad_scan_bwd_partials cad_scan_bwd_chunk_len
    cad_fold_stream_supported cad_scan_gate_fix_entries cad_scan_bwd_partials cad_scan_bwd_partials cad_scan_bwd_multi cad_scan_bwd_gate_fix
    cad_reduce_partials_multi cad_proj_wx_wgrad_supported cad_proj_wx_supported cad_proj_wx_thin_supported cad_proj_wx
    cad_proj_wgrad_only_supported cad_proj_wx_wgrad_partials cad_proj_wx_wgrad cad_proj_wx_wgrad_partials cad_proj_wx_wgrad
    cad_proj_wgrad_only_supported cad_proj_wgrad_only_supported cad_proj_wx_wgrad_partials cad_proj_wx_wgrad cad_proj_wx_wgrad_partials
    cad_proj_wx_wgrad cad_proj_wx_supported cad_proj_wx cad_proj_wx_wgrad_supported cad_proj_wx_supported cad_proj_wx_thin_supported cad_proj_wx
    cad_proj_wgrad_only_supported cad_proj_wx_wgrad_partials cad_proj_wx_wgrad cad_proj_wx_wgrad_partials cad_proj_wx_wgrad
    cad_proj_wgrad_only_supported cad_proj_wgrad_only_supported cad_proj_wx_wgrad_partials cad_proj_wx_wgrad cad_proj_wx_wgrad_partials
    cad_proj_wx_wgrad cad_proj_wx_supported cad_proj_wx cad_conv1d_bwd_slots cad_conv1d_bwd_slots cad_conv1d_bwd_multi_slotted
    cad_gemm_stream_supported cad_gemm_stream cad_gemm_stream_supported cad_gemm_stream cad_fold_f32_multi""",
    "d_d128_fp32": """
    cad_gemm_f32 cad_conv1d_fwd_multi cad_gemm_f32 cad_gemm_f32 cad_gemm_f32 cad_gemm_f32 cad_scan_chunk_len cad_scan_state_floats
    cad_scan_state_floats cad_scan_fwd_multi cad_gemm_f32 cad_gemm_f32 cad_gemm_f32 cad_fold_f32_multi cad_scan_bwd_partials
    cad_scan_bwd_chunk_len cad_fold_stream_supported cad_scan_gate_fix_entries cad_scan_bwd_partials cad_scan_bwd_partials cad_scan_bwd_multi
    cad_scan_bwd_gate_fix cad_reduce_partials_multi cad_gemm_f32 cad_gemm_f32 cad_fold_f32_multi cad_gemm_f32 cad_fold_f32_multi cad_gemm_f32
    cad_gemm_f32 cad_gemm_f32 cad_fold_f32_multi cad_gemm_f32 cad_fold_f32_multi cad_gemm_f32 cad_conv1d_bwd_slots cad_conv1d_bwd_slots
    cad_conv1d_bwd_multi_slotted cad_gemm_f32 cad_gemm_f32 cad_fold_f32_multi""",
    "i_stream_fold_emu": """
    cad_proj_supported cad_proj_wxT cad_conv1d_fwd_multi cad_proj_wx_supported cad_proj_wx cad_proj_wx_supported cad_proj_wx_supported
    cad_proj_wx cad_proj_wx_supported cad_scan_chunk_len cad_scan_state_floats cad_scan_state_floats cad_scan_fwd_multi cad_proj_xTw_supported
    cad_gemm_stream_supported cad_proj_supported cad_proj_wxT cad_scan_bwd_partials cad_scan_bwd_chunk_len cad_fold_stream_supported
    cad_scan_bwd_fold_counter_ints cad_scan_gate_fix_entries cad_scan_bwd_partials cad_scan_bwd_partials cad_scan_bwd_multi
    cad_fold_partials_stream cad_fold_partials_stream cad_scan_bwd_gate_fix cad_proj_wx_wgrad_supported cad_proj_wx_supported cad_proj_wx
    cad_proj_wgrad_only_supported cad_proj_wx_supported cad_proj_wx_wgrad_supported cad_proj_wx_supported cad_proj_wx
    cad_proj_wgrad_only_supported cad_proj_wx_supported cad_conv1d_bwd_slots cad_conv1d_bwd_slots cad_conv1d_bwd_multi_slotted
    cad_gemm_stream_supported""",
    "i_stream_fold_hip": """
    cad_proj_supported cad_proj_wxT cad_conv1d_fwd_multi cad_proj_wx_supported cad_proj_wx_thin_supported cad_proj_wx cad_proj_wx_supported
    cad_proj_wx cad_proj_wx_supported cad_proj_wx_thin_supported cad_proj_wx cad_proj_wx_supported cad_proj_wx cad_scan_chunk_len
    cad_scan_state_floats cad_scan_state_floats cad_scan_fwd_multi cad_proj_xTw_supported cad_proj_xTw cad_proj_supported cad_proj_wxT
    cad_gemm_stream_supported cad_gemm_stream cad_scan_bwd_partials cad_scan_bwd_chunk_len cad_fold_stream_supported
    cad_scan_bwd_fold_counter_ints cad_scan_gate_fix_entries cad_scan_bwd_partials cad_scan_bwd_partials cad_scan_bwd_multi
    cad_fold_partials_stream cad_fold_partials_stream cad_scan_bwd_gate_fix cad_proj_wx_wgrad_supported cad_proj_wx_wgrad_partials
    cad_proj_wx_wgrad cad_proj_wgrad_only_supported cad_proj_wx_wgrad_partials cad_proj_wx_wgrad cad_proj_wx_supported cad_proj_wx
    cad_proj_wx_wgrad_supported cad_proj_wx_wgrad cad_proj_wgrad_only_supported cad_proj_wx_wgrad cad_proj_wx_supported cad_proj_wx
    cad_conv1d_bwd_slots cad_conv1d_bwd_slots cad_conv1d_bwd_multi_slotted cad_gemm_stream_supported cad_gemm_stream cad_gemm_stream_supported
    cad_gemm_stream cad_fold_f32_multi""",
    "scan_multi_k1": """
    cad_scan_chunk_len cad_scan_state_floats cad_scan_chunk_len cad_scan_state_floats cad_scan_fwd_multi cad_scan_bwd_partials
    cad_scan_gate_fix_entries cad_scan_bwd_partials cad_scan_gate_fix_entries cad_scan_bwd_multi cad_scan_bwd_gate_fix cad_reduce_partials
    cad_reduce_partials cad_reduce_partials cad_reduce_partials""",
    "scan_multi_k2": """
    cad_scan_chunk_len cad_scan_state_floats cad_scan_chunk_len cad_scan_state_floats cad_scan_fwd_multi cad_scan_fwd_multi
    cad_scan_bwd_partials cad_scan_gate_fix_entries cad_scan_bwd_partials cad_scan_gate_fix_entries cad_scan_bwd_multi cad_scan_bwd_multi
    cad_scan_bwd_gate_fix cad_reduce_partials cad_reduce_partials cad_reduce_partials cad_reduce_partials""",
    "scan_stateful": """
    cad_scan_state_floats cad_scan_fwd cad_scan_bwd_partials cad_scan_gate_fix_entries cad_scan_bwd cad_scan_bwd_gate_fix
    cad_reduce_partials cad_reduce_partials""",
}


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


def _recorded_layer(dev, d_model, L, dtype, cache):
    """The cad_* calls of one production layer, forward + backward (the pattern of tests/test_fold_stream.py::_layer_grads)."""
    torch.manual_seed(0)
    mf, mr = Mamba(d_model, device=dev), Mamba(d_model, device=dev)
    mr.in_proj.weight = mf.in_proj.weight
    mr.out_proj.weight = mf.out_proj.weight
    hn = (torch.randn(2, 1, L, d_model, device=dev) * 0.5).to(dtype).requires_grad_(True)
    g = torch.randn(2, 1, L, d_model, device=dev).to(dtype)
    if dev.type == "cuda":
        ops.fold_side_available(dev)  # the once-per-process probe for a side stream (cad_stream_probe) is not part of a layer's schedule
    real, calls = _lib.get_lib(), []
    _lib._lib = _Recorder(real, calls)
    try:
        if cache:
            mixer.prepare_step_cache([(mf, mr)], dtype)
        out = mixer.bimamba_mixer(hn, mf, mr, 1)
        out.backward(g)
    finally:
        _lib._lib = real
    assert hn.grad is not None and all(p.grad is not None for p in list(mf.parameters()) + list(mr.parameters()))
    return calls


def _check(calls, want):
    want = want.split()
    first = next((i for i, (a, b) in enumerate(zip(calls, want)) if a != b), min(len(calls), len(want)))
    assert calls == want, f"the schedule differs from call {first} on: got {calls[first:first + 6]}, pinned {want[first:first + 6]}"


@pytest.mark.parametrize("case,d_model,L,dtype,cache", [("a_d256_bf16", 256, 256, torch.bfloat16, True),
                                                        ("c_d512_bf16", 512, 256, torch.bfloat16, True),
                                                        ("d_d128_fp32", 128, 1104, torch.float32, False)])
def test_mixer_layer_schedule(backend, case, d_model, L, dtype, cache):
    """d_model 256 (every product on its first-choice own kernel), d_model 512 (in_proj / out_proj / d(y) streamed, x_proj in two K
    halves, the chunked dW_x) and fp32 (cad_gemm_f32 throughout, the fold kernel behind the scan)."""
    name, dev = backend
    _check(_recorded_layer(dev, d_model, L, dtype, cache), SCHEDULE[case])


def _recorded_scan(dev, stateful):
    """The cad_* calls of one autograd scan, forward + backward in bf16: two sets under a shared gate (ops.selective_scan_multi), or one
    segment entered through h0 whose hT the loss uses (ops.selective_scan_stateful)."""
    E, SB, N, Lq = 16, 2, 16, 4 * int(_lib.get_lib().cad_scan_chunk_len())
    torch.manual_seed(0)
    rand = lambda *shape: (torch.randn(*shape, device=dev) * 0.5).to(torch.bfloat16).requires_grad_(True)
    sets = [(rand(E, SB, Lq), rand(E, SB, Lq), (-torch.rand(E, N, device=dev) - 0.5).requires_grad_(True), rand(N, SB, Lq), rand(N, SB, Lq),
             torch.randn(E, device=dev, requires_grad=True), torch.randn(E, device=dev, requires_grad=True)) for _ in range(2)]
    z, h0 = rand(E, SB, Lq), torch.randn(E, SB, N, device=dev, requires_grad=True)
    real, calls = _lib.get_lib(), []
    _lib._lib = _Recorder(real, calls)
    try:
        if stateful:
            u, delta, A, Bm, Cm, D, bias = sets[0]
            out, hT = ops.selective_scan_stateful(u, delta, A, Bm, Cm, D, z, bias, h0, 1, 0, 1)
            (out.float().sum() + hT.sum()).backward()
        else:
            y_f, y_r = ops.selective_scan_multi(sets, z, 1, [(0, 1), (1, 0)])
            (y_f.float().sum() + y_r.float().sum()).backward()
    finally:
        _lib._lib = real
    used = [z, *sets[0], *(sets[1] if not stateful else (h0,))]
    assert all(t.grad is not None for t in used)
    return calls


@pytest.mark.parametrize("case,lsplit", [("scan_multi_k1", None), ("scan_multi_k2", "2"), ("scan_stateful", None)])
def test_autograd_scan_schedule(backend, monkeypatch, case, lsplit):
    """The scans outside the mixer (ops.py), lists recorded at the commit BEFORE their argument structs and backward moved into shared
    helpers: one launch per pass, one gate fix, two folds per set; k = 2 adds the map / carry passes of the L-split."""
    name, dev = backend
    if lsplit is None:
        monkeypatch.delenv("CADUCEUS_AMD_LSPLIT", raising=False)
    else:
        monkeypatch.setenv("CADUCEUS_AMD_LSPLIT", lsplit)
    _check(_recorded_scan(dev, case == "scan_stateful"), SCHEDULE[case])


def test_mixer_layer_schedule_with_the_concurrent_fold(backend, monkeypatch):
    """A layer that takes the dB / dC fold on the second stream: the emulator's small layer with the chunk threshold lowered (its narrow
    products take the library, so its list is short), the device's d_model 256 layer with 16 chunks per row as it is."""
    name, dev = backend
    if name == "emu":
        monkeypatch.setattr(mixer, "_STREAM_FOLD_MIN_CHUNKS", 1)
    d_model, L = (32, 1024) if name == "emu" else (256, 8192)
    _check(_recorded_layer(dev, d_model, L, torch.bfloat16, True), SCHEDULE["i_stream_fold_" + name])
