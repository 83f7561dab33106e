// One decode token of a left-to-right Mamba parameter set (include/caduceus_hip.h, cad_mamba_step): the constant-time step behind
// `inference_params`.  Three small launches, each bound by reading its fp32 weights once:
//   1. step_in_conv_kernel   xz = W_in h (+ b_in), conv_state shifted and refilled, xc = silu(conv)      one wave per channel e
//   2. step_ssm_kernel       dbc = W_x xc, delta = W_dt dbc[:R], state update, y = (C.s + D xc) silu(z)  16 channels per workgroup
//   3. step_out_kernel       out = W_out y (+ b_out)                                                     one wave per output column
// The two dependencies (every dbc value needs all of xc; every out value needs all of y) are kernel boundaries (~1.2 us each), never a
// grid-wide barrier: a software barrier costs 26 us or more and can hang a shared device.  Kernel 2 has no third dependency because
// every workgroup recomputes the R + 2N dot products of its row (48 x 512 multiply-adds at d_model 256) from xc in LDS.
// Weights are the fp32 master tensors; a workgroup of kernels 1 / 3 holds up to ST_BT batch rows in LDS so that a weight row is read
// once per ST_BT rows.  A row's sums never depend on the other rows of the batch (fixed lane-strided order, xor-butterfly reduction).
// Rounding points (T = activation dtype): xz, xc, dbc, delta, y, out -- where the full-sequence path stores these tensors.
// The kernels live in step_kernels.h.
#include "step_kernels.h"

namespace {

template <typename T>
int step_launch(const cad_mamba_step_args& a, void* stream) {
    const int64_t BE = a.B * a.E;
    float* xc = a.scratch;
    float* z = a.scratch + BE;
    float* y = a.scratch + 2 * BE;
    const unsigned nbt = (unsigned)((a.B + ST_BT - 1) / ST_BT);
    const int nb = (int)(a.B < ST_BT ? a.B : ST_BT);
    CAD_LAUNCH((step_in_conv_kernel<T>), dim3((a.E + ST_WAVES - 1) / ST_WAVES, nbt), dim3(ST_THREADS), (size_t)nb * a.D * sizeof(float), stream,
               a, xc, z);
    CAD_LAUNCH((step_ssm_kernel<T>), dim3((a.E + ST_CH - 1) / ST_CH, (unsigned)a.B), dim3(ST_THREADS),
               (size_t)(a.E + a.R + 2 * a.N) * sizeof(float), stream, a, xc, z, y);
    CAD_LAUNCH((step_out_kernel<T>), dim3((a.D + ST_WAVES - 1) / ST_WAVES, nbt), dim3(ST_THREADS), (size_t)nb * a.E * sizeof(float), stream, a,
               y);
    return cad_after_launch();
}

}  // namespace

extern "C" int cad_mamba_step_supported(int D, int E, int N, int R, int K, int dtype) {
    return D >= 1 && D <= ST_WIDTH_MAX && E >= 1 && E <= ST_WIDTH_MAX && N >= 1 && N <= ST_NMAX && R >= 1 && R <= ST_WIDTH_MAX && K >= 1 &&
           K <= ST_KMAX && (dtype == CAD_F32 || dtype == CAD_BF16 || dtype == CAD_F16);
}

extern "C" int64_t cad_mamba_step_scratch_floats(int64_t B, int E, int N, int R) {
    (void)N, (void)R;  // (dbc lives in LDS: every workgroup of the state kernel recomputes it)
    return B > 0 && E > 0 ? 3 * B * E : 0;  // xc | z | y, (B, E) fp32 each
}

extern "C" int cad_mamba_step(const cad_mamba_step_args* a, void* stream) {
    CAD_CHECK_ARG(a && a->h && a->out && a->conv_state && a->ssm_state && a->scratch);
    CAD_CHECK_ARG(a->W_in && a->conv_w && a->W_x && a->W_dt && a->dt_bias && a->A_log && a->Dskip && a->W_out);
    CAD_CHECK_ARG(a->B >= 1 && a->B <= 65535);
    if (!cad_mamba_step_supported(a->D, a->E, a->N, a->R, a->K, a->dtype)) return CAD_ERR_UNSUPPORTED;
    switch (a->dtype) {
        case CAD_F32: return step_launch<float>(*a, stream);
        case CAD_BF16: return step_launch<bf16_t>(*a, stream);
        default: return step_launch<f16_t>(*a, stream);
    }
}
