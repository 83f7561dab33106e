// The three kernels of one decode token of a left-to-right Mamba parameter set, shared by cad_mamba_step (step.hip) and by the
// whole-stack token of cad_decode_token (decode.hip), which launches the same kernels 2 and 3 and the same arithmetic of kernel 1.
// Three small launches, each bound by reading its fp32 weights once:
//   1. step_in_conv_kernel   xz = W_in h (+ b_in), conv_state shifted and refilled, xc = silu(conv)      one wave per channel e
//   2. step_ssm_kernel       dbc = W_x xc, delta = W_dt dbc[:R], state update, y = (C.s + D xc) silu(z)  16 channels per workgroup
//   3. step_out_kernel       out = W_out y (+ b_out)                                                     one wave per output column
// The two dependencies (every dbc value needs all of xc; every out value needs all of y) are kernel boundaries (~1.2 us each), never a
// grid-wide barrier: a software barrier costs 26 us or more and can hang a shared device.  Kernel 2 has no third dependency because
// every workgroup recomputes the R + 2N dot products of its row (48 x 512 multiply-adds at d_model 256) from xc in LDS.
// Weights are the fp32 master tensors; a workgroup of kernels 1 / 3 holds up to ST_BT batch rows in LDS so that a weight row is read
// once per ST_BT rows.  A row's sums never depend on the other rows of the batch (fixed lane-strided order, xor-butterfly reduction).
// Rounding points (T = activation dtype): xz, xc, dbc, delta, y, out -- where the full-sequence path stores these tensors.
#pragma once
#include "cad_common.h"

namespace {

#define ST_WAVES 4
#define ST_THREADS (64 * ST_WAVES)
#define ST_BT 8        // batch rows per workgroup of the two projection kernels
#define ST_CH 16       // channels per workgroup of the state kernel: 16 lanes per channel
#define ST_KMAX 4
#define ST_NMAX 64
#define ST_WIDTH_MAX 2048  // d_model and d_inner: ST_BT rows of fp32 fit the 64 KB of LDS a plain launch may ask for

template <typename T>
__device__ __forceinline__ float st_round(float f) {  // the value a tensor stored in T gives back
    return to_f32(from_f32<T>(f));
}
__device__ __forceinline__ float st_wave_sum(float v) {  // every lane receives the sum (one fixed order)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ float st_silu(float x) { return x * cad_sigmoid(x); }

// acc[b] += <w[0:len], v[b][0:len]> over this lane's share (elements lane, lane + 64, ...) for the nb staged rows v (LDS, fp32)
__device__ __forceinline__ void st_row_dot(const float* __restrict__ w, const float* v, int len, int nb, int lane, float* acc) {
    for (int d = lane; d < len; d += 64) {
        const float wd = w[d];
#pragma unroll
        for (int b = 0; b < ST_BT; ++b)
            if (b < nb) acc[b] = __builtin_fmaf(wd, v[b * len + d], acc[b]);
    }
}

// stage rows [b0, b0 + nb) of src (B, len) as fp32 into LDS
template <typename T>
__device__ __forceinline__ void st_stage(const T* src, float* dst, int64_t b0, int nb, int len) {
    for (int i = threadIdx.x; i < nb * len; i += ST_THREADS) dst[i] = to_f32(src[b0 * len + i]);
}

// launch 1 behind the barrier that publishes the nb staged rows hs [nb][D] (fp32 values of T): shared by step_in_conv_kernel and by the
// decode token's variant that forms the rows itself (decode.hip)
template <typename T>
__device__ __forceinline__ void st_in_conv_rows(const cad_mamba_step_args& a, const float* hs, int64_t b0, int nb, float* xc_out,
                                                float* z_out) {
    const int D = a.D, E = a.E, K = a.K;
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * ST_WAVES + cad_uniform(threadIdx.x >> 6);
    if (e >= E) return;  // wave-uniform, behind the only barrier
    float ax[ST_BT], az[ST_BT];
#pragma unroll
    for (int b = 0; b < ST_BT; ++b) ax[b] = az[b] = 0.f;
    st_row_dot(a.W_in + (int64_t)e * D, hs, D, nb, lane, ax);
    st_row_dot(a.W_in + (int64_t)(E + e) * D, hs, D, nb, lane, az);
    float x = 0.f, z = 0.f;  // lane b keeps row b0 + b
#pragma unroll
    for (int b = 0; b < ST_BT; ++b) {
        if (b < nb) {  // wave-uniform
            const float sx = st_wave_sum(ax[b]), sz = st_wave_sum(az[b]);
            if (lane == b) x = sx, z = sz;
        }
    }
    if (lane >= nb) return;
    x = st_round<T>(x), z = st_round<T>(z);
    if (a.b_in) {  // the full-sequence path adds the bias, rounded to T, to the stored product
        x = st_round<T>(x + st_round<T>(a.b_in[e]));
        z = st_round<T>(z + st_round<T>(a.b_in[E + e]));
    }
    const int64_t row = (b0 + lane) * E + e;
    T* cs = (T*)a.conv_state + row * K;
    float win[ST_KMAX];
#pragma unroll
    for (int k = 0; k < ST_KMAX; ++k) win[k] = (k + 1 < K) ? to_f32(cs[k + 1]) : 0.f;  // the window shifted left by one
    float acc = a.conv_b ? a.conv_b[e] : 0.f;
#pragma unroll
    for (int k = 0; k < ST_KMAX; ++k) {
        if (k < K) {
            if (k == K - 1) win[k] = x;
            cs[k] = from_f32<T>(win[k]);
            acc = __builtin_fmaf(a.conv_w[(int64_t)e * K + k], win[k], acc);
        }
    }
    xc_out[row] = st_round<T>(st_silu(acc));
    z_out[row] = z;
}

template <typename T>
__global__ __launch_bounds__(ST_THREADS) void step_in_conv_kernel(cad_mamba_step_args a, float* xc_out, float* z_out) {
    CAD_DYN_SMEM(float, hs);  // [nb][D]
    const int64_t b0 = (int64_t)blockIdx.y * ST_BT;
    const int nb = (int)((a.B - b0) < ST_BT ? (a.B - b0) : ST_BT);
    st_stage<T>((const T*)a.h, hs, b0, nb, a.D);
    __syncthreads();
    st_in_conv_rows<T>(a, hs, b0, nb, xc_out, z_out);
}

template <typename T>
__global__ __launch_bounds__(ST_THREADS) void step_ssm_kernel(cad_mamba_step_args a, const float* xc_in, const float* z_in, float* y_out) {
    CAD_DYN_SMEM(float, sm);  // xc [E] | dbc [R + 2N]
    const int E = a.E, N = a.N, R = a.R, M = a.R + 2 * a.N;
    const int64_t b = blockIdx.y;
    float* xs = sm;
    float* dbc = sm + E;
    for (int i = threadIdx.x; i < E; i += ST_THREADS) xs[i] = xc_in[b * E + i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = cad_uniform(threadIdx.x >> 6);
    for (int j = wave; j < M; j += ST_WAVES) {  // wave-uniform trip count
        float s = 0.f;
        const float* w = a.W_x + (int64_t)j * E;
        for (int d = lane; d < E; d += 64) s = __builtin_fmaf(w[d], xs[d], s);
        s = st_wave_sum(s);
        if (lane == 0) dbc[j] = st_round<T>(s);
    }
    __syncthreads();
    // 16 lanes per channel: lane q of a group owns states n = q, q + 16, ...
    const int q = threadIdx.x & 15;
    const int e = blockIdx.x * ST_CH + (threadIdx.x >> 4);
    const bool live = e < E;
    float part = 0.f, xc = 0.f;
    if (live) {
        xc = xs[e];
        float delta = 0.f;
        for (int r = 0; r < R; ++r) delta = __builtin_fmaf(a.W_dt[(int64_t)e * R + r], dbc[r], delta);
        const float dt = cad_softplus(st_round<T>(delta) + a.dt_bias[e]);
        float* s = a.ssm_state + (b * E + e) * N;
        for (int n = q; n < N; n += 16) {
            const float A = -cad_exp(a.A_log[(int64_t)e * N + n]);
            const float hn = cad_exp2(dt * A * CAD_LOG2E) * s[n] + dt * dbc[R + n] * xc;
            s[n] = hn;
            part = __builtin_fmaf(dbc[R + N + n], hn, part);
        }
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) part += __shfl_xor(part, m);  // stays inside the 16-lane group; every lane takes part
    if (live && q == 0) {
        const float y = part + a.Dskip[e] * xc;
        y_out[b * E + e] = st_round<T>(y * st_silu(z_in[b * E + e]));
    }
}

template <typename T>
__global__ __launch_bounds__(ST_THREADS) void step_out_kernel(cad_mamba_step_args a, const float* y_in) {
    CAD_DYN_SMEM(float, ys);  // [nb][E]
    const int D = a.D, E = a.E;
    const int64_t b0 = (int64_t)blockIdx.y * ST_BT;
    const int nb = (int)((a.B - b0) < ST_BT ? (a.B - b0) : ST_BT);
    st_stage<float>(y_in, ys, b0, nb, E);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int d = blockIdx.x * ST_WAVES + cad_uniform(threadIdx.x >> 6);
    if (d >= D) return;  // wave-uniform, behind the only barrier
    float acc[ST_BT];
#pragma unroll
    for (int b = 0; b < ST_BT; ++b) acc[b] = 0.f;
    st_row_dot(a.W_out + (int64_t)d * E, ys, E, nb, lane, acc);
    float o = 0.f;
#pragma unroll
    for (int b = 0; b < ST_BT; ++b) {
        if (b < nb) {
            const float s = st_wave_sum(acc[b]);
            if (lane == b) o = s;
        }
    }
    if (lane >= nb) return;
    o = st_round<T>(o);
    if (a.b_out) o = st_round<T>(o + st_round<T>(a.b_out[d]));
    ((T*)a.out)[(b0 + lane) * D + d] = from_f32<T>(o);
}

}  // namespace
