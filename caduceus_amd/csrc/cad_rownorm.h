// Add + RMSNorm / LayerNorm of ONE row by one wave64, the row held as fp32 in LDS: the row reduction of addnorm.hip restated for the
// one-token kernels (decode.hip).  The summation order is cad_add_norm_fwd's at one token: with D % 4 == 0 a lane owns 4 consecutive
// channels per 256-channel step (add_norm_fwd_vec_kernel, which 16-byte aligned operands take), otherwise channels lane + 64 k
// (add_norm_fwd_kernel); a lane sums its channels in ascending order, the lanes are combined by the xor butterfly 32, 16, .. 1, and the
// LayerNorm variance is the second pass over (v - mean).  Same order is not same bits on the device: where the compiler fuses a
// multiply into an add differs between the two translations, so a statistic may differ in its last bit ("Decode token").
// addnorm.hip takes cad_row_wave_sum from here; the per-lane walk below is a second statement of its forward kernels' and is kept in
// step with them by hand (they hold the row in registers and store through their own vector paths).
#pragma once
#include "cad_common.h"

__device__ __forceinline__ float cad_row_wave_sum(float v) {  // every lane receives the sum
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// channels per lane and step of the row walk
__device__ __forceinline__ int cad_row_width(int D) { return (D & 3) ? 1 : 4; }

// row[c] (the summed residual stream, fp32) -> row[c] = the normed activation as a store in T leaves it.  All 64 lanes of the wave call
// this; the caller orders the LDS accesses of other waves around it.
template <typename T>
__device__ __forceinline__ void cad_row_norm_lds(float* row, int D, const float* __restrict__ weight, const float* __restrict__ bias, float eps,
                                                 int is_rms, int lane) {
    const int W = cad_row_width(D);
    const float invD = 1.0f / (float)D;
    float s1 = 0.f, s2 = 0.f;
    for (int c0 = lane * W; c0 < D; c0 += 64 * W) {
        for (int q = 0; q < W; ++q) {
            const float t = row[c0 + q];
            s1 += t;
            s2 += t * t;
        }
    }
    float mean = 0.f, rstd;
    if (is_rms) {
        s2 = cad_row_wave_sum(s2);
        rstd = cad_rsqrt(s2 * invD + eps);
    } else {
        s1 = cad_row_wave_sum(s1);
        mean = s1 * invD;
        float qq = 0.f;
        for (int c0 = lane * W; c0 < D; c0 += 64 * W) {
            for (int q = 0; q < W; ++q) {
                const float d = row[c0 + q] - mean;
                qq += d * d;
            }
        }
        qq = cad_row_wave_sum(qq);
        rstd = cad_rsqrt(qq * invD + eps);
    }
    for (int c0 = lane * W; c0 < D; c0 += 64 * W) {
        for (int q = 0; q < W; ++q) {
            const int c = c0 + q;
            float o;
            if (W == 4) {
                const float b = bias ? bias[c] : 0.f;
                o = (row[c] - mean) * rstd * weight[c] + b;
            } else {
                o = (row[c] - mean) * rstd * weight[c];
                if (bias) o += bias[c];
            }
            row[c] = to_f32(from_f32<T>(o));
        }
    }
}
