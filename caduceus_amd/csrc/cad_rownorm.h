// Add + RMSNorm / LayerNorm of ONE row by one wave64: the home of the row -- its lane maps, its loads, its statistics, its
// scale and where it rounds.  The pool head and its backward (pool.hip, pool_bwd.hip) are compiled from these routines, so the y the
// backward's MAX search recomputes is the forward's, bit for bit.  Two restatements remain and must be kept in step with this file: the
// forward kernels of addnorm.hip, which this order is taken from, and cad_row_norm_lds at the end of this file (decode.hip).
//
// A lane owns W channels per step of 64 W: W = 4 consecutive channels where D % 4 == 0 and the operands are 16-byte aligned (the vector
// map), W = 1 otherwise (the scalar map).  A lane sums its channels in ascending order, the lanes are combined by the xor butterfly
// 32, 16, .. 1, and the LayerNorm variance is the second pass over (v - mean).
#pragma once
#include "cad_common.h"

__device__ __forceinline__ float cad_row_wave_sum(float v) {  // every lane receives the sum
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// channels per lane and step of a row whose operands are aligned
__device__ __forceinline__ int cad_row_width(int D) { return (D & 3) ? 1 : 4; }

// first channel of lane's step k
template <int W>
__device__ __forceinline__ int cad_row_chan(int lane, int k) { return (lane + 64 * k) * W; }

// W channels of T at p -> fp32
template <typename T, int W>
__device__ __forceinline__ void cad_row_ld(const T* p, float* o) {
    if constexpr (W == 1) {
        o[0] = to_f32(p[0]);
    } else if constexpr (sizeof(T) == 4) {
        struct __attribute__((aligned(16))) V { float f[4]; };
        const V t = *(const V*)p;
        o[0] = t.f[0], o[1] = t.f[1], o[2] = t.f[2], o[3] = t.f[3];
    } else {
        cad_ld4_16<T>(p, o);
    }
}

// mean (0 for RMSNorm) and rstd of the row v = x + residual held in registers (zeros beyond D)
template <int W, int KMAX>
__device__ __forceinline__ void cad_row_stats(const float (&v)[KMAX][W], int D, float eps, int is_rms, int lane, float& mean, float& rstd) {
    const float invD = 1.0f / (float)D;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (cad_row_chan<W>(lane, k) < D) {
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const float t = v[k][q];
                s1 += t;
                s2 += t * t;
            }
        }
    }
    mean = 0.f;
    if (is_rms) {
        s2 = cad_row_wave_sum(s2);
        rstd = cad_rsqrt(s2 * invD + eps);
    } else {
        s1 = cad_row_wave_sum(s1);
        mean = s1 * invD;
        float qq = 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (cad_row_chan<W>(lane, k) < D) {
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    const float d = v[k][q] - mean;
                    qq += d * d;
                }
            }
        }
        qq = cad_row_wave_sum(qq);
        rstd = cad_rsqrt(qq * invD + eps);
    }
}

// the normed value before it is rounded.  The vector map adds its bias register, zero when there is no bias; the scalar map adds the
// bias only when there is one (the compiler may contract the two differently, and -0 + 0 is not -0)
template <int W>
__device__ __forceinline__ float cad_row_scale(float v, float mean, float rstd, float w, float b, bool has_bias) {
    if (W == 4) return (v - mean) * rstd * w + b;
    float o = (v - mean) * rstd * w;
    if (has_bias) o += b;
    return o;
}

// the value a store of o in T leaves in memory
template <typename T>
__device__ __forceinline__ float cad_row_stored(float o) { return to_f32(from_f32<T>(o)); }

// v = x + residual of one row in registers, in place -> the normed row as a store in TY leaves it (cad_add_norm_fwd's y, swap_flip = 0)
template <typename TY, int W, int KMAX>
__device__ __forceinline__ void cad_row_norm(float (&v)[KMAX][W], const float (&wreg)[KMAX][W], const float (&breg)[KMAX][W], bool has_bias,
                                             int D, float eps, int is_rms, int lane) {
    float mean, rstd;
    cad_row_stats<W, KMAX>(v, D, eps, is_rms, lane, mean, rstd);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (cad_row_chan<W>(lane, k) < D) {
#pragma unroll
            for (int q = 0; q < W; ++q) v[k][q] = cad_row_stored<TY>(cad_row_scale<W>(v[k][q], mean, rstd, wreg[k][q], breg[k][q], has_bias));
        }
    }
}

// The same for a row held as fp32 in LDS with a run-time D (decode.hip): row[c] (the summed residual stream) -> row[c] = the normed
// activation as a store in T leaves it.  All 64 lanes of the wave call this; the caller orders the LDS accesses of other waves around it.
// Stated separately from the routines above, over a run-time W with rolled loops: compiled from them the one-token kernels keep
// neither their bits nor their registers.  A change to the order above is a change to make here as well.
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

// ---- host side: the served (x_dtype, y_dtype) pairs, written once ----------------------------------------------------------------
template <typename T>
struct cad_type_tag {
    typedef T type;
};

// f(cad_type_tag<TX>, cad_type_tag<TY>) for the pair's element types; false, and f not called, where the pair is not served
template <typename F>
inline bool cad_row_type_pair(int x_dtype, int y_dtype, F&& f) {
    if (x_dtype == CAD_F32 && y_dtype == CAD_F32)
        f(cad_type_tag<float>(), cad_type_tag<float>());
    else if (x_dtype == CAD_F32 && y_dtype == CAD_BF16)
        f(cad_type_tag<float>(), cad_type_tag<bf16_t>());
    else if (x_dtype == CAD_BF16 && y_dtype == CAD_BF16)
        f(cad_type_tag<bf16_t>(), cad_type_tag<bf16_t>());
    else if (x_dtype == CAD_F32 && y_dtype == CAD_F16)
        f(cad_type_tag<float>(), cad_type_tag<f16_t>());
    else if (x_dtype == CAD_F16 && y_dtype == CAD_F16)
        f(cad_type_tag<f16_t>(), cad_type_tag<f16_t>());
    else
        return false;
    return true;
}
inline bool cad_row_types_ok(int x_dtype, int y_dtype) {
    return cad_row_type_pair(x_dtype, y_dtype, [](auto, auto) {});
}
