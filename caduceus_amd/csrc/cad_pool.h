// What the pool head's forward (pool.hip) and backward (pool_bwd.hip) share: the lane maps and their loads, the normed row (pool_row),
// the window's span and multiplicities (pool_span_of), torch.max's maximum, the served type pairs and the forward's piece geometry.
// pool.hip's header describes all of it; nothing here is compiled for one of the two files only, so that the y the backward's MAX
// search recomputes is the forward's, bit for bit.
#pragma once
#include "cad_common.h"
#include "cad_rownorm.h"

namespace {

#define POOL_WAVES 4
#define POOL_UNROLL 2
#define POOL_CHUNK (POOL_WAVES * POOL_UNROLL)  // items (pairs of rows) per workgroup iteration
#define POOL_PIECES_MAX 256                    // partial rows per (s, b)
#define POOL_DMAX 1024
#define POOL_HALF_MAX ((int64_t)1 << 22)       // 2 half + 1 < 2^24: every multiplicity is an exact fp32 integer

struct pool_geom {
    int64_t cpp;     // chunks per piece
    int64_t pieces;  // partial rows per (s, b)
};

// n rows (n >= 1), (n + 1) / 2 items -> chunks per piece and pieces
inline pool_geom pool_geometry(int64_t n) {
    const int64_t chunks = ((n + 1) / 2 + POOL_CHUNK - 1) / POOL_CHUNK;
    pool_geom g;
    g.cpp = (chunks + POOL_PIECES_MAX - 1) / POOL_PIECES_MAX;
    g.pieces = (chunks + g.cpp - 1) / g.cpp;
    return g;
}

// upper bound, known on the host, of the rows a pair pools
inline int64_t pool_rows(int mode, int64_t L, int64_t half) {
    if (mode != CAD_POOL_WINDOW) return L;
    const int64_t n = 2 * half + 1;
    return n < L ? n : L;
}

// W channels at p -> fp32
template <typename T, int W>
__device__ __forceinline__ void pool_ld(const T* p, float* o);
template <>
__device__ __forceinline__ void pool_ld<float, 1>(const float* p, float* o) { o[0] = p[0]; }
template <>
__device__ __forceinline__ void pool_ld<bf16_t, 1>(const bf16_t* p, float* o) { o[0] = to_f32(p[0]); }
template <>
__device__ __forceinline__ void pool_ld<f16_t, 1>(const f16_t* p, float* o) { o[0] = to_f32(p[0]); }
template <>
__device__ __forceinline__ void pool_ld<float, 4>(const float* p, float* o) {
    struct __attribute__((aligned(16))) V { float f[4]; };
    const V t = *(const V*)p;
    o[0] = t.f[0], o[1] = t.f[1], o[2] = t.f[2], o[3] = t.f[3];
}
template <>
__device__ __forceinline__ void pool_ld<bf16_t, 4>(const bf16_t* p, float* o) { cad_ld4_16<bf16_t>(p, o); }
template <>
__device__ __forceinline__ void pool_ld<f16_t, 4>(const f16_t* p, float* o) { cad_ld4_16<f16_t>(p, o); }

// first channel of lane's step k
template <int W>
__device__ __forceinline__ int pool_chan(int lane, int k) { return (lane + 64 * k) * W; }

// v = x + residual of one row, in place -> the normed row as a store in TY leaves it (cad_add_norm_fwd's y, see the header of pool.hip)
template <typename TY, int W, int KMAX>
__device__ __forceinline__ void pool_row(float (&v)[KMAX][W], const float (&wreg)[KMAX][W], const float (&breg)[KMAX][W], bool has_bias,
                                         int D, float eps, int is_rms, int lane) {
    const float invD = 1.0f / (float)D;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (pool_chan<W>(lane, k) < D) {
#pragma unroll
            for (int q = 0; q < W; ++q) {
                s1 += v[k][q];
                s2 += v[k][q] * v[k][q];
            }
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
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (pool_chan<W>(lane, k) < D) {
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
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (pool_chan<W>(lane, k) < D) {
#pragma unroll
            for (int q = 0; q < W; ++q) {
                float o;
                if (W == 4) {  // the vector kernel adds its bias registers, zeros when there is no bias
                    o = (v[k][q] - mean) * rstd * wreg[k][q] + breg[k][q];
                } else {
                    o = (v[k][q] - mean) * rstd * wreg[k][q];
                    if (has_bias) o += breg[k][q];
                }
                v[k][q] = to_f32(from_f32<TY>(o));
            }
        }
    }
}

// torch.max's maximum: a NaN on either side stays (v_max_f32 would drop it)
__device__ __forceinline__ float pool_max(float acc, float y) {
    if (acc != acc) return acc;
    if (y != y) return y;
    return y > acc ? y : acc;
}

// the rows lo .. hi a pair pools and the multiplicities of rows 0 and L - 1 (every row between counts once)
struct pool_span {
    int64_t lo, hi;
    float c_first, c_last;  // of row 0 and of row L - 1
};

__device__ __forceinline__ pool_span pool_span_of(int mode, int64_t L, int64_t half, const int64_t* centre, int64_t sb) {
    pool_span w;
    if (mode != CAD_POOL_WINDOW) {
        w.lo = 0, w.hi = L - 1, w.c_first = 1.f, w.c_last = 1.f;
        return w;
    }
    // offsets k = -half .. half around centre c, clamp(c + k, 0, L - 1): a centre further out than half + 1 beyond an end puts every
    // offset on that end, as half + 1 beyond it does (no int64 overflow of c +- half)
    int64_t c = centre[sb];
    c = c < -half - 1 ? -half - 1 : (c > L + half ? L + half : c);
    const int64_t lo = c - half, hi = c + half, last = L - 1;
    w.lo = lo < 0 ? 0 : (lo > last ? last : lo);
    w.hi = hi < 0 ? 0 : (hi > last ? last : hi);
    if (last == 0) {  // one row takes every offset
        w.c_first = (float)(2 * half + 1), w.c_last = 0.f;
        return w;
    }
    const int64_t n_first = (hi < 0 ? hi : 0) - lo + 1;       // offsets landing at or before row 0
    const int64_t n_last = hi - (lo > last ? lo : last) + 1;  // offsets landing at or beyond row L - 1
    w.c_first = (float)(n_first > 0 ? n_first : 0);
    w.c_last = (float)(n_last > 0 ? n_last : 0);
    return w;
}

// the multiplicity of row r of a pair with span w (L == 1: row 0 is also row L - 1 and c_last is 0); rows outside lo .. hi are not asked
__device__ __forceinline__ float pool_mult(const pool_span& w, int64_t r, int64_t L) {
    return r == 0 ? w.c_first : (r == L - 1 ? w.c_last : 1.f);
}

inline bool pool_types_ok(int x_dtype, int y_dtype) {  // cad_add_norm_fwd's pairs
    return (x_dtype == CAD_F32 && (y_dtype == CAD_F32 || y_dtype == CAD_BF16 || y_dtype == CAD_F16)) ||
           (x_dtype == CAD_BF16 && y_dtype == CAD_BF16) || (x_dtype == CAD_F16 && y_dtype == CAD_F16);
}

// the lane map a call takes: the vector map where D % 4 == 0 and the row operands are 16-byte aligned
inline bool pool_vec(int D, const void* x, const void* residual_in, const void* weight, const void* bias) {
    return (D % 4) == 0 && (((uintptr_t)x | (uintptr_t)residual_in | (uintptr_t)weight | (uintptr_t)bias) % 16) == 0;
}

}  // namespace
