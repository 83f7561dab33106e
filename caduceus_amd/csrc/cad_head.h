// The LM head's logit row, stated once for the kernels that form it: cad_lm_head_fwd (lmhead.hip), cad_lm_head_score (score.hip), the
// tail of cad_decode_token (decode.hip) and cad_lm_head_unmask (unmask.hip).
//   z[v] = <h0, W[v]> + <h1, W[comp v]>     fp32 accumulation, each strand's sum kept apart, then ONE commutative add per logit: logits(x)[v]
//                                           and logits(RC x)[comp v] (strand roles exchanged) are the same two numbers added, bit for bit,
//                                           like the reference's `fwd_logits + rc_logits` (modeling_rcps.py:240-246)
// followed by the row maximum and the log-sum-exp.  Two lane maps: the scalar row (one wave per row, any D) and the matrix-core tile
// (16 rows per wave, D = 32 NJ).  A sequence log-likelihood equals what the training loss saw because both go through this file.
#pragma once
#include <math.h>

#include "cad_common.h"
#include "cad_rownorm.h"

// ---- scalar row: one wave64 per row, lane l takes channels l + 64 k in ascending order ------------------------------------------------
// z[v], v < V, on every lane (the lanes are combined by cad_row_wave_sum's butterfly, per id).  h1 = NULL: one strand.  T is the stored
// activation in global memory, or float for a row held in LDS (the decode tail).
template <int VMAX, typename T>
__device__ __forceinline__ void cad_head_row(float (&z)[VMAX], const T* h0, const T* h1, const float* weight, const int64_t* comp, int D, int V,
                                             int lane) {
    float z1[VMAX];
#pragma unroll
    for (int v = 0; v < VMAX; ++v) z[v] = z1[v] = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float hv = to_f32(h0[c]);
#pragma unroll
        for (int v = 0; v < VMAX; ++v)
            if (v < V) z[v] += hv * weight[(int64_t)v * D + c];
    }
    if (h1) {
        for (int c = lane; c < D; c += 64) {
            const float hv = to_f32(h1[c]);
#pragma unroll
            for (int v = 0; v < VMAX; ++v)
                if (v < V) z1[v] += hv * weight[comp[v] * D + c];
        }
#pragma unroll
        for (int v = 0; v < VMAX; ++v) z[v] = z[v] + z1[v];
    }
#pragma unroll
    for (int v = 0; v < VMAX; ++v)
        z[v] = cad_row_wave_sum(z[v]);
}

// log-sum-exp of z[0 .. V) in id order; mx = the caller's starting maximum (it decides what a row without a finite logit gives)
template <int VMAX>
__device__ __forceinline__ float cad_head_row_lse(const float (&z)[VMAX], int V, float mx) {
#pragma unroll
    for (int v = 0; v < VMAX; ++v)
        if (v < V) mx = z[v] > mx ? z[v] : mx;
    float se = 0.f;
#pragma unroll
    for (int v = 0; v < VMAX; ++v)
        if (v < V) se += expf(z[v] - mx);
    return logf(se) + mx;
}

// z[i] without a dynamically indexed register array (0 outside [0, VMAX)): lane v's own logit, or the label's
template <int VMAX>
__device__ __forceinline__ float cad_head_row_at(const float (&z)[VMAX], int64_t i) {
    float r = 0.f;
#pragma unroll
    for (int v = 0; v < VMAX; ++v)
        if (v == i) r = z[v];
    return r;
}

// ---- matrix-core tile (D = 32 NJ, NJ in {4, 8, 16}: d_model 128 / 256 / 512) ----------------------------------------------------------
// A wave owns 16-row tiles: logits (16 x 16) = H (16 x D) . W^T with v_mfma_f32_16x16x4_f32 -- fp32 operands, so W stays the fp32 master
// weight -- one accumulator tile per strand.  The k axis is walked in a permuted order that makes both operands 16-byte vector loads:
// MFMA number 8 j + e takes, from lane (row or vocabulary row jl = lane & 15, k-group g = lane >> 4), element k = 8 g + 32 j + e.
// W (8 NJ floats per lane) is loaded once per wave and serves every tile it walks (tile, tile + tstep, .. < ntiles).  RCPS: the second
// strand's tile is computed with the SAME W registers and its columns are permuted by comp afterwards (ds_bpermute), then the one add.
// row_of(tile) names the row of `hid` (rows x D per strand) that this lane loads for the tile, i.e. the tile's row jl; a tail tile
// names valid rows that the caller never stores.  epilogue(tile, z): lane (column jl, rows 4 g + r) holds logit jl of the tile's rows
// 4 g + r in z[r].  The next tile's strand 0 is in flight under strand 1's MFMAs, its strand 1 under the epilogue.
// take(tile): wave-uniform; a tile it declines is neither loaded nor multiplied nor handed to the epilogue (whatever such a tile owes its
// outputs is take's own to write), and the prefetch goes to the next tile of the walk that is taken.
template <typename T, int NJ, typename Take, typename RowOf, typename Epilogue>
__device__ __forceinline__ void cad_head_mfma_walk_if(const T* hid, int64_t rows, const float* weight, const int64_t* comp, int n_strands, int V,
                                                      int64_t tile, int64_t tstep, int64_t ntiles, int lane, Take take, RowOf row_of,
                                                      Epilogue epilogue) {
    const int g = lane >> 4, jl = lane & 15;
    constexpr int D = 32 * NJ;
    constexpr int WPT = sizeof(T) * 8 / 4;  // 32-bit words per 8 elements
    struct __attribute__((aligned(16))) Raw { uint32_t w[WPT]; };
    float wreg[NJ][8];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) wreg[j][e] = jl < V ? weight[(int64_t)jl * D + 8 * g + 32 * j + e] : 0.f;
    const int cv = (n_strands == 2 && jl < V) ? (int)comp[jl] : jl;  // the column of strand 1's tile that feeds logit jl
    const int src = (lane & 48) | cv;
    auto load_tile = [&](int64_t row, int s, Raw* dst) {
        const T* h = hid + ((int64_t)s * rows + row) * D + 8 * g;
#pragma unroll
        for (int j = 0; j < NJ; ++j) dst[j] = *(const Raw*)(h + 32 * j);
    };
    auto product = [&](const Raw* h) {
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float hv[8];
            if constexpr (sizeof(T) == 2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    hv[2 * q] = cad_lo2f<T>(h[j].w[q]);
                    hv[2 * q + 1] = cad_hi2f<T>(h[j].w[q]);
                }
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) hv[q] = cad_bits2f(h[j].w[q]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) z = cad_mfma_16x16x4_f32(hv[e], wreg[j][e], z);
        }
        return z;
    };
    auto next_taken = [&](int64_t t) {
        while (t < ntiles && !take(t)) t += tstep;
        return t;
    };
    Raw h0[NJ], h1[NJ];
    tile = next_taken(tile);
    if (tile < ntiles) {
        const int64_t row = row_of(tile);
        load_tile(row, 0, h0);
        if (n_strands == 2) load_tile(row, 1, h1);
    }
    for (int64_t next; tile < ntiles; tile = next) {
        next = next_taken(tile + tstep);
        const bool more = next < ntiles;
        const int64_t nrow = more ? row_of(next) : 0;
        f32x4 z0 = product(h0);
        if (more) load_tile(nrow, 0, h0);
        if (n_strands == 2) {
            const f32x4 z1 = product(h1);
            if (more) load_tile(nrow, 1, h1);
#pragma unroll
            for (int r = 0; r < 4; ++r) z0[r] = z0[r] + __shfl(z1[r], src);
        }
        epilogue(tile, z0);
    }
}
// every tile of the walk (tile, tile + tstep, .. < ntiles)
template <typename T, int NJ, typename RowOf, typename Epilogue>
__device__ __forceinline__ void cad_head_mfma_walk(const T* hid, int64_t rows, const float* weight, const int64_t* comp, int n_strands, int V,
                                                   int64_t tile, int64_t tstep, int64_t ntiles, int lane, RowOf row_of, Epilogue epilogue) {
    cad_head_mfma_walk_if<T, NJ>(hid, rows, weight, comp, n_strands, V, tile, tstep, ntiles, lane, [](int64_t) { return true; }, row_of,
                                 epilogue);
}

// reductions over the 16 lanes that hold one row of a tile (xor butterfly 8 .. 1; every lane of the row receives the result)
__device__ __forceinline__ float cad_head_max16(float v) {
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
        const float o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ float cad_head_sum16(float v) {
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
#define CAD_HEAD_WAVES 4  // waves per workgroup: rows (scalar row) or tiles (matrix cores) in flight

// NJ of the matrix-core kernel, or 0 for the scalar row.  W resident in registers: 32 / 64 VGPRs; d_model 512 (configs[4]) with 128, in
// bf16 only (363 registers, one wave per SIMD: the fp32 instantiation would spill).  The callers add what is theirs: the forward takes
// this path for a 32-byte aligned hidden and caps its grid at 512 workgroups (its loss slots are sized from rows alone); the score takes
// it for a 16-byte aligned one and caps at two workgroups per CU.
static inline int cad_head_mfma_nj(int D, int dtype) { return (D == 128 || D == 256 || (D == 512 && dtype == CAD_BF16)) ? D / 32 : 0; }

// dtype x NJ dispatch: MFMA<T, nj> for nj in {4, 8, 16}, GEN<T> for nj = 0; the trailing arguments are CAD_LAUNCH's after the kernel
#define CAD_HEAD_LAUNCH_T(MFMA, GEN, T, nj, ...)                   \
    do {                                                           \
        if ((nj) == 4)                                             \
            CAD_LAUNCH((MFMA<T, 4>), __VA_ARGS__);                 \
        else if ((nj) == 8)                                        \
            CAD_LAUNCH((MFMA<T, 8>), __VA_ARGS__);                 \
        else                                                       \
            CAD_LAUNCH((GEN<T>), __VA_ARGS__);                     \
    } while (0)
#define CAD_HEAD_LAUNCH(MFMA, GEN, dtype, nj, ...)                 \
    do {                                                           \
        if ((nj) == 16)                                            \
            CAD_LAUNCH((MFMA<bf16_t, 16>), __VA_ARGS__);           \
        else if ((dtype) == CAD_F32)                               \
            CAD_HEAD_LAUNCH_T(MFMA, GEN, float, nj, __VA_ARGS__);  \
        else if ((dtype) == CAD_F16)                               \
            CAD_HEAD_LAUNCH_T(MFMA, GEN, f16_t, nj, __VA_ARGS__);  \
        else                                                       \
            CAD_HEAD_LAUNCH_T(MFMA, GEN, bf16_t, nj, __VA_ARGS__); \
    } while (0)
