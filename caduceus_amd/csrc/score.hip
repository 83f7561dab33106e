// Score head (include/caduceus_hip.h, cad_lm_head_score): the LM head's logit row of a scored token, the log-sum-exp over the allowed
// ids and the log-probabilities, in one launch.  The logits never reach memory: what is written is logp (n) and / or logp_all (n, V).
// The logit row is formed exactly as cad_lm_head_fwd forms it (csrc/lmhead.hip: the same lane-to-channel maps, fp32 accumulation, each
// strand's sum kept apart, then one commutative add), on the rows `row_index` names (a gathered tile) or on rows 0 .. n - 1.
// No atomics and no shared memory: every output element has one writer, and a row's result does not depend on its neighbours.
#include <math.h>

#include "cad_common.h"

namespace {

#define SC_VMAX 16
#define SC_WAVES 4

// the row of `hidden` that scored row i reads; *bad: the index lies outside [0, rows) -- nothing is read there and NaN is written
__device__ __forceinline__ int64_t sc_row_of(const cad_lm_score_args& a, int64_t i, bool* bad) {
    const int64_t row = a.row_index ? a.row_index[i] : i;
    *bad = row < 0 || row >= a.rows;
    return *bad ? 0 : row;
}

// General path: one wave per scored row, any D.
template <typename T>
__global__ __launch_bounds__(64 * SC_WAVES) void lm_score_kernel(cad_lm_score_args a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int D = a.D, V = a.V;
    const T* hid = (const T*)a.hidden;
    for (int64_t i = (int64_t)blockIdx.x * SC_WAVES + wave; i < a.n; i += (int64_t)gridDim.x * SC_WAVES) {
        bool bad;
        const int64_t row = sc_row_of(a, i, &bad);
        float acc[SC_VMAX], acc1[SC_VMAX];
#pragma unroll
        for (int v = 0; v < SC_VMAX; ++v) acc[v] = acc1[v] = 0.f;
        {
            const T* h = hid + row * D;
            for (int c = lane; c < D; c += 64) {
                const float hv = to_f32(h[c]);
#pragma unroll
                for (int v = 0; v < SC_VMAX; ++v)
                    if (v < V) acc[v] += hv * a.weight[(int64_t)v * D + c];
            }
        }
        if (a.n_strands == 2) {
            const T* h = hid + (a.rows + row) * D;
            for (int c = lane; c < D; c += 64) {
                const float hv = to_f32(h[c]);
#pragma unroll
                for (int v = 0; v < SC_VMAX; ++v)
                    if (v < V) acc1[v] += hv * a.weight[a.comp[v] * D + c];
            }
#pragma unroll
            for (int v = 0; v < SC_VMAX; ++v) acc[v] = acc[v] + acc1[v];
        }
#pragma unroll
        for (int v = 0; v < SC_VMAX; ++v) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) acc[v] += __shfl_xor(acc[v], m);
        }
        // every lane holds the whole row: z + mask, its maximum and the sum of exponentials in id order (the forward's lane 0 epilogue)
        float mx = -INFINITY;
#pragma unroll
        for (int v = 0; v < SC_VMAX; ++v) {
            if (v < V) {
                if (a.logit_mask) acc[v] += a.logit_mask[v];
                mx = acc[v] > mx ? acc[v] : mx;
            }
        }
        float se = 0.f;
#pragma unroll
        for (int v = 0; v < SC_VMAX; ++v)
            if (v < V) se += expf(acc[v] - mx);
        const float lse = logf(se) + mx;
        float mine = 0.f;  // lane v: z[v] + mask[v]
#pragma unroll
        for (int v = 0; v < SC_VMAX; ++v)
            if (lane == v) mine = acc[v];
        const float out = bad ? NAN : mine - lse;
        if (a.logp_all && lane < V) a.logp_all[i * V + lane] = out;
        if (a.logp) {
            const int64_t t = a.targets[i];
            const bool counts = t != a.ignore_index && t >= 0 && t < V;
            if (counts ? (int64_t)lane == t : lane == 0) a.logp[i] = counts ? out : 0.f;
        }
    }
}

// Matrix-core path (D = 32 NJ, NJ in {4, 8, 16}): lm_head_fwd_mfma_kernel's tile product -- v_mfma_f32_16x16x4_f32 on 16 scored rows,
// MFMA number 8 j + e takes element k = 8 g + 32 j + e from lane (row or vocabulary row jl, k-group g), so both operands are 16-byte
// loads; W stays in registers across the tiles a wave walks; strand 1's tile uses the same W registers and has its columns permuted by
// comp before the one add.  A tile's 16 rows come from row_index when it is given.  Epilogue: lane (column jl, rows 4 g + r) holds one
// logit of four rows; maximum and sum of exponentials are reductions over the 16 lanes of a row.
template <typename T, int NJ>
__global__ __launch_bounds__(64 * SC_WAVES) void lm_score_mfma_kernel(cad_lm_score_args a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4, jl = lane & 15;
    constexpr int D = 32 * NJ;
    constexpr int WPT = sizeof(T) * 8 / 4;  // 32-bit words per 8 elements
    struct __attribute__((aligned(16))) Raw { uint32_t w[WPT]; };
    const int V = a.V;
    const T* hid = (const T*)a.hidden;
    const int64_t rows = a.rows, n = a.n;
    const int64_t ntiles = (n + 15) / 16;
    float wreg[NJ][8];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) wreg[j][e] = jl < V ? a.weight[(int64_t)jl * D + 8 * g + 32 * j + e] : 0.f;
    const int cv = (a.n_strands == 2 && jl < V) ? (int)a.comp[jl] : jl;  // the column of strand 1's tile that feeds logit jl
    const int src = (lane & 48) | cv;
    const float maskv = (a.logit_mask && jl < V) ? a.logit_mask[jl] : 0.f;
    auto tile_row = [&](int64_t tile) {
        int64_t i = tile * 16 + jl;
        i = i < n ? i : n - 1;  // tail tile: valid data, never stored
        bool bad;
        return sc_row_of(a, i, &bad);
    };
    auto load_tile = [&](int64_t row, int s, Raw* dst) {
        const T* h = hid + ((int64_t)s * rows + row) * D + 8 * g;
#pragma unroll
        for (int j = 0; j < NJ; ++j) dst[j] = *(const Raw*)(h + 32 * j);
    };
    auto unpack = [&](const Raw& r, float* o) {
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                o[2 * q] = cad_lo2f<T>(r.w[q]);
                o[2 * q + 1] = cad_hi2f<T>(r.w[q]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) o[q] = cad_bits2f(r.w[q]);
        }
    };
    const int64_t tstep = (int64_t)gridDim.x * SC_WAVES;
    int64_t tile = (int64_t)blockIdx.x * SC_WAVES + wave;
    Raw h0[NJ], h1[NJ];
    if (tile < ntiles) {
        const int64_t row = tile_row(tile);
        load_tile(row, 0, h0);
        if (a.n_strands == 2) load_tile(row, 1, h1);
    }
    for (; tile < ntiles; tile += tstep) {
        const bool more = tile + tstep < ntiles;
        const int64_t nrow = more ? tile_row(tile + tstep) : 0;
        f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float hv[8];
            unpack(h0[j], hv);
#pragma unroll
            for (int e = 0; e < 8; ++e) z0 = cad_mfma_16x16x4_f32(hv[e], wreg[j][e], z0);
        }
        if (more) load_tile(nrow, 0, h0);  // the next tile's strand 0 in flight under strand 1's MFMAs
        if (a.n_strands == 2) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float hv[8];
                unpack(h1[j], hv);
#pragma unroll
                for (int e = 0; e < 8; ++e) z1 = cad_mfma_16x16x4_f32(hv[e], wreg[j][e], z1);
            }
            if (more) load_tile(nrow, 1, h1);
#pragma unroll
            for (int r = 0; r < 4; ++r) z0[r] = z0[r] + __shfl(z1[r], src);
        }
        // lane (column jl, rows 4 g + r): id jl of scored rows tile * 16 + 4 g + r
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = tile * 16 + 4 * g + r;
            const bool ok = i < n;
            const float zm = jl < V ? z0[r] + maskv : -INFINITY;  // columns beyond V count as forbidden ids
            float mx = zm;
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) {
                const float o = __shfl_xor(mx, m);
                mx = o > mx ? o : mx;
            }
            float se = jl < V ? expf(zm - mx) : 0.f;
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) se += __shfl_xor(se, m);
            bool bad = false;
            if (ok) sc_row_of(a, i, &bad);
            const float out = bad ? NAN : zm - (logf(se) + mx);
            if (a.logp_all && ok && jl < V) a.logp_all[i * V + jl] = out;
            if (a.logp && ok) {
                const int64_t t = a.targets[i];
                const bool counts = t != a.ignore_index && t >= 0 && t < V;
                if (counts ? (int64_t)jl == t : jl == 0) a.logp[i] = counts ? out : 0.f;
            }
        }
    }
}

}  // namespace

// (the forward's rule: W resident in 32 / 64 VGPRs, d_model 512 with 128 in bf16 only)
static bool lm_score_mfma(int D, int dtype) { return D == 128 || D == 256 || (D == 512 && dtype == CAD_BF16); }

extern "C" int cad_lm_head_score_supported(int D, int V, int dtype) {
    return D >= 1 && V >= 1 && V <= SC_VMAX && (dtype == CAD_F32 || dtype == CAD_BF16 || dtype == CAD_F16);
}

extern "C" int cad_lm_head_score(const cad_lm_score_args* a, void* stream) {
    CAD_CHECK_ARG(a && a->hidden && a->weight && (a->logp || a->logp_all));
    CAD_CHECK_ARG(a->rows > 0 && a->n > 0 && a->D > 0 && a->V > 0);
    CAD_CHECK_ARG(a->n_strands == 1 || (a->n_strands == 2 && a->comp));
    CAD_CHECK_ARG(!a->logp || a->targets);
    CAD_CHECK_ARG(a->row_index || a->n <= a->rows);
    if (!cad_lm_head_score_supported(a->D, a->V, a->dtype)) return CAD_ERR_UNSUPPORTED;
    CadProfScope prof(7, stream);
    const bool mfma = lm_score_mfma(a->D, a->dtype) && ((uintptr_t)a->hidden % 16) == 0;
    int64_t nb;
    if (mfma) {  // two workgroups per CU at most: a wave walks several tiles with its W registers, as in the forward
        nb = ((a->n + 15) / 16 + SC_WAVES - 1) / SC_WAVES;
        const int64_t cap = 2 * (int64_t)cad_cu_count();
        nb = nb > cap ? cap : nb;
    } else {
        nb = (a->n + SC_WAVES - 1) / SC_WAVES;
        nb = nb > 4096 ? 4096 : nb;
    }
    dim3 grid((unsigned)nb), block(64 * SC_WAVES);
#define SC_MFMA(NJ_)                                                                           \
    do {                                                                                       \
        if (a->dtype == CAD_F32)                                                               \
            CAD_LAUNCH((lm_score_mfma_kernel<float, NJ_>), grid, block, 0, stream, *a);        \
        else if (a->dtype == CAD_F16)                                                          \
            CAD_LAUNCH((lm_score_mfma_kernel<f16_t, NJ_>), grid, block, 0, stream, *a);        \
        else                                                                                   \
            CAD_LAUNCH((lm_score_mfma_kernel<bf16_t, NJ_>), grid, block, 0, stream, *a);       \
    } while (0)
    if (mfma && a->D == 128)
        SC_MFMA(4);
    else if (mfma && a->D == 256)
        SC_MFMA(8);
    else if (mfma)
        CAD_LAUNCH((lm_score_mfma_kernel<bf16_t, 16>), grid, block, 0, stream, *a);
    else if (a->dtype == CAD_F32)
        CAD_LAUNCH((lm_score_kernel<float>), grid, block, 0, stream, *a);
    else if (a->dtype == CAD_F16)
        CAD_LAUNCH((lm_score_kernel<f16_t>), grid, block, 0, stream, *a);
    else
        CAD_LAUNCH((lm_score_kernel<bf16_t>), grid, block, 0, stream, *a);
#undef SC_MFMA
    return cad_after_launch();
}
