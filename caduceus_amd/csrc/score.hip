// Score head (include/caduceus_hip.h, cad_lm_head_score): the LM head's logit row of a scored token, the log-sum-exp over the allowed
// ids and the log-probabilities, in one launch.  The logits never reach memory: what is written is logp (n) and / or logp_all (n, V).
// The logit row is cad_head.h's, the code cad_lm_head_fwd runs (csrc/lmhead.hip), on the rows `row_index` names (a gathered tile) or on
// rows 0 .. n - 1.
// No atomics and no shared memory: every output element has one writer, and a row's result does not depend on its neighbours.
#include "cad_head.h"

namespace {

#define SC_VMAX 16
#define SC_WAVES CAD_HEAD_WAVES

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
        float z[SC_VMAX];
        cad_head_row(z, hid + row * D, a.n_strands == 2 ? hid + (a.rows + row) * D : nullptr, a.weight, a.comp, D, V, lane);
        // every lane holds the whole row: z + mask, its maximum and the sum of exponentials in id order (the forward's lane 0 epilogue)
        if (a.logit_mask) {
#pragma unroll
            for (int v = 0; v < SC_VMAX; ++v)
                if (v < V) z[v] += a.logit_mask[v];
        }
        const float lse = cad_head_row_lse(z, V, -INFINITY);
        const float mine = cad_head_row_at(z, lane);  // lane v: z[v] + mask[v]
        const float out = bad ? NAN : mine - lse;
        if (a.logp_all && lane < V) a.logp_all[i * V + lane] = out;
        if (a.logp) {
            const int64_t t = a.targets[i];
            const bool counts = t != a.ignore_index && t >= 0 && t < V;
            if (counts ? (int64_t)lane == t : lane == 0) a.logp[i] = counts ? out : 0.f;
        }
    }
}

// Matrix-core path: cad_head_mfma_walk on tiles of 16 scored rows, which come from row_index when it is given.  Epilogue: maximum and sum
// of exponentials are reductions over the 16 lanes of a row.
template <typename T, int NJ>
__global__ __launch_bounds__(64 * SC_WAVES) void lm_score_mfma_kernel(cad_lm_score_args a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4, jl = lane & 15;
    const int V = a.V;
    const int64_t n = a.n;
    const float maskv = (a.logit_mask && jl < V) ? a.logit_mask[jl] : 0.f;
    cad_head_mfma_walk<T, NJ>(
        (const T*)a.hidden, a.rows, a.weight, a.comp, a.n_strands, V, (int64_t)blockIdx.x * SC_WAVES + wave, (int64_t)gridDim.x * SC_WAVES,
        (n + 15) / 16, lane,
        [&](int64_t tile) {
            int64_t i = tile * 16 + jl;
            i = i < n ? i : n - 1;  // tail tile: valid data, never stored
            bool bad;
            return sc_row_of(a, i, &bad);
        },
        [&](int64_t tile, const f32x4& z0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = tile * 16 + 4 * g + r;
                const bool ok = i < n;
                const float zm = jl < V ? z0[r] + maskv : -INFINITY;  // columns beyond V count as forbidden ids
                const float mx = cad_head_max16(zm);
                const float se = cad_head_sum16(jl < V ? expf(zm - mx) : 0.f);
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
        });
}

}  // namespace

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
    const bool mfma = cad_head_mfma_nj(a->D, a->dtype) && ((uintptr_t)a->hidden % 16) == 0;
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
    CAD_HEAD_LAUNCH(lm_score_mfma_kernel, lm_score_kernel, a->dtype, mfma ? a->D / 32 : 0, grid, block, 0, stream, *a);
    return cad_after_launch();
}
