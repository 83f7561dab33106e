// Attribution head (include/caduceus_hip.h, cad_embed_attrib): the gradient of a score with respect to the one-hot input sequence,
// straight from the gradient of the t-frame embedding output, in one launch.  With h0[b,l] = E[x] and h1[b,l] = E[comp x],
//   g[v] = d score / d onehot[b,l,v] = <dh0[b,l], E[v]> + <dh1[b,l], E[comp v]>
// is the LM head's logit row with dh as the hidden state and the embedding table as the weight: the row is cad_head.h's, the code
// cad_lm_head_fwd and cad_lm_head_score run.  What is written is grad (rows, A) -- g at the allowed ids, minus their mean when centred --
// and / or gxi (rows): that value at the row's own id.  Neither a (rows, V) tensor nor a reference-frame gradient reaches memory.
// No atomics and no shared memory: every output element has one writer, and a row's result does not depend on its neighbours.
#include "cad_head.h"

namespace {

#define AT_VMAX 16
#define AT_WAVES CAD_HEAD_WAVES

// bit v set: id v is allowed (entries outside [0, V) are dropped; the host checks the list it holds)
__device__ __forceinline__ unsigned at_allowed_bits(const cad_embed_attrib_args& a) {
    unsigned bits = 0;
    for (int k = 0; k < a.A; ++k) {
        const int64_t v = a.allowed[k];
        if (v >= 0 && v < a.V) bits |= 1u << (int)v;
    }
    return bits;
}

__device__ __forceinline__ bool at_id_allowed(unsigned bits, int64_t id, int V) { return id >= 0 && id < V && ((bits >> (int)id) & 1u); }

// General path: one wave per row, any D.  Every lane holds the whole row g[0 .. V).
template <typename T>
__global__ __launch_bounds__(64 * AT_WAVES) void embed_attrib_kernel(cad_embed_attrib_args a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int D = a.D, V = a.V, A = a.A;
    const T* dh = (const T*)a.dh;
    const unsigned bits = at_allowed_bits(a);
    const int64_t mine = lane < A ? a.allowed[lane] : -1;  // lane k: the id of column k of grad
    for (int64_t i = (int64_t)blockIdx.x * AT_WAVES + wave; i < a.rows; i += (int64_t)gridDim.x * AT_WAVES) {
        float g[AT_VMAX];
        cad_head_row(g, dh + i * D, a.n_strands == 2 ? dh + (a.rows + i) * D : nullptr, a.weight, a.comp, D, V, lane);
        float m = 0.f;
        if (a.centre) {  // the mean over the allowed ids, summed in ascending id order
            float s = 0.f;
#pragma unroll
            for (int v = 0; v < AT_VMAX; ++v)
                if ((bits >> v) & 1u) s += g[v];
            m = s / (float)A;
        }
        if (a.grad && lane < A) a.grad[i * A + lane] = cad_head_row_at(g, mine) - m;
        if (a.gxi && lane == 0) {
            const int64_t id = a.ids[i];
            a.gxi[i] = at_id_allowed(bits, id, V) ? cad_head_row_at(g, id) - m : 0.f;
        }
    }
}

// Matrix-core path: cad_head_mfma_walk on tiles of 16 consecutive rows.  Lane (column jl, rows 4 g + r) holds g[jl] of the tile's rows
// 4 g + r; the mean walks the 16 lanes of a row in ascending id order (the general path's order), and lane jl stores its own column.
template <typename T, int NJ>
__global__ __launch_bounds__(64 * AT_WAVES) void embed_attrib_mfma_kernel(cad_embed_attrib_args a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4, jl = lane & 15;
    const int V = a.V, A = a.A;
    const int64_t n = a.rows;
    const unsigned bits = at_allowed_bits(a);
    const bool col_allowed = (bits >> jl) & 1u;
    int col = 0;  // the column of grad that holds id jl: the number of allowed ids below it
#pragma unroll
    for (int v = 0; v < AT_VMAX; ++v)
        if (v < jl && ((bits >> v) & 1u)) ++col;
    cad_head_mfma_walk<T, NJ>(
        (const T*)a.dh, a.rows, a.weight, a.comp, a.n_strands, V, (int64_t)blockIdx.x * AT_WAVES + wave, (int64_t)gridDim.x * AT_WAVES,
        (n + 15) / 16, lane,
        [&](int64_t tile) {
            const int64_t i = tile * 16 + jl;
            return i < n ? i : n - 1;  // tail tile: valid data, never stored
        },
        [&](int64_t tile, const f32x4& z0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = tile * 16 + 4 * g + r;
                const bool ok = i < n;
                float m = 0.f;
                if (a.centre) {
                    float s = 0.f;
#pragma unroll
                    for (int v = 0; v < AT_VMAX; ++v) {
                        const float gv = __shfl(z0[r], (lane & 48) | v);
                        if ((bits >> v) & 1u) s += gv;
                    }
                    m = s / (float)A;
                }
                const float c = z0[r] - m;
                if (a.grad && ok && col_allowed && col < A) a.grad[i * A + col] = c;
                if (a.gxi && ok) {
                    const int64_t id = a.ids[i];
                    const bool counts = at_id_allowed(bits, id, V);
                    if (counts ? (int64_t)jl == id : jl == 0) a.gxi[i] = counts ? c : 0.f;
                }
            }
        });
}

}  // namespace

extern "C" int cad_embed_attrib_supported(int D, int V, int dtype) {
    return D >= 1 && V >= 1 && V <= AT_VMAX && (dtype == CAD_F32 || dtype == CAD_BF16 || dtype == CAD_F16);
}

extern "C" int cad_embed_attrib(const cad_embed_attrib_args* a, void* stream) {
    CAD_CHECK_ARG(a && a->dh && a->weight && a->allowed && (a->grad || a->gxi));
    CAD_CHECK_ARG(a->rows > 0 && a->D > 0 && a->V > 0);
    CAD_CHECK_ARG(a->n_strands == 1 || (a->n_strands == 2 && a->comp));
    CAD_CHECK_ARG(!a->gxi || a->ids);
    if (!cad_embed_attrib_supported(a->D, a->V, a->dtype)) return CAD_ERR_UNSUPPORTED;
    CAD_CHECK_ARG(a->A >= 1 && a->A <= a->V);
    CadProfScope prof(7, stream);
    const bool mfma = cad_head_mfma_nj(a->D, a->dtype) && ((uintptr_t)a->dh % 16) == 0;
    int64_t nb;
    if (mfma) {  // two workgroups per CU at most: a wave walks several tiles with its E registers, as in the score head
        nb = ((a->rows + 15) / 16 + AT_WAVES - 1) / AT_WAVES;
        const int64_t cap = 2 * (int64_t)cad_cu_count();
        nb = nb > cap ? cap : nb;
    } else {
        nb = (a->rows + AT_WAVES - 1) / AT_WAVES;
        nb = nb > 4096 ? 4096 : nb;
    }
    dim3 grid((unsigned)nb), block(64 * AT_WAVES);
    CAD_HEAD_LAUNCH(embed_attrib_mfma_kernel, embed_attrib_kernel, a->dtype, mfma ? a->D / 32 : 0, grid, block, 0, stream, *a);
    return cad_after_launch();
}
