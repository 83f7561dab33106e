// Unmask head (include/caduceus_hip.h, cad_lm_head_unmask): at every open row (ids_in == mask_id) the LM head's logit row, the sampler's
// id drawn from it and the model's own log-probability of that id, in one launch.  Nothing is written per vocabulary entry: what leaves
// the kernel is ids_out, conf and, if asked for, the uniform each row consumed.  A closed row copies its id and forms no logit.
// The logit row is cad_head.h's (what cad_lm_head_fwd writes and cad_lm_head_score scores), the sampler cad_sampler.h's (what
// cad_sample_tokens runs), the log-sum-exp the score head's, each in that kernel's own order of operations on the same lane map: the
// three outputs equal, bit for bit, what those kernels give for the same stored hidden state.
// No atomics and no shared memory: every output element has one writer, and a row's result does not depend on its neighbours.
#include "cad_head.h"
#include "cad_sampler.h"

namespace {

#define UM_VMAX 16
#define UM_WAVES CAD_HEAD_WAVES

// a closed row: its id stays, nothing was drawn
__device__ __forceinline__ void um_close(const cad_lm_unmask_args& a, int64_t i, int64_t id) {
    a.ids_out[i] = id;
    a.conf[i] = 0.f;
    if (a.u_out) a.u_out[i] = 0.f;
}

// the uniform of row i = b L + l: key seed, counter (row_offset + b, position + l)
__device__ __forceinline__ float um_uniform(const cad_lm_unmask_args& a, int64_t i) {
    const int64_t b = i / a.L, l = i - b * a.L;
    return dc_uniform(a.sampler.seed, (uint64_t)(a.sampler.row_offset + b), (uint64_t)(a.sampler.position + l));
}

// General path: one wave per open row, any D.
template <typename T>
__global__ __launch_bounds__(64 * UM_WAVES) void lm_unmask_kernel(cad_lm_unmask_args a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int D = a.D, V = a.V;
    const T* hid = (const T*)a.hidden;
    for (int64_t i = (int64_t)blockIdx.x * UM_WAVES + wave; i < a.rows; i += (int64_t)gridDim.x * UM_WAVES) {
        const int64_t cur = a.ids_in[i];
        if (cur != a.mask_id) {  // wave-uniform: the whole wave read the same id
            if (lane == 0) um_close(a, i, cur);
            continue;
        }
        float z[UM_VMAX];
        cad_head_row(z, hid + i * D, a.n_strands == 2 ? hid + (a.rows + i) * D : nullptr, a.weight, a.comp, D, V, lane);
        // every lane holds the whole row: z + mask and its log-sum-exp in id order (the score head's general path)
        if (a.sampler.logit_mask) {
#pragma unroll
            for (int v = 0; v < UM_VMAX; ++v)
                if (v < V) z[v] += a.sampler.logit_mask[v];
        }
        const float lse = cad_head_row_lse(z, V, -INFINITY);
        const float mine = cad_head_row_at(z, lane);  // lane v: z[v] + mask[v]
        const float u = um_uniform(a, i);
        const int id = dc_sample_row<64>(mine, V, a.sampler.top_k, a.sampler.top_p, a.sampler.temperature, u, lane);
        if (lane == id) {
            a.ids_out[i] = id;
            a.conf[i] = mine - lse;
            if (a.u_out) a.u_out[i] = u;
        }
    }
}

// Matrix-core path: cad_head_mfma_walk_if on tiles of 16 consecutive rows; a tile without an open row is closed by the 16 lanes that read
// its ids and is never loaded.  Epilogue: a row's 16 logits sit on the 16 lanes of a group, four rows per wave and pass; maximum and sum
// of exponentials are the score head's reductions over the group, the sampler runs on the group.
template <typename T, int NJ>
__global__ __launch_bounds__(64 * UM_WAVES) void lm_unmask_mfma_kernel(cad_lm_unmask_args a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4, jl = lane & 15;
    const int V = a.V;
    const int64_t n = a.rows;
    const float maskv = (a.sampler.logit_mask && jl < V) ? a.sampler.logit_mask[jl] : 0.f;
    cad_head_mfma_walk_if<T, NJ>(
        (const T*)a.hidden, n, a.weight, a.comp, a.n_strands, V, (int64_t)blockIdx.x * UM_WAVES + wave, (int64_t)gridDim.x * UM_WAVES,
        (n + 15) / 16, lane,
        [&](int64_t tile) {
            const int64_t i = tile * 16 + jl;
            const bool ok = i < n;
            const int64_t cur = ok ? a.ids_in[i] : 0;
            int open = (ok && cur == a.mask_id) ? 1 : 0;
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) open |= __shfl_xor(open, m);  // the four groups hold the same 16 rows: wave-uniform
            open = cad_uniform(open);
            if (!open && ok && g == 0) um_close(a, i, cur);
            return open != 0;
        },
        [&](int64_t tile) {
            const int64_t i = tile * 16 + jl;
            return i < n ? i : n - 1;  // tail tile: valid data, never stored
        },
        [&](int64_t tile, const f32x4& z0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = tile * 16 + 4 * g + r;
                const bool ok = i < n;
                const int64_t cur = ok ? a.ids_in[i] : 0;
                const bool open = ok && cur == a.mask_id;
                const float zm = jl < V ? z0[r] + maskv : -INFINITY;  // columns beyond V count as forbidden ids
                const float mx = cad_head_max16(zm);
                const float se = cad_head_sum16(jl < V ? expf(zm - mx) : 0.f);
                const float u = um_uniform(a, ok ? i : n - 1);
                const int id = dc_sample_row<16>(zm, V, a.sampler.top_k, a.sampler.top_p, a.sampler.temperature, u, jl);
                if (open && jl == id) {
                    a.ids_out[i] = id;
                    a.conf[i] = zm - (logf(se) + mx);
                    if (a.u_out) a.u_out[i] = u;
                }
                if (ok && !open && jl == 0) um_close(a, i, cur);
            }
        });
}

}  // namespace

extern "C" int cad_lm_head_unmask_supported(int D, int V, int dtype) {
    return D >= 1 && V >= 1 && V <= UM_VMAX && (dtype == CAD_F32 || dtype == CAD_BF16 || dtype == CAD_F16);
}

extern "C" int cad_lm_head_unmask(const cad_lm_unmask_args* a, void* stream) {
    CAD_CHECK_ARG(a && a->hidden && a->weight && a->ids_in && a->ids_out && a->conf);
    CAD_CHECK_ARG(a->rows > 0 && a->L > 0 && a->rows % a->L == 0 && a->D > 0 && a->V > 0);
    CAD_CHECK_ARG(a->n_strands == 1 || (a->n_strands == 2 && a->comp));
    CAD_CHECK_ARG(dc_sampler_ok(a->sampler));
    if (!cad_lm_head_unmask_supported(a->D, a->V, a->dtype)) return CAD_ERR_UNSUPPORTED;
    CadProfScope prof(7, stream);
    const bool mfma = cad_head_mfma_nj(a->D, a->dtype) && ((uintptr_t)a->hidden % 16) == 0;
    int64_t nb;
    if (mfma) {  // two workgroups per CU at most: a wave walks several tiles with its W registers, as in the score head
        nb = ((a->rows + 15) / 16 + UM_WAVES - 1) / UM_WAVES;
        const int64_t cap = 2 * (int64_t)cad_cu_count();
        nb = nb > cap ? cap : nb;
    } else {
        nb = (a->rows + UM_WAVES - 1) / UM_WAVES;
        nb = nb > 4096 ? 4096 : nb;
    }
    dim3 grid((unsigned)nb), block(64 * UM_WAVES);
    CAD_HEAD_LAUNCH(lm_unmask_mfma_kernel, lm_unmask_kernel, a->dtype, mfma ? a->D / 32 : 0, grid, block, 0, stream, *a);
    return cad_after_launch();
}
