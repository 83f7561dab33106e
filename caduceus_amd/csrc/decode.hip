// One generated token of a causal stack in one library call (include/caduceus_hip.h, cad_decode_token) and the token sampler
// (cad_sample_tokens).  Per layer the three launches of step_kernels.h, launch 1 in a variant that forms its own input rows:
//   1'. decode_in_conv_kernel  residual' = hidden + residual (hidden = emb[id] at layer 0), add + norm of the row in the summation order
//                              of cad_add_norm_fwd (cad_rownorm.h), rounded to T in LDS; then st_in_conv_rows, launch 1's own code.
//                              Every workgroup normalises the <= ST_BT rows it stages (redundant, D values per row against the 2 D
//                              weights per channel it reads anyway); the workgroups of column 0 write residual'.
//   2., 3.                     step_ssm_kernel, step_out_kernel: unchanged.
// and one tail launch, one wave per row: final add + norm, logits = W_head hn (cad_head.h's scalar row), sampler.
// residual' goes to the other of two buffers (a workgroup of another column may still be reading the residual), so the kernel
// boundaries stay the only grid-wide ordering: 3 n_layer + 1 plain launches, no allocation, no synchronisation.
#include <math.h>

#include "cad_head.h"
#include "cad_sampler.h"
#include "step_kernels.h"

namespace {

#define DC_WAVES 4
#define DC_VMAX 64

__global__ __launch_bounds__(64 * DC_WAVES) void sample_tokens_kernel(const float* logits, int64_t B, int V, cad_sampler_args s, int64_t* ids_out,
                                                                      float* u_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * DC_WAVES + cad_uniform(threadIdx.x >> 6);
    if (row >= B) return;  // wave-uniform
    float x = lane < V ? logits[row * V + lane] : 0.f;
    if (s.logit_mask && lane < V) x += s.logit_mask[lane];
    const float u = dc_uniform(s.seed, (uint64_t)(s.row_offset + row), (uint64_t)s.position);
    const int id = dc_sample_row(x, V, s.top_k, s.top_p, s.temperature, u, lane);
    if (lane == 0) {
        ids_out[row] = id;
        if (u_out) u_out[row] = u;
    }
}

// ---- launch 1 of a layer with the embedding / add + norm in front ------------------------------------------------------------------
struct dc_norm {
    const int64_t* ids;     // layer 0: hidden = emb[id], no residual; else NULL and hidden = a.h (T)
    const float* emb;
    const float* res_in;    // (B, D) fp32 or NULL
    float* res_out;         // (B, D) fp32, never res_in
    const float* weight;
    const float* bias;
    float eps;
    int is_rms;
    int V;
};

template <typename T>
__global__ __launch_bounds__(ST_THREADS) void decode_in_conv_kernel(cad_mamba_step_args a, dc_norm n, float* xc_out, float* z_out) {
    CAD_DYN_SMEM(float, hs);  // [nb][D]
    const int D = a.D;
    const int64_t b0 = (int64_t)blockIdx.y * ST_BT;
    const int nb = (int)((a.B - b0) < ST_BT ? (a.B - b0) : ST_BT);
    const int lane = threadIdx.x & 63;
    const int wave = cad_uniform(threadIdx.x >> 6);
    const int W = cad_row_width(D);
    for (int b = wave; b < nb; b += ST_WAVES) {  // wave-uniform: one wave per row; a lane touches the same channels in every pass
        float* row = hs + b * D;
        const int64_t g = (b0 + b) * D;
        const float* src = nullptr;
        if (n.ids) {
            int64_t id = n.ids[b0 + b];
            id = id < 0 ? 0 : (id >= n.V ? n.V - 1 : id);
            src = n.emb + id * D;
        }
        for (int c0 = lane * W; c0 < D; c0 += 64 * W) {
            for (int q = 0; q < W; ++q) {
                const int c = c0 + q;
                float t = src ? src[c] : to_f32(((const T*)a.h)[g + c]);
                if (n.res_in) t += n.res_in[g + c];
                row[c] = t;
                if (blockIdx.x == 0) n.res_out[g + c] = t;
            }
        }
        cad_row_norm_lds<T>(row, D, n.weight, n.bias, n.eps, n.is_rms, lane);
    }
    __syncthreads();
    st_in_conv_rows<T>(a, hs, b0, nb, xc_out, z_out);
}

// ---- tail: final add + norm, LM head, sampler; one wave per row ------------------------------------------------------------------
struct dc_tail {
    const void* h;          // (B, D) T: the last layer's out
    const float* res_in;    // (B, D) fp32
    const float* weight;
    const float* bias;
    const float* head_w;    // (V, D) fp32
    float* logits;          // (B, V)
    int64_t* ids_out;
    float* u_out;
    int64_t B;
    int D, V;
    float eps;
    int is_rms;
};

template <typename T, int VMAX>
__global__ __launch_bounds__(64 * DC_WAVES) void decode_tail_kernel(dc_tail a, cad_sampler_args s) {
    CAD_DYN_SMEM(float, rows);  // [DC_WAVES][D]
    const int D = a.D, V = a.V;
    const int lane = threadIdx.x & 63;
    const int wave = cad_uniform(threadIdx.x >> 6);
    const int64_t r = (int64_t)blockIdx.x * DC_WAVES + wave;
    const bool live = r < a.B;  // wave-uniform
    float* row = rows + wave * D;
    if (live) {
        const int W = cad_row_width(D);
        const int64_t g = r * D;
        for (int c0 = lane * W; c0 < D; c0 += 64 * W)
            for (int q = 0; q < W; ++q) row[c0 + q] = to_f32(((const T*)a.h)[g + c0 + q]) + a.res_in[g + c0 + q];
        cad_row_norm_lds<T>(row, D, a.weight, a.bias, a.eps, a.is_rms, lane);
    }
    __syncthreads();  // the head walks the row with another lane map
    if (!live) return;
    float z[VMAX];
    cad_head_row(z, (const float*)row, (const float*)nullptr, a.head_w, nullptr, D, V, lane);
    const float mine = cad_head_row_at(z, lane);  // lane v keeps logit v
    if (lane < V) a.logits[r * V + lane] = mine;
    float x = mine;
    if (s.logit_mask && lane < V) x += s.logit_mask[lane];
    const float u = dc_uniform(s.seed, (uint64_t)(s.row_offset + r), (uint64_t)s.position);
    const int id = dc_sample_row(x, V, s.top_k, s.top_p, s.temperature, u, lane);
    if (lane == 0) {
        a.ids_out[r] = id;
        if (a.u_out) a.u_out[r] = u;
    }
}

template <typename T>
int decode_launch(const cad_decode_args& d, void* stream) {
    const int64_t BE = d.B * d.E, BD = d.B * d.D;
    float* xc = d.scratch;
    float* z = xc + BE;
    float* y = z + BE;
    float* res[2] = {y + BE, y + BE + BD};
    T* out = (T*)(y + BE + 2 * BD);
    const unsigned nbt = (unsigned)((d.B + ST_BT - 1) / ST_BT);
    const int nb = (int)(d.B < ST_BT ? d.B : ST_BT);
    for (int l = 0; l < d.n_layer; ++l) {
        const cad_decode_layer& p = d.layers[l];
        cad_mamba_step_args a;
        a.h = out, a.out = out, a.conv_state = p.conv_state, a.ssm_state = p.ssm_state;
        a.W_in = p.W_in, a.b_in = p.b_in, a.conv_w = p.conv_w, a.conv_b = p.conv_b, a.W_x = p.W_x, a.W_dt = p.W_dt, a.dt_bias = p.dt_bias;
        a.A_log = p.A_log, a.Dskip = p.Dskip, a.W_out = p.W_out, a.b_out = p.b_out, a.scratch = d.scratch;
        a.B = d.B, a.D = d.D, a.E = d.E, a.N = d.N, a.R = d.R, a.K = d.K, a.dtype = d.dtype;
        dc_norm n;
        n.ids = l == 0 ? d.ids_in : nullptr, n.emb = d.emb, n.res_in = l == 0 ? nullptr : res[(l - 1) & 1], n.res_out = res[l & 1];
        n.weight = p.norm_w, n.bias = p.norm_b, n.eps = p.norm_eps, n.is_rms = p.norm_is_rms, n.V = d.V;
        CAD_LAUNCH((decode_in_conv_kernel<T>), dim3((d.E + ST_WAVES - 1) / ST_WAVES, nbt), dim3(ST_THREADS), (size_t)nb * d.D * sizeof(float),
                   stream, a, n, xc, z);
        CAD_LAUNCH((step_ssm_kernel<T>), dim3((d.E + ST_CH - 1) / ST_CH, (unsigned)d.B), dim3(ST_THREADS),
                   (size_t)(d.E + d.R + 2 * d.N) * sizeof(float), stream, a, xc, z, y);
        CAD_LAUNCH((step_out_kernel<T>), dim3((d.D + ST_WAVES - 1) / ST_WAVES, nbt), dim3(ST_THREADS), (size_t)nb * d.E * sizeof(float), stream,
                   a, y);
    }
    dc_tail t;
    t.h = out, t.res_in = res[(d.n_layer - 1) & 1], t.weight = d.normf_w, t.bias = d.normf_b, t.head_w = d.head_w, t.logits = d.logits;
    t.ids_out = d.ids_out, t.u_out = d.u_out, t.B = d.B, t.D = d.D, t.V = d.V, t.eps = d.normf_eps, t.is_rms = d.normf_is_rms;
    const dim3 grid((unsigned)((d.B + DC_WAVES - 1) / DC_WAVES)), block(64 * DC_WAVES);
    const size_t lds = (size_t)DC_WAVES * d.D * sizeof(float);
    if (d.V <= 16)
        CAD_LAUNCH((decode_tail_kernel<T, 16>), grid, block, lds, stream, t, d.sampler);
    else
        CAD_LAUNCH((decode_tail_kernel<T, DC_VMAX>), grid, block, lds, stream, t, d.sampler);
    return cad_after_launch();
}

}  // namespace

extern "C" int cad_sample_tokens(const float* logits, int64_t B, int V, const cad_sampler_args* s, int64_t* ids_out, float* u_out,
                                 void* stream) {
    CAD_CHECK_ARG(logits && s && ids_out && B >= 1 && V >= 1 && dc_sampler_ok(*s));
    if (V > DC_VMAX) return CAD_ERR_UNSUPPORTED;
    CAD_LAUNCH(sample_tokens_kernel, dim3((unsigned)((B + DC_WAVES - 1) / DC_WAVES)), dim3(64 * DC_WAVES), 0, stream, logits, B, V, *s, ids_out,
               u_out);
    return cad_after_launch();
}

extern "C" int cad_decode_supported(int D, int E, int N, int R, int K, int V, int dtype) {
    return cad_mamba_step_supported(D, E, N, R, K, dtype) && V >= 1 && V <= DC_VMAX;
}

extern "C" int64_t cad_decode_scratch_floats(int64_t B, int D, int E) {
    // xc | z | y (B, E) | two residual buffers | the layers' out (B, D: elements of the activation dtype in fp32-sized slots)
    return B > 0 && D > 0 && E > 0 ? 3 * B * E + 3 * B * D : 0;
}

extern "C" int cad_decode_token(const cad_decode_args* a, void* stream) {
    CAD_CHECK_ARG(a && a->layers && a->emb && a->normf_w && a->head_w && a->ids_in && a->logits && a->ids_out && a->scratch);
    CAD_CHECK_ARG(a->n_layer >= 1 && a->B >= 1 && a->B <= 65535 && dc_sampler_ok(a->sampler));
    if (!cad_decode_supported(a->D, a->E, a->N, a->R, a->K, a->V, a->dtype)) return CAD_ERR_UNSUPPORTED;
    for (int l = 0; l < a->n_layer; ++l) {
        const cad_decode_layer& p = a->layers[l];
        CAD_CHECK_ARG(p.conv_state && p.ssm_state && p.W_in && p.conv_w && p.W_x && p.W_dt && p.dt_bias && p.A_log && p.Dskip && p.W_out &&
                      p.norm_w);
    }
    switch (a->dtype) {
        case CAD_F32: return decode_launch<float>(*a, stream);
        case CAD_BF16: return decode_launch<bf16_t>(*a, stream);
        default: return decode_launch<f16_t>(*a, stream);
    }
}
