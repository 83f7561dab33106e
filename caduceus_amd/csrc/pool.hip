// Pool head (include/caduceus_hip.h, cad_pool_head): the backbone's final add + RMSNorm / LayerNorm and the pooling over the sequence in
// one pass over the pre-norm stream.  Nothing of size L is written: what leaves the kernels is the fixed-order partials in the caller's
// scratch and out (S, B, D) fp32.
//
// A row's normed value y is cad_add_norm_fwd's (csrc/addnorm.hip, swap_flip = 0): the add, the statistics, the scale, the rounding to
// y_dtype and the lane map are cad_rownorm.h's (cad_row_norm), which states that kernel's order once for this file and pool_bwd.hip.
//
// Geometry.  The rows a (s, b) pair pools -- all L of them for MEAN / MAX, the clamped window's lo .. hi for WINDOW -- are walked from
// both ends at once: item j is the two rows lo + j and hi - j (one row where they meet), and an item's value is c_a y_a + c_b y_b, two
// rounded products and one commutative add.  Everything after that sums ITEMS, so the result does not change, bit for bit, when the
// rows arrive in the opposite order -- which is what reverse-complementing the input does to a strand of the t-frame.  The items are
// cut into pieces of `cpp` chunks of POOL_CHUNK items; one workgroup walks one piece, its four waves taking items round-robin with
// POOL_UNROLL items (twice as many rows) in flight each, folds its waves in wave order through LDS and writes ONE partial row.  The
// combining launch folds a pair's partials in piece order and finishes (1 / n, or nothing for MAX).  cpp and the number of pieces follow
// from the row count alone (pool_geometry): not from B, S or the device, so a pair's bits depend on neither its neighbours nor the run.
// No atomics; every element has one writer.
#include "cad_pool.h"

namespace {

// an item's value: the two products are rounded before the add, so that (a, b) and (b, a) give the same bits
__device__ __forceinline__ float pool_pair(float ca, float ya, float cb, float yb) {
#pragma clang fp contract(off)
    const float pa = ca * ya, pb = cb * yb;
    return pa + pb;
}

// One workgroup per (pair, piece).  W = 4: the vector lane map (KMAX 256-channel steps), W = 1: the scalar one (KMAX = 16 steps of 64).
template <typename TX, typename TY, int W, int KMAX>
__global__ __launch_bounds__(64 * POOL_WAVES) void pool_partial_kernel(cad_pool_head_args a, int64_t cpp, int64_t pieces) {
    __shared__ float red[POOL_WAVES][POOL_DMAX];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int D = a.D;
    const int64_t sb = (int64_t)blockIdx.x / pieces;
    const int64_t piece = (int64_t)blockIdx.x - sb * pieces;
    const bool is_max = a.mode == CAD_POOL_MAX;
    const bool normed = a.weight != nullptr;
    const bool has_bias = normed && a.bias != nullptr;
    const pool_span span = pool_span_of(a.mode, a.L, a.half, a.centre, sb);
    const TX* x = (const TX*)a.x + sb * a.L * D;
    const float* res = a.residual_in ? a.residual_in + sb * a.L * D : nullptr;

    float wreg[KMAX][W], breg[KMAX][W], acc[KMAX][W];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int c = cad_row_chan<W>(lane, k);
#pragma unroll
        for (int q = 0; q < W; ++q) wreg[k][q] = 1.f, breg[k][q] = 0.f, acc[k][q] = is_max ? -INFINITY : 0.f;
        if (c < D && normed) {
            cad_row_ld<float, W>(a.weight + c, wreg[k]);
            if (has_bias) cad_row_ld<float, W>(a.bias + c, breg[k]);
        }
    }

    // this piece's items: first .. first + cpp POOL_CHUNK - 1, up to the one where the two ends meet
    const int64_t n_items = (span.hi - span.lo) / 2 + 1;
    const int64_t first = piece * cpp * POOL_CHUNK;
    for (int64_t i = 0; i < cpp; ++i) {
        const int64_t base = first + i * POOL_CHUNK + wave;
        if (base >= n_items) break;
        float v[POOL_UNROLL][2][KMAX][W];
        // every load of the wave's POOL_UNROLL items is issued before the first statistic is formed
#pragma unroll
        for (int u = 0; u < POOL_UNROLL; ++u) {
            const int64_t j = base + u * POOL_WAVES;
            if (j < n_items) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int64_t row = e == 0 ? span.lo + j : span.hi - j;
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) {
                        const int c = cad_row_chan<W>(lane, k);
#pragma unroll
                        for (int q = 0; q < W; ++q) v[u][e][k][q] = 0.f;
                        if (c < D) {
                            cad_row_ld<TX, W>(x + row * D + c, v[u][e][k]);
                            if (res) {
                                float t[W];
                                cad_row_ld<float, W>(res + row * D + c, t);
#pragma unroll
                                for (int q = 0; q < W; ++q) v[u][e][k][q] += t[q];
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < POOL_UNROLL; ++u) {
            const int64_t j = base + u * POOL_WAVES;
            if (j < n_items) {  // wave-uniform
                const int64_t ra = span.lo + j, rb = span.hi - j;
                const bool two = ra != rb;  // (the two ends meet on one row where the count is odd: that row is formed twice, used once)
                if (normed) {
                    cad_row_norm<TY, W, KMAX>(v[u][0], wreg, breg, has_bias, D, a.eps, a.is_rms, lane);
                    cad_row_norm<TY, W, KMAX>(v[u][1], wreg, breg, has_bias, D, a.eps, a.is_rms, lane);
                }
                // (L == 1: row 0 is also row L - 1 and c_last is 0)
                const float ca = ra == 0 ? span.c_first : (ra == a.L - 1 ? span.c_last : 1.f);
                const float cb = rb == 0 ? span.c_first : (rb == a.L - 1 ? span.c_last : 1.f);
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
#pragma unroll
                    for (int q = 0; q < W; ++q) {
                        const float ya = v[u][0][k][q], yb = v[u][1][k][q];
                        if (is_max)
                            acc[k][q] = pool_max(pool_max(acc[k][q], ya), yb);
                        else
                            acc[k][q] += two ? pool_pair(ca, ya, cb, yb) : ca * ya;
                    }
            }
        }
    }

    // the four waves' sums, folded in wave order by the thread that writes the channel
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int c = cad_row_chan<W>(lane, k);
#pragma unroll
        for (int q = 0; q < W; ++q)
            if (c + q < D) red[wave][c + q] = acc[k][q];
    }
    __syncthreads();
    float* part = a.scratch + (int64_t)blockIdx.x * D;
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        float t = red[0][c];
        for (int w = 1; w < POOL_WAVES; ++w) t = is_max ? pool_max(t, red[w][c]) : t + red[w][c];
        part[c] = t;
    }
}

// out[sb][c] = the pair's partials folded in piece order, over n for the two means
__global__ __launch_bounds__(256) void pool_combine_kernel(cad_pool_head_args a, int64_t pieces, float n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int D = a.D;
    if (i >= (int64_t)a.S * a.B * D) return;
    const int64_t sb = i / D;
    const int c = (int)(i - sb * D);
    const bool is_max = a.mode == CAD_POOL_MAX;
    const float* part = a.scratch + sb * pieces * D + c;
    float t = part[0];
    for (int64_t p = 1; p < pieces; ++p) t = is_max ? pool_max(t, part[p * D]) : t + part[p * D];
    a.out[i] = is_max ? t : t / n;
}

}  // namespace

extern "C" int cad_pool_head_supported(int D, int x_dtype, int y_dtype, int mode, int64_t half) {
    return D >= 1 && D <= POOL_DMAX && cad_row_types_ok(x_dtype, y_dtype) &&
           (mode == CAD_POOL_MEAN || mode == CAD_POOL_MAX || (mode == CAD_POOL_WINDOW && half >= 0 && half < POOL_HALF_MAX));
}

extern "C" int64_t cad_pool_head_chunk_rows(int D, int x_dtype) {
    (void)D, (void)x_dtype;  // one walk for every width and type
    return 2 * POOL_CHUNK;
}

extern "C" int64_t cad_pool_head_pieces(int64_t L, int mode, int64_t half) {
    if (L < 1 || (mode == CAD_POOL_WINDOW && (half < 0 || half >= POOL_HALF_MAX))) return 0;
    return pool_geometry(pool_rows(mode, L, half)).pieces;
}

extern "C" int64_t cad_pool_head_scratch_floats(int S, int64_t B, int64_t L, int D, int mode, int64_t half) {
    if (S < 1 || B < 1 || D < 1) return 0;
    return (int64_t)S * B * cad_pool_head_pieces(L, mode, half) * D;
}

extern "C" int cad_pool_head(const cad_pool_head_args* a, void* stream) {
    CAD_CHECK_ARG(a && a->x && a->out && a->scratch);
    CAD_CHECK_ARG((a->S == 1 || a->S == 2) && a->B > 0 && a->L > 0 && a->D > 0);
    CAD_CHECK_ARG(a->weight || !a->bias);
    CAD_CHECK_ARG(a->mode != CAD_POOL_WINDOW || a->centre);
    if (!cad_pool_head_supported(a->D, a->x_dtype, a->y_dtype, a->mode, a->half)) return CAD_ERR_UNSUPPORTED;
    const pool_geom g = pool_geometry(pool_rows(a->mode, a->L, a->half));
    const int64_t sb = (int64_t)a->S * a->B;
    if (sb * g.pieces > 0x7fffffff) return CAD_ERR_UNSUPPORTED;
    CadProfScope prof(4, stream);
    const bool vec = pool_vec(a->D, a->x, a->residual_in, a->weight, a->bias);
    dim3 grid((unsigned)(sb * g.pieces)), block(64 * POOL_WAVES);
    const bool served = cad_row_type_pair(a->x_dtype, a->y_dtype, [&](auto tx, auto ty) {
        using TX = typename decltype(tx)::type;
        using TY = typename decltype(ty)::type;
        if (vec && a->D <= 256)
            CAD_LAUNCH((pool_partial_kernel<TX, TY, 4, 1>), grid, block, 0, stream, *a, g.cpp, g.pieces);
        else if (vec && a->D <= 512)
            CAD_LAUNCH((pool_partial_kernel<TX, TY, 4, 2>), grid, block, 0, stream, *a, g.cpp, g.pieces);
        else if (vec)
            CAD_LAUNCH((pool_partial_kernel<TX, TY, 4, 4>), grid, block, 0, stream, *a, g.cpp, g.pieces);
        else
            CAD_LAUNCH((pool_partial_kernel<TX, TY, 1, 16>), grid, block, 0, stream, *a, g.cpp, g.pieces);
    });
    if (!served) return CAD_ERR_UNSUPPORTED;
    const float n = a->mode == CAD_POOL_WINDOW ? (float)(2 * a->half + 1) : (float)a->L;
    const int64_t total = sb * a->D;
    CAD_LAUNCH(pool_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, *a, g.pieces, n);
    return cad_after_launch();
}
