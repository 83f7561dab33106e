// Pool head backward (include/caduceus_hip.h, cad_pool_head_bwd / cad_pool_head_max_rows): the gradient of cad_pool_head with respect
// to x, the residual stream, the norm weight and bias, from the forward's own operands.  Nothing is saved by the forward: a row's add and
// statistics are recomputed from x (+ residual), the gradient dy of its normed value follows from g (S, B, D) and the row's multiplicity,
// and cad_add_norm_bwd's sequence turns it into dx / dres_in.  Neither y, dy nor a statistic is ever written; what leaves the kernels
// besides dx / dres_in is one slot row of dweight / dbias partial sums per workgroup.
//
// A row's statistics are cad_rownorm.h's (cad_row_stats), the routine the pool forward's cad_row_norm is built on; the MAX search calls
// cad_row_norm itself, in the forward's lane map and type pair, so the y it compares with `out` has the forward's bits.
//
// dy.  MEAN / WINDOW: dy[c] = m(r) (g[s,b,c] / n) -- one IEEE division per (s, b, c), formed once per workgroup, and one rounded product
// with the row's multiplicity m(r) of pool_span_of / pool_mult (an exact integer), not contracted into what follows.  MAX: dy[c] =
// g[s,b,c] on row rows[s,b,c] and 0 on every other row; rows is cad_pool_head_max_rows' -- per channel the lowest row whose recomputed y
// has the bits of out[s,b,c] (the lowest NaN row where out is NaN), torch.max(dim)'s choice on the stored tensor.  Then, as
// cad_add_norm_bwd:  gw = dy w,  sgx = mean_c(gw xh),  sg = mean_c(gw) (0 for RMSNorm),  dt = rstd (gw - sg - xh sgx);  dres_in = dt,
// dx = dt rounded to x_dtype.  The rounding of y to y_dtype is straight-through.  weight NULL: dt = dy.
//
// Geometry.  ALL L rows of a (s, b) pair have a writer: they are cut into pieces of `cpp` chunks of POOL_BWD_CHUNK consecutive rows, one
// workgroup per piece, its four waves taking rows round-robin with POOL_BWD_ROWS rows in flight each (every load issued before the
// first statistic; the rows' arithmetic free of branches, so that their wave sums overlap).  A row outside a window gets zeros without
// being read.  The dweight / dbias sums live in per-wave registers, are
// folded over the four waves through LDS in wave order and written as ONE slot row per workgroup; the last launch folds the slots --
// thread j of POOL_FOLD_SUB takes the pieces p = j, j + POOL_FOLD_SUB, .. of every pair in pair order, the POOL_FOLD_SUB sums are added in
// order.  cpp and the pieces follow from L alone (pool_bwd_geometry), never from the device: the bits are run-to-run identical, and a
// pair whose g is 0 adds exact zeros to chains whose shape it does not change.  No atomics; every element has one writer; the caller
// fills nothing.
#include "cad_pool.h"
#include "cad_stream.h"

namespace {

#define POOL_BWD_ROWS (2 * POOL_UNROLL)                 // rows in flight per wave: the forward's POOL_UNROLL items
#define POOL_BWD_CHUNK (POOL_WAVES * POOL_BWD_ROWS)     // rows per workgroup iteration
#define POOL_BWD_PIECES_MAX POOL_PIECES_MAX             // workgroups (slot rows) per (s, b): the forward's cap
#define POOL_FOLD_SUB 16
#define POOL_FOLD_CH 16

// L rows -> chunks per piece and pieces
pool_geom pool_bwd_geometry(int64_t L) {
    const int64_t chunks = (L + POOL_BWD_CHUNK - 1) / POOL_BWD_CHUNK;
    pool_geom g;
    g.cpp = (chunks + POOL_BWD_PIECES_MAX - 1) / POOL_BWD_PIECES_MAX;
    g.pieces = (chunks + g.cpp - 1) / g.cpp;
    return g;
}

// dy of a MEAN / WINDOW row: one rounded product (not contracted into the sums it feeds)
__device__ __forceinline__ float pool_dy(float m, float gd) {
#pragma clang fp contract(off)
    const float dy = m * gd;
    return dy;
}

// v[k] = x + residual of row `row` in this lane's channels (zeros beyond D)
template <typename TX, int W, int KMAX>
__device__ __forceinline__ void pool_load_row(float (&v)[KMAX][W], const TX* x, const float* res, int64_t row, int D, int lane) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int c = cad_row_chan<W>(lane, k);
#pragma unroll
        for (int q = 0; q < W; ++q) v[k][q] = 0.f;
        if (c < D) {
            cad_row_ld<TX, W>(x + row * D + c, v[k]);
            if (res) {
                float t[W];
                cad_row_ld<float, W>(res + row * D + c, t);
#pragma unroll
                for (int q = 0; q < W; ++q) v[k][q] += t[q];
            }
        }
    }
}

// W values of this lane's step -> dx (x_dtype) and dres_in (fp32) of row `row`: single-reader streams, written around the cache
template <typename TX, int W>
__device__ __forceinline__ void pool_store_row(TX* dx, float* dri, int64_t at, const float* d) {
    if constexpr (W == 4) {
        cad_cvt_store_stream<CAD_STREAM_NORM, TX, 4>(dx + at, d);
        if (dri) cad_cvt_store_stream<CAD_STREAM_NORM, float, 4>(dri + at, d);
    } else {
        dx[at] = from_f32<TX>(d[0]);
        if (dri) dri[at] = d[0];
    }
}

// One workgroup per (pair, piece).  W = 4: the vector lane map (KMAX 256-channel steps), W = 1: the scalar one (KMAX = 16 steps of 64).
// NORM 0: no norm (weight NULL), 1: RMSNorm, 2: LayerNorm -- a template parameter so that the arithmetic of the POOL_BWD_ROWS rows in
// flight is ONE basic block: no row is skipped by a branch (a row past L or outside the window is a row of zeros with multiplicity 0,
// only its store is guarded), so the rows' wave sums overlap.
#define POOL_NORM_NONE 0
#define POOL_NORM_RMS 1
#define POOL_NORM_LN 2
template <typename TX, int W, int KMAX, int NORM>
__global__ __launch_bounds__(64 * POOL_WAVES) void pool_bwd_kernel(cad_pool_head_bwd_args a, int64_t cpp, int64_t pieces, float n,
                                                                   float* wslots, float* bslots) {
    __shared__ float red[POOL_WAVES][POOL_DMAX];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int D = a.D;
    const int64_t sb = (int64_t)blockIdx.x / pieces;
    const int64_t piece = (int64_t)blockIdx.x - sb * pieces;
    const bool is_max = a.mode == CAD_POOL_MAX;
    constexpr bool normed = NORM != POOL_NORM_NONE;
    const pool_span span = pool_span_of(a.mode, a.L, a.half, a.centre, sb);
    const TX* x = (const TX*)a.x + sb * a.L * D;
    const float* res = a.residual_in ? a.residual_in + sb * a.L * D : nullptr;
    TX* dx = (TX*)a.dx + sb * a.L * D;
    float* dri = a.dres_in ? a.dres_in + sb * a.L * D : nullptr;
    const float invD = 1.0f / (float)D;

    // per channel of this lane: the norm weight, g / n (g itself for MAX), the row MAX routes g to, the two weight-gradient sums
    float wreg[KMAX][W], gd[KMAX][W], dw[KMAX][W], db[KMAX][W];
    int64_t sel[KMAX][W];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int c = cad_row_chan<W>(lane, k);
#pragma unroll
        for (int q = 0; q < W; ++q) wreg[k][q] = 1.f, gd[k][q] = 0.f, dw[k][q] = 0.f, db[k][q] = 0.f, sel[k][q] = -1;
        if (c < D) {
            if (normed) cad_row_ld<float, W>(a.weight + c, wreg[k]);
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const float gv = a.g[sb * D + c + q];
                gd[k][q] = is_max ? gv : gv / n;
                if (is_max) sel[k][q] = a.rows[sb * D + c + q];
            }
        }
    }

    const int64_t first = piece * cpp * POOL_BWD_CHUNK;
    for (int64_t i = 0; i < cpp; ++i) {
        const int64_t base = first + i * POOL_BWD_CHUNK + wave;
        if (base >= a.L) break;
        float v[POOL_BWD_ROWS][KMAX][W];
        // every load of the wave's POOL_BWD_ROWS rows is issued before the first statistic is formed
#pragma unroll
        for (int u = 0; u < POOL_BWD_ROWS; ++u) {
            const int64_t r = base + u * POOL_WAVES;
            if (r < a.L && r >= span.lo && r <= span.hi) {  // wave-uniform
                pool_load_row<TX, W, KMAX>(v[u], x, res, r, D, lane);
            } else {
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
#pragma unroll
                    for (int q = 0; q < W; ++q) v[u][k][q] = 0.f;
            }
        }
        // v[u] = x + residual -> xh -> dt, branch-free
#pragma unroll
        for (int u = 0; u < POOL_BWD_ROWS; ++u) {
            const int64_t r = base + u * POOL_WAVES;
            const bool inside = r < a.L && r >= span.lo && r <= span.hi;
            const float m = inside ? pool_mult(span, r, a.L) : 0.f;
            float mean = 0.f, rstd = 1.f, sg = 0.f, sgx = 0.f;
            float gw[KMAX][W];
            if (normed) {
                cad_row_stats<W, KMAX>(v[u], D, a.eps, NORM == POOL_NORM_RMS, lane, mean, rstd);
                mean = inside ? mean : 0.f, rstd = inside ? rstd : 0.f;  // a row of zeros stays one (eps may be 0)
            }
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
#pragma unroll
                for (int q = 0; q < W; ++q) gw[k][q] = 0.f;
                if (cad_row_chan<W>(lane, k) < D) {
#pragma unroll
                    for (int q = 0; q < W; ++q) {
                        const float dy = is_max ? (sel[k][q] == r ? gd[k][q] : 0.f) : pool_dy(m, gd[k][q]);
                        if (normed) {
                            const float xh = (v[u][k][q] - mean) * rstd;
                            v[u][k][q] = xh;
                            gw[k][q] = dy * wreg[k][q];
                            sg += gw[k][q];
                            sgx += gw[k][q] * xh;
                            dw[k][q] += dy * xh;
                            db[k][q] += dy;
                        } else {
                            gw[k][q] = dy;
                        }
                    }
                }
            }
            if (normed) {
                sgx = cad_row_wave_sum(sgx) * invD;
                sg = NORM == POOL_NORM_RMS ? 0.f : cad_row_wave_sum(sg) * invD;
            }
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    const float d = normed ? rstd * (gw[k][q] - sg - v[u][k][q] * sgx) : gw[k][q];
                    v[u][k][q] = inside ? d : 0.f;
                }
        }
#pragma unroll
        for (int u = 0; u < POOL_BWD_ROWS; ++u) {
            const int64_t r = base + u * POOL_WAVES;
            if (r < a.L) {  // wave-uniform
#pragma unroll
                for (int k = 0; k < KMAX; ++k) {
                    const int c = cad_row_chan<W>(lane, k);
                    if (c < D) pool_store_row<TX, W>(dx, dri, r * D + c, v[u][k]);
                }
            }
        }
    }

    // the four waves' sums, folded in wave order by the thread that writes the channel: one slot row per workgroup, zeros included
    if (!wslots) return;
    for (int pass = 0; pass < 2; ++pass) {
        float* slots = pass == 0 ? wslots : bslots;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int c = cad_row_chan<W>(lane, k);
#pragma unroll
            for (int q = 0; q < W; ++q)
                if (c + q < D) red[wave][c + q] = pass == 0 ? dw[k][q] : db[k][q];
        }
        __syncthreads();
        for (int c = threadIdx.x; c < D; c += blockDim.x) {
            float t = red[0][c];
            for (int w = 1; w < POOL_WAVES; ++w) t += red[w][c];
            slots[(int64_t)blockIdx.x * D + c] = t;
        }
        __syncthreads();
    }
}

// dweight / dbias (blockIdx.y = 0 / 1) from the slot rows: POOL_FOLD_CH channels x POOL_FOLD_SUB chains per workgroup
__global__ __launch_bounds__(POOL_FOLD_CH * POOL_FOLD_SUB) void pool_bwd_fold_kernel(const float* wslots, const float* bslots, float* dweight,
                                                                                      float* dbias, int64_t pairs, int64_t pieces, int D) {
    __shared__ float red[POOL_FOLD_SUB][POOL_FOLD_CH];
    const float* slots = blockIdx.y == 0 ? wslots : bslots;
    float* dst = blockIdx.y == 0 ? dweight : dbias;
    if (!dst) return;
    const int cl = threadIdx.x % POOL_FOLD_CH, j = threadIdx.x / POOL_FOLD_CH;
    const int c = (int)blockIdx.x * POOL_FOLD_CH + cl;
    float acc = 0.f;
    if (c < D)
        for (int64_t sb = 0; sb < pairs; ++sb)
            for (int64_t p = j; p < pieces; p += POOL_FOLD_SUB) acc += slots[(sb * pieces + p) * D + c];
    red[j][cl] = acc;
    __syncthreads();
    if (j == 0 && c < D) {
        float t = red[0][cl];
        for (int s = 1; s < POOL_FOLD_SUB; ++s) t += red[s][cl];
        dst[c] = t;
    }
}

#define POOL_NO_ROW INT64_MAX

// Per (pair, piece) and channel: the lowest row of the piece whose y has the bits of out (is NaN where out is NaN), POOL_NO_ROW if none.
// The forward's lane map, type pair and cad_row_norm, so that y is the forward's; the rows in the backward's geometry (a minimum does not
// depend on the walk).
template <typename TX, typename TY, int W, int KMAX>
__global__ __launch_bounds__(64 * POOL_WAVES) void pool_max_rows_kernel(cad_pool_head_bwd_args a, const float* out, int64_t* part, int64_t cpp,
                                                                        int64_t pieces) {
    __shared__ int64_t red[POOL_WAVES][POOL_DMAX];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int D = a.D;
    const int64_t sb = (int64_t)blockIdx.x / pieces;
    const int64_t piece = (int64_t)blockIdx.x - sb * pieces;
    const bool normed = a.weight != nullptr;
    const bool has_bias = normed && a.bias != nullptr;
    const TX* x = (const TX*)a.x + sb * a.L * D;
    const float* res = a.residual_in ? a.residual_in + sb * a.L * D : nullptr;

    float wreg[KMAX][W], breg[KMAX][W], want[KMAX][W];
    int64_t best[KMAX][W];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int c = cad_row_chan<W>(lane, k);
#pragma unroll
        for (int q = 0; q < W; ++q) wreg[k][q] = 1.f, breg[k][q] = 0.f, want[k][q] = 0.f, best[k][q] = POOL_NO_ROW;
        if (c < D) {
            if (normed) {
                cad_row_ld<float, W>(a.weight + c, wreg[k]);
                if (has_bias) cad_row_ld<float, W>(a.bias + c, breg[k]);
            }
#pragma unroll
            for (int q = 0; q < W; ++q) want[k][q] = out[sb * D + c + q];
        }
    }

    const int64_t first = piece * cpp * POOL_BWD_CHUNK;
    for (int64_t i = 0; i < cpp; ++i) {
        const int64_t base = first + i * POOL_BWD_CHUNK + wave;
        if (base >= a.L) break;
        float v[POOL_BWD_ROWS][KMAX][W];
#pragma unroll
        for (int u = 0; u < POOL_BWD_ROWS; ++u) {
            const int64_t r = base + u * POOL_WAVES;
            if (r < a.L) pool_load_row<TX, W, KMAX>(v[u], x, res, r, D, lane);
        }
#pragma unroll
        for (int u = 0; u < POOL_BWD_ROWS; ++u) {
            const int64_t r = base + u * POOL_WAVES;
            if (r >= a.L) continue;  // wave-uniform
            if (normed) cad_row_norm<TY, W, KMAX>(v[u], wreg, breg, has_bias, D, a.eps, a.is_rms, lane);
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    const float y = v[u][k][q], t = want[k][q];
                    const bool hit = t != t ? y != y : cad_f2bits(y) == cad_f2bits(t);
                    if (hit && r < best[k][q]) best[k][q] = r;
                }
        }
    }

#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int c = cad_row_chan<W>(lane, k);
#pragma unroll
        for (int q = 0; q < W; ++q)
            if (c + q < D) red[wave][c + q] = best[k][q];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        int64_t t = red[0][c];
        for (int w = 1; w < POOL_WAVES; ++w) t = red[w][c] < t ? red[w][c] : t;
        part[(int64_t)blockIdx.x * D + c] = t;
    }
}

// rows[sb][c] = the pair's per-piece minima folded in piece order
__global__ __launch_bounds__(256) void pool_max_rows_combine_kernel(const int64_t* part, int64_t* rows, int64_t total, int64_t pieces, int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t sb = i / D;
    const int c = (int)(i - sb * D);
    const int64_t* p = part + sb * pieces * D + c;
    int64_t t = p[0];
    for (int64_t k = 1; k < pieces; ++k) t = p[k * D] < t ? p[k * D] : t;
    rows[i] = t;
}

int pool_bwd_check(const cad_pool_head_bwd_args* a) {
    CAD_CHECK_ARG(a && a->x);
    CAD_CHECK_ARG((a->S == 1 || a->S == 2) && a->B > 0 && a->L > 0 && a->D > 0);
    CAD_CHECK_ARG(a->weight || !a->bias);
    CAD_CHECK_ARG(a->mode != CAD_POOL_WINDOW || a->centre);
    if (!cad_pool_head_bwd_supported(a->D, a->x_dtype, a->y_dtype, a->mode, a->half)) return CAD_ERR_UNSUPPORTED;
    if ((int64_t)a->S * a->B * pool_bwd_geometry(a->L).pieces > 0x7fffffff) return CAD_ERR_UNSUPPORTED;
    return CAD_OK;
}

}  // namespace

extern "C" int cad_pool_head_bwd_supported(int D, int x_dtype, int y_dtype, int mode, int64_t half) {
    return cad_pool_head_supported(D, x_dtype, y_dtype, mode, half);
}

extern "C" int64_t cad_pool_head_bwd_pieces(int64_t L) { return L < 1 ? 0 : pool_bwd_geometry(L).pieces; }

extern "C" int64_t cad_pool_head_bwd_scratch_floats(int S, int64_t B, int64_t L, int D, int mode, int64_t half) {
    (void)mode, (void)half;  // every row of a pair has a writer, whatever is pooled
    if (S < 1 || B < 1 || D < 1) return 0;
    return 2 * (int64_t)S * B * cad_pool_head_bwd_pieces(L) * D;
}

extern "C" int cad_pool_head_max_rows(const cad_pool_head_bwd_args* a, const float* out, int64_t* rows, float* scratch, void* stream) {
    const int st = pool_bwd_check(a);
    if (st != CAD_OK) return st;
    CAD_CHECK_ARG(a->mode == CAD_POOL_MAX && out && rows && scratch && ((uintptr_t)scratch % 8) == 0);
    const pool_geom g = pool_bwd_geometry(a->L);
    const int64_t sb = (int64_t)a->S * a->B;
    int64_t* part = (int64_t*)scratch;
    const bool vec = pool_vec(a->D, a->x, a->residual_in, a->weight, a->bias);  // the forward's choice
    dim3 grid((unsigned)(sb * g.pieces)), block(64 * POOL_WAVES);
    const bool served = cad_row_type_pair(a->x_dtype, a->y_dtype, [&](auto tx, auto ty) {
        using TX = typename decltype(tx)::type;
        using TY = typename decltype(ty)::type;
        if (vec && a->D <= 256)
            CAD_LAUNCH((pool_max_rows_kernel<TX, TY, 4, 1>), grid, block, 0, stream, *a, out, part, g.cpp, g.pieces);
        else if (vec && a->D <= 512)
            CAD_LAUNCH((pool_max_rows_kernel<TX, TY, 4, 2>), grid, block, 0, stream, *a, out, part, g.cpp, g.pieces);
        else if (vec)
            CAD_LAUNCH((pool_max_rows_kernel<TX, TY, 4, 4>), grid, block, 0, stream, *a, out, part, g.cpp, g.pieces);
        else
            CAD_LAUNCH((pool_max_rows_kernel<TX, TY, 1, 16>), grid, block, 0, stream, *a, out, part, g.cpp, g.pieces);
    });
    if (!served) return CAD_ERR_UNSUPPORTED;
    const int64_t total = sb * a->D;
    CAD_LAUNCH(pool_max_rows_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, part, rows, total, g.pieces, a->D);
    return cad_after_launch();
}

extern "C" int cad_pool_head_bwd(const cad_pool_head_bwd_args* a, void* stream) {
    const int st = pool_bwd_check(a);
    if (st != CAD_OK) return st;
    CAD_CHECK_ARG(a->g && a->dx && (a->dres_in == nullptr) == (a->residual_in == nullptr));
    CAD_CHECK_ARG(a->weight || (!a->dweight && !a->dbias));
    const bool slots = a->dweight || a->dbias;
    CAD_CHECK_ARG(!slots || a->scratch);
    if (a->mode == CAD_POOL_MAX) {  // the rows g is routed to: one more pass over the rows, before the slots reuse the scratch
        const int sr = cad_pool_head_max_rows(a, a->out, a->rows, a->scratch, stream);
        if (sr != CAD_OK) return sr;
    }
    const pool_geom g = pool_bwd_geometry(a->L);
    const int64_t sb = (int64_t)a->S * a->B;
    CadProfScope prof(5, stream);
    float* wslots = slots ? a->scratch : nullptr;
    float* bslots = slots ? a->scratch + sb * g.pieces * a->D : nullptr;
    const bool vec = pool_vec(a->D, a->x, a->residual_in, a->weight, nullptr) && (((uintptr_t)a->dx | (uintptr_t)a->dres_in) % 16) == 0;
    const float n = a->mode == CAD_POOL_WINDOW ? (float)(2 * a->half + 1) : (float)a->L;
    dim3 grid((unsigned)(sb * g.pieces)), block(64 * POOL_WAVES);
#define POOL_BWD_N(TX, NORM)                                                                                               \
    do {                                                                                                                   \
        if (vec && a->D <= 256)                                                                                            \
            CAD_LAUNCH((pool_bwd_kernel<TX, 4, 1, NORM>), grid, block, 0, stream, *a, g.cpp, g.pieces, n, wslots, bslots); \
        else if (vec && a->D <= 512)                                                                                       \
            CAD_LAUNCH((pool_bwd_kernel<TX, 4, 2, NORM>), grid, block, 0, stream, *a, g.cpp, g.pieces, n, wslots, bslots); \
        else if (vec)                                                                                                      \
            CAD_LAUNCH((pool_bwd_kernel<TX, 4, 4, NORM>), grid, block, 0, stream, *a, g.cpp, g.pieces, n, wslots, bslots); \
        else                                                                                                               \
            CAD_LAUNCH((pool_bwd_kernel<TX, 1, 16, NORM>), grid, block, 0, stream, *a, g.cpp, g.pieces, n, wslots, bslots); \
    } while (0)
#define POOL_BWD(TX)                              \
    do {                                          \
        if (!a->weight)                           \
            POOL_BWD_N(TX, POOL_NORM_NONE);       \
        else if (a->is_rms)                       \
            POOL_BWD_N(TX, POOL_NORM_RMS);        \
        else                                      \
            POOL_BWD_N(TX, POOL_NORM_LN);         \
    } while (0)
    if (a->x_dtype == CAD_F32)
        POOL_BWD(float);
    else if (a->x_dtype == CAD_BF16)
        POOL_BWD(bf16_t);
    else
        POOL_BWD(f16_t);
    if (slots) {
        dim3 fgrid((unsigned)((a->D + POOL_FOLD_CH - 1) / POOL_FOLD_CH), 2);
        CAD_LAUNCH(pool_bwd_fold_kernel, fgrid, dim3(POOL_FOLD_CH * POOL_FOLD_SUB), 0, stream, wslots, bslots, a->dweight, a->dbias, sb, g.pieces,
                   a->D);
    }
    return cad_after_launch();
}
