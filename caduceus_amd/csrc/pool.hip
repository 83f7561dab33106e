// Pool head (include/caduceus_hip.h, cad_pool_head): the backbone's final add + RMSNorm / LayerNorm and the pooling over the sequence in
// one pass over the pre-norm stream.  Nothing of size L is written: what leaves the kernels is the fixed-order partials in the caller's
// scratch and out (S, B, D) fp32.
//
// A row's normed value y is cad_add_norm_fwd's (csrc/addnorm.hip, swap_flip = 0): the add, the statistics in that kernel's summation order
// (a lane's channels in ascending order, the xor butterfly of cad_rownorm.h, the two-pass LayerNorm variance), the scale, the rounding to
// y_dtype.  The lane map is that kernel's too -- 4 consecutive channels per lane and 256-channel step where D % 4 == 0 and the operands
// are 16-byte aligned (add_norm_fwd_vec_kernel), channels lane + 64 k otherwise (add_norm_fwd_kernel) -- and pool_row below is a THIRD
// statement of the per-lane walk next to cad_rownorm.h's: a change to the order in which the forward kernels sum a row, or to where they
// round, is a change to make here as well.
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
pool_geom pool_geometry(int64_t n) {
    const int64_t chunks = ((n + 1) / 2 + POOL_CHUNK - 1) / POOL_CHUNK;
    pool_geom g;
    g.cpp = (chunks + POOL_PIECES_MAX - 1) / POOL_PIECES_MAX;
    g.pieces = (chunks + g.cpp - 1) / g.cpp;
    return g;
}

// upper bound, known on the host, of the rows a pair pools
int64_t pool_rows(int mode, int64_t L, int64_t half) {
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

// v = x + residual of one row, in place -> the normed row as a store in TY leaves it (cad_add_norm_fwd's y, see the header of this file)
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

// an item's value: the two products are rounded before the add, so that (a, b) and (b, a) give the same bits
__device__ __forceinline__ float pool_pair(float ca, float ya, float cb, float yb) {
#pragma clang fp contract(off)
    const float pa = ca * ya, pb = cb * yb;
    return pa + pb;
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

__device__ __forceinline__ pool_span pool_span_of(const cad_pool_head_args& a, int64_t sb) {
    pool_span w;
    if (a.mode != CAD_POOL_WINDOW) {
        w.lo = 0, w.hi = a.L - 1, w.c_first = 1.f, w.c_last = 1.f;
        return w;
    }
    // offsets k = -half .. half around centre c, clamp(c + k, 0, L - 1): a centre further out than half + 1 beyond an end puts every
    // offset on that end, as half + 1 beyond it does (no int64 overflow of c +- half)
    int64_t c = a.centre[sb];
    c = c < -a.half - 1 ? -a.half - 1 : (c > a.L + a.half ? a.L + a.half : c);
    const int64_t lo = c - a.half, hi = c + a.half, last = a.L - 1;
    w.lo = lo < 0 ? 0 : (lo > last ? last : lo);
    w.hi = hi < 0 ? 0 : (hi > last ? last : hi);
    if (last == 0) {  // one row takes every offset
        w.c_first = (float)(2 * a.half + 1), w.c_last = 0.f;
        return w;
    }
    const int64_t n_first = (hi < 0 ? hi : 0) - lo + 1;       // offsets landing at or before row 0
    const int64_t n_last = hi - (lo > last ? lo : last) + 1;  // offsets landing at or beyond row L - 1
    w.c_first = (float)(n_first > 0 ? n_first : 0);
    w.c_last = (float)(n_last > 0 ? n_last : 0);
    return w;
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
    const pool_span span = pool_span_of(a, sb);
    const TX* x = (const TX*)a.x + sb * a.L * D;
    const float* res = a.residual_in ? a.residual_in + sb * a.L * D : nullptr;

    float wreg[KMAX][W], breg[KMAX][W], acc[KMAX][W];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int c = pool_chan<W>(lane, k);
#pragma unroll
        for (int q = 0; q < W; ++q) wreg[k][q] = 1.f, breg[k][q] = 0.f, acc[k][q] = is_max ? -INFINITY : 0.f;
        if (c < D && normed) {
            pool_ld<float, W>(a.weight + c, wreg[k]);
            if (has_bias) pool_ld<float, W>(a.bias + c, breg[k]);
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
                        const int c = pool_chan<W>(lane, k);
#pragma unroll
                        for (int q = 0; q < W; ++q) v[u][e][k][q] = 0.f;
                        if (c < D) {
                            pool_ld<TX, W>(x + row * D + c, v[u][e][k]);
                            if (res) {
                                float t[W];
                                pool_ld<float, W>(res + row * D + c, t);
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
                    pool_row<TY, W, KMAX>(v[u][0], wreg, breg, has_bias, D, a.eps, a.is_rms, lane);
                    pool_row<TY, W, KMAX>(v[u][1], wreg, breg, has_bias, D, a.eps, a.is_rms, lane);
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
        const int c = pool_chan<W>(lane, k);
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

bool pool_types_ok(int x_dtype, int y_dtype) {  // cad_add_norm_fwd's pairs
    return (x_dtype == CAD_F32 && (y_dtype == CAD_F32 || y_dtype == CAD_BF16 || y_dtype == CAD_F16)) ||
           (x_dtype == CAD_BF16 && y_dtype == CAD_BF16) || (x_dtype == CAD_F16 && y_dtype == CAD_F16);
}

}  // namespace

extern "C" int cad_pool_head_supported(int D, int x_dtype, int y_dtype, int mode, int64_t half) {
    return D >= 1 && D <= POOL_DMAX && pool_types_ok(x_dtype, y_dtype) &&
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
    const bool vec = (a->D % 4) == 0 &&
                     (((uintptr_t)a->x | (uintptr_t)a->residual_in | (uintptr_t)a->weight | (uintptr_t)a->bias) % 16) == 0;
    dim3 grid((unsigned)(sb * g.pieces)), block(64 * POOL_WAVES);
#define POOL_FWD(TX, TY)                                                                                         \
    do {                                                                                                         \
        if (vec && a->D <= 256)                                                                                  \
            CAD_LAUNCH((pool_partial_kernel<TX, TY, 4, 1>), grid, block, 0, stream, *a, g.cpp, g.pieces);        \
        else if (vec && a->D <= 512)                                                                             \
            CAD_LAUNCH((pool_partial_kernel<TX, TY, 4, 2>), grid, block, 0, stream, *a, g.cpp, g.pieces);        \
        else if (vec)                                                                                            \
            CAD_LAUNCH((pool_partial_kernel<TX, TY, 4, 4>), grid, block, 0, stream, *a, g.cpp, g.pieces);        \
        else                                                                                                     \
            CAD_LAUNCH((pool_partial_kernel<TX, TY, 1, 16>), grid, block, 0, stream, *a, g.cpp, g.pieces);       \
    } while (0)
    if (a->x_dtype == CAD_F32 && a->y_dtype == CAD_F32)
        POOL_FWD(float, float);
    else if (a->x_dtype == CAD_F32 && a->y_dtype == CAD_BF16)
        POOL_FWD(float, bf16_t);
    else if (a->x_dtype == CAD_BF16 && a->y_dtype == CAD_BF16)
        POOL_FWD(bf16_t, bf16_t);
    else if (a->x_dtype == CAD_F32 && a->y_dtype == CAD_F16)
        POOL_FWD(float, f16_t);
    else
        POOL_FWD(f16_t, f16_t);
    const float n = a->mode == CAD_POOL_WINDOW ? (float)(2 * a->half + 1) : (float)a->L;
    const int64_t total = sb * a->D;
    CAD_LAUNCH(pool_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, *a, g.pieces, n);
    return cad_after_launch();
}
