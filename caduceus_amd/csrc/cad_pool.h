// What the pool head's forward (pool.hip) and backward (pool_bwd.hip) share about pooling: the window's span and multiplicities
// (pool_span_of), torch.max's maximum, the choice of lane map and the forward's piece geometry.  pool.hip's header describes all of it.
// The normed row itself -- lane maps, loads, statistics, scale, served type pairs -- is cad_rownorm.h's.
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

// the lane map a call takes: the vector map where D % 4 == 0 and the row operands are 16-byte aligned
inline bool pool_vec(int D, const void* x, const void* residual_in, const void* weight, const void* bias) {
    return (D % 4) == 0 && (((uintptr_t)x | (uintptr_t)residual_in | (uintptr_t)weight | (uintptr_t)bias) % 16) == 0;
}

}  // namespace
