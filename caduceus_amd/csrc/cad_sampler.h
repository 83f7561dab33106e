// The token sampler (include/caduceus_hip.h, rules 1 - 6 above cad_sampler_args), stated once for the kernels that draw an id from a
// logit row: cad_sample_tokens and the tail of cad_decode_token (decode.hip: one wave64 per row) and the tile epilogue of
// cad_lm_head_unmask (unmask.hip: a row's 16 logits on 16 lanes, four rows per wave).
// W = the number of lanes that hold one row (64 or 16); every shuffle stays inside the row's group of W lanes, and every lane of the
// wave calls, in wave-uniform control flow.  A row whose lanes >= V hold nothing goes through the same floating-point operations in
// the same order at either width: the rank, the top-p cumulative and the CDF are sequential in id order, the maximum is exact, and the
// sum butterfly of the wider group adds the upper lanes' zeros first (m = 32, 16), then runs the narrower group's steps 8 .. 1.
#pragma once
#include <math.h>

#include "cad_common.h"

// what the entry points accept (anything else: CAD_ERR_BAD_ARG before a launch)
static inline bool dc_sampler_ok(const cad_sampler_args& s) {
    return s.top_k >= 0 && s.top_p >= 0.f && s.top_p <= 1.f && s.temperature > 0.f;
}

// ---- uniforms: Philox4x32-10, counter (r, position), key seed; no state in memory ----------------------------------------------------
__device__ __forceinline__ float dc_uniform(uint64_t seed, uint64_t r, uint64_t position) {
    uint32_t c0 = (uint32_t)r, c1 = (uint32_t)(r >> 32), c2 = (uint32_t)position, c3 = (uint32_t)(position >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return (float)(c0 >> 8) * 5.9604644775390625e-8f;  // 24 bits -> [0, 1)
}

// ---- reductions over a group of W lanes (xor butterfly W / 2 .. 1; every lane of the group receives the result) ----------------------
template <int W>
__device__ __forceinline__ float dc_wave_max(float v) {
#pragma unroll
    for (int m = W / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
template <int W>
__device__ __forceinline__ float dc_wave_sum(float v) {
#pragma unroll
    for (int m = W / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
template <int W>
__device__ __forceinline__ int dc_wave_min_int(int v) {
#pragma unroll
    for (int m = W / 2; m >= 1; m >>= 1) {
        const int o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}
template <int W>
__device__ __forceinline__ int dc_wave_max_int(int v) {
#pragma unroll
    for (int m = W / 2; m >= 1; m >>= 1) {
        const int o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

// The sampler of one row by one group of W lanes: lane v < V of the group holds logit v (already masked), `lane` is the lane's place in
// its group, every lane calls; returns the id to every lane of the group.  V <= W.
template <int W = 64>
__device__ __forceinline__ int dc_sample_row(float x, int V, int top_k, float top_p, float temperature, float u, int lane) {
    const bool in = lane < V;
    x = in ? x : -INFINITY;
    // rank by (logit descending, id ascending): the number of entries that come before this one
    int rank = 0;
    for (int j = 0; j < V; ++j) {  // wave-uniform trip count
        const float xj = __shfl(x, j, W);
        rank += (xj > x || (xj == x && j < lane)) ? 1 : 0;
    }
    if (top_k == 1) return dc_wave_min_int<W>(in && rank == 0 ? lane : 64) & 63;
    const int keep_n = (top_k == 0 || top_k > V) ? V : top_k;
    bool keep = in && rank < keep_n;
    if (temperature != 1.0f) x = x / temperature;
    const float mx = dc_wave_max<W>(keep ? x : -INFINITY);
    float e = keep ? cad_exp2((x - mx) * CAD_LOG2E) : 0.f;
    if (!(e >= 0.f)) e = 0.f;  // (-inf) - (-inf): a row with every kept logit masked
    if (top_p > 0.f && top_p < 1.f) {
        const float p = e / dc_wave_sum<W>(e);
        float cum = 0.f;  // ascending cumulative probability: this entry and everything ranked behind it, added in id order
        for (int j = 0; j < V; ++j) {
            const float pj = __shfl(p, j, W);
            const int rj = __shfl(rank, j, W);
            cum += (rj >= rank && rj < keep_n) ? pj : 0.f;
        }
        if (keep && rank != 0 && cum <= 1.0f - top_p) keep = false, e = 0.f;
    }
    float cdf = 0.f;  // inclusive, in id order
    for (int j = 0; j < V; ++j) {
        const float ej = __shfl(e, j, W);
        cdf += j <= lane ? ej : 0.f;
    }
    const float total = __shfl(cdf, V - 1, W);
    const float t = u * total;
    const int first = dc_wave_min_int<W>(keep && e > 0.f && cdf > t ? lane : 64);
    const int last = dc_wave_max_int<W>(keep && e > 0.f ? lane : -1);
    const int best = dc_wave_min_int<W>(in && rank == 0 ? lane : 64);
    return first < 64 ? first : (last >= 0 ? last : (best & 63));
}
