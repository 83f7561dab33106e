// Plain-C++ types and conversions shared by the product primitives (cad_prims_gfx950.h) and their host restatement (tests/emu/cad_prims_emu.h).
// Included by those two headers once `__device__` / `__forceinline__` mean something (HIP runtime header or the emulator's).
#pragma once
#include <stdint.h>

#define CAD_WAVE 64
#define CAD_MAX_DEVICES 64   // per-device launch-attribute caches (GP_BIG_LDS / SC_BIG_LDS)

// ---- small numeric helpers ---------------------------------------------------------------------------------
typedef float f32x2 __attribute__((vector_size(8)));  // maps to v_pk_{mul,fma,add}_f32 on gfx950
typedef float f32x4 __attribute__((vector_size(16)));
typedef uint32_t u32x2 __attribute__((vector_size(8)));
typedef uint32_t u32x4 __attribute__((vector_size(16)));

struct bf16_t {
    uint16_t v;
};
struct f16_t {  // IEEE binary16 bits (the opt-in fp16 activations; arithmetic stays fp32)
    uint16_t v;
};
// the bf16-only tricks (bf16 1.0 MFMA selectors, v_perm widening, the packed slab / concurrent fold) test this, not sizeof(T) == 2
template <typename T>
struct cad_is_bf16 {
    static constexpr bool value = false;
};
template <>
struct cad_is_bf16<bf16_t> {
    static constexpr bool value = true;
};
template <typename T>
struct cad_is_f16 {
    static constexpr bool value = false;
};
template <>
struct cad_is_f16<f16_t> {
    static constexpr bool value = true;
};

__device__ __forceinline__ float cad_bits2f(uint32_t u) {
    union {
        uint32_t u;
        float f;
    } c;
    c.u = u;
    return c.f;
}
__device__ __forceinline__ uint32_t cad_f2bits(float f) {
    union {
        uint32_t u;
        float f;
    } c;
    c.f = f;
    return c.u;
}
__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(bf16_t x) { return cad_bits2f((uint32_t)x.v << 16); }
template <typename T>
__device__ __forceinline__ T from_f32(float f);
template <>
__device__ __forceinline__ float from_f32<float>(float f) {
    return f;
}
template <>
__device__ __forceinline__ bf16_t from_f32<bf16_t>(float f) {  // round-to-nearest-even, NaN preserved
    uint32_t u = cad_f2bits(f);
    bf16_t r;
    if ((u & 0x7fffffffu) > 0x7f800000u) {
        r.v = (uint16_t)((u >> 16) | 0x40);
    } else {
        u += 0x7fffu + ((u >> 16) & 1u);
        r.v = (uint16_t)(u >> 16);
    }
    return r;
}

// binary16 <-> fp32 in plain C++ (the host emulator's conversion; the device uses v_cvt_f16_f32 / v_cvt_f32_f16 behind the primitives
// seam).  Round-to-nearest-even; beyond 65504 (after rounding) +-inf, never saturated; NaN stays NaN (quiet, sign kept); subnormals exact.
// Float-arithmetic formulation of the FP16 library (Maratyszcza, MIT): the scaled add rounds the mantissa in the FPU.
__device__ __forceinline__ uint16_t cad_f32_to_f16_soft(float f) {
    const float scale_to_inf = cad_bits2f(0x77800000u);   // 2^112
    const float scale_to_zero = cad_bits2f(0x08800000u);  // 2^-110
    const uint32_t w = cad_f2bits(f);
    const uint32_t shl1_w = w + w;
    const uint32_t sign = w & 0x80000000u;
    float base = (cad_bits2f(w & 0x7fffffffu) * scale_to_inf) * scale_to_zero;
    uint32_t bias = shl1_w & 0xff000000u;
    if (bias < 0x71000000u) bias = 0x71000000u;
    base = cad_bits2f((bias >> 1) + 0x07800000u) + base;
    const uint32_t bits = cad_f2bits(base);
    const uint32_t nonsign = ((bits >> 13) & 0x00007c00u) + (bits & 0x00000fffu);
    return (uint16_t)((sign >> 16) | (shl1_w > 0xff000000u ? 0x7e00u : nonsign));
}
__device__ __forceinline__ float cad_f16_to_f32_soft(uint16_t h) {
    const uint32_t w = (uint32_t)h << 16;
    const uint32_t sign = w & 0x80000000u;
    const uint32_t two_w = w + w;
    const float normalized = cad_bits2f((two_w >> 4) + 0x70000000u) * cad_bits2f(0x07800000u);  // exponent offset (0xE0 << 23), 2^-112
    const float denormalized = cad_bits2f((two_w >> 17) | 0x3f000000u) - 0.5f;
    const uint32_t r = two_w < (1u << 27) ? cad_f2bits(denormalized) : cad_f2bits(normalized);
    return cad_bits2f(sign | r);
}
