// Host restatement of the fp16 primitives of cad_prims_gfx950.h (test infrastructure, like cad_prims_emu.h): the binary16 conversions in
// plain C++ (cad_types.h) and v_mfma_f32_16x16x32_f16 with the operand layout of the bf16 form.
#pragma once
#include <cstring>

__device__ __forceinline__ uint16_t cad_f32_to_f16(float f) { return cad_f32_to_f16_soft(f); }
__device__ __forceinline__ float cad_f16_to_f32(uint16_t h) { return cad_f16_to_f32_soft(h); }
__device__ __forceinline__ uint32_t cad_pack_f16x2(float lo, float hi) {
    return (uint32_t)cad_f32_to_f16_soft(lo) | ((uint32_t)cad_f32_to_f16_soft(hi) << 16);
}

__device__ __forceinline__ f32x4 cad_mfma_16x16x32_f16(u32x4 a, u32x4 b, f32x4 c) {
    const int lane = emu::lane_id();
    const int col = lane & 15, rg = lane >> 4;
    float bk[32];     // B[k][col]
    float ak[4][32];  // A[4 rg + r][k]
    for (int h = 0; h < 2; ++h) {
        const uint64_t* pb = emu_publish((uint64_t)b[2 * h] | ((uint64_t)b[2 * h + 1] << 32));
        for (int g = 0; g < 4; ++g) {
            const uint64_t vb = pb[g * 16 + col];
            for (int t = 0; t < 4; ++t) bk[8 * g + 4 * h + t] = cad_f16_to_f32_soft((uint16_t)((vb >> (16 * t)) & 0xffffu));
        }
        const uint64_t* pa = emu_publish((uint64_t)a[2 * h] | ((uint64_t)a[2 * h + 1] << 32));
        for (int g = 0; g < 4; ++g)
            for (int r = 0; r < 4; ++r) {
                const uint64_t va = pa[g * 16 + 4 * rg + r];
                for (int t = 0; t < 4; ++t) ak[r][8 * g + 4 * h + t] = cad_f16_to_f32_soft((uint16_t)((va >> (16 * t)) & 0xffffu));
            }
    }
    f32x4 d = c;
    for (int r = 0; r < 4; ++r) {
        float s = c[r];
        for (int k = 0; k < 32; ++k) s += ak[r][k] * bk[k];
        d[r] = s;
    }
    return d;
}
