// Streaming stores for the HBM-bound kernels around the scans (projections, conv1d, add + norm).
// Their outputs -- hundreds of MB per launch -- are written once and read by a LATER kernel; written with ordinary stores they
// displace the lines the kernels are about to read.  Nontemporal stores, measured on the MI355X (profiles/r03_ab_nt_stores.txt):
// in_proj 0.191 -> 0.151 ms (3.5 -> 4.5 TB/s), d(y) 0.100 -> 0.084 ms stand-alone; a whole training step 131.4 -> 129.8 ms with
// all three families on (same box).  The scans keep ordinary stores (no gain there, same file) and do not include this header.
// CAD_NT_MASK (tuning builds only): bit 0 projections, bit 1 conv1d, bit 2 add + norm.
#pragma once
#include "cad_common.h"

#define CAD_NT_MASK 7
#define CAD_STREAM_PROJ 0
#define CAD_STREAM_CONV 1
#define CAD_STREAM_NORM 2

template <int FAMILY, typename V>
__device__ __forceinline__ void cad_store_stream(V* p, V v) {
    if constexpr ((CAD_NT_MASK >> FAMILY) & 1)
        cad_nt_store(p, v);
    else
        *p = v;
}
// N fp32 values -> N contiguous elements of T at dst (as cad_cvt_store), streamed
template <int FAMILY, typename T, int N>
__device__ __forceinline__ void cad_cvt_store_stream(T* dst, const float* v);
template <>
__device__ __forceinline__ void cad_cvt_store_stream<CAD_STREAM_NORM, float, 4>(float* dst, const float* v) {
    cad_store_stream<CAD_STREAM_NORM>((f32x4*)dst, f32x4{v[0], v[1], v[2], v[3]});
}
template <>
__device__ __forceinline__ void cad_cvt_store_stream<CAD_STREAM_NORM, bf16_t, 4>(bf16_t* dst, const float* v) {
    cad_store_stream<CAD_STREAM_NORM>((u32x2*)dst, u32x2{cad_pack_bf16x2(v[0], v[1]), cad_pack_bf16x2(v[2], v[3])});
}
template <>
__device__ __forceinline__ void cad_cvt_store_stream<CAD_STREAM_NORM, f16_t, 4>(f16_t* dst, const float* v) {
    cad_store_stream<CAD_STREAM_NORM>((u32x2*)dst, u32x2{cad_pack_f16x2(v[0], v[1]), cad_pack_f16x2(v[2], v[3])});
}

// ---- 16-byte stores out of the MFMA D layout (the token-major writer cad_proj_xTw) --------------------------------------------------------
// A D lane (row group g = lane >> 4, column jl = lane & 15) holds four consecutive ROWS of its column = 8 packed bytes of a token-major
// output row; two accumulator tiles 16 rows apart (a, then b) give the column 64 contiguous bytes, spread as 8-byte pieces over the four
// row groups: a at 8 g, b at 32 + 8 g.  One v_permlane16_swap per dword (odd lane rows of a <-> even lane rows of b) leaves every lane
// with 16 CONTIGUOUS bytes of that run, at byte cad_d_pair16_off(lane) of it: the run leaves as ONE 16-byte store per lane (16 columns x
// 64 bytes per instruction) instead of two 8-byte ones (16 columns x 32 bytes each).  Same bytes, same addresses, half the instructions.
// Every lane of the wave must call cad_d_pair16 (no divergent caller); the store itself may be masked.
// They stay ordinary stores: the streaming policy on them is neutral in the layer (profiles/r09_ab_proj_store.txt).  cad_gemm_stream's
// token-major mode has the same D layout and measured the same way, but keeps its 8-byte stores: its instruction counts are pinned
// (tests/test_isa_async.py).
__device__ __forceinline__ u32x4 cad_d_pair16(u32x2 a, u32x2 b) {
#ifdef CAD_EMU
    const bool odd = (emu::lane_id() >> 4) & 1;
    const u32x2 give = odd ? a : b;
    const uint64_t got = emu_exchange((uint64_t)give[0] | ((uint64_t)give[1] << 32), emu::lane_id() ^ 16);
    const u32x2 take = {(uint32_t)got, (uint32_t)(got >> 32)};
    if (odd)
        a = take;
    else
        b = take;
#else
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const auto r = __builtin_amdgcn_permlane16_swap(a[k], b[k], false, false);
        a[k] = r[0], b[k] = r[1];
    }
#endif
    return u32x4{a[0], a[1], b[0], b[1]};
}
__device__ __forceinline__ int cad_d_pair16_off(int lane) {
    const int g = lane >> 4;
    return 32 * (g & 1) + 16 * (g >> 1);
}
