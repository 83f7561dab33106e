// cad_gemm_b16 (include/caduceus_hip.h): D (M x N) = [addend +] A (M x K) . B (K x N) with bf16 operands, fp32 accumulation on
// v_mfma_f32_16x16x32_bf16 and a bf16 result rounded ONCE (or, out_f32, the fp32 sums themselves) -- the dense projections of the generic
// per-op engine (caduceus_amd/engine.py: un-tied, ew_multiply and uni-directional configurations) and their gradients in bf16, which ran
// through torch.mm / hipBLASLt.  The structure is csrc/gemm_f32.hip's: every operand addressed through (row, column) element strides, one
// of which is 1; 256 threads as 2 x 2 waves; a 128 x 128 workgroup tile (4 x 4 MFMA tiles per wave) or, for few tiles and thin results, a
// 64 x 64 one; k walked in chunks of 32 through ONE LDS stage per operand, the next chunk's global loads in flight (registers) while the
// current one is multiplied.  gemm_f32's fragment rule -- MFMA k slot g holds the 8 consecutive k = 8 g .. 8 g + 7 of the chunk -- is
// exactly one bf16x8 operand here, so a chunk is ONE MFMA per tile pair.  Plain global loads, plain LDS accesses, __syncthreads().
//
// LDS: both operands as [row][k], a row = 16 dwords (k pairs) + 1 dword of padding, so the fragment of lane (g, jl) is the four dwords
// 4 g .. 4 g + 3 of row jl (17 jl + 4 g: conflict-free over a 16-lane group).  A k-contiguous operand is staged 8 k per thread (one 16-byte
// load where base, pitch and offset allow it, else eight guarded 2-byte loads) and stored as it lies; a row-contiguous one is staged
// 8 rows x 2 k per thread (two 16-byte loads, or guarded 2-byte loads) and transposed on the way into LDS: 8 dwords (k, k + 1) of 8 rows.
// The launcher orients the product so that D's unit stride runs along the MFMA result's four consecutive rows per lane (it computes
// D^T = B^T . A^T for a row-major D): a lane then stores its four elements as one 8-byte (bf16) or 16-byte (fp32) vector where alignment
// allows it.  The (M tile, N tile) index is flattened onto grid.x (M = all tokens of the token-major out_proj), the batch lies on grid.z.
#include "cad_common.h"

namespace {

constexpr int GB_KC = 32, GB_T = 256;
constexpr int GB_LSTR = GB_KC / 2 + 1;  // dwords per LDS row

struct __attribute__((aligned(8))) GbPack4 {  // four bf16
    uint32_t w[2];
};

// element e (0..7) of a bf16x8 register image
__device__ __forceinline__ uint32_t gb_half(const u32x4& v, int e) { return (v[e >> 1] >> (16 * (e & 1))) & 0xffffu; }

// Staging of one operand tile (BT rows x 32 k) into NV 16-byte register images per thread.
//   KFAST (k is the unit-stride direction): image p = the 8 k = 8 (t & 3) .. + 7 of tile row (t >> 2) + 64 p          (NV = BT / 64)
//   else  (rows are the unit-stride one):   image h = the 8 rows 8 (t % (BT/8)) .. + 7 at k = 2 (t / (BT/8)) + h       (NV = 2; threads with
//                                           t / (BT/8) >= 16 -- the upper half of the 64-row configuration -- stage nothing)
// P: the operand's element (tile row 0, first k of the chunk); rs / ks: element strides of the row and k directions; rows / K: rows and k
// of the matrix left from there; vec: 16-byte loads are aligned (launcher).  Everything outside the matrix is zero.
template <bool KFAST, int BT>
struct GbStage {
    static constexpr int NV = KFAST ? BT / 64 : 2;
    static __device__ __forceinline__ void fetch(const bf16_t* P, int64_t rs, int64_t ks, int64_t rows, int64_t K, bool vec, int t, u32x4* v) {
#pragma unroll
        for (int p = 0; p < NV; ++p) {
            u32x4 x = {0u, 0u, 0u, 0u};
            if constexpr (KFAST) {
                const int64_t row = (t >> 2) + 64 * p, k = 8 * (t & 3);
                if (row < rows && k < K) {
                    const bf16_t* q = P + row * rs + k;
                    if (vec && k + 8 <= K) {
                        x = *(const u32x4*)q;
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (k + e < K) x[e >> 1] |= (uint32_t)q[e].v << (16 * (e & 1));
                    }
                }
            } else {
                const int64_t row = 8 * (t % (BT / 8)), k = 2 * (t / (BT / 8)) + p;
                if (t / (BT / 8) < GB_KC / 2 && row < rows && k < K) {
                    const bf16_t* q = P + k * ks + row;
                    if (vec && row + 8 <= rows) {
                        x = *(const u32x4*)q;
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (row + e < rows) x[e >> 1] |= (uint32_t)q[e].v << (16 * (e & 1));
                    }
                }
            }
            v[p] = x;
        }
    }
    static __device__ __forceinline__ void stash(uint32_t* S, int t, const u32x4* v) {
        if constexpr (KFAST) {
#pragma unroll
            for (int p = 0; p < NV; ++p)
#pragma unroll
                for (int i = 0; i < 4; ++i) S[((t >> 2) + 64 * p) * GB_LSTR + 4 * (t & 3) + i] = v[p][i];
        } else {
            const int row = 8 * (t % (BT / 8)), kp = t / (BT / 8);
            if (kp < GB_KC / 2) {
#pragma unroll
                for (int e = 0; e < 8; ++e) S[(row + e) * GB_LSTR + kp] = gb_half(v[0], e) | (gb_half(v[1], e) << 16);
            }
        }
    }
};

__device__ __forceinline__ u32x4 gb_frag(const uint32_t* S, int row, int g) {
    const uint32_t* p = S + row * GB_LSTR + 4 * g;
    return u32x4{p[0], p[1], p[2], p[3]};
}

// the four results of a lane (rows m .. m + 3 of one column): TO = bf16_t rounds the fp32 sum (+ the widened addend) once, to nearest even
__device__ __forceinline__ float gb_widen(float x) { return x; }
__device__ __forceinline__ float gb_widen(bf16_t x) { return to_f32(x); }

template <typename TO>
__device__ __forceinline__ void gb_store4(TO* D, const TO* add, int64_t rs, int valid, bool vec, f32x4 acc) {
    if (vec && valid == 4) {
        if constexpr (sizeof(TO) == 4) {
            f32x4 r = acc;
            if (add) r = *(const f32x4*)add + acc;
            *(f32x4*)D = r;
        } else {
            float r[4] = {acc[0], acc[1], acc[2], acc[3]};
            if (add) {
                const GbPack4 q = *(const GbPack4*)add;
                r[0] += cad_bits2f(q.w[0] << 16), r[1] += cad_bits2f(q.w[0] & 0xffff0000u);
                r[2] += cad_bits2f(q.w[1] << 16), r[3] += cad_bits2f(q.w[1] & 0xffff0000u);
            }
            GbPack4 o;
            o.w[0] = (uint32_t)from_f32<bf16_t>(r[0]).v | ((uint32_t)from_f32<bf16_t>(r[1]).v << 16);
            o.w[1] = (uint32_t)from_f32<bf16_t>(r[2]).v | ((uint32_t)from_f32<bf16_t>(r[3]).v << 16);
            *(GbPack4*)D = o;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r < valid) {
                const float s = add ? gb_widen(add[r * rs]) + acc[r] : acc[r];
                D[r * rs] = from_f32<TO>(s);
            }
    }
}

// KA / KB: the operand's k direction is the contiguous one; WT: MFMA tiles per wave and dimension; TO: bf16_t or float result.
// a.A / a.B (and a.D / a.addend for TO = bf16_t) address bf16 elements behind the struct's float pointers.
template <bool KA, bool KB, int WT, typename TO>
__global__ __launch_bounds__(GB_T, 2) void gemm_b16_kernel(cad_gemm_f32_args a, int vec_a, int vec_b, int vec_d) {
    constexpr int BT = 32 * WT, WS = 16 * WT;  // rows (= columns) of the workgroup tile / of a wave's share
    typedef GbStage<KA, BT> SA;
    typedef GbStage<KB, BT> SB;
    __shared__ uint32_t As[BT * GB_LSTR];
    __shared__ uint32_t Bs[BT * GB_LSTR];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int g = lane >> 4, jl = lane & 15;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t gn = (a.N + BT - 1) / BT;
    const int64_t m0 = ((int64_t)blockIdx.x / gn) * BT, n0 = ((int64_t)blockIdx.x % gn) * BT;
    const int64_t a_rstr = a.a_rs, a_kstr = a.a_cs, b_rstr = a.b_cs, b_kstr = a.b_rs;  // strides of the tile-row and k directions
    const bf16_t* pa = (const bf16_t*)a.A + (int64_t)blockIdx.z * a.a_bs + m0 * a_rstr;
    const bf16_t* pb = (const bf16_t*)a.B + (int64_t)blockIdx.z * a.b_bs + n0 * b_rstr;
    u32x4 ra[SA::NV], rb[SB::NV];
    auto fetch = [&](int64_t k0) {
        SA::fetch(KA ? pa + k0 : pa + k0 * a_kstr, a_rstr, a_kstr, a.M - m0, a.K - k0, vec_a != 0, t, ra);
        SB::fetch(KB ? pb + k0 : pb + k0 * b_kstr, b_rstr, b_kstr, a.N - n0, a.K - k0, vec_b != 0, t, rb);
    };
    f32x4 acc[WT][WT];
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    SA::stash(As, t, ra);
    SB::stash(Bs, t, rb);
    __syncthreads();
    for (int64_t k0 = 0; k0 < a.K; k0 += GB_KC) {
        const bool more = k0 + GB_KC < a.K;
        if (more) fetch(k0 + GB_KC);
        u32x4 bf[WT];
#pragma unroll
        for (int j = 0; j < WT; ++j) bf[j] = gb_frag(Bs, wn * WS + 16 * j + jl, g);
#pragma unroll
        for (int i = 0; i < WT; ++i) {
            const u32x4 af = gb_frag(As, wm * WS + 16 * i + jl, g);
#pragma unroll
            for (int j = 0; j < WT; ++j) acc[i][j] = cad_mfma_16x16x32_bf16(af, bf[j], acc[i][j]);
        }
        __syncthreads();  // every wave has read the stage
        if (more) {
            SA::stash(As, t, ra);
            SB::stash(Bs, t, rb);
            __syncthreads();
        }
    }
    // lane (g, jl) of tile (i, j): column n0 + wn WS + 16 j + jl, rows m0 + wm WS + 16 i + 4 g + r
    TO* D = (TO*)a.D + (int64_t)blockIdx.z * a.d_bs;
    const TO* add = a.addend ? (const TO*)a.addend + (int64_t)blockIdx.z * a.d_bs : nullptr;
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) {
            const int64_t n = n0 + wn * WS + 16 * j + jl, m = m0 + wm * WS + 16 * i + 4 * g;
            if (n < a.N && m < a.M) {
                const int64_t o = m * a.d_rs + n * a.d_cs, left = a.M - m;
                gb_store4<TO>(D + o, add ? add + o : nullptr, a.d_rs, left < 4 ? (int)left : 4, vec_d != 0, acc[i][j]);
            }
        }
}

bool gb_aligned(const void* p, unsigned bytes) { return ((uintptr_t)p % bytes) == 0; }

}  // namespace

extern "C" int cad_gemm_b16(const cad_gemm_f32_args* a0, int out_f32, void* stream) {
    CAD_CHECK_ARG(a0 && a0->A && a0->B && a0->D && a0->M > 0 && a0->N > 0 && a0->K > 0 && a0->batch >= 1);
    CAD_CHECK_ARG((a0->a_rs == 1 || a0->a_cs == 1) && (a0->b_rs == 1 || a0->b_cs == 1));  // one contiguous direction per operand
    CAD_CHECK_ARG(a0->a_rs >= 0 && a0->a_cs >= 0 && a0->b_rs >= 0 && a0->b_cs >= 0 && a0->d_rs >= 1 && a0->d_cs >= 1);
    cad_gemm_f32_args a = *a0;
    if (a.d_rs != 1 && a.d_cs == 1) {  // D^T = B^T . A^T: D's unit stride along the four consecutive rows a lane holds
        a.A = a0->B, a.B = a0->A;
        a.M = a0->N, a.N = a0->M;
        a.a_rs = a0->b_cs, a.a_cs = a0->b_rs, a.b_rs = a0->a_cs, a.b_cs = a0->a_rs;
        a.d_rs = a0->d_cs, a.d_cs = a0->d_rs;
        a.a_bs = a0->b_bs, a.b_bs = a0->a_bs;
    }
    // 128 x 128 tiles where they fill the chip without multiplying padding; 64 x 64 for few tiles and thin results (cad_gemm_f32's rule)
    const int64_t t128 = ((a.N + 127) / 128) * ((a.M + 127) / 128) * a.batch;
    const bool small = a.M <= 64 || a.N <= 64 || t128 < 2 * (int64_t)cad_cu_count();
    const int bt = small ? 64 : 128;
    const int64_t tiles = ((a.N + bt - 1) / bt) * ((a.M + bt - 1) / bt);
    CAD_CHECK_ARG(tiles <= 0x7fffffffLL && a.batch <= 65535);
    const bool ka = a.a_cs == 1, kb = a.b_rs == 1;  // (a 1 x 1 stride pair counts as k-contiguous)
    const bool one = a.batch == 1;
    const int vec_a = gb_aligned(a.A, 16) && (ka ? a.a_rs : a.a_cs) % 8 == 0 && (one || a.a_bs % 8 == 0);
    const int vec_b = gb_aligned(a.B, 16) && (kb ? a.b_cs : a.b_rs) % 8 == 0 && (one || a.b_bs % 8 == 0);
    const unsigned dv = out_f32 ? 16 : 8;  // bytes of a lane's four results
    const int vec_d = a.d_rs == 1 && gb_aligned(a.D, dv) && (!a.addend || gb_aligned(a.addend, dv)) && a.d_cs % 4 == 0 &&
                      (one || a.d_bs % 4 == 0);
    CadProfScope prof(8, stream);
    dim3 grid((unsigned)tiles, 1, (unsigned)a.batch), block(GB_T);
#define GB_LAUNCH2(WT, TO)                                                                                       \
    do {                                                                                                         \
        if (ka && kb)                                                                                            \
            CAD_LAUNCH((gemm_b16_kernel<true, true, WT, TO>), grid, block, 0, stream, a, vec_a, vec_b, vec_d);   \
        else if (ka)                                                                                             \
            CAD_LAUNCH((gemm_b16_kernel<true, false, WT, TO>), grid, block, 0, stream, a, vec_a, vec_b, vec_d);  \
        else if (kb)                                                                                             \
            CAD_LAUNCH((gemm_b16_kernel<false, true, WT, TO>), grid, block, 0, stream, a, vec_a, vec_b, vec_d);  \
        else                                                                                                     \
            CAD_LAUNCH((gemm_b16_kernel<false, false, WT, TO>), grid, block, 0, stream, a, vec_a, vec_b, vec_d); \
    } while (0)
#define GB_LAUNCH(WT)              \
    do {                           \
        if (out_f32)               \
            GB_LAUNCH2(WT, float); \
        else                       \
            GB_LAUNCH2(WT, bf16_t); \
    } while (0)
    if (small)
        GB_LAUNCH(2);
    else
        GB_LAUNCH(4);
#undef GB_LAUNCH
#undef GB_LAUNCH2
    return cad_after_launch();
}
