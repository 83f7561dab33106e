// The W-stationary MFMA projections, element-type templates (instantiated for bf16 by gemm.hip, for fp16 by gemm_f16.hip), and the launch
// helpers all three kernel families share.
//
// cad_proj_wxT:   out (M, T) channel-major  =  W (M, K)  .  X (T, K)^T          (in_proj;  d(y) = W_out^T . dout^T)
//   * "W-stationary": a workgroup owns 128 * MB rows of W; every wave keeps its 16 * MB rows as MFMA B-fragments in
//     registers for the whole launch (MB * K / 32 * 4 VGPRs) and the workgroup walks a contiguous range of tokens;
//   * X travels global -> LDS by LDS-DMA (cad_glds16) in blocks of 64 tokens, double buffered, one barrier per block; the
//     16-byte pieces of a token row are XOR-swizzled through the per-lane SOURCE address (piece ^ (token & 15)), which
//     makes the ds_read_b128 of the A-fragments (16 tokens x 4 k-groups per instruction) bank-conflict-free;
//   * v_mfma_f32_16x16x32_bf16 with A = X fragment (rows = tokens), B = W fragment (columns = output channels): a D lane
//     then holds FOUR CONSECUTIVE TOKENS of one output channel -- exactly what the channel-major layout wants -- and
//     writes them (packed bf16) into a wave-private LDS tile, from which full 128-byte token runs go to HBM with
//     16-byte stores.
// The per-token arithmetic is independent of the token's position (fixed k order inside the MFMA), so both strands and
// both directions of the t-frame get bit-identical projections: RC-equivariance stays exact.
#pragma once
#include "cad_common.h"
#include "cad_stream.h"

namespace {

#define GP_WAVES 8

// the softplus + bias epilogue of dt_proj: bf16 results take the two-transcendental form (cad_softplus_lowp: exact far inside bf16's
// 8 bits); fp16's 11 bits take the full-accuracy form
template <typename TE>
__device__ __forceinline__ float gp_softplus(float x) {
    if constexpr (cad_is_bf16<TE>::value)
        return cad_softplus_lowp(x);
    else
        return cad_softplus(x);
}

// K = 512 (d_model 512, configs[4]) tuning knobs: W rows per wave / tokens per block / register double-buffering of the A fragments
#define GP_MB16 2
#define GP_NT16 32
#define GP_XFB16 1
template <int KS>
struct GpCfg {
    static constexpr int MB = KS >= 16 ? GP_MB16 : 4;  // 16-row blocks of W per wave: MB * KS * 4 <= 128 VGPRs
    static constexpr int MW = 16 * MB;               // output channels per wave
    static constexpr int MWG = MW * GP_WAVES;        // ... per workgroup
    static constexpr int NT = KS >= 16 ? GP_NT16 : 64;  // tokens per block (two blocks + the staging tiles fit in 160 KB)
    static constexpr int ROWB = KS * 64;             // bytes per token row (K bf16)
    static constexpr int PPR = KS * 4;               // 16-byte pieces per token row
    static constexpr int SW = (PPR < 16 ? PPR : 16) - 1;  // swizzle mask: piece ^= token & SW
    static constexpr int XBUF = NT * ROWB;           // bytes per X block
    static constexpr int SSTR = NT * 2 + 16;         // bytes per output-channel row of the staging tile (16-byte aligned, skewed)
    static constexpr int STAGE = MW * SSTR;
    static constexpr size_t LDS = 2 * (size_t)XBUF + (size_t)GP_WAVES * STAGE;
};

// issue the LDS-DMA of one NT-token block of X (tokens t0 .. t0 + NT - 1; rows beyond T re-read row T - 1, never stored)
template <int KS, typename TE>
__device__ __forceinline__ void gp_issue_block(const TE* X, int64_t ldx, int64_t t0, int64_t T, char* xbuf, int wave, int lane) {
    typedef GpCfg<KS> C;
    constexpr int PIECES = C::NT * C::PPR;           // per block
    constexpr int INSTR = PIECES / 64;               // DMA instructions per block (64 pieces each)
#pragma unroll
    for (int it = 0; it < (INSTR + GP_WAVES - 1) / GP_WAVES; ++it) {
        const int ins = it * GP_WAVES + wave;        // wave-uniform
        if (ins < INSTR) {
            const int p0 = ins * 64;
            const int p = p0 + lane;
            const int t = p / C::PPR, ps = p % C::PPR;           // token row, PHYSICAL piece slot
            const int s = (ps & ~C::SW) | ((ps ^ t) & C::SW);    // logical piece
            int64_t tok = t0 + t;
            tok = tok < T ? tok : T - 1;
            cad_glds16((const char*)(X + tok * ldx) + s * 16, cad_uniform((int)(cad_lds_off(xbuf) + p0 * 16)));
        }
    }
}

__device__ __forceinline__ void gp_wait_dma() { cad_wait_vmcnt<0>(); }

template <typename TE, int KS>
__global__ __launch_bounds__(64 * GP_WAVES, 2) void proj_wxT_kernel(cad_proj_args a) {
    typedef GpCfg<KS> C;
    CAD_DYN_SMEM(char, smem);
    const int lane = threadIdx.x & 63;
    const int wave = cad_uniform(threadIdx.x >> 6);
    const int g = lane >> 4, jl = lane & 15;
    const TE* W = (const TE*)a.W;
    const TE* X = (const TE*)a.X;
    TE* out = (TE*)a.out;
    const int64_t T = a.T;
    const int M = a.M;
    const int m_wave = blockIdx.y * C::MWG + wave * C::MW;  // first output channel of this wave
    // token blocks of this workgroup: b = blockIdx.x, + gridDim.x, ...  Interleaved on purpose: the workgroups that run
    // at the same time then read / write NEIGHBOURING 64-token runs of every row (HBM page locality: a channel-major
    // output row receives one contiguous multi-KB region from the whole grid instead of 128-byte pieces 4 KB apart)
    const int64_t nblk = (T + C::NT - 1) / C::NT;
    const int64_t b0 = blockIdx.x, bstep = gridDim.x;
    if (b0 >= nblk) return;
    char* xb[2] = {smem, smem + C::XBUF};
    char* stage = smem + 2 * C::XBUF + wave * C::STAGE;

    gp_issue_block<KS>(X, a.ldx, b0 * C::NT, T, xb[0], wave, lane);
    // B fragments of this wave's rows of W, resident for the whole launch (rows >= M read as zero)
    u32x4 wf[C::MB][KS];
#pragma unroll
    for (int mb = 0; mb < C::MB; ++mb) {
        const int m = m_wave + mb * 16 + jl;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (m < M) v = *(const u32x4*)(W + (int64_t)m * a.ldw + ks * 32 + g * 8);
            wf[mb][ks] = v;
        }
    }
    gp_wait_dma();
    __syncthreads();

    int cur = 0;
    for (int64_t b = b0; b < nblk; b += bstep, cur ^= 1) {
        if (b + bstep < nblk) gp_issue_block<KS>(X, a.ldx, (b + bstep) * C::NT, T, xb[cur ^ 1], wave, lane);
        const char* xt = xb[cur];
        // A fragments of sub-block q: token t = 16 q + jl, k = 32 ks + 8 g .. + 7  ->  logical piece 4 ks + g, swizzled with the token.
        // Double buffered in registers where they fit (KS <= 8): the reads of sub-block q + 1 are issued before the MFMAs of
        // sub-block q, so that the matrix cores do not idle for an LDS round trip four times per block.
        constexpr int XFB = KS <= 8 ? 2 : GP_XFB16;
        u32x4 xfb[XFB][KS];
        auto load_frags = [&](int q, u32x4* dst) {
            const int t = q * 16 + jl;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int s = ks * 4 + g;
                const int ps = (s & ~C::SW) | ((s ^ t) & C::SW);
                dst[ks] = *(const u32x4*)(xt + t * C::ROWB + ps * 16);
            }
        };
        if constexpr (XFB == 2) load_frags(0, xfb[0]);
#pragma unroll
        for (int q = 0; q < C::NT / 16; ++q) {  // 16-token sub-blocks
            u32x4* xf = xfb[XFB == 2 ? (q & 1) : 0];
            if constexpr (XFB == 2) {
                if (q + 1 < C::NT / 16) load_frags(q + 1, xfb[(q + 1) & 1]);
            } else {
                load_frags(q, xf);
            }
            f32x4 d[C::MB];
#pragma unroll
            for (int mb = 0; mb < C::MB; ++mb) d[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
                for (int mb = 0; mb < C::MB; ++mb) d[mb] = cad_mfma_16x16x32<TE>(xf[ks], wf[mb][ks], d[mb]);
            }
            // lane (m = mb * 16 + jl, g) holds tokens 16 q + 4 g .. + 3 of channel m: 8 bytes into the staging tile
#pragma unroll
            for (int mb = 0; mb < C::MB; ++mb) {
                u32x2 pk;
                pk[0] = cad_pack2_safe<TE>(d[mb][0], d[mb][1]);
                pk[1] = cad_pack2_safe<TE>(d[mb][2], d[mb][3]);
                *(u32x2*)(stage + (mb * 16 + jl) * C::SSTR + (q * 16 + g * 4) * 2) = pk;
            }
        }
        // (the staging tile is written as 8-byte and read as 16-byte vectors: distinct types for the compiler's alias
        // analysis, which may otherwise move the reads above the writes -- on the host emulator build as well)
        asm volatile("" ::: "memory");
        cad_wave_sync();
        // the next block has landed (this wave's share; the barrier below publishes everybody's).  Waited for BEFORE this
        // block's stores are issued, so that the wait never sits behind fresh write acknowledgements.
        gp_wait_dma();
        // staging tile -> HBM: NT / 8 lanes cover the tokens of one channel row (16 bytes each).  All rows are read from the tile
        // first and stored afterwards (one LDS round trip per block instead of one per row group); whole blocks of a fully
        // populated, 16-byte aligned output take the straight-line path.
        const int64_t t0 = b * C::NT;
        constexpr int LPR = C::NT / 8, RPI = 64 / LPR;  // lanes per row, rows per instruction
        u32x4 sv[C::MW / RPI];
#pragma unroll
        for (int r0 = 0; r0 < C::MW; r0 += RPI)
            sv[r0 / RPI] = *(const u32x4*)(stage + (r0 + lane / LPR) * C::SSTR + (lane % LPR) * 16);
        const bool fast = t0 + C::NT <= T && m_wave + C::MW <= M && (a.ldo % 8) == 0 && (((uintptr_t)out) & 15) == 0;  // wave-uniform
        if (fast) {
#pragma unroll
            for (int r0 = 0; r0 < C::MW; r0 += RPI)
                cad_store_stream<CAD_STREAM_PROJ>((u32x4*)(out + (int64_t)(m_wave + r0 + lane / LPR) * a.ldo + t0 + (lane % LPR) * 8),
                                                  sv[r0 / RPI]);
        } else {
#pragma unroll
            for (int r0 = 0; r0 < C::MW; r0 += RPI) {
                const int r = r0 + lane / LPR, c8 = lane % LPR;
                const u32x4 v = sv[r0 / RPI];
                const int m = m_wave + r;
                const int64_t t = t0 + c8 * 8;
                if (m < M) {
                    TE* dst = out + (int64_t)m * a.ldo + t;
                    if (t + 8 <= T && (((uintptr_t)dst) & 15) == 0) {
                        *(u32x4*)dst = v;
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (t + e < T) dst[e].v = (uint16_t)(v[e >> 1] >> (16 * (e & 1)));
                    }
                }
            }
        }
        __syncthreads();  // publishes the next block; orders this block's LDS reads (X tile, staging tile) before their reuse
    }
}

// ---- cad_proj_wx:  out (M, T) = W (M, K) . X (K, T) [+ acc (M, T)],  all channel-major, small K (<= 64) -------------------
// dt_proj (K = dt_rank) and the x_proj input gradient d(xc) = du + W_x^T . d(dbc) (K = dt_rank + 2 d_state): the
// streaming operands are the (M, T) output (and addend); X is a thin (K, T) panel.  Same skeleton as proj_wxT_kernel --
// W-stationary B-fragments, 64-token blocks by LDS-DMA, the D lanes' four consecutive tokens through the per-wave staging
// tile -- except that X is token-contiguous, so the A-fragments (consecutive k per lane) are TRANSPOSED on the way out
// of LDS: ds_read_b64_tr_b16 on the [k][token] tile (cad_lds_read_tr16), two reads per 8 k.  Rows k >= K of the tile are
// zero (written once), so K is padded to 32 / 64 for free.  The 32-byte token segments of a tile row are XOR-swizzled
// with the row (through the DMA source address) so that the eight rows a transposing read touches hit distinct banks.
template <int KS>
struct GxCfg {
    static constexpr int MB = 4, MW = 64, MWG = MW * GP_WAVES, NT = 64;
    static constexpr int KP = 32 * KS;               // tile rows (K padded)
    static constexpr int XROW = NT * 2;              // bytes per tile row
    static constexpr int XBUF = KP * XROW;
    static constexpr int SSTR = NT * 2 + 16;
    static constexpr int STAGE = MW * SSTR;
    static constexpr size_t LDS = 2 * (size_t)XBUF + (size_t)GP_WAVES * STAGE;
};
__device__ __forceinline__ int gx_swz(int row) { return ((row >> 1) & 1) | (((row >> 3) & 1) << 1); }

template <int KS, typename TE>
__device__ __forceinline__ void gx_issue_block(const TE* X, int64_t ldx, int K, int64_t t0, int64_t T, char* xbuf,
                                               int wave, int lane) {
    const int ninstr = K / 8;  // K rows x 8 pieces of 16 bytes, 64 pieces per DMA instruction
    for (int ins = wave; ins < ninstr; ins += GP_WAVES) {  // wave-uniform
        const int p = ins * 64 + lane;
        const int row = p >> 3, pp = p & 7;                        // tile row, PHYSICAL piece
        const int lp = (((pp >> 1) ^ gx_swz(row)) << 1) | (pp & 1);  // logical piece = 8 tokens
        int64_t tok = t0 + lp * 8;
        tok = tok + 8 <= T ? tok : T - 8;                          // tail block: valid data, never stored
        cad_glds16(X + (int64_t)row * ldx + tok, cad_uniform((int)(cad_lds_off(xbuf) + ins * 1024)));
    }
}

template <typename TE, int KS, bool ACC>
__global__ __launch_bounds__(64 * GP_WAVES, 2) void proj_wx_kernel(cad_proj_args a) {
    typedef GxCfg<KS> C;
    CAD_DYN_SMEM(char, smem);
    const int lane = threadIdx.x & 63;
    const int wave = cad_uniform(threadIdx.x >> 6);
    const int g = lane >> 4, jl = lane & 15;
    const TE* W = (const TE*)a.W;
    const TE* X = (const TE*)a.X;
    const TE* acc = (const TE*)a.acc;
    TE* out = (TE*)a.out;
    const int64_t T = a.T;
    const int M = a.M, K = a.K;
    const int m_wave = blockIdx.y * C::MWG + wave * C::MW;
    const int64_t nblk = (T + C::NT - 1) / C::NT;
    const int64_t b0 = blockIdx.x, bstep = gridDim.x;
    if (b0 >= nblk) return;
    char* xb[2] = {smem, smem + C::XBUF};
    char* stage = smem + 2 * C::XBUF + wave * C::STAGE;
    // rows K .. KP-1 of both tiles stay zero for the whole launch
    for (int i = threadIdx.x * 16; i < 2 * C::XBUF; i += 64 * GP_WAVES * 16) {
        const int row = (i % C::XBUF) / C::XROW;
        if (row >= K) *(u32x4*)(smem + i) = u32x4{0u, 0u, 0u, 0u};
    }
    gx_issue_block<KS>(X, a.ldx, K, b0 * C::NT, T, xb[0], wave, lane);
    u32x4 wf[C::MB][KS];
#pragma unroll
    for (int mb = 0; mb < C::MB; ++mb) {
        const int m = m_wave + mb * 16 + jl;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4 v = {0u, 0u, 0u, 0u};
            const int k0 = ks * 32 + g * 8;
            if (m < M && k0 + 8 <= K) v = *(const u32x4*)(W + (int64_t)m * a.ldw + k0);
            wf[mb][ks] = v;
        }
    }
    // optional epilogue: softplus(. + bias[m]) in fp32 (dt_proj + delta_bias + softplus in one pass); the D lane's channel is
    // m_wave + 16 mb + jl
    const bool act_sp = a.act == CAD_ACT_SOFTPLUS_BIAS;  // wave-uniform
    float brow[C::MB];
#pragma unroll
    for (int mb = 0; mb < C::MB; ++mb) {
        const int m = m_wave + mb * 16 + jl;
        brow[mb] = (act_sp && a.bias && m < M) ? a.bias[m] : 0.f;
    }
    gp_wait_dma();
    __syncthreads();

    int cur = 0;
    for (int64_t b = b0; b < nblk; b += bstep, cur ^= 1) {
        if (b + bstep < nblk) gx_issue_block<KS>(X, a.ldx, K, (b + bstep) * C::NT, T, xb[cur ^ 1], wave, lane);
        const char* xt = xb[cur];
        const int64_t t0 = b * C::NT;
        constexpr int LPR = C::NT / 8, RPI = 64 / LPR;
        // the addend rows of this block (plain loads, issued ahead of the MFMA phase)
        u32x4 old[C::MW / RPI];
        if constexpr (ACC) {
#pragma unroll
            for (int r0 = 0; r0 < C::MW; r0 += RPI) {
                const int m = m_wave + r0 + lane / LPR;
                const int64_t t = t0 + (lane % LPR) * 8;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (m < M && t + 8 <= T) v = *(const u32x4*)(acc + (int64_t)m * a.ldacc + t);
                old[r0 / RPI] = v;
            }
        }
#pragma unroll
        for (int q = 0; q < C::NT / 16; ++q) {
            // A fragments by transposing reads: lane (token 16 q + jl, group g) gets k = 32 ks + 8 g .. + 7
            u32x4 xf[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int r0 = ks * 32 + g * 8 + (jl >> 2);  // this lane's SOURCE row of the first 4 x 16 block
                const char* p0 = xt + r0 * C::XROW + ((q ^ gx_swz(r0)) * 32) + (jl & 3) * 8;
                const char* p1 = xt + (r0 + 4) * C::XROW + ((q ^ gx_swz(r0 + 4)) * 32) + (jl & 3) * 8;
                const u32x2 lo = cad_lds_read_tr16(p0), hi = cad_lds_read_tr16(p1);
                xf[ks] = u32x4{lo[0], lo[1], hi[0], hi[1]};
            }
            f32x4 d[C::MB];
#pragma unroll
            for (int mb = 0; mb < C::MB; ++mb) d[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
                for (int mb = 0; mb < C::MB; ++mb) d[mb] = cad_mfma_16x16x32<TE>(xf[ks], wf[mb][ks], d[mb]);
            }
            if (act_sp) {
#pragma unroll
                for (int mb = 0; mb < C::MB; ++mb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) d[mb][r] = gp_softplus<TE>(d[mb][r] + brow[mb]);
            }
#pragma unroll
            for (int mb = 0; mb < C::MB; ++mb) {
                u32x2 pk;
                pk[0] = cad_pack2_safe<TE>(d[mb][0], d[mb][1]);
                pk[1] = cad_pack2_safe<TE>(d[mb][2], d[mb][3]);
                *(u32x2*)(stage + (mb * 16 + jl) * C::SSTR + (q * 16 + g * 4) * 2) = pk;
            }
        }
        asm volatile("" ::: "memory");
        cad_wave_sync();
        gp_wait_dma();
#pragma unroll
        for (int r0 = 0; r0 < C::MW; r0 += RPI) {
            const int r = r0 + lane / LPR, c8 = lane % LPR;
            u32x4 v = *(const u32x4*)(stage + r * C::SSTR + c8 * 16);
            const int m = m_wave + r;
            const int64_t t = t0 + c8 * 8;
            if constexpr (ACC) {  // out = bf16(acc + bf16 product): element-wise on the packed pairs
                const u32x4 o = old[r0 / RPI];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float lo = cad_lo2f<TE>(v[e]) + cad_lo2f<TE>(o[e]);
                    const float hi = cad_hi2f<TE>(v[e]) + cad_hi2f<TE>(o[e]);
                    v[e] = cad_pack2<TE>(lo, hi);
                }
            }
            if (m < M && t + 8 <= T) cad_store_stream<CAD_STREAM_PROJ>((u32x4*)(out + (int64_t)m * a.ldo + t), v);
        }
        __syncthreads();
    }
}

}  // namespace

// ---- launch helpers of the three kernel families (proj_ring.h and gemm_stream.h include this header) -------------------------------------
// raise the kernel's dynamic LDS limit where needed (CAD_BIG_LDS, cad_prims_gfx950.h: cached per kernel and device), then launch
// 64 * GP_WAVES threads per workgroup
#define GP_LAUNCH(kern, grid, lds, stream, args)                              \
    do {                                                                      \
        CAD_BIG_LDS(kern, lds);                                               \
        CAD_LAUNCH(kern, grid, dim3(64 * GP_WAVES), lds, stream, args);       \
    } while (0)
// grid of a kernel whose workgroups walk the work items (token blocks, tiles) of ONE row group: one workgroup per CU, capped by the items
static inline dim3 gp_grid_per_cu(int64_t nitems) {
    const int64_t gx = cad_cu_count();
    return dim3((unsigned)(gx > nitems ? nitems : gx));
}
// grid of the W-stationary kernels (C = GpCfg / GxCfg): y = row groups of C::MWG output channels, x = cad_cu_count() / y (~ one workgroup
// per CU), clamped to [1, token blocks]
template <typename C>
static dim3 gp_grid_wstat(const cad_proj_args* a) {
    const int64_t nblk = (a->T + C::NT - 1) / C::NT;
    const int my = (a->M + C::MWG - 1) / C::MWG;
    int64_t gx = cad_cu_count() / my;
    if (gx < 1) gx = 1;
    if (gx > nblk) gx = nblk;
    return dim3((unsigned)gx, (unsigned)my);
}

template <typename TE, int KS>
static int launch_wxT(const cad_proj_args* a, void* stream) {
    typedef GpCfg<KS> C;
    GP_LAUNCH((proj_wxT_kernel<TE, KS>), gp_grid_wstat<C>(a), C::LDS, stream, *a);
    return cad_after_launch();
}

template <typename TE>
static int proj_wxT(const cad_proj_args* a, void* stream) {
    CAD_CHECK_ARG(a && a->W && a->X && a->out && a->T > 0 && a->M > 0 && a->K > 0 && a->act == 0);
    CAD_CHECK_ARG(a->ldw >= a->K && a->ldx >= a->K && a->ldo >= a->T);
    CAD_CHECK_ARG((a->ldw % 8) == 0 && (a->ldx % 8) == 0 && (((uintptr_t)a->W | (uintptr_t)a->X) % 16) == 0);
    CadProfScope prof(8, stream);
    switch (a->K) {
        case 32: return launch_wxT<TE, 1>(a, stream);
        case 64: return launch_wxT<TE, 2>(a, stream);
        case 128: return launch_wxT<TE, 4>(a, stream);
        case 256: return launch_wxT<TE, 8>(a, stream);
        case 512: return launch_wxT<TE, 16>(a, stream);
        default: return CAD_ERR_UNSUPPORTED;
    }
}

template <typename TE, int KS>
static int launch_wx(const cad_proj_args* a, void* stream) {
    typedef GxCfg<KS> C;
    if (a->acc)
        GP_LAUNCH((proj_wx_kernel<TE, KS, true>), gp_grid_wstat<C>(a), C::LDS, stream, *a);
    else
        GP_LAUNCH((proj_wx_kernel<TE, KS, false>), gp_grid_wstat<C>(a), C::LDS, stream, *a);
    return cad_after_launch();
}
