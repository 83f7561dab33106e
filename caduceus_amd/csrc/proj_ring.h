// The MFMA projections built on GtCfg's ring of [64 rows][128 tokens] LDS chunks, element-type templates: the thin-M / deep-K cad_proj_wx,
// cad_proj_wx_wgrad, cad_proj_xTw.  From proj_wstat.h: GP_WAVES, gx_swz, the thin-K launch_wx that proj_wx falls back to, the launch helpers.
#pragma once
#include "proj_wstat.h"

namespace {

// ---- cad_proj_wx, thin M / deep K:  out (M <= 64, T) = W (M, K) . X (K, T),  K a multiple of 64 -----------------------------
// x_proj (M = dt_rank + 2 d_state, K = d_inner) and d(dt_lr) = W_dt^T . d(delta) (M = dt_rank): the streaming operand is the
// (K, T) channel-major activation, read exactly once; W (<= 64 x K) lives in LDS for the whole launch.  A workgroup owns blocks of
// 128 tokens (one 16-token column per wave) and walks K in chunks of 64 rows through a RING of 4 LDS tiles filled by LDS-DMA
// three chunks ahead (counted s_waitcnt: vmcnt retires in order, two DMA instructions per wave and chunk); A fragments by
// transposing reads as above, B fragments (W) by ds_read_b128 from the padded LDS copy, fp32 accumulation over the whole K in
// the MFMA accumulators, 8-byte stores of four consecutive tokens per lane (the output is 1/10 of the traffic).
struct GtCfg {
    static constexpr int NT = 128, KC = 64, RING = 4;
    static constexpr int XROW = NT * 2;               // bytes per tile row
    static constexpr int XBUF = KC * XROW;            // 16 KB per chunk
    static constexpr int DPW = (KC * NT * 2 / 16 / 64) / GP_WAVES;  // DMA instructions per wave and chunk (= 2)
    static constexpr size_t lds(int M, int K) { return (size_t)RING * XBUF + (size_t)((M + 15) / 16 * 16) * (K * 2 + 16); }
};
static_assert(GtCfg::DPW == 2, "the counted waits below assume two DMA instructions per wave and chunk");
static_assert((GtCfg::RING & (GtCfg::RING - 1)) == 0, "ring slots are advanced with a mask");

// cad_glds16 with the streaming (nt) cache policy, for a channel-major operand that exactly ONE workgroup reads exactly once: the
// [64 rows][128 tokens] ring chunks of the thin kernels and of cad_proj_xTw.  One production mixer layer, same box, three interleaved rounds,
// average of its 16 projection launches: 0.1075 / 0.1084 / 0.1087 -> 0.1049 / 0.1054 / 0.1054 ms; in a traced step d(dt_lr) + dW_dt 73.9 ->
// 54.5 us, x_proj 61.4 -> 54.8 us, out_proj unchanged (alone behind a 512 MiB fill: 0.209 -> 0.172 ms); profiles/r08_ab_proj_stream.txt.
// The same policy LOSES wherever a second workgroup meets the lines in L2 and stays
// off there (same file): the token-major X of cad_proj_wxT that the two row halves of in_proj share (+1.3 %), both operands of the
// weight-gradient cad_gemm_stream (+3.7 %); neutral on the B operand of d(x2d) and on the addend of d(xc).
__device__ __forceinline__ void gp_glds16_stream(const void* gsrc /* per lane */, uint32_t lds_base /* wave-uniform, SGPR */) {
#ifdef CAD_EMU
    cad_glds16(gsrc, lds_base);
#else
    uint32_t keep;  // (M0: as cad_glds16)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_base)
                 : "memory");
#endif
}

template <typename TE>
__device__ __forceinline__ void gt_issue_chunk(const TE* X, int64_t ldx, int k0, int64_t t0, int64_t T, char* xbuf, int wave,
                                               int lane) {
#pragma unroll
    for (int i = 0; i < GtCfg::DPW; ++i) {
        const int ins = wave * GtCfg::DPW + i;       // 16 instructions of 64 pieces: 4 tile rows each
        const int p = ins * 64 + lane;
        const int row = p >> 4, pp = p & 15;                         // tile row, PHYSICAL 16-byte piece
        const int lp = (((pp >> 1) ^ gx_swz(row)) << 1) | (pp & 1);  // logical piece = 8 tokens
        int64_t tok = t0 + lp * 8;
        tok = tok + 8 <= T ? tok : T - 8;                            // tail block: valid data, never stored
        gp_glds16_stream(X + (int64_t)(k0 + row) * ldx + tok, cad_uniform((int)(cad_lds_off(xbuf) + ins * 1024)));
    }
}

// W -> LDS (rows >= M zero): the padded copy (MB * 16 rows of K elements, WSTR bytes apart) that the B-fragment reads of both thin kernels
// address; uses their W, M, K, MB, WSTR, wl and a.  (A macro, not a __forceinline__ function: as a function -- whole loop or loop body,
// five signatures tried -- the compiler lays out or schedules the copy loop of the thin kernels differently from the loop written in place.)
#define GT_COPY_W_TO_LDS()                                                              \
    for (int i = threadIdx.x; i < MB * 16 * (K / 8); i += 64 * GP_WAVES) {              \
        const int m = i / (K / 8), c8 = i % (K / 8);                                    \
        u32x4 v = {0u, 0u, 0u, 0u};                                                     \
        if (m < M) v = *(const u32x4*)(W + (int64_t)m * a.ldw + c8 * 8);                \
        *(u32x4*)(wl + m * WSTR + c8 * 16) = v;                                         \
    }

template <typename TE, int MB>
__global__ __launch_bounds__(64 * GP_WAVES, 1) void proj_wx_thin_kernel(cad_proj_args a) {
    typedef GtCfg C;
    CAD_DYN_SMEM(char, smem);
    const int lane = threadIdx.x & 63;
    const int wave = cad_uniform(threadIdx.x >> 6);
    const int g = lane >> 4, jl = lane & 15;
    const TE* W = (const TE*)a.W;
    const TE* X = (const TE*)a.X;
    TE* out = (TE*)a.out;
    const int64_t T = a.T;
    const int M = a.M, K = a.K;
    const int NCH = K / C::KC;
    const int64_t nblk = (T + C::NT - 1) / C::NT;
    const int64_t b0 = blockIdx.x, bstep = gridDim.x;
    if (b0 >= nblk) return;
    const int64_t nmine = (nblk - b0 + bstep - 1) / bstep;
    const int64_t total = nmine * NCH;               // (block, chunk) iterations of this workgroup
    char* wl = smem + C::RING * C::XBUF;             // W copy: row stride WSTR (padded: the 16 rows of a B fragment read spread over the banks)
    const int WSTR = K * 2 + 16;
    // the (block, chunk) position of the next chunk to issue and of the chunk being consumed are carried as counters (no 64-bit
    // division by the run-time NCH between the barrier and the next DMA issue; time-neutral when measured: this kernel's 88 us in the
    // step against 56 us in a loop is the memory-side cache, profiles/r03_ab_conv_addnorm.txt (3))
    int ich = 0, islot = 0;
    int64_t iblk = b0;
    auto issue_next = [&]() {
        gt_issue_chunk(X, a.ldx, ich * C::KC, iblk * C::NT, T, smem + islot * C::XBUF, wave, lane);
        islot = (islot + 1) & (C::RING - 1);
        if (++ich == NCH) {
            ich = 0;
            iblk += bstep;
        }
    };
    for (int64_t it = 0; it < C::RING - 1; ++it)
        if (it < total) issue_next();
    GT_COPY_W_TO_LDS()
    f32x4 d[MB];
    int ch = 0, slot = 0;
    int64_t blk = b0;
    for (int64_t it = 0; it < total; ++it) {
        // chunk `it` has landed: of this wave's DMA, at most the two later chunks (4 instructions) may still be in flight --
        // fewer near the end of the stream, where everything is waited for
        if (it + C::RING - 2 < total)
            cad_wait_vmcnt<4>();
        else
            cad_wait_vmcnt<0>();
        __syncthreads();  // every wave's share of the chunk is visible; the tile consumed LAST iteration is free again
        if (it + C::RING - 1 < total) issue_next();
        if (ch == 0) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) d[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const char* xt = smem + slot * C::XBUF;
#pragma unroll
        for (int ks = 0; ks < C::KC / 32; ++ks) {
            const int r0 = ks * 32 + g * 8 + (jl >> 2);
            const char* p0 = xt + r0 * C::XROW + ((wave ^ gx_swz(r0)) * 32) + (jl & 3) * 8;
            const char* p1 = xt + (r0 + 4) * C::XROW + ((wave ^ gx_swz(r0 + 4)) * 32) + (jl & 3) * 8;
            const u32x2 lo = cad_lds_read_tr16(p0), hi = cad_lds_read_tr16(p1);
            const u32x4 xf = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const u32x4 wf = *(const u32x4*)(wl + (mb * 16 + jl) * WSTR + (ch * C::KC + ks * 32 + g * 8) * 2);
                d[mb] = cad_mfma_16x16x32<TE>(xf, wf, d[mb]);
            }
        }
        slot = (slot + 1) & (C::RING - 1);
        if (++ch == NCH) {
            const int64_t t = blk * C::NT + wave * 16 + g * 4;  // this lane's four consecutive tokens
            const TE* acc = (const TE*)a.acc;  // wave-uniform: the other K half of a product too deep for one W copy in LDS
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const int m = mb * 16 + jl;
                f32x4 v = d[mb];
                if (acc && m < M && t + 4 <= T) {  // out = bf16(acc + the fp32 sums): the addend is widened, the sum rounded once
                    const u32x2 o = *(const u32x2*)(acc + (int64_t)m * a.ldacc + t);
                    v[0] += cad_lo2f<TE>(o[0]), v[1] += cad_hi2f<TE>(o[0]);
                    v[2] += cad_lo2f<TE>(o[1]), v[3] += cad_hi2f<TE>(o[1]);
                }
                u32x2 pk;
                pk[0] = cad_pack2_safe<TE>(v[0], v[1]);
                pk[1] = cad_pack2_safe<TE>(v[2], v[3]);
                if (m < M && t + 4 <= T) *(u32x2*)(out + (int64_t)m * a.ldo + t) = pk;
            }
            ch = 0;
            blk += bstep;
        }
    }
}


// ---- cad_proj_wx_wgrad: the thin-M / deep-K product AND the weight gradient of the same operand from ONE pass over X -----------
// d(dt_lr) (M = dt_rank rows) = W_dt^T . d(delta)  and  dW_dt (K = d_inner, M) = d(delta) . dt_lr^T  both stream the (K, T) tensor
// d(delta); the second used to be a K-split hipBLASLt bmm + sum that read the 268 MB again.  Same skeleton as proj_wx_thin_kernel
// (ring of four [64 rows][128 tokens] LDS tiles filled by LDS-DMA, counted waits); on top of it, per (block, chunk) every wave
// runs two more MFMAs with the ROLES of the tile swapped: A = 16 channel rows of the tile x 32 tokens (token-contiguous rows are
// A fragments as they lie: plain ds_read_b128), B = the matching 32 tokens of the M rows of Y (a [M][128] tile per block, double
// buffered, XOR-swizzled through the DMA source addresses), accumulated in registers over ALL blocks of the workgroup -- NCH x MB
// accumulator tiles per wave (the chunk loop is unrolled, so the tiles are addressed statically).  Wave w owns channel block w & 3
// of every chunk and the token half w >> 2; the halves are summed through LDS at the end and the workgroup writes its (K, M) fp32
// partial slot; the caller sums the <= 256 slots (fixed order).
// PROD = false: the weight gradient alone (a.W / a.out unused) -- dW_x = xc . d(dbc)^T of the x_proj backward (M = dt_rank + 2 d_state).
template <typename TE, int MB, int NCH, bool PROD>
__global__ __launch_bounds__(64 * GP_WAVES, 1) void proj_wx_thin_wgrad_kernel(cad_proj_args a) {
    typedef GtCfg C;
    CAD_DYN_SMEM(char, smem);
    const int lane = threadIdx.x & 63;
    const int wave = cad_uniform(threadIdx.x >> 6);
    const int g = lane >> 4, jl = lane & 15;
    const TE* W = (const TE*)a.W;
    const TE* X = (const TE*)a.X;
    const TE* Y = (const TE*)a.wg_y;
    TE* out = (TE*)a.out;
    const int64_t T = a.T;
    const int M = a.M;
    constexpr int K = NCH * C::KC;
    constexpr int YBUF = MB * 16 * C::XROW;           // bytes per Y tile: [MB * 16 rows][128 tokens]
    const int64_t nblk = T / C::NT;                   // (T % 128 == 0: no tail block, every staged token is a real token)
    const int64_t b0 = blockIdx.x, bstep = gridDim.x;
    const int64_t nmine = (nblk - b0 + bstep - 1) / bstep;  // >= 1: the grid never exceeds the number of blocks
    const int64_t total = nmine * NCH;
    char* wl = smem + C::RING * C::XBUF;
    constexpr int WSTR = K * 2 + 16;
    char* yt = wl + (PROD ? MB * 16 * WSTR : 0);  // (the weight-gradient-only form keeps no W copy: M = 64 at K = 512 would not fit otherwise)
    auto issue = [&](int64_t it) {
        const int64_t blk = b0 + (it / NCH) * bstep;
        gt_issue_chunk(X, a.ldx, (int)(it % NCH) * C::KC, blk * C::NT, T, smem + (int)(it % C::RING) * C::XBUF, wave, lane);
    };
    // Y tile of block number bi (of this workgroup): MB * 4 DMA instructions of four rows each, dealt over the waves;
    // physical 16-byte piece pp of row r holds logical piece pp ^ (r & 15): the 16 rows a B-fragment read touches hit 16 distinct
    // pieces = all 64 banks
    auto issue_y = [&](int64_t bi) {
#pragma unroll
        for (int q0 = 0; q0 < MB * 4; q0 += GP_WAVES) {
            const int q = q0 + wave;
            if (q < MB * 4) {
                const int row = q * 4 + (lane >> 4), pp = lane & 15;
                const int lp = pp ^ (row & 15);
                const int64_t blk = b0 + bi * bstep;
                const int rr = row < M ? row : M - 1;  // rows >= M: valid data, their columns of the result are never stored
                cad_glds16(Y + (int64_t)rr * a.ld_wg_y + blk * C::NT + lp * 8,
                           cad_uniform((int)(cad_lds_off(yt) + (int)(bi & 1) * YBUF + q * 1024)));
            }
        }
    };
    issue_y(0);  // BEFORE the chunks: vmcnt retires in order, so the first counted wait below also covers it
    for (int64_t it = 0; it < C::RING - 1; ++it)
        if (it < total) issue(it);
    if constexpr (PROD) GT_COPY_W_TO_LDS()
    f32x4 d[MB];
    f32x4 dw[NCH][MB];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) dw[ch][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int rb = wave & 3, kh = wave >> 2;
    for (int64_t bi = 0; bi < nmine; ++bi) {
        const char* ytile = yt + (int)(bi & 1) * YBUF;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const int64_t it = bi * NCH + ch;
            if (it + C::RING - 2 < total)
                cad_wait_vmcnt<4>();  // (a Y tile issued behind the chunks only makes this wait stricter)
            else
                cad_wait_vmcnt<0>();
            __syncthreads();
            if (it + C::RING - 1 < total) issue(it + C::RING - 1);
            if (ch == 0 && bi + 1 < nmine) issue_y(bi + 1);  // a whole block ahead of its use
            if (PROD && ch == 0) {
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) d[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            const char* xt = smem + (int)(it % C::RING) * C::XBUF;
            // (1) out += W . X: transposing reads, as proj_wx_thin_kernel
            if constexpr (PROD) {
#pragma unroll
            for (int ks = 0; ks < C::KC / 32; ++ks) {
                const int r0 = ks * 32 + g * 8 + (jl >> 2);
                const char* p0 = xt + r0 * C::XROW + ((wave ^ gx_swz(r0)) * 32) + (jl & 3) * 8;
                const char* p1 = xt + (r0 + 4) * C::XROW + ((wave ^ gx_swz(r0 + 4)) * 32) + (jl & 3) * 8;
                const u32x2 lo = cad_lds_read_tr16(p0), hi = cad_lds_read_tr16(p1);
                const u32x4 xf = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    const u32x4 wf = *(const u32x4*)(wl + (mb * 16 + jl) * WSTR + (ch * C::KC + ks * 32 + g * 8) * 2);
                    d[mb] = cad_mfma_16x16x32<TE>(xf, wf, d[mb]);
                }
            }
            }
            // (2) dW[chunk rows, :] += X_tile . Y_tile^T over this wave's 64 tokens: A = channel rows rb * 16 .. + 15 (token-
            // contiguous: eight tokens of a row are one 16-byte piece), B = rows of Y
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int lp = kh * 8 + ks * 4 + g;  // logical 16-byte piece = tokens 8 lp .. 8 lp + 7 of the block
                const int r = rb * 16 + jl;
                const int pp = (((lp >> 1) ^ gx_swz(r)) << 1) | (lp & 1);
                const u32x4 af = *(const u32x4*)(xt + r * C::XROW + pp * 16);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    const int yr = mb * 16 + jl;
                    const u32x4 bf = *(const u32x4*)(ytile + yr * C::XROW + ((lp ^ (yr & 15)) * 16));
                    dw[ch][mb] = cad_mfma_16x16x32<TE>(af, bf, dw[ch][mb]);
                }
            }
            if (PROD && ch == NCH - 1) {
                const int64_t blk = b0 + bi * bstep;
                const int64_t t = blk * C::NT + wave * 16 + g * 4;
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    const int m = mb * 16 + jl;
                    u32x2 pk;
                    pk[0] = cad_pack2_safe<TE>(d[mb][0], d[mb][1]);
                    pk[1] = cad_pack2_safe<TE>(d[mb][2], d[mb][3]);
                    if (m < M) *(u32x2*)(out + (int64_t)m * a.ldo + t) = pk;
                }
            }
        }
    }
    // the two token halves of every accumulator tile meet in LDS (the ring is free now), then the (K, M) partial slot is written
    __syncthreads();
    float* ex = (float*)smem;  // [4 channel blocks][NCH][MB][64 lanes][4]
    if (kh == 1) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) *(f32x4*)(ex + (((rb * NCH + ch) * MB + mb) * 64 + lane) * 4) = dw[ch][mb];
    }
    __syncthreads();
    if (kh == 0) {
        float* slot = a.wg_partials + (int64_t)blockIdx.x * K * M;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const f32x4 o = *(const f32x4*)(ex + (((rb * NCH + ch) * MB + mb) * 64 + lane) * 4);
                const int m = mb * 16 + jl;
                if (m < M) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) slot[(int64_t)(ch * C::KC + rb * 16 + g * 4 + r) * M + m] = dw[ch][mb][r] + o[r];
                }
            }
    }
}


// ---- cad_proj_xTw:  out (T, M) TOKEN-major  =  sum over panels p of  X_p (K, T)^T . W (M, K)^T ----------------------------------------
// out_proj of the tied BiMamba mixer: out = W_out (y_f + y_r) with y_f, y_r the two scans' channel-major outputs -- two panels that
// share ONE weight, so the kernel walks K = d_inner per panel with the SAME resident W fragments (the library GEMM it replaces
// multiplied the concatenation [y_f ; y_r] by a doubled weight [W_out, W_out] that had to be built per layer and step).
// "W-stationary" as cad_proj_wxT: wave w owns output features 16 MB w .. and keeps their MB x K / 32 A-fragments in registers for the
// whole launch; the workgroup walks blocks of 128 tokens, X travels by LDS-DMA in [64 rows][128 tokens] chunks through the ring of
// cad_proj_wx's thin kernel (same swizzle, same counted waits).  MFMA roles: A = W fragment (rows = output features), B = X fragment
// by transposing reads (columns = tokens), so a D lane holds FOUR CONSECUTIVE FEATURES of one token = 8 contiguous bytes of the
// token-major output; fp32 accumulation over both panels and all of K, one rounding to bf16.
// The output leaves with ordinary stores: the pieces of a token row meet in L2 (streaming stores of 8-byte pieces measured 0.277 vs
// 0.212 ms, profiles/r04_out_proj.txt; of the 16-byte pieces below: within the noise, profiles/r09_ab_proj_store.txt).  With 32 features
// per wave (MB = 2) the two accumulator tiles of a token exchange lane rows (cad_d_pair16, cad_stream.h) and leave as 16 bytes per lane.
#define GP_XTW_RING 4           // LDS tiles of the X ring: RING - 1 chunks (16 KB each) in flight per CU (8 slots measured SLOWER:
                               // 0.222 vs 0.206 ms, profiles/r04_out_proj.txt)
template <typename TE, int MB, int KS>
__global__ __launch_bounds__(64 * GP_WAVES, 2) void proj_xTw_kernel(cad_proj_tm_args a) {
    typedef GtCfg C;
    CAD_DYN_SMEM(char, smem);
    const int lane = threadIdx.x & 63;
    const int wave = cad_uniform(threadIdx.x >> 6);
    const int g = lane >> 4, jl = lane & 15;
    const TE* W = (const TE*)a.W;
    TE* out = (TE*)a.out;
    const int64_t T = a.T;
    const int M = a.M;
    constexpr int NCH = KS / 2;                       // 64-row chunks per panel
    constexpr int XR = GP_XTW_RING;                   // ring slots
    constexpr int INFL = (XR - 2) * C::DPW;           // DMA instructions of the later chunks that may stay in flight at a wait
    static_assert((XR & (XR - 1)) == 0 && XR >= 4, "ring slots are advanced with a mask");
    const int NP = a.X2 ? 2 : 1;
    const int per_blk = NP * NCH;                     // chunks per token block
    const int64_t nblk = (T + C::NT - 1) / C::NT;
    const int64_t b0 = blockIdx.x, bstep = gridDim.x;
    if (b0 >= nblk) return;
    const int64_t nmine = (nblk - b0 + bstep - 1) / bstep;
    const int64_t total = nmine * per_blk;
    const int m_wave = wave * 16 * MB;
    // position of the next chunk to issue, carried as counters (no division on the issue path)
    int ich = 0, ipan = 0, islot = 0;
    int64_t iblk = b0;
    auto issue_next = [&]() {
        gt_issue_chunk((const TE*)(ipan ? a.X2 : a.X), a.ldx, ich * C::KC, iblk * C::NT, T, smem + islot * C::XBUF, wave, lane);
        islot = (islot + 1) & (XR - 1);
        if (++ich == NCH) {
            ich = 0;
            if (++ipan == NP) {
                ipan = 0;
                iblk += bstep;
            }
        }
    };
    for (int64_t it = 0; it < XR - 1; ++it)
        if (it < total) issue_next();
    // A fragments of this wave's rows of W, resident for the whole launch (rows >= M read as zero)
    u32x4 wf[MB][KS];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int m = m_wave + mb * 16 + jl;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (m < M) v = *(const u32x4*)(W + (int64_t)m * a.ldw + ks * 32 + g * 8);
            wf[mb][ks] = v;
        }
    }
    f32x4 d[C::NT / 16][MB];
    int slot = 0;
    int64_t blk = b0;
    // The wave's 32 features of a token (MB = 2) are 64 contiguous bytes of the output row: they leave as one 16-byte store per lane
    // (cad_d_pair16, cad_stream.h) where the rows are 16-byte aligned -- wave-uniform; elsewhere as 8-byte pieces, twice the instructions
    constexpr bool WIDE = MB == 2;
    const bool wide = WIDE && (a.ldo % 8) == 0 && (((uintptr_t)out) & 15) == 0;
    // output stores per wave and block that the counted waits allow for (the 8-byte form issues more: its waits are only stricter)
    constexpr int NST = (C::NT / 16) * (WIDE ? 1 : MB);
    static_assert(INFL + NST <= 63, "vmcnt is a 6-bit counter");
    int since_store = XR;                             // iterations since the last store burst (wave-uniform)
    for (int64_t bi = 0; bi < nmine; ++bi, blk += bstep) {
#pragma unroll
        for (int q = 0; q < C::NT / 16; ++q)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) d[q][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int pan = 0; pan < NP; ++pan) {
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const int64_t it = (bi * NP + pan) * NCH + ch;
                // chunk `it` has landed when at most the vector-memory operations issued AFTER its DMA are outstanding (vmcnt retires in
                // issue order on gfx9-class hardware, loads, LDS-DMA and stores alike): the two later chunks (4 instructions) and -- for the
                // three waits that follow a block's output stores -- those NST stores.  A plain vmcnt(4) there drained the stores AND the
                // freshly issued prefetch once per block (200 instead of ~140 us per launch, profiles/r04_out_proj.txt).
                if (it + XR - 2 >= total || since_store < 0)
                    cad_wait_vmcnt<0>();
                else if (since_store < XR - 1)
                    cad_wait_vmcnt<INFL + NST>();
                else
                    cad_wait_vmcnt<INFL>();
                ++since_store;
                __syncthreads();  // every wave's share of the chunk is visible; the tile consumed LAST iteration is free again
                if (it + XR - 1 < total) issue_next();
                const char* xt = smem + slot * C::XBUF;
                slot = (slot + 1) & (XR - 1);
                // (k step outer, token sub-block inner: consecutive MFMAs go to sixteen different accumulator tiles)
#pragma unroll
                for (int ks = 0; ks < C::KC / 32; ++ks) {
#pragma unroll
                    for (int q = 0; q < C::NT / 16; ++q) {
                        const int r0 = ks * 32 + g * 8 + (jl >> 2);
                        const char* p0 = xt + r0 * C::XROW + ((q ^ gx_swz(r0)) * 32) + (jl & 3) * 8;
                        const char* p1 = xt + (r0 + 4) * C::XROW + ((q ^ gx_swz(r0 + 4)) * 32) + (jl & 3) * 8;
                        const u32x2 lo = cad_lds_read_tr16(p0), hi = cad_lds_read_tr16(p1);
                        const u32x4 xf = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb) d[q][mb] = cad_mfma_16x16x32<TE>(wf[mb][ch * 2 + ks], xf, d[q][mb]);
                    }
                }
            }
        }
        // lane (token 16 q + jl, features m_wave + 16 mb + 4 g .. + 3): 8 bytes of the token's output row
#pragma unroll
        for (int q = 0; q < C::NT / 16; ++q) {
            const int64_t t = blk * C::NT + q * 16 + jl;
            if constexpr (WIDE) {
                u32x2 pk[2];
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    pk[mb][0] = cad_pack2_safe<TE>(d[q][mb][0], d[q][mb][1]);
                    pk[mb][1] = cad_pack2_safe<TE>(d[q][mb][2], d[q][mb][3]);
                }
                if (wide) {  // (wave-uniform; the exchange runs on all lanes, the store under the same mask rules as below)
                    const u32x4 v = cad_d_pair16(pk[0], pk[1]);
                    if (t < T && m_wave + 32 <= M) *(u32x4*)((char*)(out + t * a.ldo + m_wave) + cad_d_pair16_off(lane)) = v;
                } else {
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb) {
                        const int m = m_wave + mb * 16 + g * 4;
                        if (t < T && m + 4 <= M) *(u32x2*)(out + t * a.ldo + m) = pk[mb];
                    }
                }
                continue;
            }
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const int m = m_wave + mb * 16 + g * 4;
                u32x2 pk;
                pk[0] = cad_pack2_safe<TE>(d[q][mb][0], d[q][mb][1]);
                pk[1] = cad_pack2_safe<TE>(d[q][mb][2], d[q][mb][3]);
                // (every lane issues the store: the counted waits above rely on exactly NST store instructions per block; lanes of a tail
                // block / beyond M are masked off by the exec mask, the instruction still counts)
                if (t < T && m + 4 <= M) *(u32x2*)(out + t * a.ldo + m) = pk;
            }
        }
        // (a block with masked-off store instructions -- the tail block, or a wave beyond M -- issued an unknown number of them: the
        // next three waits drain everything instead)
        // ... and so does a configuration whose blocks are shorter than the ring is deep (two store bursts inside one wait's window)
        since_store = (blk * C::NT + C::NT <= T && m_wave + 16 * MB <= M && per_blk >= XR - 1) ? 0 : -XR;
    }
}

}  // namespace

// thin M / deep K variant (x_proj, d(dt_lr)): M <= 64 output rows, K a multiple of 64 up to 1024; the addend (may alias out) carries the
// other K half of a product whose W does not fit LDS in one piece (x_proj at d_inner 1024: 64 rows x 1024)
template <typename TE, int MB>
static int launch_wx_thin(const cad_proj_args* a, void* stream) {
    const size_t lds = GtCfg::lds(MB * 16, a->K);
    GP_LAUNCH((proj_wx_thin_kernel<TE, MB>), gp_grid_per_cu((a->T + GtCfg::NT - 1) / GtCfg::NT), lds, stream, *a);
    return cad_after_launch();
}

template <typename TE>
static int proj_wx(const cad_proj_args* a, void* stream) {
    CAD_CHECK_ARG(a && a->W && a->X && a->out && a->T > 0 && a->M > 0 && a->K > 0);
    if (a->act == 0 && cad_proj_wx_thin_supported(a->M, a->K, a->T)) {
        CAD_CHECK_ARG(a->ldw >= a->K && a->ldx >= a->T && a->ldo >= a->T);
        CAD_CHECK_ARG((a->ldw % 8) == 0 && (a->ldx % 8) == 0 && (a->ldo % 4) == 0);
        CAD_CHECK_ARG((((uintptr_t)a->W | (uintptr_t)a->X) % 16) == 0 && ((uintptr_t)a->out % 8) == 0);
        CAD_CHECK_ARG(a->acc == nullptr || (a->ldacc >= a->T && (a->ldacc % 4) == 0 && ((uintptr_t)a->acc % 8) == 0));
        CadProfScope prof(8, stream);
        switch ((a->M + 15) / 16) {
            case 1: return launch_wx_thin<TE, 1>(a, stream);
            case 2: return launch_wx_thin<TE, 2>(a, stream);
            case 3: return launch_wx_thin<TE, 3>(a, stream);
            default: return launch_wx_thin<TE, 4>(a, stream);
        }
    }
    if (!cad_proj_wx_supported(a->K, a->T)) return CAD_ERR_UNSUPPORTED;
    CAD_CHECK_ARG(a->act == 0 || (a->act == CAD_ACT_SOFTPLUS_BIAS && a->acc == nullptr));
    CAD_CHECK_ARG(a->ldw >= a->K && a->ldx >= a->T && a->ldo >= a->T && (a->acc == nullptr || a->ldacc >= a->T));
    CAD_CHECK_ARG((a->ldw % 8) == 0 && (a->ldx % 8) == 0 && (a->ldo % 8) == 0 && (a->ldacc % 8) == 0);
    CAD_CHECK_ARG((((uintptr_t)a->W | (uintptr_t)a->X | (uintptr_t)a->out | (uintptr_t)a->acc) % 16) == 0);
    CadProfScope prof(8, stream);
    return a->K <= 32 ? launch_wx<TE, 1>(a, stream) : launch_wx<TE, 2>(a, stream);
}

// LDS of the weight-gradient kernels: ring (+ the W copy of the product form) + two Y tiles; the final exchange of the accumulator tiles
// reuses the front of it.  The ONE statement of the formula: the launcher and the *_supported predicates (gemm.hip) both call it.
static constexpr size_t gt_wgrad_lds(int M, int K, bool prod) {
    const int mb = (M + 15) / 16;
    const size_t lds = (prod ? GtCfg::lds(mb * 16, K) : (size_t)GtCfg::RING * GtCfg::XBUF) + 2 * (size_t)mb * 16 * GtCfg::XROW;
    const size_t exch = (size_t)4 * (K / GtCfg::KC) * mb * 1024;
    return lds < exch ? exch : lds;
}

template <typename TE, int MB, int NCH, bool PROD>
static int launch_wx_wgrad(const cad_proj_args* a, void* stream) {
    constexpr size_t lds = gt_wgrad_lds(MB * 16, NCH * GtCfg::KC, PROD);
    if (lds > 160 * 1024) return CAD_ERR_UNSUPPORTED;  // (the *_supported predicates exclude these shapes)
    const dim3 grid((unsigned)cad_proj_wx_wgrad_partials(a->T));  // (a fixed slot count, not the CU count: part of the summation order)
    GP_LAUNCH((proj_wx_thin_wgrad_kernel<TE, MB, NCH, PROD>), grid, lds, stream, *a);
    return cad_after_launch();
}

template <typename TE>
static int proj_wx_wgrad(const cad_proj_args* a, void* stream) {
    CAD_CHECK_ARG(a && a->X && a->wg_y && a->wg_partials && a->acc == nullptr && a->act == 0);
    CAD_CHECK_ARG(a->ldx >= a->T && a->ld_wg_y >= a->T && (a->ldx % 8) == 0 && (a->ld_wg_y % 8) == 0);
    CAD_CHECK_ARG((((uintptr_t)a->X | (uintptr_t)a->wg_y) % 16) == 0);
    CadProfScope prof(8, stream);
    if (a->W == nullptr && a->out == nullptr) {  // weight gradient alone
        if (!cad_proj_wgrad_only_supported(a->M, a->K, a->T)) return CAD_ERR_UNSUPPORTED;
        const int mb = (a->M + 15) / 16;
#define GW_ONLY(MB_)                                                                                     \
    return a->K == 256 ? launch_wx_wgrad<TE, MB_, 4, false>(a, stream) : launch_wx_wgrad<TE, MB_, 8, false>(a, stream)
        switch (mb) {
            case 1: GW_ONLY(1);
            case 2: GW_ONLY(2);
            case 3: GW_ONLY(3);
            default: GW_ONLY(4);
        }
#undef GW_ONLY
    }
    CAD_CHECK_ARG(a->W && a->out);
    if (!cad_proj_wx_wgrad_supported(a->M, a->K, a->T)) return CAD_ERR_UNSUPPORTED;
    CAD_CHECK_ARG(a->ldw >= a->K && a->ldo >= a->T && (a->ldw % 8) == 0 && (a->ldo % 4) == 0);
    CAD_CHECK_ARG(((uintptr_t)a->W % 16) == 0 && ((uintptr_t)a->out % 8) == 0);
    if (a->M == 16) return a->K == 256 ? launch_wx_wgrad<TE, 1, 4, true>(a, stream) : launch_wx_wgrad<TE, 1, 8, true>(a, stream);
    return a->K == 256 ? launch_wx_wgrad<TE, 2, 4, true>(a, stream) : launch_wx_wgrad<TE, 2, 8, true>(a, stream);
}


// ---- cad_proj_xTw ------------------------------------------------------------------------------------------------------------------
template <typename TE, int MB, int KS>
static int launch_xTw(const cad_proj_tm_args* a, void* stream) {
    const size_t lds = (size_t)GP_XTW_RING * GtCfg::XBUF;
    GP_LAUNCH((proj_xTw_kernel<TE, MB, KS>), gp_grid_per_cu((a->T + GtCfg::NT - 1) / GtCfg::NT), lds, stream, *a);
    return cad_after_launch();
}

template <typename TE>
static int proj_xTw(const cad_proj_tm_args* a, void* stream) {
    CAD_CHECK_ARG(a && a->W && a->X && a->out && a->T > 0 && a->M > 0 && a->K > 0);
    if (!cad_proj_xTw_supported(a->M, a->K, a->T)) return CAD_ERR_UNSUPPORTED;
    CAD_CHECK_ARG(a->ldw >= a->K && a->ldx >= a->T && a->ldo >= a->M);
    CAD_CHECK_ARG((a->ldw % 8) == 0 && (a->ldx % 8) == 0 && (a->ldo % 4) == 0);
    CAD_CHECK_ARG((((uintptr_t)a->W | (uintptr_t)a->X | (uintptr_t)a->X2) % 16) == 0 && ((uintptr_t)a->out % 8) == 0);
    CadProfScope prof(8, stream);
    if (a->M == 256) return a->K == 512 ? launch_xTw<TE, 2, 16>(a, stream) : launch_xTw<TE, 2, 8>(a, stream);
    return a->K == 512 ? launch_xTw<TE, 1, 16>(a, stream) : launch_xTw<TE, 1, 8>(a, stream);
}
