// Dense projections of the Mamba mixer on the matrix cores (include/caduceus_hip.h, cad_proj_*): hand-written bf16 MFMA
// kernels for the skinny GEMMs around the scan -- in_proj / out_proj and their gradients -- whose small dimension
// (K = d_model or 2 d_model, a few hundred) makes them HBM-bound streaming problems: every activation byte is touched
// once, the weights stay on chip for the whole launch.
// The kernels are element-type templates in three headers, one per family; this translation unit instantiates them for bf16,
// gemm_f16.hip for fp16 (cad_*_f16), so that each object holds the kernels of one element type:
//   proj_wstat.h    W-stationary: cad_proj_wxT, the thin-K cad_proj_wx; the launch helpers of all three families
//   proj_ring.h     ring of [64 rows][128 tokens] chunks: the thin-M / deep-K cad_proj_wx, cad_proj_wx_wgrad, cad_proj_xTw
//   gemm_stream.h   both operands streamed: cad_gemm_stream
// The exported shape predicates are stated here, once; the launchers of both translation units call them through the C ABI.
#include "proj_wstat.h"
#include "proj_ring.h"
#include "gemm_stream.h"

extern "C" int cad_proj_supported(int K) { return K == 32 || K == 64 || K == 128 || K == 256 || K == 512; }
extern "C" int cad_proj_wx_supported(int K, int64_t T) { return K >= 8 && K <= 64 && (K % 8) == 0 && T >= 8 && (T % 8) == 0; }
extern "C" int cad_proj_wx_thin_supported(int M, int K, int64_t T) {
    return M >= 1 && M <= 64 && K > 64 && K <= 1024 && (K % 64) == 0 && T >= 8 && (T % 8) == 0 &&
           GtCfg::lds(M, K) <= 160 * 1024;
}
extern "C" int cad_proj_wx_wgrad_supported(int M, int K, int64_t T) {
    return (M == 16 || M == 32) && (K == 256 || K == 512) && T >= GtCfg::NT && (T % GtCfg::NT) == 0 &&
           gt_wgrad_lds(M, K, true) <= 160 * 1024;
}
// the weight gradient alone (cad_proj_args.W == NULL, out == NULL): any M <= 64
extern "C" int cad_proj_wgrad_only_supported(int M, int K, int64_t T) {
    return M >= 1 && M <= 64 && (K == 256 || K == 512) && T >= GtCfg::NT && (T % GtCfg::NT) == 0 &&
           gt_wgrad_lds(M, K, false) <= 160 * 1024;
}
int cad_cu_count_override();  // api.hip: the value set by cad_debug_set_cu_count (tests only), 0 = none
extern "C" int cad_proj_wx_wgrad_partials(int64_t T) {
    const int64_t nblk = T / GtCfg::NT;
    int cap = 256;  // (a fixed number, not the CU count: the slot count is part of the summation order)
    const int forced = cad_cu_count_override();  // tests only: fewer workgroups, several blocks each
    if (forced > 0 && forced < cap) cap = forced;
    return (int)(nblk < cap ? (nblk < 1 ? 1 : nblk) : cap);
}
extern "C" int cad_proj_xTw_supported(int M, int K, int64_t T) {
    return (M == 128 || M == 256) && (K == 256 || K == 512) && T >= 8 && (T % 8) == 0;
}
extern "C" int cad_gemm_stream_supported(int64_t R, int64_t C, int64_t K, int nslices) {
    return R >= GsCfg::RT && (R % GsCfg::RT) == 0 && C >= GsCfg::CT && (C % GsCfg::CT) == 0 && nslices >= 1 && K > 0 &&
           (K % nslices) == 0 && ((K / nslices) % GsCfg::KC) == 0;
}

extern "C" int cad_proj_wxT(const cad_proj_args* a, void* stream) { return proj_wxT<bf16_t>(a, stream); }
extern "C" int cad_proj_wx(const cad_proj_args* a, void* stream) { return proj_wx<bf16_t>(a, stream); }
extern "C" int cad_proj_wx_wgrad(const cad_proj_args* a, void* stream) { return proj_wx_wgrad<bf16_t>(a, stream); }
extern "C" int cad_proj_xTw(const cad_proj_tm_args* a, void* stream) { return proj_xTw<bf16_t>(a, stream); }
extern "C" int cad_gemm_stream(const cad_gemm_stream_args* a, void* stream) { return gemm_stream<bf16_t>(a, stream); }
