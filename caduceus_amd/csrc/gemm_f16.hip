// fp16 siblings of the MFMA projection entry points (include/caduceus_hip.h, cad_*_f16): the kernel templates of gemm.hip's three headers
// instantiated for binary16 operands (v_mfma_f32_16x16x32_f16, the same operand packing as the bf16 instruction; fp32 accumulation; results
// rounded to nearest even, +-inf beyond 65504).  A translation unit of its own, so that each object holds the kernels of one element type.
#include "proj_wstat.h"
#include "proj_ring.h"
#include "gemm_stream.h"

extern "C" int cad_proj_wxT_f16(const cad_proj_args* a, void* stream) { return proj_wxT<f16_t>(a, stream); }
extern "C" int cad_proj_wx_f16(const cad_proj_args* a, void* stream) { return proj_wx<f16_t>(a, stream); }
extern "C" int cad_proj_wx_wgrad_f16(const cad_proj_args* a, void* stream) { return proj_wx_wgrad<f16_t>(a, stream); }
extern "C" int cad_proj_xTw_f16(const cad_proj_tm_args* a, void* stream) { return proj_xTw<f16_t>(a, stream); }
// (CAD_GEMM_OUT_T_BF16 mode: the token-major result in fp16)
extern "C" int cad_gemm_stream_f16(const cad_gemm_stream_args* a, void* stream) { return gemm_stream<f16_t>(a, stream); }
