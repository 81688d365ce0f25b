// metrpo_debug_gemm, backward epilogue group (see gemm_debug.h): the (EPI, TA, TB) combinations dyn_train.hip, det_gemm.hip, policy_gemm.hip and svg.hip launch.
#include "metrpo_internal.h"
#include "gemm_debug.h"

bool gemm_debug_run_bwd(const metrpo_debug_gemm_args& a, const GemmEpi& ep, hipStream_t st) {
    const bool ta = a.ta != 0, tb = a.tb != 0;
    if (a.epi == EPI_RELU_MASK && !ta && tb) gemm_debug_tiles<EPI_RELU_MASK, false, true>(a, ep, st);
    else if (a.epi == EPI_PLAIN && !ta && tb) gemm_debug_tiles<EPI_PLAIN, false, true>(a, ep, st);
    else if (a.epi == EPI_DTANH && !ta && !tb) gemm_debug_tiles<EPI_DTANH, false, false>(a, ep, st);
    else if (a.epi == EPI_DTANH && !ta && tb) gemm_debug_tiles<EPI_DTANH, false, true>(a, ep, st);
    else if (a.epi == EPI_ADAM && ta && !tb) gemm_debug_tiles<EPI_ADAM, true, false>(a, ep, st);
    else if (a.epi == EPI_PARTIAL && ta && !tb) gemm_debug_tiles<EPI_PARTIAL, true, false>(a, ep, st);
    else if (a.epi == EPI_PARTIAL && !ta && !tb && a.tm == 1 && a.tn == 1)           // shipped on 64x64 tiles only (gemm_skinny_bias)
        gemm_mfma_launch<1, 1, EPI_PARTIAL, false, false>(a.A, a.strideA, a.lda, a.W, a.strideW, a.ldw, nullptr, 0, a.ldc, a.M, a.N, a.Kd, a.heads, ep, st);
    else return false;
    return true;
}
