// metrpo_debug_gemm: a diagnostics hook that runs ONE call of the shared MFMA GEMM's host entries (gemm_mfma.h) on caller-owned device
// memory, so that tests can pin k_gemm_mfma's instantiations directly (tests/test_gpu_gemm.py).  Not declared in include/metrpo.h.
// The instantiations are split by epilogue group over two translation units to keep each compile short:
//   gemm_debug.hip      the entry, gemm_skinny_bias, gemm_relu_fused_out and the forward epilogues (BIAS_ID / BIAS_RELU / BIAS_TANH)
//   gemm_debug_bwd.hip  the backward epilogues (RELU_MASK, PLAIN, DTANH, PARTIAL, ADAM)
#pragma once
#include <cstdint>
#include "gemm_mfma.h"

enum { GEMM_DEBUG_OP_AUTO = 0, GEMM_DEBUG_OP_SKINNY = 1, GEMM_DEBUG_OP_FUSED_OUT = 2 };

struct metrpo_debug_gemm_args {            // mirrored by _lib.DebugGemmArgs
    int32_t op, epi, ta, tb;               // op AUTO: gemm_auto<epi, ta, tb> (a shipped combination), or gemm_mfma_launch<tm, tn, epi, ta, tb> when tm, tn are given
    int32_t tm, tn;                        // 0: the entry's own rule; 1 or 2: force the tile (both or neither; FUSED_OUT: tm == tn)
    int32_t M, N, Kd, heads;
    int32_t lda, ldw, ldc, ldm;
    int64_t strideA, strideW, strideC, strideBias, strideMask, strideAdam, stridePart, strideW2;
    const float* A; const float* W; float* C; const float* bias; const float* mask;
    float* am; float* av; float* bvec; float* bam; float* bav; float* part; const float* w2;
    float lr_t, beta1, beta2, eps, decay;
    int32_t splits, kchunk;                // EPI_PARTIAL under op AUTO: free parameters
    int32_t no;                            // FUSED_OUT: columns of the output layer
    int32_t act, defer;                    // SKINNY: activation 0 / 1 / 2; defer != 0 passes a SkinnyDefer
    // on return: what was launched
    int32_t o_tm, o_tn, o_al, o_pd;        // k_gemm_mfma<o_tm, o_tn, .., o_al, o_pd>
    int32_t o_splits, o_kchunk;            // partials written to `part` (0: C was written directly) and rows per split
    int32_t o_gx, o_gy, o_gz;              // grid of the k_gemm_mfma launch
    int32_t o_reduced;                     // SKINNY: k_splitk_bias_reduce ran (C holds the result)
    int64_t o_stride_part;
};

// gemm_auto's launch with an optional forced tile; the instantiations are those gemm_auto<EPI, TA, TB> makes anyway
template <int EPI, bool TA, bool TB>
static inline void gemm_debug_tiles(const metrpo_debug_gemm_args& a, const GemmEpi& ep, hipStream_t st) {
#define GD_ARGS_ a.A, a.strideA, a.lda, a.W, a.strideW, a.ldw, a.C, a.strideC, a.ldc, a.M, a.N, a.Kd, a.heads, ep, st
    if (a.tm == 0) gemm_auto<EPI, TA, TB>(GD_ARGS_);
    else if (a.tm == 2 && a.tn == 2) gemm_mfma_launch<2, 2, EPI, TA, TB>(GD_ARGS_);
    else if (a.tm == 2) gemm_mfma_launch<2, 1, EPI, TA, TB>(GD_ARGS_);
    else if (a.tn == 2) gemm_mfma_launch<1, 2, EPI, TA, TB>(GD_ARGS_);
    else gemm_mfma_launch<1, 1, EPI, TA, TB>(GD_ARGS_);
#undef GD_ARGS_
}

// op AUTO, backward epilogues (gemm_debug_bwd.hip); false: not a shipped (epi, ta, tb, tile) combination
bool gemm_debug_run_bwd(const metrpo_debug_gemm_args& a, const GemmEpi& ep, hipStream_t st);
