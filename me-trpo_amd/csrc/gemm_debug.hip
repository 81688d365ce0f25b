// metrpo_debug_gemm: one call of the shared MFMA GEMM's host entries on caller-owned device memory (see gemm_debug.h).  It launches only what the
// library's own callers launch, reads and writes no context state (a rejected call records its reason in the context's error string, like
// every entry point), allocates nothing and measures nothing.  The caller sizes every buffer for the extents, strides and offsets it passes.
#include "metrpo_internal.h"
#include "gemm_debug.h"

static bool run_fwd(const metrpo_debug_gemm_args& a, const GemmEpi& ep, hipStream_t st) {
    if (a.ta || a.tb) return false;
    if (a.epi == EPI_BIAS_ID) gemm_debug_tiles<EPI_BIAS_ID, false, false>(a, ep, st);
    else if (a.epi == EPI_BIAS_RELU) gemm_debug_tiles<EPI_BIAS_RELU, false, false>(a, ep, st);
    else if (a.epi == EPI_BIAS_TANH) gemm_debug_tiles<EPI_BIAS_TANH, false, false>(a, ep, st);
    else return false;
    return true;
}

static void report(metrpo_debug_gemm_args* a, int tm, int tn, int epi, const GemmEpi& ep) {
    const GemmForm f = gemm_launch_form(tm, tn, epi, a->ta != 0, a->tb != 0, a->A, a->strideA, a->lda, a->W, a->strideW, a->ldw, a->M, a->N, a->Kd, a->heads, ep);
    a->o_tm = tm; a->o_tn = tn; a->o_al = f.al ? 1 : 0; a->o_pd = f.pd;
    a->o_gx = (int32_t)f.gx; a->o_gy = (int32_t)f.gy; a->o_gz = (int32_t)f.gz;
}

extern "C" int32_t metrpo_debug_gemm(metrpo_ctx* c, metrpo_debug_gemm_args* a, void* stream) {
    if (!c || !a) return METRPO_ENULL;
    hipStream_t st = (hipStream_t)stream;
    auto bad = [&](const char* why) { return set_err(c, METRPO_EINVAL, std::string("debug_gemm: ") + why); };
    if (a->M < 1 || a->N < 1 || a->Kd < 1 || a->heads < 1) return bad("M, N, Kd and heads must be positive");
    if (!a->A || !a->W) return bad("A and W must be given");
    if (a->tm < 0 || a->tm > 2 || a->tn < 0 || a->tn > 2 || ((a->tm == 0) != (a->tn == 0))) return bad("tm and tn: both 0, or each 1 or 2");
    a->o_splits = 0; a->o_kchunk = a->Kd; a->o_reduced = 0; a->o_stride_part = 0;
    GemmEpi ep = {};
    if (a->op == GEMM_DEBUG_OP_AUTO) {
        const int e = a->epi;
        ep.bias = a->bias; ep.strideBias = a->strideBias;
        ep.mask = a->mask; ep.strideMask = a->strideMask; ep.ldm = a->ldm;
        ep.am = a->am; ep.av = a->av; ep.strideAdam = a->strideAdam;
        ep.lr_t = a->lr_t; ep.beta1 = a->beta1; ep.beta2 = a->beta2; ep.eps = a->eps; ep.decay = a->decay;
        ep.bvec = a->bvec; ep.bam = a->bam; ep.bav = a->bav;
        if (e <= EPI_BIAS_TANH && e >= 0 && !a->bias) return bad("the bias epilogues need a bias");
        if ((e == EPI_RELU_MASK || e == EPI_DTANH) && !a->mask) return bad("this epilogue needs a mask");
        if (e == EPI_ADAM && (!a->am || !a->av || !a->C || (a->bvec && (!a->bam || !a->bav)))) return bad("EPI_ADAM needs C, am, av (and bam, bav with bvec)");
        if (e != EPI_PARTIAL && !a->C) return bad("C must be given");
        if (e == EPI_PARTIAL) {
            if (!a->part || a->splits < 1 || a->kchunk < 1) return bad("EPI_PARTIAL needs part, splits >= 1 and kchunk >= 1");
            if ((long long)a->splits * a->kchunk < a->Kd || (long long)(a->splits - 1) * a->kchunk >= a->Kd) return bad("splits * kchunk must cover Kd with no empty split");
            if (a->ldc != a->N) return bad("EPI_PARTIAL writes dense M x N partials: ldc must equal N");
            if (a->stridePart < (long long)a->M * a->N + a->N) return bad("stridePart below M * N + N");
            ep.part = a->part; ep.stridePart = a->stridePart; ep.splits = a->splits; ep.kchunk = a->kchunk;
            a->o_splits = a->splits; a->o_kchunk = a->kchunk; a->o_stride_part = a->stridePart;
        }
        GemmTile t = {a->tm, a->tn};
        metrpo_debug_gemm_args r = *a;
        if (e == EPI_PARTIAL && !a->ta && !a->tb && a->tm == 0) { r.tm = r.tn = 1; t = GemmTile{1, 1}; }        // its one shipped tile (gemm_mfma_launch<1, 1>)
        else if (a->tm == 0) t = gemm_auto_tile(a->M, a->N, a->heads);
        if (!run_fwd(r, ep, st) && !gemm_debug_run_bwd(r, ep, st)) return bad("not a combination of (epi, ta, tb, tile) the library launches");
        report(a, t.tm, t.tn, e, ep);
    } else if (a->op == GEMM_DEBUG_OP_SKINNY) {
        if (a->ta || a->tb || a->tm) return bad("gemm_skinny_bias takes plain operands and picks its own tile");
        if (!a->bias || !a->C || a->act < 0 || a->act > 2) return bad("gemm_skinny_bias needs bias, C and act 0, 1 or 2");
        SkinnyDefer df = {0, 0};
        gemm_skinny_bias(a->A, a->strideA, a->lda, a->W, a->strideW, a->ldw, a->bias, a->strideBias, a->C, a->strideC, a->M, a->N, a->Kd, a->heads, a->part, st,
                         a->act, a->defer ? &df : nullptr);
        const SkinnyPlan sp = skinny_plan(a->M, a->N, a->Kd, a->heads, a->part != nullptr);
        if (sp.splits <= 1) {
            const GemmTile t = gemm_auto_tile(a->M, a->N, a->heads);
            ep.bias = a->bias; ep.strideBias = a->strideBias;
            report(a, t.tm, t.tn, a->act == 1 ? EPI_BIAS_RELU : a->act == 2 ? EPI_BIAS_TANH : EPI_BIAS_ID, ep);
            a->o_reduced = 0;
        } else {
            ep.splits = sp.splits; ep.kchunk = sp.kchunk;
            report(a, 1, 1, EPI_PARTIAL, ep);
            a->o_splits = sp.splits; a->o_kchunk = sp.kchunk; a->o_stride_part = sp.stridePart;
            a->o_reduced = (a->defer && a->act == 0) ? 0 : 1;
            if (a->defer && (df.splits != (a->o_reduced ? 0 : sp.splits) || df.stridePart != (a->o_reduced ? 0 : sp.stridePart)))
                return set_err(c, METRPO_ESTATE, "debug_gemm: gemm_skinny_bias's deferred report differs from skinny_plan");
        }
    } else if (a->op == GEMM_DEBUG_OP_FUSED_OUT) {
        if (a->ta || a->tb) return bad("gemm_relu_fused_out takes plain operands");
        if (a->tm != a->tn) return bad("gemm_relu_fused_out runs on square tiles");
        if (!a->bias || !a->w2 || !a->part) return bad("gemm_relu_fused_out needs bias, w2 and part");
        if (a->no < 1 || a->no > 64) return bad("no must be 1 .. 64");
        const int tile = a->tm ? a->tm : gemm_fused_out_tile(a->M, a->N, a->heads, a->no);
        if (tile == 0) return bad("gemm_fused_out_tile: the fused output layer does not apply to this shape");
        if (a->N % (64 * tile) != 0) return bad("the fused output layer needs N to be a multiple of the tile's columns");
        int splits = 0; long long stride = 0;
        gemm_relu_fused_out(tile, a->A, a->strideA, a->lda, a->W, a->strideW, a->ldw, a->bias, a->strideBias, a->w2, a->strideW2, a->no, a->M, a->N, a->Kd, a->heads,
                            a->part, st, &splits, &stride);
        report(a, tile, tile, a->no <= 32 ? EPI_RELU_OUT : a->no <= 48 ? EPI_RELU_OUT48 : EPI_RELU_OUT64, ep);
        a->o_splits = splits; a->o_stride_part = stride;
    } else {
        return bad("unknown op");
    }
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}
