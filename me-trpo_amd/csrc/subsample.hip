// metrpo_subsample_batch (include/metrpo.h): device gather of the sub-batch the Fisher-vector products of a subsampled TRPO update see.
// [rllab] ConjugateGradientOptimizer.optimize, subsample_factor < 1:
//     inds = np.random.choice(n, int(n * subsample_factor), replace=False);  subsample_inputs = tuple(x[inds] for x in inputs)
// Gathered: what the FVP kernels of every update family read (observations, valid flag) and the old distribution with its stride rule
// (a broadcast old_log_std stays the caller's pointer).  Actions and advantages are not: the sub-batch serves f_Hx_plain only.
//
// Bandwidth-bound: rows of w <= 55 floats at random row positions.  A workgroup takes SUB_ROWS consecutive OUTPUT rows at a time; their source
// rows are resolved once (index load, clamp) into LDS, then the SUB_ROWS x w floats of a field are walked as one flat range: consecutive lanes
// read consecutive floats of a source row (64 / w rows per wave for a narrow field) and write one contiguous, fully coalesced output range.
#include "metrpo_internal.h"
#include <algorithm>

namespace {

constexpr int SUB_ROWS = 256;          // output rows per workgroup pass = threads per workgroup (one index / valid flag per thread)

struct SubK {
    const float* obs; const float* mean; const float* ls;      // source fields (mean / ls NULL: not gathered)
    const uint8_t* valid;                                      // NULL: all valid
    float* o_obs; float* o_mean; float* o_ls; uint8_t* o_valid;
    const int32_t* idx;
    long long N, m;
    int ns, na;
    double* count;             // += valid gathered rows (NULL: not wanted)
    double* err;               // sticky: an index had to be clamped
};

// rows x w floats: element e of the pass is float e % w of output row base + e / w
__device__ __forceinline__ void gather_field(const float* __restrict__ src, float* __restrict__ dst, const int* s_row, long long base, int rows, int w) {
    float* __restrict__ d = dst + base * w;
    const int n = rows * w;
    for (int e = threadIdx.x; e < n; e += SUB_ROWS) {
        const int rl = e / w, col = e - rl * w;
        d[e] = src[(long long)s_row[rl] * w + col];
    }
}

__global__ void __launch_bounds__(SUB_ROWS) k_subsample(SubK k) {
    __shared__ int s_row[SUB_ROWS];
    __shared__ int s_cnt[SUB_ROWS / WAVE];
    int cnt = 0;
    for (long long base = (long long)blockIdx.x * SUB_ROWS; base < k.m; base += (long long)gridDim.x * SUB_ROWS) {
        const int rows = (int)((k.m - base < SUB_ROWS) ? k.m - base : SUB_ROWS);
        __syncthreads();                                       // the previous pass has read s_row
        if ((int)threadIdx.x < rows) {
            long long r = k.idx[base + threadIdx.x];
            if (r < 0 || r >= k.N) {                           // never read outside the batch: clamp, and say so (metrpo_trpo_update_fvp / metrpo_comm_check)
                r = (r < 0) ? 0 : k.N - 1;
                *k.err = 1.0;
            }
            s_row[threadIdx.x] = (int)r;
            if (k.valid != nullptr) {
                const uint8_t v = k.valid[r];
                k.o_valid[base + threadIdx.x] = v;
                cnt += (v != 0) ? 1 : 0;
            }
        }
        __syncthreads();
        gather_field(k.obs, k.o_obs, s_row, base, rows, k.ns);
        if (k.mean != nullptr) gather_field(k.mean, k.o_mean, s_row, base, rows, k.na);
        if (k.ls != nullptr) gather_field(k.ls, k.o_ls, s_row, base, rows, k.na);
    }
    if (k.count == nullptr) return;
    if (k.valid == nullptr) {                                  // all valid: the count is m
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(k.count, (double)k.m);
        return;
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) s_cnt[threadIdx.x / WAVE] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < SUB_ROWS / WAVE; ++w) t += s_cnt[w];
        if (t != 0) atomicAdd(k.count, (double)t);             // whole numbers below 2^53: exact in any order
    }
}

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

int launch_subsample(metrpo_ctx* c, const metrpo_batch* b, const int32_t* d_idx, long long m, double inv_n_global, metrpo_batch* out, double* d_valid_count,
                     hipStream_t st) {
    const int ns = c->pd.ns, na = c->pd.na;
    if (b->N > 2147483647LL) return set_err(c, METRPO_EUNSUPPORTED, "subsample_batch: int32 row indices cover N < 2^31");
    const bool has_mean = b->d_old_mean != nullptr;
    const bool rows_ls = b->d_old_log_std != nullptr && b->old_log_std_stride != 0;
    if (rows_ls && b->old_log_std_stride != na) return set_err(c, METRPO_EINVAL, "subsample_batch: old_log_std_stride must be 0 or na");
    const size_t o_obs = 0;
    const size_t o_mean = o_obs + up16(sizeof(float) * (size_t)m * ns);
    const size_t o_ls = o_mean + (has_mean ? up16(sizeof(float) * (size_t)m * na) : 0);
    const size_t o_valid = o_ls + (rows_ls ? up16(sizeof(float) * (size_t)m * na) : 0);
    const size_t need = o_valid + (b->d_valid ? up16((size_t)m) : 0);
    { const int rc = ws_grow(c, c->d_sub, need); if (rc) return rc; }      // the one growth path: an outgrown workspace is retired, never freed here
    char* ws = (char*)c->d_sub.p;
    SubK k = {};
    k.obs = b->d_obs; k.mean = b->d_old_mean; k.ls = rows_ls ? b->d_old_log_std : nullptr; k.valid = b->d_valid;
    k.o_obs = (float*)(ws + o_obs); k.o_mean = has_mean ? (float*)(ws + o_mean) : nullptr; k.o_ls = rows_ls ? (float*)(ws + o_ls) : nullptr;
    k.o_valid = b->d_valid ? (uint8_t*)(ws + o_valid) : nullptr;
    k.idx = d_idx; k.N = b->N; k.m = m; k.ns = ns; k.na = na; k.count = d_valid_count; k.err = sub_err_cell(c);
    // the workspace keeps its address from call to call while its contents change: no activation cache of an update family may be keyed to it
    // (the sub-batch products of run_trpo_update run uncached and leave the keys alone; this covers a caller that hands the sub-batch to another entry point)
    if (c->pg_fwd_obs == k.o_obs) c->pg_fwd_rows = -1;
    if (c->f3_obs == k.o_obs) c->f3_rows = -1;
    const long long passes = (m + SUB_ROWS - 1) / SUB_ROWS;
    const int grid = (int)std::max<long long>(1, std::min<long long>(passes, (long long)c->n_sm * 8));
    hipLaunchKernelGGL(k_subsample, dim3(grid), dim3(SUB_ROWS), 0, st, k);
    HIP_TRY(c, hipGetLastError());
    *out = metrpo_batch{};
    out->d_obs = k.o_obs; out->d_act = nullptr; out->d_adv = nullptr; out->d_old_mean = k.o_mean;
    out->d_old_log_std = rows_ls ? k.o_ls : b->d_old_log_std; out->old_log_std_stride = rows_ls ? na : 0;
    out->d_valid = k.o_valid; out->N = m; out->inv_n_global = inv_n_global;
    return METRPO_OK;
}
