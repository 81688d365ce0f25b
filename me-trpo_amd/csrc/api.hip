// C-ABI entry points of libmetrpo.so (include/metrpo.h): context management, argument checking,
// dispatch to the kernels, and the host driver of one TRPO update.
#include "metrpo_internal.h"
#include <atomic>
#include <chrono>
#include <cstring>
#include "cg_device.h"
#include "trace.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>

// serialised: the concurrent rounds of rollout_gemm.hip enqueue from several host threads and may fail together
static std::mutex g_err_mutex;
int set_err(metrpo_ctx* c, int code, const std::string& msg) {
    if (c) { std::lock_guard<std::mutex> lock(g_err_mutex); c->err = msg; }
    return code;
}

extern "C" int32_t metrpo_abi_version(void) { return METRPO_ABI_VERSION; }

extern "C" const char* metrpo_status_string(int32_t s) {
    switch (s) {
    case METRPO_OK: return "ok";
    case METRPO_EINVAL: return "invalid argument";
    case METRPO_ENULL: return "null pointer";
    case METRPO_EHIP: return "HIP runtime error";
    case METRPO_EUNSUPPORTED: return "unsupported configuration";
    case METRPO_ESTATE: return "dynamics/policy not set";
    }
    return "unknown status";
}

static bool build_net(NetDesc* n, int n_in, const int32_t* hidden, const int32_t* acts, int n_hidden, int n_out,
                      int default_act, bool align16) {
    if (n_hidden < 0 || n_hidden > METRPO_MAX_LAYERS || n_in <= 0 || n_out <= 0) return false;
    n->n_layers = n_hidden + 1;
    n->dims[0] = n_in;
    for (int l = 0; l < n_hidden; ++l) {
        if (hidden[l] <= 0) return false;
        n->dims[l + 1] = hidden[l];
        n->act[l] = acts ? acts[l] : default_act;
        if (n->act[l] < METRPO_ACT_IDENTITY || n->act[l] > METRPO_ACT_TANH) return false;
    }
    n->dims[n_hidden + 1] = n_out;
    n->act[n_hidden] = METRPO_ACT_IDENTITY;
    int off = 0, aoff = 0, mw = 0;
    auto up = [&](int v) { return align16 ? ((v + 3) & ~3) : v; };
    for (int l = 0; l < n->n_layers; ++l) {
        n->w_off[l] = off; off = up(off + n->dims[l] * n->dims[l + 1]);
        n->b_off[l] = off; off = up(off + n->dims[l + 1]);
        n->api_w_off[l] = aoff; aoff += n->dims[l] * n->dims[l + 1];
        n->api_b_off[l] = aoff; aoff += n->dims[l + 1];
    }
    for (int l = 0; l <= n->n_layers; ++l) mw = std::max(mw, n->dims[l]);
    n->n_params = off;
    n->api_n_params = aoff;
    n->max_width = mw;
    return true;
}

// CG workspace layout (doubles): gout[1+P] | x[P] | r[P] | p[P] | z[P] | step[P] | scal[8] | lk[2] | ls[4]
struct CgView { double *gout, *x, *r, *p, *z, *step, *scal, *lk, *ls; };
static CgView cg_view(metrpo_ctx* c) {
    const int P = c->pd.P;
    CgView v;
    v.gout = c->d_cg.p; v.x = v.gout + 1 + P; v.r = v.x + P; v.p = v.r + P; v.z = v.p + P; v.step = v.z + P;
    v.scal = v.step + P; v.lk = v.scal + 8;      // lk directly behind scal[8], ls behind lk: run_trpo_update reads scal | lk | ls back as ONE 14-double copy
    v.ls = v.lk + 2;                             // device-side line-search state (cg_device.h: CgTail::ls)
    return v;
}

// Dense caller-visible dynamics layout <-> 16-byte aligned resident layout (NetDesc).  grid = (blocks, n_models).
struct RepackDesc { int n_seg; int api_off[2 * MAXL], dev_off[2 * MAXL], len[2 * MAXL]; int api_stride, dev_stride; };
__global__ void k_repack_dyn(RepackDesc d, const float* __restrict__ src, float* __restrict__ dst, int to_device) {
    const int k = blockIdx.y;
    for (int s = 0; s < d.n_seg; ++s) {
        const float* a = src + (size_t)k * (to_device ? d.api_stride : d.dev_stride) + (to_device ? d.api_off[s] : d.dev_off[s]);
        float* b = dst + (size_t)k * (to_device ? d.dev_stride : d.api_stride) + (to_device ? d.dev_off[s] : d.api_off[s]);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < d.len[s]; i += gridDim.x * blockDim.x) b[i] = a[i];
    }
}
static void repack_dyn(const metrpo_ctx* c, const float* src, float* dst, int n_models, bool to_device, hipStream_t st) {
    const NetDesc& n = c->pd.dyn;
    RepackDesc d;
    d.n_seg = 2 * n.n_layers; d.api_stride = n.api_n_params; d.dev_stride = n.n_params;
    for (int l = 0; l < n.n_layers; ++l) {
        d.api_off[2 * l] = n.api_w_off[l]; d.dev_off[2 * l] = n.w_off[l]; d.len[2 * l] = n.dims[l] * n.dims[l + 1];
        d.api_off[2 * l + 1] = n.api_b_off[l]; d.dev_off[2 * l + 1] = n.b_off[l]; d.len[2 * l + 1] = n.dims[l + 1];
    }
    hipLaunchKernelGGL(k_repack_dyn, dim3(64, n_models), dim3(256), 0, st, d, src, dst, to_device ? 1 : 0);
}


// Diagnostics hook (not part of include/metrpo.h; bench.py's roofline.update.fvp): with option TIME_FVP set, launch_fvp_tail brackets the Fisher-vector-product
// KERNEL of every CG iteration (not its reduction) with HIP events on the update's stream.  Returns their mean in microseconds, the count in *n.
extern "C" int32_t metrpo_debug_fvp_us(metrpo_ctx* c, double* mean_us, int32_t* n) {
    if (!c || !mean_us || !n) return METRPO_ENULL;
    *mean_us = 0.0; *n = 0;
    const int pairs = c->fvp_ev_n / 2;
    if (pairs == 0) return METRPO_OK;
    HIP_TRY(c, hipEventSynchronize(c->fvp_ev[2 * pairs - 1]));
    double sum = 0.0;
    for (int i = 0; i < pairs; ++i) { float ms = 0.0f; HIP_TRY(c, hipEventElapsedTime(&ms, c->fvp_ev[2 * i], c->fvp_ev[2 * i + 1])); sum += ms; }
    *mean_us = sum / pairs * 1e3; *n = pairs; c->fvp_ev_n = 0;
    return METRPO_OK;
}

// Diagnostics hook (not part of include/metrpo.h; tests/test_gpu_update_kernels.py): what the last policy-update launch of this context ran on, as the host wrote it down when it
// enqueued the launch (no device work, no synchronisation).  out[7] = family (0 generic, 1 fused 2 x 32, 2 GEMM path, 3 fused 100-50-25; -1: none yet), UpdOp as launched,
// index into the fused 2 x 32 kernel table (-1 elsewhere), sample tile PT of the generic kernels, partial rows of the reduction, splits and kchunk of the GEMM path.
extern "C" int32_t metrpo_debug_last_update(const metrpo_ctx* c, int32_t* out) {
    if (!c || !out) return METRPO_ENULL;
    const auto& l = c->upd_last;
    out[0] = l.family; out[1] = l.op; out[2] = l.table; out[3] = l.pt; out[4] = l.nrows; out[5] = l.splits; out[6] = l.kchunk;
    return METRPO_OK;
}

// Diagnostics hook (tests/test_gpu_wide_rollout_edges.py): what the last metrpo_rollout of this context launched, as the host wrote it down while it enqueued it (no device work,
// no synchronisation).  out[16] = family (as metrpo_last_rollout_kernel), then metrpo_ctx::RollLast field by field; everything behind the family is 0 (pre-step kind: -1)
// on the families that are neither GEMM-class nor resident.
extern "C" int32_t metrpo_debug_last_rollout_launch(const metrpo_ctx* c, int32_t* out) {
    if (!c || !out) return METRPO_ENULL;
    const auto& l = c->roll_last;
    const int v[16] = {c->last_rollout_kernel, l.pre, l.post_width, l.sk_mode, l.late, l.l0_route, l.fuse_tile, l.out_splits, l.persist_wide, l.nclose, l.rounds,
                       l.res_ws, l.res_threads, l.res_pw, l.res_rg, l.res_rot};
    for (int i = 0; i < 16; ++i) out[i] = v[i];
    return METRPO_OK;
}

// Diagnostics hook (not part of include/metrpo.h; tests/test_gpu_trpo_solve.py): the Fisher-vector products of the last CG solve metrpo_trpo_update / _begin (and their _fvp forms)
// enqueued, as the host wrote them down (no device work, no synchronisation; after an update the last noted LAUNCH is a line-search evaluation).  out[8] = family and UpdOp as
// launched of the products (op 1, or 3 = OP_FVPC where they read the gradient launch's activation cache; -1: the solve made none, -2: they disagree), index into the fused 2 x 32
// kernel table (-1 elsewhere), number of products (the explicit step-scale product included), then four flags: SolveScope::cache_activations, SolveScope::publish_image, the CG
// vector steps ran as tails of the reductions (0: stand-alone k_cg_* kernels), a separate FVP batch was in force.  family = -1: no solve yet.
extern "C" int32_t metrpo_debug_last_solve(const metrpo_ctx* c, int32_t* out) {
    if (!c || !out) return METRPO_ENULL;
    const auto& s = c->solve_last;
    out[0] = s.family; out[1] = s.op; out[2] = s.table; out[3] = s.n_fvp; out[4] = s.cache_activations; out[5] = s.publish_image; out[6] = s.fused_tails; out[7] = s.fvp_batch;
    return METRPO_OK;
}

// Diagnostics hook (tests/test_gpu_api.py): outgrown workspaces this context holds back instead of freeing them inside a launch entry point (metrpo_internal.h: ws_grow);
// sweep != 0 frees them now (a synchronising call, like the sweep the library runs by itself past WS_RETIRED_MAX).  Returns the count in front of the sweep.
extern "C" int32_t metrpo_debug_ws_retired(metrpo_ctx* c, unsigned long long* bytes, int32_t sweep) {
    if (!c) return METRPO_ENULL;
    const int32_t n = (int32_t)c->ws_retired.size();
    if (bytes) *bytes = (unsigned long long)c->ws_retired_bytes;
    if (sweep) ws_sweep(c);
    return n;
}
// Diagnostics hook (tools/persist_stats.py): per-workgroup statistics of the last persistent stream-K launch made with option PERSIST_STATS set
// (mlp_persist.h: SkpArgs::stats), 8 values per workgroup; returns the number of workgroups (0: none recorded).
extern "C" int32_t metrpo_debug_persist_stats(metrpo_ctx* c, unsigned long long* out, int32_t cap_wgs, void* stream) {
    if (!c || !out) return METRPO_ENULL;
    if (!c->d_skp_stats.p || c->skp_stats_n == 0) return 0;
    const int n = std::min(cap_wgs, c->skp_stats_n);
    HIP_TRY(c, hipMemcpyAsync(out, c->d_skp_stats.p, sizeof(unsigned long long) * 8 * n, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(c, hipStreamSynchronize((hipStream_t)stream));
    return n;
}

// ---- option table (metrpo_internal.h: METRPO_OPT_LIST) ----
static const char* const OPT_NAMES[OPT_COUNT] = {
#define X(n) #n,
    METRPO_OPT_LIST(X)
#undef X
};
const char* metrpo_opt_name(int id) { return (id >= 0 && id < OPT_COUNT) ? OPT_NAMES[id] : nullptr; }
int metrpo_opt_id(const char* key) {
    if (!key) return -1;
    std::string k(key);
    for (auto& ch : k) ch = (char)toupper((unsigned char)ch);
    if (k.rfind("METRPO_", 0) == 0) k = k.substr(7);
    for (int i = 0; i < OPT_COUNT; ++i) if (k == OPT_NAMES[i]) return i;
    return -1;
}
// fields of the context derived from an option (id < 0: all of them)
static void opt_apply(metrpo_ctx* c, int id) {
    if (id < 0) c->upd_tiles_per_wave = 1;
    // (NO_RESIDENT does not touch c->exclusive -- the caller's metrpo_set_exclusive value: ctx_exclusive() combines the two at every use.)
    if (id == OPT_XCHG_TIMEOUT_MS && ctx_opt(c, OPT_XCHG_TIMEOUT_MS)) { const long long v = atoll(ctx_opt(c, OPT_XCHG_TIMEOUT_MS)); if (v > 0) c->xg_timeout = (unsigned long long)v * 100000ull; }
}
// value == NULL unsets the key.  Read by the NEXT launch; options that size a workspace or select a kernel table entry at set_dynamics / set_policy time
// (none today) would say so here.
extern "C" int32_t metrpo_set_option(metrpo_ctx* c, const char* key, const char* value) {
    if (!c || !key) return METRPO_ENULL;
    const int id = metrpo_opt_id(key);
    if (id < 0) return set_err(c, METRPO_EINVAL, std::string("set_option: unknown key '") + key + "'");
    c->opt_set[id] = (value != nullptr); c->opt_val[id] = value ? value : "";
    opt_apply(c, id);
    return METRPO_OK;
}
// returns the value's length (copied into buf, NUL-terminated, truncated to cap - 1), METRPO_UNSET when the key is unset, METRPO_EINVAL for an unknown key
extern "C" int32_t metrpo_get_option(metrpo_ctx* c, const char* key, char* buf, int32_t cap) {
    if (!c || !key) return METRPO_ENULL;
    const int id = metrpo_opt_id(key);
    if (id < 0) return set_err(c, METRPO_EINVAL, std::string("get_option: unknown key '") + key + "'");
    if (!c->opt_set[id]) return METRPO_UNSET;
    if (buf && cap > 0) { const size_t n = std::min<size_t>(c->opt_val[id].size(), (size_t)cap - 1); memcpy(buf, c->opt_val[id].data(), n); buf[n] = 0; }
    return (int32_t)c->opt_val[id].size();
}
// key of option i (NULL beyond the table): lets a binding enumerate the switches
extern "C" const char* metrpo_option_name(int32_t i) { return metrpo_opt_name(i); }

extern "C" int32_t metrpo_create(metrpo_ctx** out, int32_t device, const metrpo_dims* d) {
    if (!out || !d) return METRPO_ENULL;
    *out = nullptr;
    if (d->ns <= 0 || d->na <= 0 || d->n_models <= 0 || d->n_drop < 0 || d->n_drop >= d->ns) return METRPO_EINVAL;
    if (d->env < METRPO_ENV_SWIMMER || d->env > METRPO_ENV_SNAKE) return METRPO_EINVAL;
    // the analytic rewards index fixed state columns (see metrpo_env)
    const int min_ns[] = {6, 10, 16, 1, 6, 8};
    if (d->ns < min_ns[d->env]) return METRPO_EINVAL;
    metrpo_ctx* c = new (std::nothrow) metrpo_ctx();
    if (!c) return METRPO_EINVAL;
    c->device = device; c->dims = *d;
    for (int i = 0; i < OPT_COUNT; ++i) {                     // the ONLY place the library reads the environment for kernel selection: defaults of the option table
        const std::string ev = std::string("METRPO_") + metrpo_opt_name(i);
        const char* e = getenv(ev.c_str());
        c->opt_set[i] = (e != nullptr); c->opt_val[i] = e ? e : "";
    }
    opt_apply(c, -1);
    ProblemDesc& pd = c->pd;
    pd.env = d->env; pd.ns = d->ns; pd.na = d->na; pd.K = d->n_models; pd.n_drop = d->n_drop;
    pd.nin = d->ns + d->na - d->n_drop;
    if (!build_net(&pd.dyn, pd.nin, d->dyn_hidden, d->dyn_act, d->dyn_n_hidden, d->ns, METRPO_ACT_RELU, true) ||
        !build_net(&pd.pol, d->ns, d->pol_hidden, nullptr, d->pol_n_hidden, d->na, METRPO_ACT_TANH, false)) {
        delete c;
        return METRPO_EINVAL;
    }
    pd.P = pd.pol.n_params + d->na;
    *out = c;
    if (hipSetDevice(device) != hipSuccess) { c->err = "hipSetDevice failed"; return METRPO_EHIP; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_sm = prop.multiProcessorCount;
    const size_t ncg = (size_t)(1 + pd.P) + 5 * (size_t)pd.P + 8 + 2 + 4 + 2;      // ... | scal[8] | lk[2] | ls[4] | validation time-out cell (val_err_cell) | sub-batch index cell (sub_err_cell)
    int rc;
    if ((rc = ws_grow(c, c->d_dyn, sizeof(float) * (size_t)pd.K * pd.dyn.n_params)) || (rc = ws_grow(c, c->d_norm, sizeof(float) * (2 * (pd.ns + pd.na) + 2 * pd.ns))) ||
        (rc = ws_grow(c, c->d_theta, sizeof(float) * pd.P)) || (rc = ws_grow(c, c->d_vf, sizeof(float) * pd.P)) || (rc = ws_grow(c, c->d_theta_try, sizeof(float) * pd.P)) ||
        (rc = ws_grow(c, c->d_cg, sizeof(double) * ncg)) || (rc = ws_grow(c, c->d_valbuf, sizeof(double) * pd.K)) || (rc = ws_grow(c, c->d_ticket, sizeof(unsigned int))))
        return rc;
    if (hipHostMalloc(&c->h_pinned, sizeof(double) * 24) != hipSuccess) { c->err = "pinned host allocation failed"; return METRPO_EHIP; }
    if (hipMemset(c->d_dyn.p, 0, sizeof(float) * (size_t)pd.K * pd.dyn.n_params) != hipSuccess) { c->err = "hipMemset failed"; return METRPO_EHIP; }
    if (hipMemset(c->d_cg.p, 0, sizeof(double) * ncg) != hipSuccess) { c->err = "hipMemset failed"; return METRPO_EHIP; }   // scal[S_COMMERR] starts clear
    if (hipMemset(c->d_ticket.p, 0, sizeof(unsigned int)) != hipSuccess) { c->err = "hipMemset failed"; return METRPO_EHIP; }   // the reductions' arrival counter resets itself
    c->mfma_cfg = mfma_select_config(c);
    c->pol_mfma = policy_mfma_select(pd);
    c->pol_f3 = policy_f3_select(pd);
    c->coop_cfg = coop_select_config(c);
    if (c->coop_cfg < 0 && pd.dyn.n_layers == 3 && pd.dyn.dims[1] <= 64 && pd.dyn.dims[2] <= 64) {      // narrow nets (either width below 64): zero-padded to the fused kernel's 64 x 64
        const int32_t hid64[2] = {64, 64}, acts[2] = {pd.dyn.act[0], pd.dyn.act[1]};
        if (build_net(&c->dyn_pad, pd.nin, hid64, acts, 2, pd.ns, METRPO_ACT_RELU, true)) {
            const NetDesc real = pd.dyn;
            pd.dyn = c->dyn_pad;
            const int cfg = coop_select_config(c);                         // the table's view of the padded shape (env dims, activations, policy, K, LDS)
            pd.dyn = real;
            if (cfg >= 0) {
                const size_t bytes = sizeof(float) * (size_t)pd.K * c->dyn_pad.n_params;
                if (ws_grow(c, c->d_dyn_pad, bytes) != METRPO_OK || hipMemset(c->d_dyn_pad.p, 0, bytes) != hipSuccess) { c->err = "hipMalloc failed (padded dynamics)"; return METRPO_EHIP; }
                c->coop_pad_cfg = cfg;
            }
        }
    }
    c->det_cfg = det_mfma_select(c);
    c->det_padded = (c->coop_cfg < 0 && c->coop_pad_cfg >= 0) ? 1 : 0;
    c->det_gemm = det_gemm_applicable(c) ? 1 : 0;
    (void)sched_cus(c, nullptr);                              // CU census here, not inside the first resident / cooperative launch (probe.hip)
    return METRPO_OK;
}

extern "C" int32_t metrpo_destroy(metrpo_ctx* c) {
    if (!c) return METRPO_ENULL;
    if (c->nccl_comm) (void)metrpo_comm_destroy(c);
    (void)metrpo_comm_ipc_detach(c);
    if (c->xg_region) (void)hipFree(c->xg_region);
    if (c->side_ready) {
        for (int i = 0; i < METRPO_MAX_PAR_ROUNDS - 1; ++i) { (void)hipStreamDestroy(c->side_stream[i]); (void)hipEventDestroy(c->ev_join[i]); }
        (void)hipEventDestroy(c->ev_fork);
    }
    for (int i = 0; i < c->fvp_ev_made; ++i) (void)hipEventDestroy(c->fvp_ev[i]);
    ws_sweep(c);
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    if (c->h_upd) (void)hipHostFree(c->h_upd);
    if (c->h_lb) (void)hipHostFree(c->h_lb);
    delete c;                                                 // frees the context's device buffers (DevBuf)
    return METRPO_OK;
}

extern "C" const char* metrpo_last_error(const metrpo_ctx* c) { return c ? c->err.c_str() : "null ctx"; }
extern "C" int32_t metrpo_dyn_param_count(const metrpo_ctx* c) { return c ? c->pd.dyn.api_n_params : METRPO_ENULL; }
extern "C" int32_t metrpo_policy_param_count(const metrpo_ctx* c) { return c ? c->pd.P : METRPO_ENULL; }

extern "C" int32_t metrpo_set_dynamics(metrpo_ctx* c, const float* p, const float* in_mean, const float* in_std,
                                       const float* diff_mean, const float* diff_std, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!p || !in_mean || !in_std || !diff_mean || !diff_std) return set_err(c, METRPO_ENULL, "set_dynamics: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const ProblemDesc& pd = c->pd;
    const int nx = pd.ns + pd.na;
    repack_dyn(c, p, c->d_dyn.p, pd.K, true, st);
    HIP_TRY(c, hipMemcpyAsync(c->d_norm.p, in_mean, sizeof(float) * nx, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_norm.p + nx, in_std, sizeof(float) * nx, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_norm.p + 2 * nx, diff_mean, sizeof(float) * pd.ns, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_norm.p + 2 * nx + pd.ns, diff_std, sizeof(float) * pd.ns, hipMemcpyDeviceToDevice, st));
    c->have_dyn = true;
    if (c->mfma_cfg >= 0) return mfma_prepare_dynamics(c, st);
    return METRPO_OK;
}

extern "C" int32_t metrpo_set_policy(metrpo_ctx* c, const float* theta, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!theta) return set_err(c, METRPO_ENULL, "set_policy: NULL pointer");
    if (c->upd_pending) return set_err(c, METRPO_ESTATE, "set_policy: an update begun with metrpo_trpo_update_begin is still open (metrpo_trpo_update_end decides which theta stands)");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(c, hipMemcpyAsync(c->d_theta.p, theta, sizeof(float) * c->pd.P, hipMemcpyDeviceToDevice, st));
    c->have_pol = true;
    if (c->mfma_cfg >= 0) return mfma_prepare_policy(c, st);
    return METRPO_OK;
}

extern "C" int32_t metrpo_get_policy(metrpo_ctx* c, float* out, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!out) return set_err(c, METRPO_ENULL, "get_policy: NULL pointer");
    if (!c->have_pol) return set_err(c, METRPO_ESTATE, "policy not set");
    HIP_TRY(c, hipMemcpyAsync(out, c->d_theta.p, sizeof(float) * c->pd.P, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return METRPO_OK;
}

#define NEED_POL(c) if (!(c)->have_pol) return set_err((c), METRPO_ESTATE, "metrpo_set_policy has not been called")
#define NEED_DYN(c) if (!(c)->have_dyn) return set_err((c), METRPO_ESTATE, "metrpo_set_dynamics has not been called")

extern "C" int32_t metrpo_policy_actions(metrpo_ctx* c, const float* obs, const float* eps, int32_t B, float* actions,
                                         float* mean, void* stream) {
    if (!c) return METRPO_ENULL;
    NEED_POL(c);
    if (B < 0) return set_err(c, METRPO_EINVAL, "policy_actions: B < 0");
    if (B == 0) return METRPO_OK;
    if (!obs || !actions || !mean) return set_err(c, METRPO_ENULL, "policy_actions: NULL pointer");
    return launch_policy_actions(c, obs, eps, B, actions, mean, (hipStream_t)stream);
}

static bool sam_ok(int m) { return m >= METRPO_SAM_STEP_RAND && m <= METRPO_SAM_ONE_MODEL; }

extern "C" int32_t metrpo_step(metrpo_ctx* c, const float* s, const float* a, int32_t B, int32_t sam_mode,
                               const int32_t* model_idx, const float* noise, float* s_next, float* reward,
                               uint8_t* done, float* next_all, void* stream) {
    if (!c) return METRPO_ENULL;
    NEED_DYN(c);
    if (!sam_ok(sam_mode)) return set_err(c, METRPO_EINVAL, "sam mode is not defined");      // env_helpers.py:634
    if (B == 0) return METRPO_OK;
    if (!s || !a || !s_next || !reward || !done) return set_err(c, METRPO_ENULL, "step: NULL pointer");
    if ((sam_mode == METRPO_SAM_STEP_RAND || sam_mode == METRPO_SAM_EPS_RAND) && !model_idx)
        return set_err(c, METRPO_ENULL, "step: model_idx required for step_rand/eps_rand");
    if (sam_mode == METRPO_SAM_MODEL_MEAN_STD && !noise) return set_err(c, METRPO_ENULL, "step: noise required for model_mean_std");
    if (B < 0) return set_err(c, METRPO_EINVAL, "step: B < 0");
    if (B == 0) return METRPO_OK;
    return launch_step(c, s, a, B, sam_mode, model_idx, noise, s_next, reward, done, next_all, (hipStream_t)stream);
}

// a shape that the fast kernels' tables do not hold: remembered for metrpo_rollout_note and reported ONCE per context on stderr (option QUIET silences it)
static void note_off_table(metrpo_ctx* c, const std::string& why) {
    c->rollout_note = why;
    if (!c->fallback_logged && ctx_opt(c, OPT_QUIET) == nullptr) fprintf(stderr, "metrpo: rollout off the fast path: %s\n", why.c_str());
    c->fallback_logged = 1;
}
extern "C" int32_t metrpo_rollout(metrpo_ctx* c, const metrpo_rollout_args* a, void* stream) {
    TraceRange trace_("metrpo:rollout (obtain_samples: policy + env)");
    if (!c) return METRPO_ENULL;
    if (!a) return set_err(c, METRPO_ENULL, "rollout: args NULL");
    NEED_DYN(c); NEED_POL(c);
    if (!sam_ok(a->sam_mode)) return set_err(c, METRPO_EINVAL, "sam mode is not defined");
    if (a->B < 0 || a->T < 0 || a->H <= 0 || a->n_pool <= 0) return set_err(c, METRPO_EINVAL, "rollout: bad B/T/H/n_pool");
    if (!a->d_pool || !a->d_obs || !a->d_act || !a->d_rew || !a->d_mean || !a->d_done || !a->d_tpath)
        return set_err(c, METRPO_ENULL, "rollout: required pointer is NULL");
    if (a->t0 < 0) return set_err(c, METRPO_EINVAL, "rollout: t0 < 0");
    if (a->stop_batch < 0 || (a->stop_batch > 0 && a->d_stop_cum == nullptr)) return set_err(c, METRPO_EINVAL, "rollout: stop_batch needs d_stop_cum (and must not be negative)");
    if ((a->d_init_obs != nullptr) != (a->d_init_ts != nullptr) || (a->d_init_obs != nullptr) != (a->d_init_model != nullptr))
        return set_err(c, METRPO_EINVAL, "rollout: d_init_obs, d_init_ts and d_init_model must be given together");
    if (a->B == 0 || a->T == 0) return METRPO_OK;
    c->rollout_note.clear();
    c->roll_last = metrpo_ctx::RollLast();
    if (c->dyn_precision == METRPO_DYN_BF16) {                                               // opt-in (metrpo_set_dyn_precision: GEMM-class shapes only)
        c->last_rollout_kernel = 7;
        return launch_rollout_gemm(c, a, (hipStream_t)stream);
    }
    if (c->mfma_cfg >= 0 || c->coop_cfg >= 0 || c->coop_pad_cfg >= 0) {
        int coop = 0;
        const int rc = launch_rollout_mfma(c, a, (hipStream_t)stream, &coop);
        if (rc != METRPO_EUNSUPPORTED) {
            c->last_rollout_kernel = coop ? 2 : 1;
            if (!coop && c->rollout_variant == 0)
                note_off_table(c, c->coop_cfg < 0 ? "the cooperative fused kernel (rollout_coop.hip) holds 2 x 64 dynamics + 2 x 32 policy with K = 1 ... 10 heads (Ant: 8, half-cheetah: 9 -- LDS); this shape (K = " +
                                  std::to_string(c->pd.K) + ") runs on the head-per-wave fused kernel (rollout_mfma.hip), ~2.5x the cooperative kernel's time per head"
                                  : "the cooperative fused kernel holds K = " + std::to_string(c->pd.K) + " > 5 heads only with a CU to itself per workgroup; more 16-env tiles than CUs on a device that "
                                    "is not exclusive (metrpo_set_exclusive / NO_RESIDENT): head-per-wave fused kernel (rollout_mfma.hip)");
            return rc;
        }
        if (c->coop_cfg >= 0 && c->rollout_variant == 0)
            note_off_table(c, "the cooperative fused kernel holds K = " + std::to_string(c->pd.K) + " > 8 heads only with a CU to itself per workgroup; more 16-env tiles than CUs on a device that "
                              "is not exclusive: step-wise tile GEMMs (rollout_gemm.hip), ~8x the fused kernel's time");
    }
    if (gemm_path_applicable(c)) {                                                           // large dynamics nets
        const int rc = launch_rollout_resident(c, a, (hipStream_t)stream);                   // ... at small batch: the whole time loop in one launch
        if (rc != METRPO_EUNSUPPORTED) return rc;
        c->last_rollout_kernel = 3;
        if (c->coop_cfg < 0 && c->mfma_cfg < 0 && mfma_shape_config(c) >= 0 && c->rollout_variant == 0)
            note_off_table(c, "K = " + std::to_string(c->pd.K) + " heads of this 2 x 64-class shape are beyond the fused kernels (cooperative: K <= 10, half-cheetah 9, Ant 8 -- "
                              "LDS; head-per-wave: K <= 8): step-wise tile GEMMs (rollout_gemm.hip), ~3x the fused kernels' time per head (profiles/r06_coop_heads.txt)");
        {
            bool m256 = true; std::string w;
            for (int l = 1; l < c->pd.dyn.n_layers; ++l) { m256 = m256 && (c->pd.dyn.dims[l] % 256 == 0); w += (l > 1 ? "x" : "") + std::to_string(c->pd.dyn.dims[l]); }
            if (!m256 && c->rollout_note.empty() && c->rollout_variant == 0)
                note_off_table(c, "dynamics hidden widths " + w + " are neither the fused kernels' 64x64 nor multiples of 256 (stream-K / persistent / resident kernels): step-wise tile "
                                  "GEMMs (rollout_gemm.hip), 3-4 launches per step -- at B = 5000 hidden 96 takes 3.8 ms where 64 takes 0.43 (INTEGRATION.md section 9)");
        }
        return launch_rollout_gemm(c, a, (hipStream_t)stream);
    }
    c->last_rollout_kernel = 0;
    {
        std::string w;
        for (int l = 1; l < c->pd.dyn.n_layers; ++l) w += (l > 1 ? "x" : "") + std::to_string(c->pd.dyn.dims[l]);
        note_off_table(c, "dynamics hidden widths " + w + " have no matrix-core rollout kernel (fused kernels: two hidden layers of 64; GEMM / stream-K / resident paths: every "
                          "hidden layer >= 16, ns <= 64): thread-per-env kernel (rollout_generic.hip), ~80x the fused kernels' time per env step");
    }
    return launch_rollout_generic(c, a, (hipStream_t)stream);
}
// why the last metrpo_rollout of this context ran outside the fast dispatch table ("" when it did not)
extern "C" const char* metrpo_rollout_note(const metrpo_ctx* c) { return c ? c->rollout_note.c_str() : ""; }
// which kernel family the last metrpo_rollout of this context ran on (-1: none yet): 0 generic, 1 head-per-wave MFMA, 2 cooperative MFMA,
// 3 step-wise GEMM, 4 resident (rollout_resident.hip), 5 step-wise with the stream-K fused ensemble kernel (mlp_streamk.h), 6 persistent stream-K (mlp_persist.h:
// all steps of a chunk in one launch), 7 step-wise GEMM with bf16 operands (rollout_bf16.hip; metrpo_set_dyn_precision below)
extern "C" int32_t metrpo_last_rollout_kernel(const metrpo_ctx* c) { return c ? c->last_rollout_kernel : METRPO_ENULL; }
// Operand precision of the dynamics forward inside metrpo_rollout.  BF16 exactly where the f32 rollout runs on a GEMM-class family (3, 5, 6): the GEMM path takes
// the shape and it is not one of the fused 2 x 64-class shapes; anywhere else the setter refuses and the precision stays what it was
extern "C" int32_t metrpo_set_dyn_precision(metrpo_ctx* c, int32_t precision) {
    if (!c) return METRPO_ENULL;
    if (precision != METRPO_DYN_F32 && precision != METRPO_DYN_BF16) return set_err(c, METRPO_EINVAL, "set_dyn_precision: unknown precision " + std::to_string(precision));
    if (precision == METRPO_DYN_BF16 && (!gemm_path_applicable(c) || c->mfma_cfg >= 0 || c->coop_cfg >= 0 || c->coop_pad_cfg >= 0 || mfma_shape_config(c) >= 0)) {
        std::string w;
        for (int l = 1; l < c->pd.dyn.n_layers; ++l) w += (l > 1 ? "x" : "") + std::to_string(c->pd.dyn.dims[l]);
        return set_err(c, METRPO_EUNSUPPORTED, "set_dyn_precision: bf16 operands need a shape of the step-wise GEMM rollout families (every hidden layer >= 16 units, ns <= 64, not a fused "
                                               "2 x 64-class shape); dynamics hidden " + w + ", ns = " + std::to_string(c->pd.ns) + ", K = " + std::to_string(c->pd.K) + " is not one: precision stays f32");
    }
    c->dyn_precision = precision;
    return METRPO_OK;
}
extern "C" int32_t metrpo_get_dyn_precision(const metrpo_ctx* c) { return c ? c->dyn_precision : METRPO_ENULL; }

extern "C" int32_t metrpo_sampler_progress(metrpo_ctx* c, const uint8_t* done, const int32_t* tpath, int32_t T, int32_t B, int32_t t0,
                                           int64_t batch_size, double* counts, double* state, int32_t* stop, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!done || !tpath || !counts || !state || !stop) return set_err(c, METRPO_ENULL, "sampler_progress: NULL pointer");
    if (T < 0 || B < 0 || t0 < 0 || batch_size < 0) return set_err(c, METRPO_EINVAL, "sampler_progress: bad T/B/t0/batch_size");
    if (T == 0 || B == 0) return METRPO_OK;
    return launch_sampler_progress(c, done, tpath, T, B, t0, batch_size, counts, state, stop, (hipStream_t)stream);
}

// test/diagnostic hook: force the generic kernel regardless of the MFMA table
extern "C" int32_t metrpo_rollout_generic(metrpo_ctx* c, const metrpo_rollout_args* a, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!a) return set_err(c, METRPO_ENULL, "rollout: args NULL");
    NEED_DYN(c); NEED_POL(c);
    if (!sam_ok(a->sam_mode)) return set_err(c, METRPO_EINVAL, "sam mode is not defined");
    if (a->B <= 0 || a->T <= 0 || a->H <= 0 || a->n_pool <= 0) return set_err(c, METRPO_EINVAL, "rollout: bad B/T/H/n_pool");
    if (!a->d_pool || !a->d_obs || !a->d_act || !a->d_rew || !a->d_mean || !a->d_done || !a->d_tpath)
        return set_err(c, METRPO_ENULL, "rollout: required pointer is NULL");
    return launch_rollout_generic(c, a, (hipStream_t)stream);
}
extern "C" int32_t metrpo_has_mfma_path(const metrpo_ctx* c) { return (c && c->mfma_cfg >= 0) ? 1 : 0; }
// test hook: 0 = fastest rollout kernel available, 1 = head-per-wave MFMA kernel even where the cooperative one exists,
// 2 = cooperative kernel in its two-workgroups-per-CU instantiation whatever the batch (rollout_coop.hip picks by tile count otherwise)
extern "C" int32_t metrpo_set_rollout_variant(metrpo_ctx* c, int32_t v) {
    if (!c) return METRPO_ENULL;
    c->rollout_variant = v;
    return (v != 1 && (c->coop_cfg >= 0 || (v == 0 && c->coop_pad_cfg >= 0))) ? 2 : (c->mfma_cfg >= 0 ? 1 : (gemm_path_applicable(c) ? 3 : 0));
}
// which policy-update kernels a batch of N samples would run on: 1 fused MFMA (policy_mfma.hip), 2 GEMM path (policy_gemm.hip), 0 generic
extern "C" int32_t metrpo_update_path(const metrpo_ctx* c, int64_t N) {
    if (!c) return METRPO_ENULL;
    return policy_gemm_applicable(c, N, false) ? 2 : ((c->pol_mfma >= 0 || f3_active(c, false)) ? 1 : 0);
}
// test hook: 0 forces the generic (VALU) update kernels, 1 restores the MFMA ones when available
extern "C" int32_t metrpo_set_update_path(metrpo_ctx* c, int32_t use_mfma) {
    if (!c) return METRPO_ENULL;
    // 0: generic (VALU) kernels, 1: fastest path of the shape (fused MFMA kernels, else the GEMM path for large N), 2: GEMM path forced
    c->pol_path = (use_mfma == 2) ? 2 : (use_mfma ? 1 : 0);
    c->pol_mfma = (use_mfma == 1) ? policy_mfma_select(c->pd) : -1;
    c->pol_f3 = (use_mfma == 1) ? policy_f3_select(c->pd) : 0;
    c->pg_fwd_rows = -1; c->f3_rows = -1;
    return (c->pol_mfma >= 0 || f3_active(c, false)) ? 1 : (c->pol_path == 2 ? 2 : 0);
}

extern "C" int32_t metrpo_validation_cost(metrpo_ctx* c, const float* s0, int32_t Bv, int32_t T, double gamma,
                                          double* costs, void* stream) {
    TraceRange trace_("metrpo:validation_cost");
    if (!c) return METRPO_ENULL;
    NEED_DYN(c); NEED_POL(c);
    if (!s0 || !costs) return set_err(c, METRPO_ENULL, "validation_cost: NULL pointer");
    if (Bv <= 0 || T < 0) return set_err(c, METRPO_EINVAL, "validation_cost: bad Bv/T");
    return launch_validation_cost(c, s0, Bv, T, gamma, costs, (hipStream_t)stream);
}

extern "C" int32_t metrpo_gae(metrpo_ctx* c, const float* obs, const float* rew, const uint8_t* done,
                              const int32_t* tpath, int32_t T, int32_t B, const double* coeffs, double gamma, double lam,
                              float* adv, float* ret, uint8_t* valid, double* stats, void* stream) {
    TraceRange trace_("metrpo:process_samples:gae");
    if (!c) return METRPO_ENULL;
    if (!obs || !rew || !done || !tpath || !adv || !ret || !valid || !stats) return set_err(c, METRPO_ENULL, "gae: NULL pointer");
    if (T < 0 || B < 0) return set_err(c, METRPO_EINVAL, "gae: bad T/B");
    if (T == 0 || B == 0) return METRPO_OK;
    return launch_gae(c, obs, rew, done, tpath, T, B, coeffs, gamma, lam, adv, ret, valid, stats, (hipStream_t)stream);
}

extern "C" int32_t metrpo_process_begin(metrpo_ctx* c, float* old_log_std, double* acc, int64_t n_acc, void* stream) {
    TraceRange trace_("metrpo:process_samples:begin");
    if (!c) return METRPO_ENULL;
    if (n_acc < 0 || n_acc > (1LL << 30) || (n_acc > 0 && !acc)) return set_err(c, METRPO_EINVAL, "process_begin: bad accumulator range");
    if (!old_log_std && n_acc == 0) return METRPO_OK;
    return launch_process_begin(c, old_log_std, n_acc > 0 ? acc : nullptr, n_acc, (hipStream_t)stream);
}

extern "C" int32_t metrpo_center_advantages(metrpo_ctx* c, float* adv, const uint8_t* valid, int64_t N,
                                            const double* stats, void* stream) {
    TraceRange trace_("metrpo:process_samples:center");
    if (!c) return METRPO_ENULL;
    if (!adv || !stats) return set_err(c, METRPO_ENULL, "center: NULL pointer");
    if (N <= 0) return METRPO_OK;
    return launch_center(c, adv, valid, N, stats, (hipStream_t)stream);
}

extern "C" int32_t metrpo_baseline_gram(metrpo_ctx* c, const float* obs, const float* ret, const int32_t* tpath,
                                        const uint8_t* valid, int64_t N, double* AtA, double* Aty, void* stream) {
    TraceRange trace_("metrpo:process_samples:baseline_gram");
    if (!c) return METRPO_ENULL;
    if (!obs || !ret || !tpath || !AtA || !Aty) return set_err(c, METRPO_ENULL, "gram: NULL pointer");
    if (N <= 0) return METRPO_OK;
    return launch_gram(c, obs, ret, tpath, valid, N, AtA, Aty, (hipStream_t)stream);
}

extern "C" int32_t metrpo_baseline_solve(metrpo_ctx* c, const double* AtA, const double* Aty, double reg_coeff, double* coeffs, void* stream) {
    TraceRange trace_("metrpo:process_samples:baseline_solve");
    if (!c) return METRPO_ENULL;
    if (!AtA || !Aty || !coeffs) return set_err(c, METRPO_ENULL, "baseline_solve: NULL pointer");
    if (!(reg_coeff >= 0.0)) return set_err(c, METRPO_EINVAL, "baseline_solve: reg_coeff must be >= 0");
    return launch_baseline_solve(c, AtA, Aty, reg_coeff, coeffs, (hipStream_t)stream);
}

extern "C" int32_t metrpo_loss_grad(metrpo_ctx* c, const metrpo_batch* b, double* out, void* stream) {
    if (!c) return METRPO_ENULL;
    NEED_POL(c);
    if (!out) return set_err(c, METRPO_ENULL, "loss_grad: out NULL");
    return launch_loss_grad(c, b, out, (hipStream_t)stream);
}
// algos/vpg.py:88 (surr_obj) and :100-118 (optimize_policy: FirstOrderOptimizer, one Adam step), policy_update.hip
extern "C" int32_t metrpo_vpg_loss_grad(metrpo_ctx* c, const metrpo_batch* b, double* out, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!out) return set_err(c, METRPO_ENULL, "vpg_loss_grad: out NULL");
    NEED_POL(c);
    return launch_vpg_loss_grad(c, b, out, (hipStream_t)stream);
}
extern "C" int32_t metrpo_vpg_update(metrpo_ctx* c, const metrpo_batch* b, const metrpo_vpg_params* pr, double* d_loss, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!pr) return set_err(c, METRPO_ENULL, "vpg_update: params NULL");
    NEED_POL(c);
    if (c->upd_pending) return set_err(c, METRPO_ESTATE, "vpg_update: a TRPO update is still open (metrpo_trpo_update_end first)");
    return run_vpg_update(c, b, pr, d_loss, (hipStream_t)stream);
}
// algos/ppo.py:107-119 (lr, ent, clipped_lr, clipped_surr_loss, clipped_surr_pen_loss), policy_update.hip
extern "C" int32_t metrpo_ppo_loss_grad(metrpo_ctx* c, const metrpo_batch* b, const metrpo_ppo_params* pr, double* out, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!pr) return set_err(c, METRPO_ENULL, "ppo_loss_grad: params NULL");
    if (!out) return set_err(c, METRPO_ENULL, "ppo_loss_grad: out NULL");
    NEED_POL(c);
    return launch_ppo_loss_grad(c, b, pr, out, (hipStream_t)stream);
}
// algos/ppo.py:157-177 (optimize_policy: optimizer.optimize on the inputs of :158-165); the optimiser of ppo.py:61-62 as include/metrpo.h states it
extern "C" int32_t metrpo_ppo_update(metrpo_ctx* c, const metrpo_batch* b, const metrpo_ppo_params* pr, int32_t n_epochs, double* d_losses, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!pr) return set_err(c, METRPO_ENULL, "ppo_update: params NULL");
    NEED_POL(c);
    if (c->upd_pending) return set_err(c, METRPO_ESTATE, "ppo_update: a TRPO update is still open (metrpo_trpo_update_end first)");
    return run_ppo_update(c, b, pr, n_epochs, d_losses, (hipStream_t)stream);
}
// algos/ppo.py:120-121 (use_kl_penalty: clipped_surr_pen_loss += kl_penalty_var * max(0, mean_kl - step_size)), policy_update.hip
extern "C" int32_t metrpo_ppo_kl_loss_grad(metrpo_ctx* c, const metrpo_batch* b, const metrpo_ppo_params* pr, const metrpo_ppo_kl_params* kp, const double* d_mean_kl,
                                           double* out, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!pr || !kp) return set_err(c, METRPO_ENULL, "ppo_kl_loss_grad: params NULL");
    if (!out) return set_err(c, METRPO_ENULL, "ppo_kl_loss_grad: out NULL");
    NEED_POL(c);
    return launch_ppo_kl_loss_grad(c, b, pr, kp, d_mean_kl, out, (hipStream_t)stream);
}
extern "C" int32_t metrpo_ppo_kl_update(metrpo_ctx* c, const metrpo_batch* b, const metrpo_ppo_params* pr, const metrpo_ppo_kl_params* kp, int32_t n_epochs, double* d_losses,
                                        double* d_mean_kls, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!pr || !kp) return set_err(c, METRPO_ENULL, "ppo_kl_update: params NULL");
    NEED_POL(c);
    if (c->upd_pending) return set_err(c, METRPO_ESTATE, "ppo_kl_update: a TRPO update is still open (metrpo_trpo_update_end first)");
    return run_ppo_kl_update(c, b, pr, kp, n_epochs, d_losses, d_mean_kls, (hipStream_t)stream);
}
// model_based_rl.py:391-398 (ScipyOptimizerInterface, method='L-BFGS-B') and :1197-1202 (the 'l-bfgs' branch), lbfgs.hip
static int lbfgs_opts_check(metrpo_ctx* c, const metrpo_lbfgs_opts* o, const char* who) {
    if (!o) return set_err(c, METRPO_ENULL, std::string(who) + ": opts NULL");
    if (o->m <= 0 || o->maxls <= 0) return set_err(c, METRPO_EINVAL, std::string(who) + ": m and maxls must be positive");
    if (!(o->ftol >= 0.0) || !(o->gtol >= 0.0)) return set_err(c, METRPO_EINVAL, std::string(who) + ": ftol and gtol must be >= 0");
    return METRPO_OK;
}
extern "C" int32_t metrpo_lbfgs_begin(metrpo_ctx* c, int32_t n, const double* x0, const metrpo_lbfgs_opts* o, double* x_eval, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!x0 || !x_eval) return set_err(c, METRPO_ENULL, "lbfgs_begin: NULL pointer");
    if (n <= 0) return set_err(c, METRPO_EINVAL, "lbfgs_begin: n must be positive");
    int rc;
    if ((rc = lbfgs_opts_check(c, o, "lbfgs_begin"))) return rc;
    return lbfgs_begin(c, n, x0, nullptr, o, x_eval, (hipStream_t)stream);
}
extern "C" int32_t metrpo_lbfgs_iterate(metrpo_ctx* c, const double* f, const double* g, double* x_eval, int32_t* task, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!f || !g || !x_eval || !task) return set_err(c, METRPO_ENULL, "lbfgs_iterate: NULL pointer");
    if (!c->lb_open) return set_err(c, METRPO_ESTATE, "lbfgs_iterate: no minimisation open (metrpo_lbfgs_begin first)");
    return lbfgs_iterate(c, f, g, x_eval, task, (hipStream_t)stream);
}
extern "C" int32_t metrpo_lbfgs_get_result(metrpo_ctx* c, metrpo_lbfgs_result* out, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!out) return set_err(c, METRPO_ENULL, "lbfgs_get_result: out NULL");
    if (!c->lb_open) return set_err(c, METRPO_ESTATE, "lbfgs_get_result: no minimisation open (metrpo_lbfgs_begin first)");
    return lbfgs_get_result(c, out, (hipStream_t)stream);
}
extern "C" int32_t metrpo_lbfgs_policy(metrpo_ctx* c, const float* init, int32_t B, int32_t T, double gamma, const metrpo_lbfgs_opts* o,
                                       metrpo_lbfgs_result* out, void* stream) {
    TraceRange trace_("metrpo:lbfgs_policy");
    if (!c) return METRPO_ENULL;
    if (!init || !out) return set_err(c, METRPO_ENULL, "lbfgs_policy: NULL pointer");
    int rc;
    if ((rc = lbfgs_opts_check(c, o, "lbfgs_policy"))) return rc;
    if (o->lookahead < 1 || o->lookahead > 16) return set_err(c, METRPO_EINVAL, "lbfgs_policy: lookahead must be in 1..16");
    NEED_DYN(c); NEED_POL(c);
    if (B <= 0 || T <= 0) return set_err(c, METRPO_EINVAL, "lbfgs_policy: B and T must be positive");
    if (c->upd_pending) return set_err(c, METRPO_ESTATE, "lbfgs_policy: an update begun with metrpo_trpo_update_begin is still open (metrpo_trpo_update_end first)");
    return run_lbfgs_policy(c, init, B, T, gamma, o, out, (hipStream_t)stream);
}
extern "C" int32_t metrpo_fvp(metrpo_ctx* c, const metrpo_batch* b, const double* v, double* hv, void* stream) {
    if (!c) return METRPO_ENULL;
    NEED_POL(c);
    return launch_fvp(c, b, v, hv, (hipStream_t)stream);
}
extern "C" int32_t metrpo_loss_kl(metrpo_ctx* c, const metrpo_batch* b, const float* theta, double* out, void* stream) {
    if (!c) return METRPO_ENULL;
    NEED_POL(c);
    if (!out) return set_err(c, METRPO_ENULL, "loss_kl: out NULL");
    return launch_loss_kl(c, b, theta, out, (hipStream_t)stream);
}

// ---- ensemble dynamics training ----------------------------------------------------------
extern "C" int32_t metrpo_dyn_train_reset(metrpo_ctx* c, void* stream) {
    if (!c) return METRPO_ENULL;
    c->adam_t = 0;
    if (c->d_adam.p) {
        const size_t nP = (((size_t)c->pd.K * c->pd.dyn.n_params) + 3) & ~(size_t)3;
        HIP_TRY(c, hipMemsetAsync(c->d_adam.p, 0, 2 * nP * sizeof(float), (hipStream_t)stream));
    }
    return METRPO_OK;
}

// optimizer state in / out (checkpoints, formats.py): the moments cross the ABI in metrpo_get_dynamics' dense layout, t as the step count
// the next metrpo_dyn_train_step continues from.  Before the first step the state is zero; a set allocates it as that step would.
extern "C" int32_t metrpo_get_dyn_adam(metrpo_ctx* c, float* m, float* v, int64_t* t_out, void* stream) {
    if (!c) return METRPO_EINVAL;
    if (!m || !v || !t_out) return set_err(c, METRPO_EINVAL, "get_dyn_adam: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (!c->d_adam.p) {
        const size_t n = (size_t)c->pd.K * c->pd.dyn.api_n_params * sizeof(float);
        HIP_TRY(c, hipMemsetAsync(m, 0, n, st));
        HIP_TRY(c, hipMemsetAsync(v, 0, n, st));
        *t_out = 0;
        return METRPO_OK;
    }
    const float* am = (const float*)c->d_adam.p;
    repack_dyn(c, am, m, c->pd.K, false, st);
    repack_dyn(c, am + dyn_adam_floats(c), v, c->pd.K, false, st);
    HIP_TRY(c, hipGetLastError());
    *t_out = c->adam_t;
    return METRPO_OK;
}

extern "C" int32_t metrpo_set_dyn_adam(metrpo_ctx* c, const float* m, const float* v, int64_t t, void* stream) {
    if (!c) return METRPO_EINVAL;
    if (!m || !v) return set_err(c, METRPO_EINVAL, "set_dyn_adam: NULL pointer");
    if (t < 0) return set_err(c, METRPO_EINVAL, "set_dyn_adam: t < 0");
    const int rc = ensure_dyn_adam(c);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* am = (float*)c->d_adam.p;
    repack_dyn(c, m, am, c->pd.K, true, st);                          // the padding slots of the resident layout stay zero
    repack_dyn(c, v, am + dyn_adam_floats(c), c->pd.K, true, st);
    HIP_TRY(c, hipGetLastError());
    c->adam_t = t;
    return METRPO_OK;
}

extern "C" int32_t metrpo_dyn_train_step(metrpo_ctx* c, const float* x, const float* y, const metrpo_train_params* tp, double* loss_out,
                                         void* stream) {
    TraceRange trace_("metrpo:dyn_train_step");
    if (!c) return METRPO_ENULL;
    NEED_DYN(c);
    if (!x || !y || !tp) return set_err(c, METRPO_ENULL, "dyn_train_step: NULL pointer");
    if (tp->batch_size <= 0 || !(tp->lr >= 0.0)) return set_err(c, METRPO_EINVAL, "dyn_train_step: bad batch_size / lr");
    return launch_dyn_train_step(c, x, y, tp, loss_out, (hipStream_t)stream);
}

extern "C" int32_t metrpo_dyn_eval_losses(metrpo_ctx* c, const float* x, const float* y, int64_t n, double reg_constant, double* losses,
                                          void* stream) {
    if (!c) return METRPO_ENULL;
    NEED_DYN(c);
    if (!x || !y || !losses) return set_err(c, METRPO_ENULL, "dyn_eval_losses: NULL pointer");
    if (n <= 0) return set_err(c, METRPO_EINVAL, "dyn_eval_losses: n must be positive");
    return launch_dyn_eval_losses(c, x, y, n, reg_constant, losses, (hipStream_t)stream);
}

extern "C" int32_t metrpo_get_dynamics(metrpo_ctx* c, float* out, void* stream) {
    if (!c) return METRPO_ENULL;
    NEED_DYN(c);
    if (!out) return set_err(c, METRPO_ENULL, "get_dynamics: NULL pointer");
    repack_dyn(c, c->d_dyn.p, out, c->pd.K, false, (hipStream_t)stream);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

extern "C" int32_t metrpo_set_dynamics_model(metrpo_ctx* c, int32_t model, const float* p, void* stream) {
    if (!c) return METRPO_ENULL;
    NEED_DYN(c);
    if (!p) return set_err(c, METRPO_ENULL, "set_dynamics_model: NULL pointer");
    if (model < 0 || model >= c->pd.K) return set_err(c, METRPO_EINVAL, "set_dynamics_model: model index out of range");
    repack_dyn(c, p, c->d_dyn.p + (size_t)model * c->pd.dyn.n_params, 1, true, (hipStream_t)stream);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

extern "C" int32_t metrpo_set_normalizers(metrpo_ctx* c, const float* in_mean, const float* in_std, const float* diff_mean,
                                          const float* diff_std, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!in_mean || !in_std || !diff_mean || !diff_std) return set_err(c, METRPO_ENULL, "set_normalizers: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const int nx = c->pd.ns + c->pd.na, ns = c->pd.ns;
    HIP_TRY(c, hipMemcpyAsync(c->d_norm.p, in_mean, sizeof(float) * nx, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_norm.p + nx, in_std, sizeof(float) * nx, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_norm.p + 2 * nx, diff_mean, sizeof(float) * ns, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_norm.p + 2 * nx + ns, diff_std, sizeof(float) * ns, hipMemcpyDeviceToDevice, st));
    return METRPO_OK;
}

extern "C" int32_t metrpo_rms_accumulate(metrpo_ctx* c, const float* x, int64_t n, int32_t dim, double* rsum, double* rsumsq, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!x || !rsum || !rsumsq) return set_err(c, METRPO_ENULL, "rms_accumulate: NULL pointer");
    if (n < 0 || dim <= 0) return set_err(c, METRPO_EINVAL, "rms_accumulate: bad n / dim");
    if (n == 0) return METRPO_OK;
    return launch_rms_accumulate(c, x, n, dim, rsum, rsumsq, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// TRPO update driver: [rllab] ConjugateGradientOptimizer.optimize + krylov.cg, vectors resident on
// the device in float64 (the reference keeps them in host NumPy float64), one block per vector op.
// ------------------------------------------------------------------------------------------------
__global__ void k_cg_init(int P, const double* __restrict__ gout, double* x, double* r, double* p, float* pf, double* scal) {
    __shared__ double sh[16];
    cg_init_body(P, gout, x, r, p, PfOut{pf, nullptr, nullptr}, scal, sh);
}

__global__ void k_cg_step(CgTail t, int) {
    __shared__ double sh[16];
    cg_tail_run(t, sh);
}

__global__ void k_cg_finish_implicit(int P, double max_kl, const double* x, const double* r, const double* gout, double* step, double* scal) {
    __shared__ double sh[16];
    cg_finish_implicit(P, max_kl, x, r, gout + 1, step, scal, sh);
}

__global__ void k_cg_finish(int P, double reg, double max_kl, const double* x, double* z, double* step, double* scal) {
    __shared__ double sh[16];
    cg_finish_body(P, reg, max_kl, x, z, step, scal, sh);
}

// the update's outcome into pinned host memory as a launch of its own (no speculated trial whose reduction could carry it: cg_device.h ls_publish)
__global__ void k_ls_publish(const double* __restrict__ src, double* dst, unsigned long long stamp) { ls_publish(src, dst, stamp); }
__global__ void k_ls_reset(double* ls) { if (threadIdx.x == 0) { ls[0] = -1.0; ls[1] = NAN; ls[2] = NAN; ls[3] = 0.0; } }
__global__ void k_zero_f(float* p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.0f;
}

__global__ void k_try_theta(int P, double ratio, const float* __restrict__ prev, const double* __restrict__ step, float* cur, const double* __restrict__ ls,
                            double* ls_reset = nullptr) {
    // trial 0 of a device-decided search also opens it (ls <- "not stopped yet": what k_ls_reset does as a launch of its own); it is never skipped itself
    if (ls_reset != nullptr && blockIdx.x == 0 && threadIdx.x == 0) { ls_reset[0] = -1.0; ls_reset[1] = NAN; ls_reset[2] = NAN; ls_reset[3] = 0.0; }
    if (ls != nullptr && ls[0] >= 0.0) return;                      // speculative trial after the search stopped: cur must keep the accepted theta's source
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P) cur[i] = (float)((double)prev[i] - ratio * step[i]);     // cur_param = prev_param - ratio * flat_descent_step
}

// phase: 0 = the whole update with the line search decided on the host (one synchronisation per trial, as the reference does);
//        1 = metrpo_trpo_update_begin: solve + the first `spec` line-search trials enqueued with the accept test on the DEVICE (ls_decide), no
//            synchronisation; 2 = metrpo_trpo_update_end: fetch the outcome, continue on the host from trial `spec` if the search has not stopped
static int run_trpo_update_impl(metrpo_ctx* c, const metrpo_batch* b, const metrpo_trpo_params* pr, metrpo_trpo_diag* diag,
                                double* g_out, double* dir_out, hipStream_t st, int phase, int spec, const metrpo_batch* fb);
// The arrival counter of the fused tails (d_ticket) resets itself in the last block of every reduction, so a completed update leaves it
// at zero.  An update that FAILED half-way (a launch error, a time-out) may not: it is cleared on the error path, where the cost of a
// 4-byte memset does not matter -- a stale count would silently disable every later CG tail.
int run_trpo_update(metrpo_ctx* c, const metrpo_batch* b, const metrpo_trpo_params* pr, metrpo_trpo_diag* diag,
                    double* g_out, double* dir_out, hipStream_t st, int phase, int spec, const metrpo_batch* fb) {
    const int rc = run_trpo_update_impl(c, b, pr, diag, g_out, dir_out, st, phase, spec, fb);
    if (rc != METRPO_OK) {
        (void)hipGetLastError(); (void)hipMemsetAsync(c->d_ticket.p, 0, sizeof(unsigned int), st); c->upd_pending = 0;
    }
    return rc;
}
// Can this update's line search be decided on the device?  Needs the single-launch-sequence update (no host callback / stand-alone
// all-reduce between a reduction and its consumer) on the fused MFMA or generic kernels; the GEMM path has its own reductions.
static bool device_line_search_ok(const metrpo_ctx* c, const metrpo_batch* b, const metrpo_trpo_params* pr) {
    return update_fusion(c, b->N, pr->allreduce != nullptr).carries_next_step();
}
// fb == b in every field (or NULL) is the whole-batch update: the launches and results of ABI 4's entry points, bit for bit
static bool same_batch(const metrpo_batch* a, const metrpo_batch* b) {
    return a->d_obs == b->d_obs && a->d_act == b->d_act && a->d_adv == b->d_adv && a->d_old_mean == b->d_old_mean && a->d_old_log_std == b->d_old_log_std &&
           a->old_log_std_stride == b->old_log_std_stride && a->d_valid == b->d_valid && a->N == b->N && a->inv_n_global == b->inv_n_global;
}
static int run_trpo_update_impl(metrpo_ctx* c, const metrpo_batch* b, const metrpo_trpo_params* pr, metrpo_trpo_diag* diag,
                                double* g_out, double* dir_out, hipStream_t st, int phase, int spec, const metrpo_batch* fb) {
    const int P = c->pd.P;
    // [rllab] optimize(): loss_before, flat_g and every f_loss_constraint trial see `inputs` (b); Hx -- the cg_iters products of krylov.cg and the
    // d.(H d) of the step scale -- sees subsample_inputs (fb).  The partials of those launches are pre-scaled by fb's inv_n_global.
    const bool sub = fb != nullptr && fb != b && !same_batch(fb, b);
    const metrpo_batch* hb = sub ? fb : b;
    CgView v = cg_view(c);
    int rc;
    // sum over ranks: the caller's callback if given, else the RCCL communicator attached to the ctx (comm.hip), else single rank
#define AR(buf, n) do { if (pr->allreduce) { if ((rc = pr->allreduce(pr->allreduce_user, (buf), (n), (void*)st)) != 0) \
                                                 return set_err(c, METRPO_EINVAL, "allreduce callback failed"); } \
                        else if (fusion.exchange_in_tail) { /* summed in the tail of the reduction that produced buf */ } \
                        else if (c->nccl_comm || xg) { if ((rc = comm_allreduce_f64(c, (buf), (n), st)) != 0) return rc; } } while (0)
    // krylov.cg with every vector step fused into the tail of the kernel that produced its input (no all-reduce in between) or
    // as stand-alone one-block kernels after the caller's all-reduce.  The step scale needs d.(H d): by default it is taken
    // from the CG recurrence (cg_device.h: A x = g - r), explicit_final_hvp = 1 spends the extra FVP rllab spends.
    // Sharded over a peer-mapped transport (comm.hip, one-shot exchange): the reductions of the update kernels add the ranks' shares in
    // their own tail (SolveScope::exchange_in_tail), so the update keeps its single-rank launch sequence -- CG vector steps included.  The GEMM path
    // (policy_gemm.hip) has its own reduction kernels: there the exchange is the stand-alone one-shot kernel between them and the CG step.
    const bool xg = (pr->allreduce == nullptr && c->xg_world > 1);
    const UpdFusion fusion = update_fusion(c, b->N, pr->allreduce != nullptr);
    const bool fused = fusion.fused;
    SolveScope search;                   // what the line search's evaluations may rely on; the solve below adds its caches
    search.exchange_in_tail = fusion.exchange_in_tail;
    const int implicit_hd = pr->explicit_final_hvp ? 0 : 1;
    CgTail tl; tl.pub_dst = nullptr; tl.pub_stamp = 0; tl.P = P; tl.last = 0; tl.implicit_hd = implicit_hd; tl.reg = pr->reg_coeff; tl.tol = pr->residual_tol; tl.max_kl = pr->max_kl;
    tl.x = v.x; tl.r = v.r; tl.p = v.p; tl.z = v.z; tl.step = v.step; tl.scal = v.scal; tl.gout = v.gout; tl.pf = c->d_vf.p; tl.ticket = c->d_ticket.p;
    tl.vpos = nullptr; tl.imgval = nullptr; tl.ls = nullptr; tl.lk = nullptr; tl.th = nullptr; tl.th_try = nullptr; tl.trial = 0; tl.accept_violation = 0;
    const int nspec = std::min(spec, (int)pr->max_backtracks);
    // Device-decided line search (phase 1): theta of trial 0 is built by the tail that finishes the step size, theta of trial n + 1 by trial n's accept test
    // when the search goes on (cg_device.h: CgTail::nx_*) -- no k_try_theta launches in front of the evaluations.  Where the step does not come out of a
    // cg_tail_run (one-launch solve, cg_iters = 0, explicit H.d without a fused tail) the launches stay.
    bool try0_built = false;
    if (phase != 2) {
    tl.op = 3;
    SolveScope solve = search;
    solve.cache_activations = true;      // the gradient kernel publishes tanh activations, the CG products of this solve reuse them
    // ... and, when every CG vector comes out of a fused tail, its weight-fragment image; the tails add the tangent entries (policy_mfma.hip)
    solve.publish_image = fused && c->pol_mfma >= 0 && fusion.finalize_reduces;
    // A separate FVP batch: the activation caches and the weight-fragment image a gradient launch leaves (d_hcache / OP_FVPC, d_f3, the GEMM path's forward pass)
    // belong to `b` and must not be read for `fb`.  Its products run uncached (OP_FVP) and nothing is cached for them: DESIGN.md section 1 (row a16s)
    if (sub) solve = search;
    if (solve.publish_image) {
        if ((rc = policy_mfma_image_buffers(c))) return rc;
        tl.vpos = c->d_pol_vpos.p; tl.imgval = c->d_pol_imgval.p;
    }
    if ((rc = launch_loss_grad(c, b, v.gout, st, fused ? &tl : nullptr, solve))) return rc;
    // host-side record of this solve's products (metrpo_debug_last_solve): the gradient launch fixes the family, every product adds what upd_last says of it
    c->solve_last = {c->upd_last.family, -1, c->upd_last.table, 0, solve.cache_activations ? 1 : 0, solve.publish_image ? 1 : 0, fused ? 1 : 0, sub ? 1 : 0};
    auto note_fvp = [&]() {
        auto& s = c->solve_last;
        if (s.n_fvp > 0 && (s.op != c->upd_last.op || s.family != c->upd_last.family || s.table != c->upd_last.table)) s.op = -2;      // (the products of one solve disagree)
        else { s.family = c->upd_last.family; s.op = c->upd_last.op; s.table = c->upd_last.table; }
        s.n_fvp += 1;
    };
    if (!fused) {
        AR(v.gout, 1 + P);
        hipLaunchKernelGGL(k_cg_init, dim3(1), dim3(1024), 0, st, P, v.gout, v.x, v.r, v.p, c->d_vf.p, v.scal);   // same block shape as the fused tail: identical summation order
    }
    if (pr->cg_iters == 0) {
        hipLaunchKernelGGL(k_zero_f, dim3((P + 255) / 256), dim3(256), 0, st, c->d_vf.p, P);
        hipLaunchKernelGGL(k_cg_finish_implicit, dim3(1), dim3(1024), 0, st, P, pr->max_kl, v.x, v.r, v.gout, v.step, v.scal);
    }
    const bool fold_try = (phase == 1 && nspec >= 1);
    auto arm_try0 = [&]() { tl.nx_try = c->d_theta_try.p; tl.nx_prev = c->d_theta.p; tl.nx_ratio = 1.0; tl.nx_ls = v.ls; try0_built = true; };      // backtrack_ratio ^ 0
    for (int i = 0; i < pr->cg_iters; ++i) {
        tl.op = 1; tl.last = (i == pr->cg_iters - 1) ? 1 : 0;
        if (fold_try && tl.last && implicit_hd) arm_try0();
        if ((rc = launch_fvp_tail(c, hb, c->d_vf.p, v.p, v.z, fused ? &tl : nullptr, st, solve))) return rc;
        note_fvp();
        if (fused) continue;
        AR(v.z, P);
        hipLaunchKernelGGL(k_cg_step, dim3(1), dim3(1024), 0, st, tl, pr->cg_iters);
    }
    if (!implicit_hd && pr->cg_iters > 0) {                      // rllab's literal route: one more f_Hx on the descent direction
        tl.op = 2; tl.last = 0;
        if (fused && fold_try) arm_try0();
        if ((rc = launch_fvp_tail(c, hb, c->d_vf.p, v.x, v.z, fused ? &tl : nullptr, st, solve))) return rc;
        note_fvp();
        if (!fused) {
            AR(v.z, P);
            hipLaunchKernelGGL(k_cg_finish, dim3(1), dim3(1024), 0, st, P, pr->reg_coeff, pr->max_kl, v.x, v.z, v.step, v.scal);
        }
    }
    tl.vpos = nullptr; tl.imgval = nullptr; tl.nx_try = nullptr; tl.nx_prev = nullptr; tl.nx_ls = nullptr;
    if (g_out) HIP_TRY(c, hipMemcpyAsync(g_out, v.gout + 1, sizeof(double) * P, hipMemcpyDeviceToDevice, st));
    if (dir_out) HIP_TRY(c, hipMemcpyAsync(dir_out, v.x, sizeof(double) * P, hipMemcpyDeviceToDevice, st));
    }
    if (phase == 1) {
        // ---- the first `nspec` trials of the backtracking line search, each one's accept test in the tail of its own reduction (ls_decide): an
        //      accepted trial's theta is in place when the caller's next launch reads it; trials after the one that stopped the search leave at once
        if (!c->h_upd) { HIP_TRY(c, hipHostMalloc((void**)&c->h_upd, sizeof(double) * 17)); memset(c->h_upd, 0, sizeof(double) * 17); }
        c->upd_stamp += 1;                                          // _end waits for THIS stamp, not for what the caller enqueues after _begin
        if (nspec == 0) hipLaunchKernelGGL(k_ls_reset, dim3(1), dim3(64), 0, st, v.ls);
        for (int n = 0; n < nspec; ++n) {
            const double ratio = std::pow(pr->backtrack_ratio, (double)n);
            // trial 0 opens the search (ls reset rides in its k_try_theta), the last trial's reduction publishes the outcome: no launches of their own
            if (n == 0 && !try0_built)
                hipLaunchKernelGGL(k_try_theta, dim3((P + 255) / 256), dim3(256), 0, st, P, ratio, c->d_theta.p, v.step, c->d_theta_try.p, (const double*)nullptr, v.ls);
            CgTail dt = tl;
            if (n + 1 < nspec) { dt.nx_try = c->d_theta_try.p; dt.nx_prev = c->d_theta.p; dt.nx_ratio = std::pow(pr->backtrack_ratio, (double)(n + 1)); dt.nx_ls = nullptr; }
            dt.op = 4; dt.ls = v.ls; dt.lk = v.lk; dt.th = c->d_theta.p; dt.th_try = c->d_theta_try.p; dt.trial = n; dt.accept_violation = pr->accept_violation;
            if (n == nspec - 1) { dt.pub_dst = c->h_upd; dt.pub_stamp = c->upd_stamp; }
            if ((rc = launch_loss_kl(c, b, c->d_theta_try.p, v.lk, st, &dt, search))) return rc;
        }
        if (c->mfma_cfg >= 0 && (rc = mfma_prepare_policy(c, st))) return rc;      // of whatever theta the trials left in place
        if (nspec == 0) hipLaunchKernelGGL(k_ls_publish, dim3(1), dim3(64), 0, st, (const double*)v.scal, c->h_upd, c->upd_stamp);
        HIP_TRY(c, hipGetLastError());
        c->upd_pending = 1; c->upd_spec = nspec; c->upd_batch = *b; c->upd_params = *pr;
        return METRPO_OK;
    }
    // read-backs: ONE copy per line-search trial fetches scal[8] | lk[2] | ls[4] (loss at theta, beta, CG iterations, trial loss and KL)
    if (sub) HIP_TRY(c, hipMemcpyAsync(c->h_pinned + 16, sub_err_cell(c), sizeof(double), hipMemcpyDeviceToHost, st));      // (rides in front of the first trial's synchronisation)
    double loss = NAN, kl = NAN, loss_before = NAN;
    int n_iter = 0, n_start = 0;
    bool first = true, stopped = false, taken = false;
    if (phase == 2) {
        {   // the outcome _begin's last kernel published (a busy wait: this thread has nothing else to do, and a blocking wait costs 10-20 us to wake)
            volatile unsigned long long* stamp = (volatile unsigned long long*)(c->h_upd + 16);
            const auto t0 = std::chrono::steady_clock::now();
            long spins = 0;
            while (*stamp != c->upd_stamp) {
                if ((++spins & 0xFFFF) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) {
                    HIP_TRY(c, hipStreamSynchronize(st));         // surfaces a device fault; a healthy stream has published by now
                    if (*stamp != c->upd_stamp) return set_err(c, METRPO_EHIP, "trpo_update_end: the update's outcome never arrived");
                }
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            for (int i = 0; i < 14; ++i) c->h_pinned[i] = c->h_upd[i];
        }
        if (c->xg_world > 1 && c->h_pinned[S_COMMERR] != 0.0) return set_err(c, METRPO_EHIP, "trpo_update: one-shot all-reduce timed out (a rank did not arrive)");
        if (c->h_pinned[S_ROLLERR] != 0.0) return rollout_error_seen(c, st);
        loss_before = c->h_pinned[S_LOSS0]; first = false;
        loss = c->h_pinned[11]; kl = c->h_pinned[12];
        n_start = nspec; n_iter = nspec > 0 ? nspec - 1 : 0;
        if (c->h_pinned[10] >= 0.0) { stopped = true; n_iter = (int)c->h_pinned[10]; taken = c->h_pinned[13] != 0.0; }
    }
    for (int n = n_start; n < pr->max_backtracks && !stopped; ++n) {
        n_iter = n;
        const double ratio = std::pow(pr->backtrack_ratio, (double)n);
        hipLaunchKernelGGL(k_try_theta, dim3((P + 255) / 256), dim3(256), 0, st, P, ratio, c->d_theta.p, v.step, c->d_theta_try.p, (const double*)nullptr, (double*)nullptr);
        if ((rc = launch_loss_kl(c, b, c->d_theta_try.p, v.lk, st, nullptr, search))) return rc;
        AR(v.lk, 2);
        HIP_TRY(c, hipMemcpyAsync(c->h_pinned, v.scal, sizeof(double) * 10, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (c->xg_world > 1 && c->h_pinned[S_COMMERR] != 0.0) return set_err(c, METRPO_EHIP, "trpo_update: one-shot all-reduce timed out (a rank did not arrive)");
        if (c->h_pinned[S_ROLLERR] != 0.0) return rollout_error_seen(c, st);
        if (first) { loss_before = c->h_pinned[S_LOSS0]; first = false; }
        loss = c->h_pinned[8]; kl = c->h_pinned[9];
        if (loss < loss_before && kl <= pr->max_kl) break;
    }
    if (first) {
        HIP_TRY(c, hipMemcpyAsync(c->h_pinned, v.scal, sizeof(double) * 10, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st)); loss_before = c->h_pinned[S_LOSS0];
    }
    bool accepted = true;
    if ((std::isnan(loss) || std::isnan(kl) || loss >= loss_before || kl >= pr->max_kl) && !pr->accept_violation) accepted = false;
    if (stopped) accepted = taken;                               // decided on the device: an accepted trial's theta is already the policy
    else if (accepted) {
        std::swap(c->d_theta.p, c->d_theta_try.p);               // both ctx-owned and of one size, every launch takes c->d_theta afresh: no copy
        if (c->mfma_cfg >= 0 && (rc = mfma_prepare_policy(c, st))) return rc;
        c->upd_changed_in_end = (phase == 2) ? 1 : 0;        // theta changed on the HOST side of a two-half update: work enqueued after _begin used theta_prev
    }
    if (diag) {
        diag->loss_before = loss_before; diag->loss = loss; diag->kl = kl;
        diag->beta = c->h_pinned[S_BETA]; diag->n_backtrack = n_iter; diag->accepted = accepted ? 1 : 0;
        diag->cg_iters_run = (int)c->h_pinned[S_ITERS];
    }
    HIP_TRY(c, hipGetLastError());
#undef AR
    if (sub && c->h_pinned[16] != 0.0) {                        // the update is complete; the sub-batch it used was gathered from clamped rows
        (void)hipMemsetAsync(sub_err_cell(c), 0, sizeof(double), st);
        return set_err(c, METRPO_EINVAL, "trpo_update: the FVP sub-batch was gathered with a row index outside [0, N) (clamped by metrpo_subsample_batch)");
    }
    return METRPO_OK;
}

extern "C" int32_t metrpo_trpo_update(metrpo_ctx* c, const metrpo_batch* b, const metrpo_trpo_params* pr,
                                      metrpo_trpo_diag* diag, double* g_out, double* dir_out, void* stream) {
    TraceRange trace_("metrpo:trpo_update (optimize_policy)");
    if (!c) return METRPO_ENULL;
    NEED_POL(c);
    if (!b || !pr) return set_err(c, METRPO_ENULL, "trpo_update: NULL pointer");
    if (pr->cg_iters < 0 || pr->max_backtracks < 1) return set_err(c, METRPO_EINVAL, "trpo_update: bad cg_iters/max_backtracks");
    if (c->upd_pending) return set_err(c, METRPO_ESTATE, "trpo_update: an update begun with metrpo_trpo_update_begin is still open (call metrpo_trpo_update_end)");
    return run_trpo_update(c, b, pr, diag, g_out, dir_out, (hipStream_t)stream, 0, 0);
}

// The same update in two halves, so that the host can go on enqueuing work (the next rollout) while the line search is being decided: _begin
// launches gradient, CG solve and the first `spec_trials` trials of the backtracking search with the accept test on the device and returns
// WITHOUT synchronising; launches that follow it on the stream see the accepted trial's theta (or theta_prev).  _end synchronises, reports the
// diagnostics and -- only if none of the speculative trials stopped the search -- runs the remaining trials the ordinary way.  If the returned
// *late_out is 1, the policy changed inside _end: work enqueued in between used theta_prev and must be redone.
// Where the accept test cannot run on the device (host all-reduce callback, RCCL transport, GEMM update path) _begin does the whole update
// synchronously and _end only hands out the stored diagnostics.  d_g_out / d_dir_out as in metrpo_trpo_update.
extern "C" int32_t metrpo_trpo_update_begin(metrpo_ctx* c, const metrpo_batch* b, const metrpo_trpo_params* pr, int32_t spec_trials,
                                            double* g_out, double* dir_out, void* stream) {
    TraceRange trace_("metrpo:trpo_update_begin (optimize_policy, line search decided on the device)");
    if (!c) return METRPO_ENULL;
    NEED_POL(c);
    if (!b || !pr) return set_err(c, METRPO_ENULL, "trpo_update_begin: NULL pointer");
    if (pr->cg_iters < 0 || pr->max_backtracks < 1 || spec_trials < 1) return set_err(c, METRPO_EINVAL, "trpo_update_begin: bad cg_iters / max_backtracks / spec_trials");
    if (c->upd_pending) return set_err(c, METRPO_ESTATE, "trpo_update_begin: the previous update is still open (call metrpo_trpo_update_end)");
    if (!device_line_search_ok(c, b, pr)) {
        const int rc = run_trpo_update(c, b, pr, &c->upd_diag, g_out, dir_out, (hipStream_t)stream, 0, 0);
        if (rc == METRPO_OK) { c->upd_pending = 2; c->upd_spec = pr->max_backtracks; }      // complete: _end hands out upd_diag
        return rc;
    }
    return run_trpo_update(c, b, pr, nullptr, g_out, dir_out, (hipStream_t)stream, 1, spec_trials);
}
// ---- open-loop prediction error of the ensemble (env_helpers.py:96-172, :175-269; include/metrpo.h) ----
extern "C" int32_t metrpo_model_error_windows(metrpo_ctx* c, const float* d_Os, int32_t n, int32_t T, float* d_init_obs, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!d_Os || !d_init_obs) return set_err(c, METRPO_ENULL, "model_error_windows: NULL pointer");
    if (n <= 0 || T <= 0 || (long long)n * T > 2147483647LL / c->pd.ns) return set_err(c, METRPO_EINVAL, "model_error_windows: n and T must be positive (n * T * ns < 2^31)");
    return launch_window_starts(c, d_Os, n, T, T, d_init_obs, (hipStream_t)stream);
}
extern "C" int32_t metrpo_model_error(metrpo_ctx* c, const metrpo_model_error_args* a, void* stream) {
    TraceRange trace_("metrpo:model_error (evaluate_model_predictions / get_error_distribution)");
    if (!c) return METRPO_ENULL;
    if (!a) return set_err(c, METRPO_ENULL, "model_error: args NULL");
    if (!a->d_Os || !a->d_Rs || !a->hs) return set_err(c, METRPO_ENULL, "model_error: d_Os, d_Rs and hs are required");
    if (!a->d_state_diff || !a->d_cost_diff || !a->d_valid || !a->d_sums) return set_err(c, METRPO_ENULL, "model_error: NULL output buffer");
    if (a->n <= 0 || a->T <= 0) return set_err(c, METRPO_EINVAL, "model_error: n and T must be positive");
    if (a->n_h <= 0 || a->n_h > METRPO_MODEL_ERROR_MAX_HORIZONS) return set_err(c, METRPO_EINVAL, "model_error: n_h must be in 1 ... " + std::to_string(METRPO_MODEL_ERROR_MAX_HORIZONS));
    if (a->hs[0] < 1) return set_err(c, METRPO_EINVAL, "model_error: horizons start at 1");
    for (int i = 1; i < a->n_h; ++i)
        if (a->hs[i] <= a->hs[i - 1]) return set_err(c, METRPO_EINVAL, "model_error: hs is not sorted (strictly increasing)");
    if (a->hs[a->n_h - 1] > a->T) return set_err(c, METRPO_EINVAL, "model_error: horizon h = " + std::to_string(a->hs[a->n_h - 1]) + " > T = " + std::to_string(a->T));
    if (a->model < -1 || a->model >= c->pd.K) return set_err(c, METRPO_EINVAL, "model_error: model = " + std::to_string(a->model) + " is neither -1 nor a head below K = " + std::to_string(c->pd.K));
    {   // every index of the call fits an int: the largest is (hmax + 1) * W * ns
        const long long W = (long long)a->n * (a->t0_only ? 1 : a->T);
        if (W * (a->hs[a->n_h - 1] + 1) > 2147483647LL / std::max(c->pd.ns, c->pd.na) || (long long)a->n * (a->T + 1) > 2147483647LL / c->pd.ns)
            return set_err(c, METRPO_EINVAL, "model_error: (hmax + 1) * windows * ns must stay below 2^31");
    }
    const bool any_dbg = a->d_dbg_obs || a->d_dbg_rew || a->d_dbg_done || a->d_dbg_last_obs;
    const bool all_dbg = a->d_dbg_obs && a->d_dbg_rew && a->d_dbg_done && a->d_dbg_last_obs;
    if (any_dbg != all_dbg) return set_err(c, METRPO_EINVAL, "model_error: the d_dbg_* trajectory must be given whole or not at all");
    if (!all_dbg) {
        NEED_DYN(c);
        if (a->known_actions) { if (!a->d_As) return set_err(c, METRPO_ENULL, "model_error: known_actions needs d_As"); }
        else NEED_POL(c);
    }
    return run_model_error(c, a, (hipStream_t)stream);
}
// ---- subsampled Fisher-vector products ([rllab] ConjugateGradientOptimizer subsample_factor < 1; include/metrpo.h) ----
// T chained metrpo_step calls under supplied actions, fused where the shape allows (rollout_actions.hip)
extern "C" int32_t metrpo_rollout_actions(metrpo_ctx* c, const metrpo_rollout_actions_args* a, void* stream) {
    TraceRange trace_("metrpo:rollout_actions (open-loop replay of supplied actions)");
    if (!c) return METRPO_ENULL;
    if (!a) return set_err(c, METRPO_ENULL, "rollout_actions: args NULL");
    NEED_DYN(c);
    if (!sam_ok(a->sam_mode)) return set_err(c, METRPO_EINVAL, "sam mode is not defined");
    if (a->B < 0 || a->T < 0) return set_err(c, METRPO_EINVAL, "rollout_actions: bad B/T");
    if (a->uniform_model < -1 || a->uniform_model >= c->pd.K)
        return set_err(c, METRPO_EINVAL, "rollout_actions: uniform_model = " + std::to_string(a->uniform_model) + " is neither -1 nor a head below K = " + std::to_string(c->pd.K));
    if (a->B == 0 || a->T == 0) return METRPO_OK;
    if (!a->d_init_obs || !a->d_actions || !a->d_obs || !a->d_rew || !a->d_done) return set_err(c, METRPO_ENULL, "rollout_actions: required pointer is NULL");
    if (a->sam_mode == METRPO_SAM_EPS_RAND && a->uniform_model < 0 && !a->d_model) return set_err(c, METRPO_ENULL, "rollout_actions: eps_rand needs d_model or uniform_model");
    if (a->sam_mode == METRPO_SAM_STEP_RAND && !a->d_model_idx) return set_err(c, METRPO_ENULL, "rollout_actions: d_model_idx required for step_rand");
    if (a->sam_mode == METRPO_SAM_MODEL_MEAN_STD && !a->d_sel_noise) return set_err(c, METRPO_ENULL, "rollout_actions: d_sel_noise required for model_mean_std");
    return run_rollout_actions(c, a, (hipStream_t)stream);
}
extern "C" int32_t metrpo_last_rollout_actions_kernel(const metrpo_ctx* c) { return c ? c->last_ract_kernel : METRPO_ENULL; }

// ---- disagreement of the heads at supplied (s, a) rows (env_helpers.py:625 returned instead of consumed; disagreement.hip) ----
extern "C" int32_t metrpo_ensemble_disagreement(metrpo_ctx* c, const metrpo_disagreement_args* a, void* stream) {
    TraceRange trace_("metrpo:ensemble_disagreement (std over the heads at supplied rows)");
    if (!c) return METRPO_ENULL;
    if (!a) return set_err(c, METRPO_ENULL, "ensemble_disagreement: args NULL");
    NEED_DYN(c);
    if (a->N < 0 || a->N > 2147483647LL) return set_err(c, METRPO_EINVAL, "ensemble_disagreement: N must be in 0 ... 2^31 - 1");
    if (a->rows_per_group < 0) return set_err(c, METRPO_EINVAL, "ensemble_disagreement: rows_per_group must not be negative");
    if (a->N == 0) return METRPO_OK;
    if (!a->d_obs || !a->d_actions) return set_err(c, METRPO_ENULL, "ensemble_disagreement: d_obs and d_actions are required");
    return run_disagreement(c, a, (hipStream_t)stream);
}
extern "C" int32_t metrpo_last_disagreement_kernel(const metrpo_ctx* c) { return c ? c->last_dis_kernel : METRPO_ENULL; }

// ---- the terminal value of the four scoring calls below (sact_sum.h: TermVal): context state like theta, copied stream-ordered into d_tv = w1 | w2 | bias ----
extern "C" int32_t metrpo_set_terminal_value(metrpo_ctx* c, const float* d_w1, const float* d_w2, const float* d_bias, int32_t n_bias, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!d_w1 || !d_w2 || !d_bias) return set_err(c, METRPO_ENULL, "set_terminal_value: NULL pointer");
    if (n_bias < 1) return set_err(c, METRPO_EINVAL, "set_terminal_value: n_bias = " + std::to_string(n_bias) + " must be at least 1");
    hipStream_t st = (hipStream_t)stream;
    const size_t ns = c->pd.ns;
    // a larger n_bias than any before: the outgrown buffer is retired, not freed -- a scoring call already enqueued may still read it
    { const int rc = ws_grow(c, c->d_tv, sizeof(float) * (2 * ns + (size_t)n_bias)); if (rc) { c->tv_n_bias = 0; return rc; } }
    c->tv_n_bias = 0;                                            // a failed copy leaves none set
    HIP_TRY(c, hipMemcpyAsync(c->d_tv.p, d_w1, sizeof(float) * ns, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_tv.p + ns, d_w2, sizeof(float) * ns, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_tv.p + 2 * ns, d_bias, sizeof(float) * (size_t)n_bias, hipMemcpyDeviceToDevice, st));
    c->tv_n_bias = n_bias; c->tv_kind = 1;
    return METRPO_OK;
}
// ... its second form, a two-layer tanh net (sact_sum.h: TermVal's mlp_*): setting either form replaces the other, in the same buffer
extern "C" int32_t metrpo_set_terminal_value_mlp(metrpo_ctx* c, const float* d_params, int32_t h1, int32_t h2, const float* d_bias, int32_t n_bias, void* stream) {
    if (!c) return METRPO_ENULL;
    if (!d_params || !d_bias) return set_err(c, METRPO_ENULL, "set_terminal_value_mlp: NULL pointer");
    if (h1 < 1 || h1 > 32 || h2 < 1 || h2 > 32)
        return set_err(c, METRPO_EINVAL, "set_terminal_value_mlp: hidden widths " + std::to_string(h1) + ", " + std::to_string(h2) + " must lie in 1 ... 32");
    if (n_bias < 1) return set_err(c, METRPO_EINVAL, "set_terminal_value_mlp: n_bias = " + std::to_string(n_bias) + " must be at least 1");
    return run_set_terminal_value_mlp(c, d_params, h1, h2, d_bias, n_bias, (hipStream_t)stream);
}
extern "C" int32_t metrpo_terminal_value_kind(const metrpo_ctx* c) { return c ? (c->tv_n_bias < 1 ? 0 : c->tv_kind) : METRPO_ENULL; }
extern "C" int32_t metrpo_clear_terminal_value(metrpo_ctx* c) {
    if (!c) return METRPO_ENULL;
    c->tv_n_bias = 0;                                            // the buffer stays: enqueued calls may still read it
    return METRPO_OK;
}
extern "C" int32_t metrpo_has_terminal_value(const metrpo_ctx* c) { return c ? c->tv_n_bias : METRPO_ENULL; }
// What the four scoring entry points check alike, in this order: dynamics (need_pol: and a policy, with no update left open), B / T, S, gamma, the terminal
// value's n_bias against S (one bias for every candidate, or one per start state), chunk (0 where the call has none).  Each call's own pointers stay with it.
static int score_check(metrpo_ctx* c, const char* name, int32_t B, int32_t T, int32_t S, double gamma, int32_t chunk, bool need_pol) {
    const std::string n(name);
    NEED_DYN(c);
    if (need_pol) {
        NEED_POL(c);
        if (c->upd_pending) return set_err(c, METRPO_ESTATE, n + ": an update begun with metrpo_trpo_update_begin is still open (metrpo_trpo_update_end decides which theta stands)");
    }
    if (B < 0 || T < 0) return set_err(c, METRPO_EINVAL, n + ": bad B/T");
    if (S < 1 || B % S != 0) return set_err(c, METRPO_EINVAL, n + ": S = " + std::to_string(S) + " must be at least 1 and divide B = " + std::to_string(B));
    if (!std::isfinite(gamma)) return set_err(c, METRPO_EINVAL, n + ": gamma is not finite");
    if (c->tv_n_bias > 1 && c->tv_n_bias != S)
        return set_err(c, METRPO_EINVAL, n + ": the terminal value has n_bias = " + std::to_string(c->tv_n_bias) + ", neither 1 nor S = " + std::to_string(S));
    if (chunk < 0) return set_err(c, METRPO_EINVAL, n + ": chunk must not be negative");
    return METRPO_OK;
}

// ---- every head's discounted return of supplied action sequences (model_based_rl.py:122-141 under supplied actions; score_actions.hip) ----
extern "C" int32_t metrpo_score_actions(metrpo_ctx* c, const metrpo_score_actions_args* a, void* stream) {
    TraceRange trace_("metrpo:score_actions (per-head returns of candidate action sequences)");
    if (!c) return METRPO_ENULL;
    if (!a) return set_err(c, METRPO_ENULL, "score_actions: args NULL");
    { const int rc = score_check(c, "score_actions", a->B, a->T, a->S, a->gamma, 0, false); if (rc) return rc; }
    if (a->B == 0 || a->T == 0) return METRPO_OK;
    if (!a->d_init_obs || !a->d_actions || !a->d_ret) return set_err(c, METRPO_ENULL, "score_actions: required pointer is NULL");
    return run_score_actions(c, a, (hipStream_t)stream);
}
extern "C" int32_t metrpo_last_score_actions_kernel(const metrpo_ctx* c) { return c ? c->last_sact_kernel : METRPO_ENULL; }

// ---- gradient of every head's return with respect to the supplied action sequences (score_actions_grad.hip) ----
extern "C" int32_t metrpo_score_actions_grad(metrpo_ctx* c, const metrpo_score_actions_grad_args* a, void* stream) {
    TraceRange trace_("metrpo:score_actions_grad (per-head return gradients of candidate action sequences)");
    if (!c) return METRPO_ENULL;
    if (!a) return set_err(c, METRPO_ENULL, "score_actions_grad: args NULL");
    { const int rc = score_check(c, "score_actions_grad", a->B, a->T, a->S, a->gamma, a->chunk, false); if (rc) return rc; }
    if (a->B == 0 || a->T == 0) return METRPO_OK;
    if (!a->d_init_obs || !a->d_actions || !a->d_grad) return set_err(c, METRPO_ENULL, "score_actions_grad: required pointer is NULL");
    return run_score_actions_grad(c, a, (hipStream_t)stream);
}
extern "C" int32_t metrpo_last_score_actions_grad_kernel(const metrpo_ctx* c) { return c ? c->last_sagr_kernel : METRPO_ENULL; }

// ---- every head's discounted return of noise sequences around the policy (closed loop: a = clip(pi(s) + noise); score_policy_actions.hip) ----
extern "C" int32_t metrpo_score_policy_actions(metrpo_ctx* c, const metrpo_score_policy_actions_args* a, void* stream) {
    TraceRange trace_("metrpo:score_policy_actions (per-head returns of noise sequences around the policy)");
    if (!c) return METRPO_ENULL;
    if (!a) return set_err(c, METRPO_ENULL, "score_policy_actions: args NULL");
    { const int rc = score_check(c, "score_policy_actions", a->B, a->T, a->S, a->gamma, 0, true); if (rc) return rc; }
    if (a->B == 0 || a->T == 0) return METRPO_OK;
    if (!a->d_init_obs || !a->d_ret) return set_err(c, METRPO_ENULL, "score_policy_actions: required pointer is NULL");
    return run_score_policy_actions(c, a, (hipStream_t)stream);
}
extern "C" int32_t metrpo_last_score_policy_actions_kernel(const metrpo_ctx* c) { return c ? c->last_spol_kernel : METRPO_ENULL; }

// ---- gradient of every head's closed-loop return with respect to the noise sequences around the policy (score_policy_actions_grad.hip) ----
extern "C" int32_t metrpo_score_policy_actions_grad(metrpo_ctx* c, const metrpo_score_policy_actions_grad_args* a, void* stream) {
    TraceRange trace_("metrpo:score_policy_actions_grad (per-head return gradients of noise sequences around the policy)");
    if (!c) return METRPO_ENULL;
    if (!a) return set_err(c, METRPO_ENULL, "score_policy_actions_grad: args NULL");
    { const int rc = score_check(c, "score_policy_actions_grad", a->B, a->T, a->S, a->gamma, a->chunk, true); if (rc) return rc; }
    if (a->B == 0 || a->T == 0) return METRPO_OK;
    if (!a->d_init_obs || !a->d_grad) return set_err(c, METRPO_ENULL, "score_policy_actions_grad: required pointer is NULL");
    return run_score_policy_actions_grad(c, a, (hipStream_t)stream);
}
extern "C" int32_t metrpo_last_score_policy_actions_grad_kernel(const metrpo_ctx* c) { return c ? c->last_spag_kernel : METRPO_ENULL; }

// ---- 'svg' policy update: value gradients along recorded rollouts (svg_utils.py:12-66; svg.hip) ----
static int svg_check(metrpo_ctx* c, const metrpo_svg_args* a) {
    if (!a) return set_err(c, METRPO_ENULL, "svg: args NULL");
    NEED_DYN(c); NEED_POL(c);
    if (c->pd.env == METRPO_ENV_ANT)
        return set_err(c, METRPO_EUNSUPPORTED, "svg: Ant's cost_tf takes a fourth argument (com_ant_env.py:70); the reference's cost_tf(None, a_in, s_in) "
                                               "(svg_utils.py:123-125) raises for it, so 'svg' is not defined on Ant");
    if (a->n < 1 || a->T < 1) return set_err(c, METRPO_EINVAL, "svg: n and T must be at least 1");
    if (a->model < 0 || a->model >= c->pd.K) return set_err(c, METRPO_EINVAL, "svg: model = " + std::to_string(a->model) + " is no head below K = " + std::to_string(c->pd.K));
    if (a->path < 0 || a->path > 2) return set_err(c, METRPO_EINVAL, "svg: path must be 0 (auto), 1 (generic) or 2 (GEMM)");
    if (a->chunk < 0) return set_err(c, METRPO_EINVAL, "svg: chunk must not be negative");
    if ((long long)a->n * a->T > 2147483647LL / ((long long)c->pd.ns * (c->pd.ns + c->pd.na))) return set_err(c, METRPO_EINVAL, "svg: n * T * ns * (ns + na) must stay below 2^31");
    if (!a->d_obs || !a->d_act || !a->d_grad) return set_err(c, METRPO_ENULL, "svg: d_obs, d_act and d_grad are required");
    return METRPO_OK;
}
extern "C" int32_t metrpo_svg_grad(metrpo_ctx* c, const metrpo_svg_args* a, void* stream) {
    TraceRange trace_("metrpo:svg_grad (svg_gradient)");
    if (!c) return METRPO_ENULL;
    if (const int rc = svg_check(c, a)) return rc;
    return run_svg(c, a, 0.0, false, (hipStream_t)stream);
}
extern "C" int32_t metrpo_svg_update(metrpo_ctx* c, const metrpo_svg_args* a, double lr, void* stream) {
    TraceRange trace_("metrpo:svg_update (svg_gradient + svg_update)");
    if (!c) return METRPO_ENULL;
    if (const int rc = svg_check(c, a)) return rc;
    if (c->upd_pending) return set_err(c, METRPO_ESTATE, "svg_update: an update begun with metrpo_trpo_update_begin is still open (call metrpo_trpo_update_end)");
    if (!std::isfinite(lr)) return set_err(c, METRPO_EINVAL, "svg_update: bad learning rate");
    return run_svg(c, a, lr, true, (hipStream_t)stream);
}
extern "C" int32_t metrpo_last_svg_path(const metrpo_ctx* c) { return c ? c->last_svg_path : METRPO_ENULL; }

extern "C" int32_t metrpo_subsample_batch(metrpo_ctx* c, const metrpo_batch* b, const int32_t* d_idx, int64_t m, double inv_n_global, metrpo_batch* out,
                                          double* d_valid_count, void* stream) {
    TraceRange trace_("metrpo:subsample_batch");
    if (!c) return METRPO_ENULL;
    if (!b || !d_idx || !out || !b->d_obs) return set_err(c, METRPO_ENULL, "subsample_batch: NULL pointer");
    if (b->N <= 0 || m <= 0 || m > 2147483647LL) return set_err(c, METRPO_EINVAL, "subsample_batch: N and m must be positive (m < 2^31)");
    if (!(inv_n_global > 0.0)) return set_err(c, METRPO_EINVAL, "subsample_batch: inv_n_global must be positive");
    return launch_subsample(c, b, d_idx, m, inv_n_global, out, d_valid_count, (hipStream_t)stream);
}
extern "C" int32_t metrpo_trpo_update_fvp(metrpo_ctx* c, const metrpo_batch* b, const metrpo_batch* fvp_batch, const metrpo_trpo_params* pr,
                                          metrpo_trpo_diag* diag, double* g_out, double* dir_out, void* stream) {
    TraceRange trace_("metrpo:trpo_update_fvp (optimize_policy, subsampled Hx)");
    if (!c) return METRPO_ENULL;
    NEED_POL(c);
    if (!b || !pr) return set_err(c, METRPO_ENULL, "trpo_update_fvp: NULL pointer");
    if (pr->cg_iters < 0 || pr->max_backtracks < 1) return set_err(c, METRPO_EINVAL, "trpo_update_fvp: bad cg_iters/max_backtracks");
    if (c->upd_pending) return set_err(c, METRPO_ESTATE, "trpo_update_fvp: an update begun with metrpo_trpo_update_begin is still open (call metrpo_trpo_update_end)");
    return run_trpo_update(c, b, pr, diag, g_out, dir_out, (hipStream_t)stream, 0, 0, fvp_batch);
}
extern "C" int32_t metrpo_trpo_update_fvp_begin(metrpo_ctx* c, const metrpo_batch* b, const metrpo_batch* fvp_batch, const metrpo_trpo_params* pr,
                                                int32_t spec_trials, double* g_out, double* dir_out, void* stream) {
    TraceRange trace_("metrpo:trpo_update_fvp_begin (optimize_policy, subsampled Hx, line search decided on the device)");
    if (!c) return METRPO_ENULL;
    NEED_POL(c);
    if (!b || !pr) return set_err(c, METRPO_ENULL, "trpo_update_fvp_begin: NULL pointer");
    if (pr->cg_iters < 0 || pr->max_backtracks < 1 || spec_trials < 1) return set_err(c, METRPO_EINVAL, "trpo_update_fvp_begin: bad cg_iters / max_backtracks / spec_trials");
    if (c->upd_pending) return set_err(c, METRPO_ESTATE, "trpo_update_fvp_begin: the previous update is still open (call metrpo_trpo_update_end)");
    if (!device_line_search_ok(c, b, pr)) {
        const int rc = run_trpo_update(c, b, pr, &c->upd_diag, g_out, dir_out, (hipStream_t)stream, 0, 0, fvp_batch);
        if (rc == METRPO_OK) { c->upd_pending = 2; c->upd_spec = pr->max_backtracks; }
        return rc;
    }
    return run_trpo_update(c, b, pr, nullptr, g_out, dir_out, (hipStream_t)stream, 1, spec_trials, fvp_batch);      // (the line search of _end sees `b` alone)
}
extern "C" int32_t metrpo_trpo_update_end(metrpo_ctx* c, metrpo_trpo_diag* diag, int32_t* late_out, void* stream) {
    TraceRange trace_("metrpo:trpo_update_end");
    if (!c) return METRPO_ENULL;
    if (late_out) *late_out = 0;
    if (!c->upd_pending) return set_err(c, METRPO_ESTATE, "trpo_update_end: no update is open");
    if (c->upd_pending == 2) { if (diag) *diag = c->upd_diag; c->upd_pending = 0; return METRPO_OK; }
    metrpo_trpo_diag d = {};
    c->upd_changed_in_end = 0;
    const int rc = run_trpo_update(c, &c->upd_batch, &c->upd_params, &d, nullptr, nullptr, (hipStream_t)stream, 2, c->upd_spec);
    c->upd_pending = 0;
    if (rc == METRPO_OK) {
        if (diag) *diag = d;
        // not inferred from n_backtrack: with accept_violation and spec_trials >= max_backtracks no trial stops the search, _end still installs the last
        // trial's theta, and n_backtrack (= spec_trials - 1) is below upd_spec
        if (late_out) *late_out = c->upd_changed_in_end;
    }
    return rc;
}

// ---- BPTT policy update -----------------------------------------------------------------------
extern "C" int32_t metrpo_bptt_grad(metrpo_ctx* c, const float* init, int32_t B, int32_t T, double gamma, double* costs, double* grad,
                                    void* stream) {
    TraceRange trace_("metrpo:bptt_grad");
    if (!c) return METRPO_ENULL;
    NEED_DYN(c); NEED_POL(c);
    if (B <= 0 || T <= 0) return set_err(c, METRPO_EINVAL, "bptt_grad: B and T must be positive");
    if (!init) return set_err(c, METRPO_ENULL, "bptt_grad: NULL pointer");
    return launch_bptt_grad(c, init, B, T, gamma, costs, grad, (hipStream_t)stream);
}

extern "C" int32_t metrpo_bptt_grad_stochastic(metrpo_ctx* c, const float* init, int32_t B, int32_t T, double gamma, const float* noise,
                                               uint64_t seed, double* costs, double* grad, int32_t* n_saturates, void* stream) {
    TraceRange trace_("metrpo:bptt_grad_stochastic");
    if (!c) return METRPO_ENULL;
    NEED_DYN(c); NEED_POL(c);
    if (B <= 0 || T <= 0) return set_err(c, METRPO_EINVAL, "bptt_grad_stochastic: B and T must be positive");
    if (!init) return set_err(c, METRPO_ENULL, "bptt_grad_stochastic: NULL pointer");
    BpttNoise nz;
    nz.eps = noise; nz.log_std = c->d_theta.p + c->pd.pol.n_params; nz.n_sat = n_saturates; nz.seed = seed; nz.T = T;
    return launch_bptt_grad(c, init, B, T, gamma, costs, grad, (hipStream_t)stream, &nz);
}

extern "C" int32_t metrpo_policy_adam_reset(metrpo_ctx* c, void* stream) {
    if (!c) return METRPO_ENULL;
    return launch_policy_adam(c, nullptr, 0.0, 0.9, 0.999, 1e-8, 0.0, true, (hipStream_t)stream);
}

extern "C" int32_t metrpo_get_policy_adam(metrpo_ctx* c, float* m, float* v, int64_t* t_out, void* stream) {
    if (!c) return METRPO_EINVAL;
    if (!m || !v || !t_out) return set_err(c, METRPO_EINVAL, "get_policy_adam: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t n = sizeof(float) * (size_t)c->pd.P;
    if (!c->d_pol_adam.p) {
        HIP_TRY(c, hipMemsetAsync(m, 0, n, st));
        HIP_TRY(c, hipMemsetAsync(v, 0, n, st));
        *t_out = 0;
        return METRPO_OK;
    }
    const float* am = (const float*)c->d_pol_adam.p;
    HIP_TRY(c, hipMemcpyAsync(m, am, n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(v, am + c->pd.P, n, hipMemcpyDeviceToDevice, st));
    *t_out = c->pol_adam_t;
    return METRPO_OK;
}

extern "C" int32_t metrpo_set_policy_adam(metrpo_ctx* c, const float* m, const float* v, int64_t t, void* stream) {
    if (!c) return METRPO_EINVAL;
    if (!m || !v) return set_err(c, METRPO_EINVAL, "set_policy_adam: NULL pointer");
    if (t < 0 || t > INT32_MAX) return set_err(c, METRPO_EINVAL, "set_policy_adam: t outside [0, 2^31)");
    const int rc = ensure_policy_adam(c);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = sizeof(float) * (size_t)c->pd.P;
    float* am = (float*)c->d_pol_adam.p;
    HIP_TRY(c, hipMemcpyAsync(am, m, n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(am + c->pd.P, v, n, hipMemcpyDeviceToDevice, st));
    c->pol_adam_t = (int)t;
    return METRPO_OK;
}

extern "C" int32_t metrpo_policy_adam_step(metrpo_ctx* c, const double* grad, double lr, double beta1, double beta2, double eps,
                                           double clip_val, void* stream) {
    if (!c) return METRPO_ENULL;
    NEED_POL(c);
    if (!grad) return set_err(c, METRPO_ENULL, "policy_adam_step: NULL pointer");
    if (!(lr >= 0.0)) return set_err(c, METRPO_EINVAL, "policy_adam_step: bad learning rate");
    return launch_policy_adam(c, grad, lr, beta1, beta2, eps, clip_val, false, (hipStream_t)stream);
}

// test hook (not in metrpo.h): 0 = generic sweep / validation kernels, 1 = fastest path the shape has.  Returns the path in use:
// 1 fused MFMA sweeps (bptt_mfma.hip), 2 GEMM-path sweeps (det_gemm.hip), 0 generic.
extern "C" int32_t metrpo_set_det_path(metrpo_ctx* c, int32_t use_mfma) {
    if (!c) return METRPO_ENULL;
    c->det_cfg = use_mfma ? det_mfma_select(c) : -1;
    c->det_gemm = (use_mfma && det_gemm_applicable(c)) ? 1 : 0;
    return c->det_cfg >= 0 ? 1 : (c->det_gemm ? 2 : 0);
}
