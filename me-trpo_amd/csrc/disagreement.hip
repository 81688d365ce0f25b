// metrpo_ensemble_disagreement (include/metrpo.h): the spread of the K heads' next states at N supplied (s, a) rows -- np.std(next_possible_observations,
// axis=0), env_helpers.py:625, returned instead of consumed.  One step of the model on N independent rows: no chain of dependent steps.
//
// Fused kernel (k_disagreement): k_rollout_actions' ALL-heads step (rollout_actions.hip) with T = 1, turned into a loop over tiles.  From
// dyn_tile_step.h it takes the wave's head (DynWaveHead: set-up and step) and the K-head exchange with its head-order mean (HeadExchange).  The double
// buffer of input rows is its own (load_tile / commit below), not that header's ActTile: a tile brings state rows and validity bytes with its actions,
// rows are zeroed by the row's flag in LDS and not by the row count alone, and the walk is over 64-bit tile indices, not the steps of one tile.
//   * wave k of the workgroup owns head k (K <= 8 waves) on the shared head of dyn_head_mfma.h; its weight fragments are register-resident (swimmer 92,
//     Ant 132 registers).  k_rollout_actions amortises them over the T steps of one tile; here a workgroup STRIDES over the 16-row tiles with the
//     weights resident, and the grid is the workgroups the CUs this process reaches can hold (probe.hip's census), not one workgroup per tile.
//   * biases, the tile's state and clipped actions live in the wave's own LDS (every wave loads the tile: the K copies come out of the cache); the K
//     next states of a tile meet in LDS behind ONE barrier per tile (exchange area double-buffered), and every output is formed once from there: each
//     wave stores its own head's d_next_all rows, ONE wave -- the waves that have a SIMD to themselves take turns -- forms mean, std, score, maxdev and
//     rew_std.  Mean in head order k = 0 .. K-1 divided by K (as metrpo_step), variance two-pass by fmaf in head order.
//   * the NEXT tile's state and action rows (and validity bytes) are loaded at the top of a tile and read behind that tile's matrix instructions into the
//     other of two LDS buffers -- IN FRONT of the tile's stores (k_rollout_actions: the vector-memory counter is in order, so the wait for a load is
//     also a wait for every older store; placed there it meets only the stores of the tile before).
//   * edge tile (N % 16 != 0) and skipped rows (d_valid): zero state and zero action in LDS.  Rows >= N are never read from or written to memory (the
//     index is clamped into the tile's block); a skipped row's loaded values are dropped by a select and zeros are stored for it.
//   * d_rew_std: env_cost (env_model.h, the function k_rollout_actions calls) on every head's own LDS row, combined like the states.
//
// Generic path (every other shape): metrpo_step's kernel once (one_model, its d_next_all into the caller's buffer or a workspace; s_next, reward and done
// go to the workspace and are dropped), then k_dis_reduce, one thread per row.
//
// d_sums: k_dis_sums, a second small launch on d_score / d_valid, one workgroup of a fixed shape per group adding in a fixed order.
#include "dyn_tile_step.h"

struct DisK {
    long long N;
    const float* obs; const float* act; const uint8_t* valid;
    float* score; float* maxdev; float* sd; float* mean; float* next_all; float* rew_std;
};

// per-wave LDS (floats): ST[2] | ACT[2] | ROK[2] (1.0f: the row is inside N and not skipped) | dynamics biases
template <int ENV> struct DisLds {
    using C = Cfg<ENV, 64, 32>;
    static constexpr int ST_SZ = 16 * C::NS, ACT_SZ = al4(16 * C::NA);
    static constexpr int ST = 0, ACT = 2 * ST_SZ, ROK = ACT + 2 * ACT_SZ, BD0 = ROK + 32, BD1 = BD0 + C::BD, BD2 = BD1 + C::BD, W_SZ = BD2 + C::NSP;
};

template <int ENV>
__global__ void __launch_bounds__(512) k_disagreement(DisK r, int K, const float* __restrict__ dynp, const float* __restrict__ norm) {
    using C = Cfg<ENV, 64, 32>;
    using L = DisLds<ENV>;
    constexpr int NS = C::NS, NA = C::NA, NSP = C::NSP;
    constexpr int NLD = cdiv(16 * NA, 64), NST = cdiv(16 * NS, 64);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = lane & 15, q = lane >> 4;
    float* W = lds + wave * L::W_SZ;
    const HeadExchange<C> xch = {lds + K * L::W_SZ, K};
    const long long ntiles = (r.N + 15) >> 4;
    long long tile = blockIdx.x;                                 // the grid never exceeds the tiles
    if (tile >= ntiles) return;

    DynWaveHead<C> head;
    head.load(dynp + (size_t)wave * C::PD, norm, W + L::BD0, W + L::BD1, W + L::BD2, lane);

    // a tile's rows as every lane loads them: straight-line loads, the index clamped into the tile's block (nothing out of bounds, no masked branch:
    // the compiler waits for them where they are used).  Without d_valid the byte comes from d_obs and is dropped.
    float s_nx[NST], a_nx[NLD];
    unsigned v_nx;
    auto load_tile = [&](long long tl) {
        const long long b0 = tl * 16;
        const int nr = (int)min(16LL, r.N - b0);
        const float* __restrict__ sp = r.obs + b0 * NS;
        const float* __restrict__ ap = r.act + b0 * NA;
#pragma unroll
        for (int j = 0; j < NST; ++j) s_nx[j] = sp[min(lane + 64 * j, nr * NS - 1)];
#pragma unroll
        for (int j = 0; j < NLD; ++j) a_nx[j] = ap[min(lane + 64 * j, nr * NA - 1)];
        const uint8_t* vp = r.valid ? r.valid + b0 + min(e, nr - 1) : (const uint8_t*)sp;
        const unsigned vb = *vp;
        v_nx = r.valid ? vb : 1u;
    };
    // the loaded rows become buffer `buf`: skipped rows and rows >= N are zero state and zero action; np.clip(actions, *bounds), env_helpers.py:599
    auto commit = [&](int buf, long long tl) {
        const int nr = (int)min(16LL, r.N - tl * 16);
        float* ROKb = W + L::ROK + 16 * buf;
        float* STb = W + L::ST + buf * L::ST_SZ;
        float* ACTb = W + L::ACT + buf * L::ACT_SZ;
        if (lane < 16) ROKb[lane] = (lane < nr && v_nx != 0u) ? 1.0f : 0.0f;
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int i = lane + 64 * j;
            if (i < 16 * NS) STb[i] = (ROKb[i / NS] != 0.0f) ? s_nx[j] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = lane + 64 * j;
            if (i < 16 * NA) ACTb[i] = (ROKb[i / NA] != 0.0f) ? fminf(fmaxf(a_nx[j], -1.0f), 1.0f) : 0.0f;
        }
        wave_lds_sync();
    };

    load_tile(tile);
    commit(0, tile);
    loop_invariant_loads_done();

    // The wave that forms a tile's outputs.  The barrier keeps the waves in step, so whatever one wave does on top of its head is on every tile's critical
    // path -- unless that wave has a SIMD to itself.  A workgroup's waves go to the CU's four SIMDs cyclically, so waves w and w + 4 share one: at K = 5 .. 7
    // the waves K - 4 .. 3 are alone on theirs and idle while a shared SIMD evaluates its second head; they take turns.  K <= 4 and K = 8: all waves do.
    const int t_lo = (K > 4 && K < 8) ? K - 4 : 0, t_hi = (K > 4 && K < 8) ? 4 : K;
    int turn = t_lo;
    for (int it = 0;; ++it) {
        const int par = it & 1;
        // ---- the rows of the workgroup's next tile (the last tile reads its own rows again: no branch, nothing out of bounds), issued now and read
        //      behind the matrix instructions, IN FRONT of this tile's stores ----
        const long long tnext = tile + gridDim.x;
        const bool more = tnext < ntiles;
        const long long tload = more ? tnext : tile;
        load_tile(tload);
        const float* ST = W + L::ST + par * L::ST_SZ;
        const float* ACT = W + L::ACT + par * L::ACT_SZ;
        const float* ROKc = W + L::ROK + 16 * par;
        f32x4 nx[C::OUT_CB];
        head.step(nx, ST, NS, ACT, e);
        xch.put(par, wave, e, q, nx);
        __syncthreads();                                                         // all K heads of this tile are in NXT[par]
        // ---- the prefetched rows become the next tile's.  The wait for them is the loop's only vmcnt wait; it also covers the stores of the tile before
        //      -- a whole tile of matrix work old -- and none of this tile's, which follow below (the empty statements take the loaded values on EVERY
        //      path: dyn_tile_step.h, ActTile::commit) ----
#pragma unroll
        for (int j = 0; j < NST; ++j) asm volatile("" ::"v"(s_nx[j]));
#pragma unroll
        for (int j = 0; j < NLD; ++j) asm volatile("" ::"v"(a_nx[j]));
        asm volatile("" ::"v"(v_nx));
        commit(par ^ 1, tload);

        const long long b0 = tile * 16;
        const int nrows = (int)min(16LL, r.N - b0);
        const long long row = b0 + e;
        const bool in_n = e < nrows;
        const bool ok = ROKc[e] != 0.0f;
        if (r.next_all != nullptr && in_n) {                                     // this wave's head, metrpo_step's layout [K][N][ns]
            float* __restrict__ dst = r.next_all + ((size_t)wave * r.N + row) * NS;
#pragma unroll
            for (int cb = 0; cb < C::OUT_CB; ++cb)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int dim = 16 * cb + 4 * q + rr;
                    if (dim < NS) dst[dim] = ok ? nx[cb][rr] : 0.0f;
                }
        }
        if (wave == turn) {
            // ---- get_next_observation's mean and std (env_helpers.py:621-625) over the K heads, from LDS; lane (e, q) holds dims 16 cb + 4 q + r of row e.
            //      The padded dims are exact zeros in every head (zero weights, bias, normaliser and state) and add exact zeros ----
            const float* nxt_all = xch.heads(par);
            const float fK = (float)K;
            float ssq = 0.0f;
#pragma unroll
            for (int cb = 0; cb < C::OUT_CB; ++cb) {
                const int off = e * NSP + 16 * cb + 4 * q;
                const f32x4 m = xch.mean(nxt_all, K, off);
                f32x4 var = {0.f, 0.f, 0.f, 0.f};
                for (int k = 0; k < K; ++k) {
                    const f32x4 d = xch.head(nxt_all, k, off) - m;
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) var[rr] = fmaf(d[rr], d[rr], var[rr]);
                }
                var = var / fK;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int dim = 16 * cb + 4 * q + rr;
                    ssq += var[rr];
                    if (dim < NS && in_n) {
                        if (r.mean != nullptr) r.mean[(size_t)row * NS + dim] = ok ? m[rr] : 0.0f;
                        if (r.sd != nullptr) r.sd[(size_t)row * NS + dim] = ok ? sqrtf(var[rr]) : 0.0f;
                    }
                }
            }
            const float score = sqrtf(xor_sum(ssq));
            float maxdev = 0.0f;
            if (r.maxdev != nullptr) {
                for (int k = 0; k < K; ++k) {
                    float dk = 0.0f;
#pragma unroll
                    for (int cb = 0; cb < C::OUT_CB; ++cb) {
                        const int off = e * NSP + 16 * cb + 4 * q;
                        const f32x4 d = xch.head(nxt_all, k, off) - xch.mean(nxt_all, K, off);
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) dk = fmaf(d[rr], d[rr], dk);
                    }
                    maxdev = fmaxf(maxdev, sqrtf(xor_sum(dk)));
                }
            }
            float rstd = 0.0f;
            if (r.rew_std != nullptr) {                                          // r_k = -cost_np_vec(s, clip(a), s'_k) (:601), every head's own next state
                float rs = 0.0f;
                for (int k = 0; k < K; ++k) rs += -env_cost(ENV, NS, NA, EnvVec{nxt_all + ((size_t)k * 16 + e) * NSP, 1}, EnvVec{ACT + e * NA, 1});
                const float rm = rs / fK;
                float rv = 0.0f;
                for (int k = 0; k < K; ++k) {
                    const float d = -env_cost(ENV, NS, NA, EnvVec{nxt_all + ((size_t)k * 16 + e) * NSP, 1}, EnvVec{ACT + e * NA, 1}) - rm;
                    rv = fmaf(d, d, rv);
                }
                rstd = sqrtf(rv / fK);
            }
            if (q == 0 && in_n) {
                if (r.score != nullptr) r.score[row] = ok ? score : 0.0f;
                if (r.maxdev != nullptr) r.maxdev[row] = ok ? maxdev : 0.0f;
                if (r.rew_std != nullptr) r.rew_std[row] = ok ? rstd : 0.0f;
            }
        }
        if (!more) break;
        tile = tnext;
        turn = (turn + 1 == t_hi) ? t_lo : turn + 1;
    }
}

// -------------------------------------------------------------------------------------------------
// Generic path's reduction: one thread per row over metrpo_step's d_next_all [K][N][ns]; the arithmetic of the fused kernel's output wave with the
// dims summed in index order.  U: the thread's clipped action in LDS (env_cost reads it through a pointer).
__global__ void __launch_bounds__(256) k_dis_reduce(int env, int ns, int na, int K, DisK r, int zero_next_all) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= r.N) return;
    const size_t N = (size_t)r.N;
    if (r.valid != nullptr && r.valid[n] == 0) {
        if (r.score != nullptr) r.score[n] = 0.0f;
        if (r.maxdev != nullptr) r.maxdev[n] = 0.0f;
        if (r.rew_std != nullptr) r.rew_std[n] = 0.0f;
        for (int i = 0; i < ns; ++i) {
            if (r.sd != nullptr) r.sd[n * ns + i] = 0.0f;
            if (r.mean != nullptr) r.mean[n * ns + i] = 0.0f;
            if (zero_next_all) for (int k = 0; k < K; ++k) r.next_all[((size_t)k * N + n) * ns + i] = 0.0f;
        }
        return;
    }
    const float* __restrict__ xa = r.next_all;
    const float fK = (float)K;
    auto mean_of = [&](int i) {
        float m = 0.0f;
        for (int k = 0; k < K; ++k) m += xa[((size_t)k * N + n) * ns + i];                                       // head order, as metrpo_step
        return m / fK;
    };
    float ssq = 0.0f;
    for (int i = 0; i < ns; ++i) {
        const float m = mean_of(i);
        float var = 0.0f;
        for (int k = 0; k < K; ++k) { const float d = xa[((size_t)k * N + n) * ns + i] - m; var = fmaf(d, d, var); }
        var = var / fK;
        ssq += var;
        if (r.mean != nullptr) r.mean[n * ns + i] = m;
        if (r.sd != nullptr) r.sd[n * ns + i] = sqrtf(var);
    }
    if (r.score != nullptr) r.score[n] = sqrtf(ssq);
    if (r.maxdev != nullptr) {
        float maxdev = 0.0f;
        for (int k = 0; k < K; ++k) {
            float dk = 0.0f;
            for (int i = 0; i < ns; ++i) { const float d = xa[((size_t)k * N + n) * ns + i] - mean_of(i); dk = fmaf(d, d, dk); }
            maxdev = fmaxf(maxdev, sqrtf(dk));
        }
        r.maxdev[n] = maxdev;
    }
    if (r.rew_std != nullptr) {
        float* U = lds + (size_t)threadIdx.x * na;
        for (int d = 0; d < na; ++d) U[d] = fminf(fmaxf(r.act[n * na + d], -1.0f), 1.0f);                        // env_helpers.py:599
        float rs = 0.0f;
        for (int k = 0; k < K; ++k) rs += -env_cost(env, ns, na, EnvVec{xa + ((size_t)k * N + n) * ns, 1}, EnvVec{U, 1});
        const float rm = rs / fK;
        float rv = 0.0f;
        for (int k = 0; k < K; ++k) { const float d = -env_cost(env, ns, na, EnvVec{xa + ((size_t)k * N + n) * ns, 1}, EnvVec{U, 1}) - rm; rv = fmaf(d, d, rv); }
        r.rew_std[n] = sqrtf(rv / fK);
    }
}

// d_sums [G][4]: valid rows, sum score, sum score^2, max score of group g = rows [g * rpg, min(N, (g + 1) * rpg)) (rpg = 0: all rows).  One workgroup per
// group, thread t takes rows t, t + blockDim, ... in float64, then block_sum's fixed tree: a function of the inputs and of the block size alone, and the
// block size is a function of the group size (launch_dis_sums).
__device__ __forceinline__ double block_max(double v, double* sh /* >= 16 doubles */) {
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(v, off, WAVE); v = o > v ? o : v; }
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) sh[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; ++i) r = sh[i] > r ? sh[i] : r;
    }
    return r;
}
__global__ void __launch_bounds__(1024) k_dis_sums(const float* __restrict__ score, const uint8_t* __restrict__ valid, long long N, long long rpg, double* __restrict__ sums) {
    __shared__ double sh[16];
    const long long lo = rpg > 0 ? (long long)blockIdx.x * rpg : 0, hi = rpg > 0 ? min(N, lo + rpg) : N;
    double cnt = 0.0, s1 = 0.0, s2 = 0.0, mx = 0.0;
    for (long long n = lo + threadIdx.x; n < hi; n += blockDim.x) {
        if (valid != nullptr && valid[n] == 0) continue;
        const double v = (double)score[n];
        cnt += 1.0; s1 += v; s2 += v * v; mx = v > mx ? v : mx;
    }
    cnt = block_sum(cnt, sh); s1 = block_sum(s1, sh); s2 = block_sum(s2, sh); mx = block_max(mx, sh);
    if (threadIdx.x == 0) { double* o = sums + 4 * (size_t)blockIdx.x; o[0] = cnt; o[1] = s1; o[2] = s2; o[3] = mx; }
}

static int launch_dis_sums(metrpo_ctx* c, const float* score, const metrpo_disagreement_args* a, hipStream_t st) {
    const long long rpg = a->rows_per_group, per = rpg > 0 ? std::min<long long>(rpg, a->N) : a->N;
    const long long G = rpg > 0 ? (a->N + rpg - 1) / rpg : 1;
    const int bs = per > 16384 ? 1024 : 256;                     // fixed by the group size
    hipLaunchKernelGGL(k_dis_sums, dim3((unsigned)G), dim3(bs), 0, st, score, a->d_valid, (long long)a->N, rpg, a->d_sums);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

// -------------------------------------------------------------------------------------------------
typedef void (*dis_kernel_t)(DisK, int, const float*, const float*);
struct DisEntry { int env; dis_kernel_t kern; int w_sz, nsp; };
#define DENTRY(ENVID) {ENVID, k_disagreement<ENVID>, DisLds<ENVID>::W_SZ, Cfg<ENVID, 64, 32>::NSP}
static const DisEntry kDis[] = {FUSED_HEAD_ENVS(DENTRY)};

static int launch_dis_fused(metrpo_ctx* c, const DisEntry& en, bool padded, const DisK& r, hipStream_t st) {
    const int K = c->pd.K;
    const float* dyn;
    { const int rc = fused_head_dyn(c, padded, st, &dyn); if (rc) return rc; }
    const size_t sh = sizeof(float) * ((size_t)K * en.w_sz + head_exchange_floats(K, en.nsp));
    { const int rc = allow_dynamic_lds(c, (const void*)en.kern, sh); if (rc) return rc; }
    if (c->dis_per_cu <= 0) {                                    // workgroups a CU holds (registers, LDS): asked once, the shape is the context's
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)en.kern, K * 64, sh) != hipSuccess) { (void)hipGetLastError(); per_cu = 1; }
        c->dis_per_cu = std::max(1, std::min(per_cu, 8));
    }
    const long long ntiles = (r.N + 15) / 16;
    const long long grid = std::min<long long>(ntiles, (long long)c->dis_per_cu * sched_cus(c, st));
    hipLaunchKernelGGL(en.kern, dim3((unsigned)grid), dim3(K * 64), sh, st, r, K, dyn, c->d_norm.p);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

int run_disagreement(metrpo_ctx* c, const metrpo_disagreement_args* a, hipStream_t st) {
    const ProblemDesc& pd = c->pd;
    const size_t N = (size_t)a->N, ns = pd.ns, K = pd.K;
    bool padded = false;
    const DisEntry* en = a->force_generic ? nullptr : fused_head_entry(kDis, c, 8, &padded);      // a wave per head
    // ---- workspace: scores (only d_sums asked for) | generic: every head's next state (unless the caller takes it) | s_next | reward | done ----
    const bool ws_score = a->d_score == nullptr && a->d_sums != nullptr;
    const bool ws_all = en == nullptr && a->d_next_all == nullptr;
    size_t off = 0;
    const size_t o_score = off; off += ws_score ? N : 0;
    const size_t o_all = off;   off += ws_all ? K * N * ns : 0;
    const size_t o_next = off;  off += en == nullptr ? N * ns : 0;
    const size_t o_rew = off;   off += en == nullptr ? N : 0;
    const size_t o_done = off;  off += en == nullptr ? (N + 3) / 4 : 0;
    if (off > 0) { const int rc = ws_grow(c, c->d_dis, sizeof(float) * off); if (rc) return rc; }
    float* ws = (float*)c->d_dis.p;
    DisK r = {};
    r.N = a->N; r.obs = a->d_obs; r.act = a->d_actions; r.valid = a->d_valid;
    r.score = ws_score ? ws + o_score : a->d_score;
    r.maxdev = a->d_maxdev; r.sd = a->d_std; r.mean = a->d_mean; r.next_all = a->d_next_all; r.rew_std = a->d_rew_std;
    if (en != nullptr) {
        const int rc = launch_dis_fused(c, *en, padded, r, st);
        if (rc) return rc;
    } else {
        if (ws_all) r.next_all = ws + o_all;
        int rc = launch_step(c, a->d_obs, a->d_actions, (int)a->N, METRPO_SAM_ONE_MODEL, nullptr, nullptr, ws + o_next, ws + o_rew, (uint8_t*)(ws + o_done), r.next_all, st);
        if (rc) return rc;
        const int bs = 256;
        const size_t sh = sizeof(float) * (size_t)bs * pd.na;
        hipLaunchKernelGGL(k_dis_reduce, dim3((unsigned)((N + bs - 1) / bs)), dim3(bs), sh, st, pd.env, pd.ns, pd.na, pd.K, r, ws_all ? 0 : 1);
        HIP_TRY(c, hipGetLastError());
    }
    if (a->d_sums != nullptr) { const int rc = launch_dis_sums(c, r.score, a, st); if (rc) return rc; }
    c->last_dis_kernel = en != nullptr ? 1 : 0;
    return METRPO_OK;
}
