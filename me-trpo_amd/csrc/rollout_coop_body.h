// Body of the cooperative rollout kernels (rollout_coop_kernel.h): the tile-step of both forms, every phase written once.
// NOT a header of its own: it is included INSIDE a function -- k_rollout_coop (the 4-wave form) and coop_split_group (a head group of the 8-wave form) --
// which supplies   ENV, K, ONE, DRAWS, G (constants)   and   r, dynp, theta, norm, lds, w (w = hidden col-block = SIMD of the wave).
// G = -1: the four waves own all K heads; G = 0 / 1: head group of the 8-wave form (ONE is true there).
// Why text and not a called function: the register assignment of these kernels moves with how they are factored.  The 4-wave kernel turned into
// a thin __global__ entry over an inlined body, with not one statement changed, took k_rollout_coop<half_cheetah, 8, true, false> from 184 to 424 bytes of
// scratch and <ant, 8, true, true> from 512 to 764 (profiles/r17_coop_one_body.txt); included, it is the function it was.
// What the forms disagree on is the role block below and the three items under COOP_SPLIT_FORM; nothing else names a form.
// Three things stay in two statements, side by side, chosen by the includer's COOP_SPLIT_FORM (0: k_rollout_coop, 1: coop_split_group).  Written once they
// compute the same, but each moved the register assignment of one form away from what it was (profiles/r17_coop_one_body.txt, section 1):
//   - the loops over output col-blocks.  The head-split form exists for OUT_CB == 1 only and is written without them: a one-trip loop is unrolled
//     late, and until then the arrays it indexes (xc, nx, wd2, po) are memory, not values (k_rollout_coop_split<snake, 4, false> 56 -> 68 bytes of scratch);
//   - the piece deal below, which the head-split form (always ONE) states unconditionally (same kernels);
//   - the singleton-job flags pol / rngw / reww: the 4-wave form compares the wave index where it uses them, the head-split form once (evaluated once
//     they moved the scalar spills of the 4-wave kernels, and k_rollout_coop<swimmer, 5, false, false> ran 1 % slower).
#if COOP_SPLIT_FORM
#define COOP_FOR_CB if (const int cb = 0; true)
#else
#define COOP_FOR_CB _Pragma("unroll") for (int cb = 0; cb < OUT_CB; ++cb)
#endif
    static_assert(std::is_same<std::remove_cv_t<decltype(ENV)>, int>::value && std::is_same<std::remove_cv_t<decltype(K)>, int>::value && ENV >= 0 && K >= 1 &&
                  std::is_same<std::remove_cv_t<decltype(ONE)>, bool>::value && std::is_same<std::remove_cv_t<decltype(DRAWS)>, bool>::value && (ONE || !ONE) && (DRAWS || !DRAWS) &&
                  std::is_same<std::remove_cv_t<decltype(G)>, int>::value && (COOP_SPLIT_FORM ? G == 0 || G == 1 : G == -1), "includer: constants ENV, K, ONE, DRAWS, and G matching COOP_SPLIT_FORM");
    static_assert(std::is_same<std::remove_cv_t<std::remove_reference_t<decltype(r)>>, RolloutK>::value && std::is_same<std::remove_cv_t<decltype(w)>, int>::value &&
                  std::is_convertible<decltype(dynp), const float*>::value && std::is_convertible<decltype(theta), const float*>::value &&
                  std::is_convertible<decltype(norm), const float*>::value && std::is_convertible<decltype(lds), float*>::value, "includer: RolloutK r, const float* dynp / theta / norm, float* lds, int w");
    // ---------------- role block ------------------------------------------------------------------------------------------------
    constexpr int NWV = (G < 0) ? 4 : 8;                                // waves of the workgroup
    constexpr int K0 = (G == 1) ? K / 2 : 0, KG = (G < 0) ? K : (G == 0) ? K / 2 : K - K / 2;     // heads K0 .. K0 + KG - 1 are this wave's
    // Layer 0 of col-block 0 is NOT computed by wave 0 (the policy wave, whose step is the longest).  4 waves: waves 1, 2, 3 take it for heads
    // {0,1}, {2,3}, {4,..} on top of their own col-block -- they idle while the policy is evaluated anyway; the MFMAs are issued on every one of
    // them (zero weights beyond head K - 1), only the H0 store is guarded.  8 waves: wave 4 alone (`helper`) takes it for group 0's heads.
    constexpr int XH = (G < 0) ? (K + 2) / 3 : (G == 1) ? K / 2 : 0;    // heads of col-block 0 per helper wave
    constexpr bool SOLO = (G != 1);                                     // the group with the singleton jobs: policy, draws, reward
    using L = Coop<ENV, K, NWV>;
    using C = typename L::C;
    constexpr int NS = C::NS, NA = C::NA, NSP = C::NSP, DH = 64, PH = 32, OUT_CB = C::OUT_CB;
    static_assert(G < 0 || (ONE && OUT_CB == 1 && K >= 2 && K <= 5), "head-split form: one workgroup per CU, one output col-block, 2 ... 5 heads");
    const int tid = threadIdx.x, lane = tid & 63, wave = (G == 1) ? 4 + w : w;
    const int e = lane & 15, q = lane >> 4;
    // singleton jobs: pol() the policy and the obs / act / mean stores, rngw() the next step's draws, reww() the reward stores
#if COOP_SPLIT_FORM
    const bool pol_v = SOLO && w == 0, rngw_v = SOLO && w == 1, reww_v = SOLO && w == 2;
    const auto pol = [=] { return pol_v; }; const auto rngw = [=] { return rngw_v; }; const auto reww = [=] { return reww_v; };
#else
    const auto pol = [=] { return w == 0; }; const auto rngw = [=] { return w == 1; }; const auto reww = [=] { return w == 2; };
#endif
    const bool helper = (G < 0) ? w >= 1 : (G == 1 && w == 0);                         // holds col-block-0 layer-0 fragments of XH heads
    const int hx_base = (G < 0) ? XH * (w - 1) : 0;                                    // hx_base + j: the head whose col-block-0 layer 0 is the helper's j-th
    if (r.stop != nullptr && *r.stop != 0) return;           // the sampling loop already ended (metrpo_sampler_progress)
    // ---------------- which (tile, step range) pieces this workgroup runs ------------------------------------------------------
    // !ONE: workgroup = tile, all T steps.  ONE: the launch has at most one workgroup per CU and the tiles x T tile-steps are dealt
    // out evenly in tile-major order (wrap-around rule): workgroup i owns the linear range [i Q, (i+1) Q), i.e. the END of tile
    // c_first (steps s_first..T-1), whole tiles, and the BEGINNING of tile c_last (steps 0..e_last-1).  It runs the beginning piece
    // first, then the whole tiles, then the ending piece, whose state it takes over from workgroup i-1 through a hand-over slot in
    // HBM (flag = launch epoch, agent-scope release / acquire).  Workgroup i-1 runs that tile's beginning before anything else and
    // waits for nobody first, so with in-order dispatch the wait cannot deadlock; Q >= T keeps a tile on at most two workgroups.
#if COOP_SPLIT_FORM
    const long long total = (long long)((r.B + 15) / 16) * r.T;
    const long long Q = (total + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * Q, hi = (lo + Q < total) ? lo + Q : total;
    if (lo >= hi) return;
    const int c_first = (int)(lo / r.T), s_first = (int)(lo % r.T), c_last = (int)((hi - 1) / r.T), e_last = (int)((hi - 1) % r.T) + 1;
#else
    int c_first = blockIdx.x, c_last = blockIdx.x, s_first = 0, e_last = r.T;
    if (ONE) {
        const long long total = (long long)((r.B + 15) / 16) * r.T;
        const long long Q = (total + gridDim.x - 1) / gridDim.x;
        const long long lo = (long long)blockIdx.x * Q, hi = (lo + Q < total) ? lo + Q : total;
        if (lo >= hi) return;
        c_first = (int)(lo / r.T); s_first = (int)(lo % r.T); c_last = (int)((hi - 1) / r.T); e_last = (int)((hi - 1) % r.T) + 1;
    }
#endif
    const int npc = c_last - c_first + 1;
    int b0 = 0, b = 0;
    bool active = false;
    uint64_t genv = 0;
    float* ST = lds + wave * L::WV;  float* NX = ST + 16 * NSP;
    float* ACT = lds + 16 * NSP + 16 * NS;                                         // clipped actions of the tile: written by wave 0 (the policy wave), read by all

    float* BD0 = lds + L::O_BD0; float* BD1 = lds + L::O_BD1; float* BD2 = lds + L::O_BD2;
    float* BP0 = lds + L::O_BP0; float* BP1 = lds + L::O_BP1; float* BP2 = lds + L::O_BP2;
    float* PW = lds + L::O_PW; float* H0 = lds + L::O_H0; float* PART = lds + L::O_PART;
    float* AK = lds + L::O_AK;                                          // [action | mean][16 envs][na], staged for wave 0's coalesced stores
    float* RNGB = lds + L::O_RNG;                                       // [2 parities][16 envs][dstep (4 x u32) | z of q-lane 0..3 (4 floats each)]

    // ---------------- one-time: dynamics fragments of the wave's heads -> registers ----------------------------------
    float wd0[KG][C::NIN_KS], wd1[KG][16], wd2[KG][4][OUT_CB];
#pragma unroll
    for (int k = 0; k < KG; ++k) {
        const float* __restrict__ pk = dynp + (size_t)(K0 + k) * C::PD;
#pragma unroll
        for (int s = 0; s < C::NIN_KS; ++s) { const int i = 4 * s + q; wd0[k][s] = (i < C::NIN) ? pk[C::dW0 + i * DH + 16 * w + e] : 0.0f; }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) { const int i = chained_in(kk, q); wd1[k][kk] = pk[C::dW1 + i * DH + 16 * w + e]; }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
            COOP_FOR_CB { const int i = 16 * w + 4 * q + rr, o = 16 * cb + e; wd2[k][rr][cb] = (o < NS) ? pk[C::dW2 + i * NS + o] : 0.0f; }
    }
    float wx0[(ONE && XH > 0) ? XH : 1][C::NIN_KS];                    // the helper's col-block-0 fragments: registers when the workgroup owns the CU, else an LDS image (no room)
    float* WXL = lds + L::O_WX + ((G < 0 && helper) ? w - 1 : 0) * XH * C::NIN_KS * 64 + lane;
#pragma unroll
    for (int j = 0; j < XH; ++j) {
        const int hx = hx_base + j;
        const float* __restrict__ pk = dynp + (size_t)((G < 0 && !(helper && hx < K)) ? 0 : hx) * C::PD;       // 4 waves: a wave without a j-th head reads head 0 (and keeps zeros)
#pragma unroll
        for (int s = 0; s < C::NIN_KS; ++s) {
            const int i = 4 * s + q;
            const float wv = (i < C::NIN && helper && hx < K) ? pk[C::dW0 + i * DH + e] : 0.0f;
            if (ONE) wx0[j][s] = wv; else if (helper) WXL[(j * C::NIN_KS + s) * 64] = wv;
        }
    }
    // shared images: biases and policy fragments (each element written by exactly one thread)
    for (int i = tid; i < K * 64; i += 64 * NWV) { const int k = i >> 6, u = i & 63; BD0[i] = dynp[(size_t)k * C::PD + C::db0 + u]; BD1[i] = dynp[(size_t)k * C::PD + C::db1 + u]; }
    for (int i = tid; i < K * NSP; i += 64 * NWV) { const int k = i / NSP, u = i % NSP; BD2[i] = (u < NS) ? dynp[(size_t)k * C::PD + C::db2 + u] : 0.0f; }
    if (tid < 32) { BP0[tid] = theta[C::pb0 + tid]; BP1[tid] = theta[C::pb1 + tid]; }
    if (tid < 16) BP2[tid] = (tid < NA) ? theta[C::pb2 + tid] : 0.0f;
    for (int i = tid; i < L::NPF * 64; i += 64 * NWV) {
        const int f = i >> 6, ln = i & 63, ee = ln & 15, qq = ln >> 4;
        float wv = 0.0f;
        if (f < L::P0KS * 2) { const int j = f >> 1, cb = f & 1, in = chained_in(j, qq); wv = (in < NS) ? theta[C::pW0 + in * PH + 16 * cb + ee] : 0.0f; }
        else if (f < L::P0KS * 2 + 16) { const int g = f - L::P0KS * 2, kk = g >> 1, cb = g & 1, in = chained_in(kk, qq); wv = theta[C::pW1 + in * PH + 16 * cb + ee]; }
        else { const int kk = f - L::P0KS * 2 - 16, in = chained_in(kk, qq); wv = (ee < NA) ? theta[C::pW2 + in * NA + ee] : 0.0f; }
        PW[i] = wv;
    }
    const float* pw0 = PW + lane, *pw1 = PW + L::P0KS * 2 * 64 + lane, *pw2 = PW + (L::P0KS * 2 + 16) * 64 + lane;
    float sig[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) sig[rr] = (4 * q + rr < NA) ? expf(fmaxf(theta[C::pLS + 4 * q + rr], LOG_MIN_STD)) : 0.0f;
    DynInNorm<C> in;
    DynOutNorm<C> out;
    in.load(norm, q);
    out.load(norm, q);
    // Per-step draws (Philox block 0 of RNG_STEP: action noise dims 0,1 | step model | reset row/model) are produced ONE STEP AHEAD.
    auto step_draws = [&](int tt, uint4& ds, float (&zz)[4]) {
        ds = rng_draw(r.seed, genv, tt, RNG_STEP, 0);
        {   // unconditional (no branch); unused when determ / draws are supplied.
            // lane q owns action dims 4q..4q+3 = chunks 2q, 2q+1 (chunk 0 = ds)
            const uint4 b0k = (q == 0) ? ds : ((NA > 4) ? rng_draw(r.seed, genv, tt, RNG_STEP, 2 * q) : ds);
            normal2(b0k.x, b0k.y, zz[0], zz[1]);
            if (NA > 2) { const uint4 b1k = rng_draw(r.seed, genv, tt, RNG_STEP, 2 * q + 1); normal2(b1k.x, b1k.y, zz[2], zz[3]); }
        }
    };
    constexpr bool LOCAL_REWARD = (ENV == METRPO_ENV_SWIMMER || ENV == METRPO_ENV_HALF_CHEETAH || ENV == METRPO_ENV_SNAKE);
    constexpr int RDIM = env_key_dim(ENV, NS);                             // reward reads next_state[RDIM]
    // One workgroup per CU and a small state (one col-block): the policy weight fragments and biases of this lane stay in registers for
    // the whole launch -- the policy chain is the step's critical path before B0 and otherwise starts with an LDS round trip.  (Only wave 0 uses them.)
    constexpr bool PWREG = SOLO && ONE && OUT_CB == 1;
    float w0r[PWREG ? L::P0KS * 2 : 1], w1r[PWREG ? 16 : 1], w2r[PWREG ? 8 : 1];
    f32x4 bp0r[2], bp1r[2], bp2r;
    if (PWREG || G == 1) __syncthreads();                                  // PW / BP images complete (a barrier: the other head group joins it)
    if constexpr (PWREG) {
#pragma unroll
        for (int f = 0; f < L::P0KS * 2; ++f) w0r[f] = pw0[f * 64];
#pragma unroll
        for (int f = 0; f < 16; ++f) w1r[f] = pw1[f * 64];
#pragma unroll
        for (int f = 0; f < 8; ++f) w2r[f] = pw2[f * 64];
        bp0r[0] = *(const f32x4*)&BP0[4 * q]; bp0r[1] = *(const f32x4*)&BP0[16 + 4 * q];
        bp1r[0] = *(const f32x4*)&BP1[4 * q]; bp1r[1] = *(const f32x4*)&BP1[16 + 4 * q];
        bp2r = *(const f32x4*)&BP2[4 * q];
    }
    PH_DECL
    for (int pc = 0; pc < npc; ++pc) {
    const int tile = (pc == npc - 1) ? c_first : (pc == 0 ? c_last : c_first + pc);
    const int t_begin = (tile == c_first) ? s_first : 0, t_end = (tile == c_last) ? e_last : r.T;
    b0 = tile * 16; b = b0 + e; active = b < r.B; genv = r.stream_offset + (uint64_t)b;
    // ---------------- vec_env.reset() (env_helpers.py:585-595), or the state handed over by the previous owner -------------
    const bool resume = r.init_obs != nullptr;
    int cur_model = 0, ts = 0;
    if (ONE && t_begin > 0) {
        // The producer is the previous workgroup, which runs this very piece FIRST and waits for nobody; workgroups are dispatched in
        // ascending order per XCD, so the smallest unfinished workgroup is always resident and the chain cannot deadlock.  Should the
        // platform ever break that assumption (CU masks, partition modes), the wait gives up after ~2 s of wall clock and raises the
        // ctx's sticky error cell (reported by the next metrpo_trpo_update / metrpo_comm_check) instead of hanging the GPU.
        if (tid == 0) {
            unsigned long long t0 = 0; int spins = 0;
            while (__hip_atomic_load(&r.mig_flag[tile], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != r.mig_epoch) {
                __builtin_amdgcn_s_sleep(4);
                if (++spins == 4096) t0 = wall_clock64();
                if (spins > 4096 && (spins & 1023) == 0 && wall_clock64() - t0 > 200000000ull) { if (r.mig_err) *r.mig_err = 1.0; break; }
            }
        }
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        cur_model = r.mig_model[b]; ts = r.mig_ts[b];
        COOP_FOR_CB
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int dim = 16 * cb + 4 * q + rr;
                ST[e * NSP + dim] = (dim < NS) ? r.mig_obs[(size_t)b * NS + dim] : 0.0f;
            }
    } else {
        int row = 0;
        if (active && !resume) {
            const uint4 d0 = rng_draw(r.seed, genv, 0, RNG_RESET, 0);
            row = (DRAWS && r.reset_idx != nullptr) ? r.reset_idx[b] : rng_index(d0.x, r.n_pool);
            cur_model = (DRAWS && r.reset_model != nullptr) ? r.reset_model[b] : rng_index(d0.y, K);
        }
        if (active && resume) { cur_model = r.init_model[b]; ts = r.init_ts[b]; }      // continuation of a chunked rollout
        COOP_FOR_CB
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int dim = 16 * cb + 4 * q + rr;
                ST[e * NSP + dim] = (dim < NS) ? (resume ? r.init_obs[(size_t)(active ? b : 0) * NS + dim] : r.pool[(size_t)row * NS + dim]) : 0.0f;
            }
    }
    __syncthreads();

    f32x4 xc[OUT_CB];                                                  // the tile's current state in registers: lane (e, q) holds dims 16 cb + 4 q + r (0 beyond ns)
    COOP_FOR_CB
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) { const int dim = 16 * cb + 4 * q + rr; xc[cb][rr] = ST[e * NSP + dim]; }
    uint4 dstep = make_uint4(0, 0, 0, 0); float z[4] = {0.f, 0.f, 0.f, 0.f};
    step_draws(r.t0 + t_begin, dstep, z);
    // vmcnt(0) HERE: every global load above (weight fragments, normaliser, initial state) is complete before the step loop.  Without
    // it the compiler places the wait for those loop-invariant loads at their first use INSIDE the loop, where it is executed every
    // step and then also waits for the stores of the previous step (HBM acknowledge latency on the step's critical path).
    __builtin_amdgcn_s_waitcnt(0x0F70);
    for (int t = t_begin; t < t_end; ++t) {
        PH_MARK(9)
        const size_t trow = (size_t)t * r.B;                               // uniform row base; lane offsets stay 32-bit (scalar base + offset addressing)
        const unsigned ub = (unsigned)b;
        // dynamics layer 0, k-steps that read only the STATE (inputs 4s..4s+3 all below ns - n_drop): independent of the action, so
        // every other wave runs them while wave 0 evaluates the policy
        constexpr int KS_STATE = (NS - C::NDROP) / 4;
        f32x4 h0[KG], hx0[XH > 0 ? XH : 1];
        if (!pol()) {
#pragma unroll
            for (int k = 0; k < KG; ++k) h0[k] = *(const f32x4*)&BD0[(K0 + k) * 64 + 16 * w + 4 * q];
#pragma unroll
            for (int j = 0; j < XH; ++j) { const int hx = hx_base + j; hx0[j] = *(const f32x4*)&BD0[(hx < K ? hx : 0) * 64 + 4 * q]; }
#pragma unroll
            for (int s = 0; s < KS_STATE; ++s) {
                const float x = in.get_state(ST, NSP, e, s);
#pragma unroll
                for (int k = 0; k < KG; ++k) { if (COOP_SKIP & 32) h0[k][0] += x; else h0[k] = MFMA16(wd0[k][s], x, h0[k]); }
                if (G < 0 || helper) {                                     // 4 waves: every wave in here is one
#pragma unroll
                    for (int j = 0; j < XH; ++j) { if (COOP_SKIP & 32) hx0[j][0] += x; else hx0[j] = MFMA16(ONE ? wx0[ONE ? j : 0][s] : WXL[(j * C::NIN_KS + s) * 64], x, hx0[j]); }
                }
            }
        }
        if (rngw() && !(COOP_SKIP & 16)) {
            // Next step's Philox block + Box-Muller for the 16 envs of the tile, produced by wave 1 while wave 0 evaluates the policy
            // (waves 1-3 have nothing else to do until the action exists) and handed over through LDS, double-buffered by step
            // parity: every wave picks its copy up after barrier B2.  (It used to be dealt out in pieces between the layer-1 MFMAs
            // of every wave: 16x redundant, and ~1000 cycles of VALU inside the phase two co-resident workgroups fight over.)
            uint4 dn; float zn[4] = {0.f, 0.f, 0.f, 0.f};
            step_draws(r.t0 + t + 1, dn, zn);
            float* dst = RNGB + (((t + 1) & 1) * 16 + e) * 20;
            if (q == 0) *(uint4*)dst = dn;
            *(float4*)(dst + 4 + 4 * q) = make_float4(zn[0], zn[1], zn[2], zn[3]);          // lane q owns action dims 4q .. 4q+3
        }
        // ---- policy -----------------------------
        // Weight fragments of a layer are fetched as one batch BEFORE the activation of the previous layer is evaluated (the LDS
        // latency hides under the tanh VALU work), and each tanh is issued right before the MFMA pair that consumes it, so the
        // matrix pipe works through k-step kk while the VALU evaluates the activation of k-step kk+1.
        // The policy (30 MFMAs, 16 tanh per lane) is evaluated by wave 0 ONLY and its clipped action handed to the other waves through
        // LDS (one more barrier per step).  Evaluating it redundantly in all 4 waves kept the step free of that barrier but cost
        // 90 of the 580 MFMAs and three quarters of the tanh VALU work of a tile-step -- issue slots a co-resident workgroup can use.
        if (pol()) {
            f32x4 p0[2], p1[2];
            if (COOP_SKIP & 1) { p0[0] = p0[1] = p1[0] = p1[1] = xc[0]; }
            f32x4 m0, m1 = {0.f, 0.f, 0.f, 0.f};
            if (!(COOP_SKIP & 1)) {
            {
                // layer 0 straight from the state registers xc (D layout of the previous step's output): k-step (cb_in, rr) contracts input
                // dims 16 cb_in + 4 q + rr, the weight fragments are stored in that order -- no LDS round trip between the end of a step
                // and the first policy MFMA of the next
                float w0[L::P0KS * 2];
#pragma unroll
                for (int f = 0; f < L::P0KS * 2; ++f) w0[f] = PWREG ? w0r[PWREG ? f : 0] : pw0[f * 64];
                if (PWREG) { p0[0] = bp0r[0]; p0[1] = bp0r[1]; } else { p0[0] = *(const f32x4*)&BP0[4 * q]; p0[1] = *(const f32x4*)&BP0[16 + 4 * q]; }
#pragma unroll
                for (int j = 0; j < L::P0KS; ++j) {
                    p0[0] = MFMA16(w0[2 * j], xc[j >> 2][j & 3], p0[0]);
                    p0[1] = MFMA16(w0[2 * j + 1], xc[j >> 2][j & 3], p0[1]);
                }
            }
            {
                // Straight-line code plus an explicit issue pipeline (sched_group_barrier): each tanh (v_mul, v_exp, v_add, v_rcp, v_fma:
                // ~45 cycles of VALU / transcendental issue) is placed behind the MFMA pair (layer 1) or MFMA (layer 2) of the PREVIOUS
                // k-step, so that it runs while the matrix pipe works.  Left to itself the compiler evaluates all eight tanh of a layer
                // first and then lets every MFMA wait for the final fma of its operand.
                float w1[16], w2[8];
#pragma unroll
                for (int f = 0; f < 16; ++f) w1[f] = PWREG ? w1r[PWREG ? f : 0] : pw1[f * 64];
#pragma unroll
                for (int f = 0; f < 8; ++f) w2[f] = PWREG ? w2r[PWREG ? f : 0] : pw2[f * 64];
                if (PWREG) { p1[0] = bp1r[0]; p1[1] = bp1r[1]; m0 = bp2r; }
                else { p1[0] = *(const f32x4*)&BP1[4 * q]; p1[1] = *(const f32x4*)&BP1[16 + 4 * q]; m0 = *(const f32x4*)&BP2[4 * q]; }
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const float hv = (COOP_SKIP & 64) ? p0[kk >> 2][kk & 3] : tanh_fast(p0[kk >> 2][kk & 3]);
                    p1[0] = MFMA16(w1[2 * kk], hv, p1[0]);
                    p1[1] = MFMA16(w1[2 * kk + 1], hv, p1[1]);
                }
#pragma unroll
                for (int kk = 0; kk < 8; kk += 2) {
                    const float ha = (COOP_SKIP & 64) ? p1[kk >> 2][kk & 3] : tanh_fast(p1[kk >> 2][kk & 3]);
                    m0 = MFMA16(w2[kk], ha, m0);
                    const float hb = (COOP_SKIP & 64) ? p1[(kk + 1) >> 2][(kk + 1) & 3] : tanh_fast(p1[(kk + 1) >> 2][(kk + 1) & 3]);
                    m1 = MFMA16(w2[kk + 1], hb, m1);
                }
                __builtin_amdgcn_sched_group_barrier(0x100, 64, 0);                // every LDS read of the block (inputs, weight fragments, biases) up front
                __builtin_amdgcn_sched_group_barrier(0x008, L::P0KS * 2, 0);       // layer 0
                __builtin_amdgcn_sched_group_barrier(0x402, 5, 0);                 // tanh of k-step 0
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {                                    // layer 1, k-step kk: the wave cannot issue past an MFMA the pipe
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);             // has no room for, so the tanh of k-step kk+1 (the last one: layer 2's
                    __builtin_amdgcn_sched_group_barrier(0x402, 3, 0);             // first) is split around the pair's second MFMA instead of queuing
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);             // behind it
                    __builtin_amdgcn_sched_group_barrier(0x402, 2, 0);
                }
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);             // layer 2, k-step kk
                    if (kk < 7) __builtin_amdgcn_sched_group_barrier(0x402, 5, 0);
                }
            }
            } else m0 = xc[0];
            const f32x4 mu = m0 + m1;
            PH_MARK(0)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int d = 4 * q + rr;
                if (d < NA) {
                    float a = mu[rr];
                    if (!r.determ) {
                        const float zz = (DRAWS && r.eps != nullptr) ? (active ? (r.eps + trow * NA)[ub * NA + d] : 0.0f) : z[rr];
                        a = fmaf(zz, sig[rr], a);
                    }
                    AK[e * NA + d] = a; AK[16 * NA + e * NA + d] = mu[rr];
                    const float ac = fminf(fmaxf(a, -1.0f), 1.0f);            // env_helpers.py:599
                    ACT[e * NA + d] = ac;
                }
            }
        }
        __syncthreads();                                                   // B0: actions visible
        PH_MARK(1)
        // ---- dynamics layer 0: the other waves finish their col-block and the helpers their share of col-block 0; wave 0 issues the step's global
        //      stores meanwhile (it has no layer-0 work, and nothing waits for a store: barriers wait for LDS traffic only) -------
        if (!pol()) {
            float xin[C::NIN_KS];
#pragma unroll
            for (int s = KS_STATE; s < C::NIN_KS; ++s) xin[s] = in.get(ST, NSP, ACT, e, s);
#pragma unroll
            for (int s = KS_STATE; s < C::NIN_KS; ++s) {
#pragma unroll
                for (int k = 0; k < KG; ++k) { if (COOP_SKIP & 8) h0[k][0] += xin[s]; else h0[k] = MFMA16(wd0[k][s], xin[s], h0[k]); }
                if (G < 0 || helper) {
#pragma unroll
                    for (int j = 0; j < XH; ++j) { if (COOP_SKIP & 8) hx0[j][0] += xin[s]; else hx0[j] = MFMA16(ONE ? wx0[ONE ? j : 0][s] : WXL[(j * C::NIN_KS + s) * 64], xin[s], hx0[j]); }
                }
            }
#pragma unroll
            for (int k = 0; k < KG; ++k) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) h0[k][rr] = relu1(h0[k][rr]);
                *(f32x4*)&H0[(K0 + k) * 1024 + w * 256 + q * 64 + e * 4] = h0[k];        // H0[k][cb][q][env][r]
            }
            if (G < 0 || helper) {
#pragma unroll
                for (int j = 0; j < XH; ++j) {
                    const int hx = hx_base + j;
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) hx0[j][rr] = relu1(hx0[j][rr]);
                    if (hx < K) *(f32x4*)&H0[hx * 1024 + q * 64 + e * 4] = hx0[j];
                }
            }
        } else if (!(COOP_SKIP & 256)) {
            {                                                              // unclipped action and mean: coalesced linear copies of the tile
                const size_t base_a = (trow + b0) * NA;
                const int lim_a = min(16, r.B - b0) * NA;
#pragma unroll
                for (int j = 0; j < (16 * NA + 63) / 64; ++j) {
                    const int i = lane + 64 * j;
                    if (i < lim_a) { (r.act + base_a)[(unsigned)i] = AK[i]; (r.mean + base_a)[(unsigned)i] = AK[16 * NA + i]; }
                }
            }
            const size_t base = (trow + b0) * NS;               // obs[t]: coalesced linear copy of the tile
            const int lim = min(16, r.B - b0) * NS;
            float ov[(16 * NS + 63) / 64];                                 // all LDS reads first: one register per store, no store waits for another
#pragma unroll
            for (int j = 0; j < (16 * NS + 63) / 64; ++j) { const int i = min(lane + 64 * j, 16 * NS - 1); ov[j] = ST[(i / NS) * NSP + i % NS]; }
#pragma unroll
            for (int j = 0; j < (16 * NS + 63) / 64; ++j) { const int i = lane + 64 * j; if (i < lim) (r.obs + base)[(unsigned)i] = ov[j]; }
        }
        PH_MARK(2)
        __syncthreads();                                                   // B1: layer-0 activations of all heads visible
        PH_MARK(3)
        float su2 = 0.0f;                                                  // sum_d clip(a_d)^2 of the own env (ACT is complete since B1)
        if constexpr (SOLO) {                                              // for the reward; every wave of the group, so that all contract the same multiply-adds
#pragma unroll
            for (int d = 0; d < NA; ++d) { const float ac = ACT[e * NA + d]; su2 = fmaf(ac, ac, su2); }
        }
        // ---- layer 1 (own col-block) and the layer-2 partial over the own 16 hidden units, the wave's heads ----------------
        PH_MARK(10)
        __builtin_amdgcn_s_setprio(1);          // the matrix-heavy phase wins issue arbitration over a co-resident workgroup's VALU phases
        f32x4 h1[KG];
#pragma unroll
        for (int k = 0; k < KG; ++k) h1[k] = *(const f32x4*)&BD1[(K0 + k) * 64 + 16 * w + 4 * q];
        constexpr int NHB = ONE ? 2 : 1;                                   // ONE: layer-0 activations fetched one col-block ahead (registers to spare)
        f32x4 hb[NHB][KG];
        if (ONE) {
#pragma unroll
            for (int k = 0; k < KG; ++k) hb[0][k] = *(const f32x4*)&H0[(K0 + k) * 1024 + q * 64 + e * 4];
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            if (ONE) {
                if (cb < 3) {
#pragma unroll
                    for (int k = 0; k < KG; ++k) hb[(cb + 1) % NHB][k] = *(const f32x4*)&H0[(K0 + k) * 1024 + (cb + 1) * 256 + q * 64 + e * 4];
                }
            } else {
#pragma unroll
                for (int k = 0; k < KG; ++k) hb[0][k] = *(const f32x4*)&H0[(K0 + k) * 1024 + cb * 256 + q * 64 + e * 4];
            }
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
                for (int k = 0; k < KG; ++k) { if (COOP_SKIP & 4) h1[k] += hb[cb % NHB][k]; else h1[k] = MFMA16(wd1[k][cb * 4 + rr], hb[cb % NHB][k][rr], h1[k]); }
                __builtin_amdgcn_sched_barrier(0x94);                      // only SALU / VMEM / LDS instructions may cross
                if (ONE) pin_order(h1);                                    // and the K chains advance in lock-step (mfma_common.h)
            }
        }
        PH_MARK(11)
#pragma unroll
        for (int k = 0; k < KG; ++k)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) h1[k][rr] = relu1(h1[k][rr]);
        __builtin_amdgcn_sched_barrier(0);      // all ReLUs first: a v_max feeding the very next MFMA's operand stalls it (0.386 -> 0.373 ms at B = 4096)
        {
            f32x4 po[KG][OUT_CB];
#pragma unroll
            for (int k = 0; k < KG; ++k)
                COOP_FOR_CB po[k][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                COOP_FOR_CB
#pragma unroll
                    for (int k = 0; k < KG; ++k) { if (COOP_SKIP & 2) po[k][cb] += h1[k]; else po[k][cb] = MFMA16(wd2[k][rr][cb], h1[k][rr], po[k][cb]); }
#pragma unroll
            for (int k = 0; k < KG; ++k)
                COOP_FOR_CB *(f32x4*)&PART[(((K0 + k) * 4 + w) * 16 + e) * NSP + 16 * cb + 4 * q] = po[k][cb];
        }
        __builtin_amdgcn_s_setprio(0);
        PH_MARK(4)
        __syncthreads();                                                   // B2: all partial sums visible
        PH_MARK(5)
        // ---- selection (env_helpers.py:617-634): out_k = b2_k + sum_w partial ; next = dmean + dstd*out + s ----
        ts += 1;
        int sel = cur_model;
        if (r.sam_mode == METRPO_SAM_STEP_RAND) sel = (DRAWS && r.model_idx != nullptr) ? (active ? (r.model_idx + trow)[ub] : 0) : rng_index(dstep.z, K);
        if (r.sam_mode == METRPO_SAM_ONE_MODEL) sel = 0;
        const bool simple = (r.sam_mode == METRPO_SAM_STEP_RAND || r.sam_mode == METRPO_SAM_EPS_RAND || r.sam_mode == METRPO_SAM_ONE_MODEL);
        f32x4 nx[OUT_CB];
        COOP_FOR_CB {
            const int off = e * NSP + 16 * cb + 4 * q;
            const f32x4 sv = xc[cb];
            auto head = [&](int k) -> f32x4 {
                if (COOP_SKIP & 128) return sv * 0.999f;
                const float* pp = PART + (size_t)k * 4 * 16 * NSP + off;
                f32x4 o = *(const f32x4*)&BD2[k * NSP + 16 * cb + 4 * q];
                o += (*(const f32x4*)&pp[0] + *(const f32x4*)&pp[16 * NSP]) + (*(const f32x4*)&pp[2 * 16 * NSP] + *(const f32x4*)&pp[3 * 16 * NSP]);
                return out.apply(cb, o, sv);
            };
            if (simple) nx[cb] = head(sel);
            else {
                f32x4 hv[K], m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < K; ++k) { hv[k] = head(k); m += hv[k]; }
                m /= (float)K;
                if (r.sam_mode == METRPO_SAM_MODEL_MEAN) nx[cb] = m;
                else if (r.sam_mode == METRPO_SAM_MODEL_MEAN_STD) {
                    f32x4 var = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < K; ++k) { const f32x4 d = hv[k] - m; var += d * d; }
                    float zz[4] = {0.f, 0.f, 0.f, 0.f};
                    if (!DRAWS || r.sel_noise == nullptr) normal4(rng_draw(r.seed, genv, r.t0 + t, RNG_SELNOISE, 4 * cb + q), zz);
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int dim = 16 * cb + 4 * q + rr;
                        const float nz = (DRAWS && r.sel_noise != nullptr) ? ((active && dim < NS) ? (r.sel_noise + trow * NS)[ub * NS + dim] : 0.0f) : zz[rr];
                        nx[cb][rr] = fmaf(nz, sqrtf(var[rr] / (float)K), m[rr]);
                    }
                } else {                                                  // model_med: np.median over K
                    constexpr int r_lo = (K - 1) / 2, r_hi = K / 2;
                    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        int rank[4] = {0, 0, 0, 0};
#pragma unroll
                        for (int j = 0; j < K; ++j)
#pragma unroll
                            for (int rr = 0; rr < 4; ++rr) rank[rr] += (hv[j][rr] < hv[k][rr]) || (hv[j][rr] == hv[k][rr] && j < k);
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) { if (rank[rr] == r_lo) lo[rr] = hv[k][rr]; if (rank[rr] == r_hi) hi[rr] = hv[k][rr]; }
                    }
                    nx[cb] = (lo + hi) * 0.5f;
                }
            }
        }
        PH_MARK(6)
        // ---- reward (:601), is_done (:603), horizon (:604): the reward is the SOLO group's, its stores wave 2's; the other group's is_done
        //      is the horizon alone (its envs have no other) ----------------------------------------------
        float cost = 0.0f;
        bool dn = false;
        if constexpr (!SOLO) dn = (ts >= r.H);
        else if (LOCAL_REWARD) {
            // the reward reads ONE next-state dim: the lane that owns it (q == RDIM/4 of col-block 0) evaluates and stores it from
            // registers -- no LDS round trip; is_done is the horizon only (uniform)
            cost = env_cost_terms(ENV, NA, nx[RDIM / 16][RDIM & 3], 0.0f, 0.0f, su2, 0.0f);
            dn = (ts >= r.H);
            if (reww() && q == ((RDIM & 15) >> 2) && active) { (r.rew + trow)[ub] = -cost; (r.done + trow)[ub] = dn ? 1 : 0; (r.tpath + trow)[ub] = ts - 1; }
        } else {
            float pen = 0.0f; int fin = 1;
            COOP_FOR_CB
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int dim = 16 * cb + 4 * q + rr;
                    if (dim < NS) {
                        NX[e * NS + dim] = nx[cb][rr];
                        if (ENV == METRPO_ENV_HOPPER && dim >= 2) pen += env_hopper_pen_term(nx[cb][rr]);
                        if (ENV == METRPO_ENV_ANT) fin &= isfinite(nx[cb][rr]) ? 1 : 0;
                    }
                }
            wave_lds_sync();
            const float* xn = NX + e * NS;
            if (ENV == METRPO_ENV_HOPPER) pen = xor_sum(pen);
            cost = env_cost_terms(ENV, NA, xn[env_key_dim(ENV, NS)], xn[0], xn[1], su2, pen);
            if (ENV == METRPO_ENV_ANT) {
                int f2 = fin & __shfl_xor(fin, 16, 64);
                f2 &= __shfl_xor(f2, 32, 64);
                dn = env_done(ENV, xn[2], f2 != 0);
            }
            dn = dn || (ts >= r.H);
            if (reww() && q == 0 && active) { (r.rew + trow)[ub] = -cost; (r.done + trow)[ub] = dn ? 1 : 0; (r.tpath + trow)[ub] = ts - 1; }
        }
        PH_MARK(7)
        // ---- reset(dones) (:585-595) or advance; every wave keeps its own copy of the tile state ----------
        if (__any(dn)) {                                                   // rare: horizon reached / Ant fell
            int row = 0;
            if (dn) {
                if (active) {
                    row = (DRAWS && r.reset_idx != nullptr) ? (r.reset_idx + trow + r.B)[ub] : rng_index(dstep.w, r.n_pool);
                    cur_model = (DRAWS && r.reset_model != nullptr) ? (r.reset_model + trow + r.B)[ub] : rng_index16(dstep.z, K);
                }
                ts = 0;
            }
            COOP_FOR_CB
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int dim = 16 * cb + 4 * q + rr;
                    if (dim < NS) { const float xv = dn ? r.pool[(unsigned)(row * NS + dim)] : nx[cb][rr]; ST[e * NSP + dim] = xv; xc[cb][rr] = xv; }
                }
        } else {
            COOP_FOR_CB {
                xc[cb] = nx[cb];
                *(f32x4*)&ST[e * NSP + 16 * cb + 4 * q] = nx[cb];              // padded dims: dstd = dmean = 0 and zero weights keep them 0
            }
        }
        {                                                                  // written by wave 1 before B0 of this step
            const float* src = RNGB + (((t + 1) & 1) * 16 + e) * 20;
            dstep = *(const uint4*)src;
            if (SOLO) { const float4 zf = *(const float4*)(src + 4 + 4 * q); z[0] = zf.x; z[1] = zf.y; z[2] = zf.z; z[3] = zf.w; }
        }
        wave_lds_sync();
        PH_MARK(8)
    }
    if (ONE && t_end < r.T) {                                              // hand the tile over (another workgroup runs steps t_end..T-1)
        if (pol()) {
            const int lim = 16 * NS;
            for (int i = lane; i < lim; i += 64) r.mig_obs[(size_t)b0 * NS + i] = ST[(i / NS) * NSP + i % NS];
            if (q == 0) { r.mig_ts[b] = ts; r.mig_model[b] = cur_model; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            if (lane == 0) __hip_atomic_store(&r.mig_flag[tile], r.mig_epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        if (pol() && r.last_obs != nullptr) {
            const int lim = min(16, r.B - b0) * NS;
            for (int i = lane; i < lim; i += 64) r.last_obs[(size_t)b0 * NS + i] = ST[(i / NS) * NSP + i % NS];
        }
        if (pol() && q == 0 && active) {
            if (r.last_ts != nullptr) r.last_ts[b] = ts;
            if (r.last_model != nullptr) r.last_model[b] = cur_model;
        }
    }
    __syncthreads();                                                       // the next piece re-initialises the tile state in LDS
    }
    PH_DUMP
#undef COOP_FOR_CB
