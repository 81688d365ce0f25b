// The per-candidate return of metrpo_score_actions and metrpo_score_policy_actions (include/metrpo.h): what score_actions.hip's and
// score_policy_actions.hip's fused kernels carry per lane and what k_sact_reduce applies to a stored trajectory.
#pragma once

// one step of the return: ret += gamma^t alive_t r_t in float64, then the discount, then the mask (model_based_rl.py:134-137: the step that ends an
// episode still counts).  A step that is not counted adds nothing (no 0 * r).
struct SactSum {
    double sum = 0.0, disc = 1.0;
    int n = 0;
    bool alive = true;
    __device__ __forceinline__ void step(float rew, bool done, double gamma, int stop) {
        if (alive) { sum += disc * (double)rew; ++n; }
        disc *= gamma;
        if (stop && done) alive = false;
    }
};
