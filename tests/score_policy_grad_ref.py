"""NumPy restatement of metrpo_score_policy_actions_grad (include/metrpo.h): per head k and candidate b the gradient of the head's CLOSED-LOOP return
(score_policy_ref.score_policy_actions' ret: a_t = policy_mean(s_t) + noise_t sigma formed from the head's own state) with respect to the noise
sequences and the start state.  It is score_grad_ref.walk with the policy in the loop and one more adjoint term:

    w_t      = gamma^t alive_t                      (gamma^t by repeated multiplication; the mask is a constant of the differentiation)
    G        = lambda_t+1 - w_t dc/dx_next
    gU       = -w_t dc/du + (action rows of F^T G)
    gm       = gU where -1 <= a_t <= 1, else 0       (tf.clip_by_value, on the head's own UNCLIPPED a_t)
    grad_t   = gm                                    (noise_in_std: gm * exp(max(log_std, LOG_MIN_STD)))
    lambda_t = G + (state rows of F^T G) + J_pi(s_t)^T gm

J_pi^T gm is oracle.bptt_oracle.policy_costs_and_grad's input adjoint of the policy (tanh' = 1 - p^2) written out here.

`walk` runs in `dtype` throughout and keeps the signed distance of every kink argument from its kink (the clip site is |a_t| - 1 of every head's own
action).  mut: one of the wrong restatements tests/test_score_policy_grad_ref.py has the bounds catch -- score_grad_ref's six and
    'no_policy_path'   lambda_t without J_pi^T gm (what metrpo_score_actions_grad fed with act_out gives)
    'gate_on_mean'     the clip gate taken on mean_t instead of a_t
    'sigma_missing'    grad_t = gm where the noise is in units of the policy's std (it changes nothing where it is not)
    'policy_at_next'   the policy term taken a step late: lambda_t gets J_pi(s_t+1)^T gm_t+1 (an off-by-one of the reverse loop)
"""
import numpy as np

from oracle import metrpo_oracle as O
from oracle import bptt_oracle as Bp
from score_actions_ref import start_rows
import score_grad_ref as G0

MUTS = G0.MUTS + ('no_policy_path', 'gate_on_mean', 'sigma_missing', 'policy_at_next')


def _policy_vjp(Ws, hs, gm):
    """J_pi(s)^T gm from the stored hidden activations hs = [s, p0, p1, ...]"""
    dh = gm @ Ws[-1].T
    for l in range(len(Ws) - 2, -1, -1):
        dh = (dh * (1 - np.square(hs[l + 1]))) @ Ws[l].T
    return dh


def walk(dm, theta, pdims, env, init_obs, noise=None, T=None, gamma=1.0, stop_at_done=True, noise_in_std=False, dtype=np.float64, mut=None, grad=True):
    """init_obs [S, ns] or [ns]; noise [T, B, na] or None (then T= steps, B = S: the gradient at noise = 0).  -> dict(ret [K, B], len [K, B] int,
    grad [K, T, B, na], gm [K, T, B, na] (dR / d a_t, total), lam0 [K, B, ns], act [K, T, B, na] unclipped, obs [K, T+1, B, ns], rew [K, T, B],
    w [K, T, B] (float64 arrays of `dtype` values), sites: name -> [B, n] over all heads and steps)."""
    f = dtype
    assert mut is None or mut in MUTS
    d = dm.astype(f)
    init = np.atleast_2d(np.asarray(init_obs, np.float64))
    if noise is None:
        B, T = init.shape[0], int(T)
        nz = np.zeros((T, B, d.na), f)
    else:
        nz = np.asarray(noise, f)
        T, B = nz.shape[:2]
    th = np.asarray(theta, f)
    Ws, bs, _ = O.policy_unflatten(th, pdims)
    sigma = np.exp(O.policy_log_std(th, pdims)).astype(f)
    scale = sigma if noise_in_std else np.ones_like(sigma)
    K, ns, na, L = d.K, d.ns, d.na, len(d.Ws)
    s0 = start_rows(init, B).astype(f)
    ret = np.zeros((K, B)); length = np.zeros((K, B), np.int64)
    G_out = np.zeros((K, T, B, na)); GM = np.zeros((K, T, B, na)); lam0 = np.zeros((K, B, ns))
    rews = np.zeros((K, T, B)); wts = np.zeros((K, T, B)); acts = np.zeros((K, T, B, na)); obss = np.zeros((K, T + 1, B, ns))
    sites = {}

    def site(name, v):
        sites.setdefault(name, []).append(np.asarray(v, np.float64).reshape(B, -1))

    for k in range(K):
        xs, hs_all, ps_all, ws, araws, means, us = [s0], [], [], [], [], [], []
        alive = np.ones(B, bool)
        disc = 1.0                                                       # float64 by repeated multiplication, rounded where it becomes a weight
        for t in range(T):
            x = xs[-1]
            with np.errstate(all='ignore'):
                m, ps = O._policy_forward(Ws, bs, x)
                m = m.astype(f)
                araw = (nz[t] * scale + m).astype(f)
                site('clip', np.abs(araw) - 1.0)
                a = np.clip(araw, f(-1.0), f(1.0))
                h = ((np.concatenate([x, a], axis=1) - d.in_mean) / d.in_std)[:, d.n_drop:]
                hs = [h]
                for l in range(L):
                    h = h @ d.Ws[l][k] + d.bs[l][k]
                    if l < L - 1:
                        if d.acts[l] == 'relu':
                            site('relu', h)
                        h = O._ACTS[d.acts[l]](h); hs.append(h)
                xn = (d.diff_mean[:ns] + d.diff_std[:ns] * h + x).astype(f)
                if env == 'half_cheetah':
                    site('hc_inner', np.abs(xn[:, 9] - f(1e-1 * 0.5) * np.sum(np.square(a), axis=1)) - 10.0)
                elif env == 'hopper':
                    site('hopper_045', 0.45 - xn[:, 0]); site('hopper_02', np.abs(xn[:, 1]) - 0.2); site('hopper_100', np.abs(xn[:, 2:]) - 100.0)
                elif env == 'ant' and stop_at_done:
                    site('ant_lo', xn[:, 2] - 0.2); site('ant_hi', 1.0 - xn[:, 2])
                r = -O.cost_np_vec(env, x, a, xn)
            dn = np.asarray(O.is_done(env, xn, xn), bool)
            if mut == 'mask_first' and stop_at_done:
                alive = alive & ~dn
            g = disc * gamma if mut == 'gamma_shift' else disc
            ret[k] = np.where(alive, ret[k] + g * np.asarray(r, np.float64), ret[k])
            length[k] += alive
            w = np.where(alive, f(g), f(0.0)).astype(f)
            disc = disc * gamma
            if stop_at_done and mut != 'mask_first':
                alive = alive & ~dn
            xs.append(xn); hs_all.append(hs); ps_all.append(ps); ws.append(w); araws.append(araw); means.append(m); us.append(a)
            rews[k, t] = r; wts[k, t] = w; acts[k, t] = araw
        obss[k] = np.stack(xs)
        if not grad:
            continue
        lam = np.zeros((B, ns), f)
        in_std = np.ones_like(d.in_std) if mut == 'no_in_std' else d.in_std
        for t in range(T - 1, -1, -1):
            gu_c, gx_c = Bp._cost_grads(env, us[t], xs[t + 1], ws[t])          # of +w c
            G = (lam - gx_c).astype(f)
            dd = G if mut == 'no_diff_std' else G * d.diff_std[:ns]
            hs = hs_all[t]
            for l in range(L - 1, -1, -1):
                dd = dd @ d.Ws[l][k].T
                if l > 0:
                    dd = dd * G0._act_deriv(d.acts[l - 1], hs[l])
            gxu = np.zeros((B, ns + na), f)
            gxu[:, d.n_drop:] = dd
            gxu = gxu / in_std
            gU = -gu_c + gxu[:, ns:]
            gated = means[t] if mut == 'gate_on_mean' else araws[t]
            gate = np.ones_like(gU, bool) if mut == 'no_clip_gate' else (gated >= -1.0) & (gated <= 1.0)
            gm = np.where(gate, gU, f(0.0)).astype(f)
            GM[k, t] = gm
            G_out[k, t] = gm if mut == 'sigma_missing' else gm * scale
            lam = ((0 if mut == 'no_residual' else G) + gxu[:, :ns]).astype(f)
            if mut == 'policy_at_next':
                if t + 1 < T:
                    lam = (lam + _policy_vjp(Ws, ps_all[t + 1], GM[k, t + 1].astype(f))).astype(f)
            elif mut != 'no_policy_path':
                lam = (lam + _policy_vjp(Ws, ps_all[t], gm)).astype(f)
        lam0[k] = lam
    return dict(ret=ret, len=length, grad=G_out, gm=GM, lam0=lam0, act=acts, obs=obss, rew=rews, w=wts,
                sites={n: np.concatenate(v, axis=1) for n, v in sites.items()})


def score_policy_actions_grad(dm, theta, pdims, env, init_obs, noise=None, T=None, gamma=1.0, stop_at_done=True, noise_in_std=False):
    """The float64 reference: dict(ret, len, grad, gm, lam0, grad_mean [T, B, na], act, obs, rew, w)."""
    out = walk(dm, theta, pdims, env, init_obs, noise, T, gamma, stop_at_done, noise_in_std)
    out['grad_mean'] = out['grad'].sum(axis=0) / dm.K
    return out
