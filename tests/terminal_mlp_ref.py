"""NumPy restatement of the four scoring calls of include/metrpo.h with the terminal value's MLP form set (metrpo_set_terminal_value_mlp): the walk of
tests/terminal_value_ref.py -- open loop (supplied actions) or closed loop (a_t = policy_mean(s_t) + noise_t sigma) -- with the terminal term

    o_d      = clip(s_T,d, -10, 10)
    p0       = tanh(o W0 + b0);   p1 = tanh(p0 W1 + b1)           W0 [ns, h1], W1 [h1, h2]: in-major
    V        = bias_row + b2 + sum_j W2[j] p1[j]                    bias_row = bias[b // (B // S)] where there is one bias per start state
    ret     += gamma^T alive_T V                                    alive_T: after the last step's mask update; gamma^T by repeated multiplication
    w_T      = alive_T ? gamma^T : 0
    lambda_T = w_T dV/ds_T,   dV/ds = (W0 (W1 (W2 * (1 - p1^2)) * (1 - p0^2)))  where -10 <= s_T,d <= 10, else 0

and from there the reverse recursion of the header, unchanged (closed loop: the seed reaches J_pi(s_T-1) through G like any lambda).

`walk` runs in `dtype` throughout (float64: the reference; float32 beside it: the kink guard and the share of the bounds fp32 arithmetic alone uses)
and keeps the signed distance of every kink argument from its kink: score_grad_ref's sites and tv_clip = |s_T,d| - 10 (tanh has no kink).
mut: one of the wrong restatements tests/test_terminal_mlp_ref.py has the bounds catch --
    'mlp_no_deriv'       no 1 - p^2 factor in the adjoint
    'mlp_w1_transposed'  W1 read out-major (square nets only; others are left as they are)
    'mlp_no_b2'          b2 dropped
    'tv_no_clip'         o unclipped
    'tv_no_clip_gate'    the gradient passes outside +-10
    'tv_bias_row'        bias[0] for every start state
    'tv_no_alive'        bootstraps behind a done
    'tv_gamma_shift'     gamma^(T-1)
    'tv_no_policy_path'  closed loop: the seed is not carried through J_pi
"""
import numpy as np

from oracle import metrpo_oracle as O
from oracle import bptt_oracle as Bp
from score_actions_ref import start_rows
import score_grad_ref as G0
from score_policy_grad_ref import _policy_vjp

MUTS = ('mlp_no_deriv', 'mlp_w1_transposed', 'mlp_no_b2', 'tv_no_clip', 'tv_no_clip_gate', 'tv_bias_row', 'tv_no_alive', 'tv_gamma_shift',
        'tv_no_policy_path')
TANH_FAST_ABS = 2e-7                 # the stated absolute error of tanh_fast (csrc/device_common.h)


def pack(tv):
    """(W0, b0, W1, b1, W2, b2, bias) -> the library's d_params, float32"""
    return np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in tv[:6]])


def value_terms(tv, sT, per, f=np.float64, mut=None):
    """tv = (W0 [ns, h1], b0 [h1], W1 [h1, h2], b1 [h2], W2 [h2], b2 [1], bias [n_bias]); sT [B, ns]; per = B // S.
    -> (V [B], dV/ds [B, ns], mag [B], clip site [B, ns], tanh_term [B]) in `f`, where
    mag = |bias_row| + |b2| + sum_j |W2_j p1_j| + sum_d |dV/ds_d o_d| and tanh_term = 2e-7 (sum_j |W2_j| + sum_j |W2_j| (1 - p1_j^2) sum_i |W1_ij|)."""
    W0, b0, W1, b1, W2, b2, bias = (np.asarray(x, f) for x in tv)
    b0, b1, W2, b2, bias = b0.reshape(-1), b1.reshape(-1), W2.reshape(-1), b2.reshape(-1), bias.reshape(-1)
    if mut == 'mlp_w1_transposed' and W1.shape[0] == W1.shape[1]:
        W1 = W1.T
    if mut == 'mlp_no_b2':
        b2 = np.zeros_like(b2)
    B = sT.shape[0]
    row = np.zeros(B, int) if (bias.shape[0] == 1 or mut == 'tv_bias_row') else np.arange(B) // per
    assert row.max() < bias.shape[0]
    o = sT if mut == 'tv_no_clip' else np.clip(sT, f(-10.0), f(10.0))
    p0 = np.tanh(o @ W0 + b0).astype(f)
    p1 = np.tanh(p0 @ W1 + b1).astype(f)
    v = (bias[row] + (b2[0] + p1 @ W2)).astype(f)
    d1 = np.ones_like(p1) if mut == 'mlp_no_deriv' else (f(1.0) - p1 * p1)
    d0 = np.ones_like(p0) if mut == 'mlp_no_deriv' else (f(1.0) - p0 * p0)
    g0 = ((W2 * d1) @ W1.T) * d0
    dfull = (g0 @ W0.T).astype(f)
    inside = np.ones_like(sT, bool) if mut in ('tv_no_clip', 'tv_no_clip_gate') else (sT >= -10.0) & (sT <= 10.0)
    dv = np.where(inside, dfull, f(0.0)).astype(f)
    mag = np.abs(bias[row]) + np.abs(b2[0]) + np.sum(np.abs(W2 * p1), axis=1) + np.sum(np.abs(dv * o), axis=1)
    tanh_term = TANH_FAST_ABS * (np.sum(np.abs(W2)) + (np.abs(W2) * (1.0 - p1 * p1)) @ np.sum(np.abs(W1), axis=0))
    return v, dv, mag, np.abs(sT) - 10.0, tanh_term


def walk(dm, env, init_obs, seq, tv, policy=None, T=None, gamma=1.0, stop_at_done=True, noise_in_std=False, dtype=np.float64, mut=None, grad=True):
    """policy None: seq = actions [T, B, na] unclipped (open loop).  policy = (theta, pdims): seq = noise [T, B, na] or None (then T= steps, B = S).
    tv = value_terms' 7-tuple, or None: no terminal value.
    -> dict(ret [K, B], len [K, B] int, grad [K, T, B, na], lam0 [K, B, ns], act [K, T, B, na] unclipped, rew [K, T, B], w [K, T, B], wT [K, B],
    tv_mag [K, B], tv_tanh [K, B], sites: name -> [B, n] over all heads and steps)."""
    f = dtype
    assert mut is None or mut in MUTS
    d = dm.astype(f)
    init = np.atleast_2d(np.asarray(init_obs, np.float64))
    K, ns, na, L = d.K, d.ns, d.na, len(d.Ws)
    closed = policy is not None
    if closed:
        th = np.asarray(policy[0], f)
        Ws, bs, _ = O.policy_unflatten(th, policy[1])
        sigma = np.exp(O.policy_log_std(th, policy[1])).astype(f)
        scale = sigma if noise_in_std else np.ones_like(sigma)
        if seq is None:
            B, T = init.shape[0], int(T)
            nz = np.zeros((T, B, na), f)
        else:
            nz = np.asarray(seq, f)
            T, B = nz.shape[:2]
    else:
        araw_ol = np.asarray(seq, f)
        T, B = araw_ol.shape[:2]
        scale = np.ones(na, f)
    per = B // init.shape[0]
    s0 = start_rows(init, B).astype(f)
    ret = np.zeros((K, B)); length = np.zeros((K, B), np.int64)
    G_out = np.zeros((K, T, B, na)); lam0 = np.zeros((K, B, ns))
    rews = np.zeros((K, T, B)); wts = np.zeros((K, T, B)); acts = np.zeros((K, T, B, na)); wTs = np.zeros((K, B)); mags = np.zeros((K, B)); tanhs = np.zeros((K, B))
    sites = {}

    def site(name, v):
        sites.setdefault(name, []).append(np.asarray(v, np.float64).reshape(B, -1))

    for k in range(K):
        xs, hs_all, ps_all, ws, araws, us = [s0], [], [], [], [], []
        alive = np.ones(B, bool)
        disc = 1.0                                                       # float64 by repeated multiplication, rounded where it becomes a weight
        disc_before = 1.0
        for t in range(T):
            x = xs[-1]
            with np.errstate(all='ignore'):
                ps = None
                if closed:
                    m, ps = O._policy_forward(Ws, bs, x)
                    araw = (nz[t] * scale + m.astype(f)).astype(f)
                else:
                    araw = araw_ol[t]
                if closed or k == 0:
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
            ret[k] = np.where(alive, ret[k] + disc * np.asarray(r, np.float64), ret[k])
            length[k] += alive
            w = np.where(alive, f(disc), f(0.0)).astype(f)
            disc_before = disc
            disc = disc * gamma
            if stop_at_done:
                alive = alive & ~dn
            xs.append(xn); hs_all.append(hs); ps_all.append(ps); ws.append(w); araws.append(araw); us.append(a)
            rews[k, t] = r; wts[k, t] = w; acts[k, t] = araw
        # ---- the terminal term ----
        seed = np.zeros((B, ns), f)
        if tv is not None:
            v, dv, mag, csite, tterm = value_terms(tv, xs[T], per, f, mut)
            site('tv_clip', csite)
            al = np.ones(B, bool) if mut == 'tv_no_alive' else alive
            g = disc_before if mut == 'tv_gamma_shift' else disc
            ret[k] = np.where(al, ret[k] + g * np.asarray(v, np.float64), ret[k])
            wT = np.where(al, f(g), f(0.0)).astype(f)
            seed = (wT[:, None] * dv).astype(f)
            wTs[k] = wT; mags[k] = mag; tanhs[k] = tterm
        if not grad:
            continue

        def reverse(lam, weights, policy_path):
            g_out = np.zeros((T, B, na))
            for t in range(T - 1, -1, -1):
                gu_c, gx_c = Bp._cost_grads(env, us[t], xs[t + 1], weights[t])          # of +w c
                G = (lam - gx_c).astype(f)
                dd = G * d.diff_std[:ns]
                hs = hs_all[t]
                for l in range(L - 1, -1, -1):
                    dd = dd @ d.Ws[l][k].T
                    if l > 0:
                        dd = dd * G0._act_deriv(d.acts[l - 1], hs[l])
                gxu = np.zeros((B, ns + na), f)
                gxu[:, d.n_drop:] = dd
                gxu = gxu / d.in_std
                gU = -gu_c + gxu[:, ns:]
                gm = np.where((araws[t] >= -1.0) & (araws[t] <= 1.0), gU, f(0.0)).astype(f)
                g_out[t] = gm * scale
                lam = (G + gxu[:, :ns]).astype(f)
                if closed and policy_path:
                    lam = (lam + _policy_vjp(Ws, ps_all[t], gm)).astype(f)
            return g_out, lam

        if mut == 'tv_no_policy_path' and closed:
            # the recursion is linear in (weights, seed): the seed's part on its own, without the policy's term
            ga, la = reverse(np.zeros((B, ns), f), ws, True)
            gb, lb = reverse(seed, [np.zeros_like(w) for w in ws], False)
            G_out[k], lam0[k] = ga + gb, la + lb
        else:
            G_out[k], lam0[k] = reverse(seed, ws, True)
    return dict(ret=ret, len=length, grad=G_out, lam0=lam0, act=acts, rew=rews, w=wts, wT=wTs, tv_mag=mags, tv_tanh=tanhs,
                sites={n: np.concatenate(v, axis=1) for n, v in sites.items()})
