"""NumPy restatement of metrpo_score_actions_grad (include/metrpo.h): per head k and candidate b the gradient of the head's predicted discounted
RETURN with respect to the UNCLIPPED supplied actions and the start state.  Forward walk (tests/score_actions_ref.py's loop, with the tape kept),
then the reverse recursion of the header from lambda_T = 0:

    w_t      = gamma^t alive_t                      (gamma^t by repeated multiplication; the mask is a constant of the differentiation)
    G        = lambda_t+1 - w_t dc/dx_next
    gU       = -w_t dc/du + (action rows of F^T G)
    lambda_t = G + (state rows of F^T G)
    grad_t   = gU where -1 <= a_t <= 1, else 0       (tf.clip_by_value)

F^T G is oracle.bptt_oracle._dyn_vjp's chain written out here (diff_std, the layers with their activation derivatives, the column drop, 1/in_std, the
residual identity), so that a number format and a deliberate mistake can be put in; the cost derivatives are oracle.bptt_oracle._cost_grads.

`walk` runs in `dtype` throughout (float64: the reference; float32 beside it: the kink guard and the share of the bounds fp32 arithmetic alone uses)
and keeps the signed distance of every kink argument from its kink.  mut: one of the wrong restatements tests/test_score_grad_ref.py has the bounds
catch -- 'no_clip_gate', 'mask_first' (mask applied before the step's cost), 'no_residual', 'no_in_std', 'gamma_shift' (gamma^(t+1)), 'no_diff_std'.
"""
import numpy as np

from oracle import metrpo_oracle as O
from oracle import bptt_oracle as Bp
from score_actions_ref import start_rows

MUTS = ('no_clip_gate', 'mask_first', 'no_residual', 'no_in_std', 'gamma_shift', 'no_diff_std')


def _act_deriv(name, h):
    if name == 'relu':
        return (h > 0).astype(h.dtype)
    if name == 'tanh':
        return 1 - np.square(h)
    return np.ones_like(h)


def walk(dm, env, init_obs, actions, gamma=1.0, stop_at_done=True, dtype=np.float64, mut=None, grad=True):
    """init_obs [S, ns] or [ns], actions [T, B, na] unclipped.  -> dict(ret [K, B], len [K, B] int, grad [K, T, B, na], lam0 [K, B, ns] (float64
    arrays of `dtype` values), rew [K, T, B], w [K, T, B], sites: name -> [B, n] over all heads and steps)."""
    f = dtype
    assert mut is None or mut in MUTS
    d = dm.astype(f)
    araw = np.asarray(actions, f)
    a = np.clip(araw, f(-1.0), f(1.0))
    T, B = a.shape[:2]
    K, ns, na, L = d.K, d.ns, d.na, len(d.Ws)
    s0 = start_rows(init_obs, B).astype(f)
    ret = np.zeros((K, B)); length = np.zeros((K, B), np.int64)
    G_out = np.zeros((K, T, B, na)); lam0 = np.zeros((K, B, ns))
    rews = np.zeros((K, T, B)); wts = np.zeros((K, T, B))
    sites = {}

    def site(name, v):
        sites.setdefault(name, []).append(np.asarray(v, np.float64).reshape(B, -1))

    for t in range(T):
        site('clip', np.abs(araw[t]) - 1.0)
    for k in range(K):
        xs, hs_all, ws = [s0], [], []
        alive = np.ones(B, bool)
        disc = 1.0                                                       # float64 by repeated multiplication, rounded where it becomes a weight
        for t in range(T):
            x = xs[-1]
            h = ((np.concatenate([x, a[t]], axis=1) - d.in_mean) / d.in_std)[:, d.n_drop:]
            hs = [h]
            for l in range(L):
                h = h @ d.Ws[l][k] + d.bs[l][k]
                if l < L - 1:
                    if d.acts[l] == 'relu':
                        site('relu', h)
                    h = O._ACTS[d.acts[l]](h); hs.append(h)
            xn = (d.diff_mean[:ns] + d.diff_std[:ns] * h + x).astype(f)
            if env == 'half_cheetah':
                site('hc_inner', np.abs(xn[:, 9] - f(1e-1 * 0.5) * np.sum(np.square(a[t]), axis=1)) - 10.0)
            elif env == 'hopper':
                site('hopper_045', 0.45 - xn[:, 0]); site('hopper_02', np.abs(xn[:, 1]) - 0.2); site('hopper_100', np.abs(xn[:, 2:]) - 100.0)
            elif env == 'ant' and stop_at_done:
                site('ant_lo', xn[:, 2] - 0.2); site('ant_hi', 1.0 - xn[:, 2])
            with np.errstate(all='ignore'):
                r = -O.cost_np_vec(env, x, a[t], xn)
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
            xs.append(xn); hs_all.append(hs); ws.append(w)
            rews[k, t] = r; wts[k, t] = w
        if not grad:
            continue
        lam = np.zeros((B, ns), f)
        in_std = np.ones_like(d.in_std) if mut == 'no_in_std' else d.in_std
        for t in range(T - 1, -1, -1):
            gu_c, gx_c = Bp._cost_grads(env, a[t], xs[t + 1], ws[t])          # of +w c
            G = (lam - gx_c).astype(f)
            dd = G if mut == 'no_diff_std' else G * d.diff_std[:ns]
            hs = hs_all[t]
            for l in range(L - 1, -1, -1):
                dd = dd @ d.Ws[l][k].T
                if l > 0:
                    dd = dd * _act_deriv(d.acts[l - 1], hs[l])
            gxu = np.zeros((B, ns + na), f)
            gxu[:, d.n_drop:] = dd
            gxu = gxu / in_std
            gU = -gu_c + gxu[:, ns:]
            gate = np.ones_like(gU, bool) if mut == 'no_clip_gate' else (araw[t] >= -1.0) & (araw[t] <= 1.0)
            G_out[k, t] = np.where(gate, gU, 0.0)
            lam = ((0 if mut == 'no_residual' else G) + gxu[:, :ns]).astype(f)
        lam0[k] = lam
    return dict(ret=ret, len=length, grad=G_out, lam0=lam0, rew=rews, w=wts, sites={n: np.concatenate(v, axis=1) for n, v in sites.items()})


def score_actions_grad(dm, env, init_obs, actions, gamma=1.0, stop_at_done=True):
    """The float64 reference: dict(ret, len, grad, lam0, grad_mean [T, B, na], rew, w)."""
    out = walk(dm, env, init_obs, actions, gamma, stop_at_done)
    out['grad_mean'] = out['grad'].sum(axis=0) / dm.K
    return out
