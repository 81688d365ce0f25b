"""NumPy restatement of the reference's svg_gradient / svg_update (svg_utils.py:12-66) on the oracle's dynamics ensemble and policy.
TEST INFRASTRUCTURE ONLY.

Per rollout of (s_t, a_t, s_t+1) triplets (s_t+1 is never read), lambda = 0, g_theta = 0, t = L-1 ... 0:

    c_s, c_a = d cost(x_next = s_t, u = a_t) / d (s_t, a_t)          the "current state cost" of svg_utils.py:123-125
    Pi_t     = d policy_mean(s_t) / d s_t   [na x ns]                raw mean net, no clip
    F_t      = d head_k([s_t, a_t]) / d [s_t, a_t]  [ns x (ns+na)]   normalisers, column drop, residual; a_t as recorded
    q_t      = c_a + gamma lambda F_t[:, ns:]
    g_theta  = q_t J_theta(s_t) + gamma g_theta
    lambda   = c_s + q_t Pi_t + gamma lambda F_t[:, :ns]

avg_grads = the mean over the rollouts.  `dtype` is the precision of the Jacobians F, Pi, of the cost adjoints and of the policy VJP;
the scan itself (lambda, q, gamma^t) is always float64 -- dtype = float32 is the form the device computes.  `wrong` names one deliberate
mistake (tests/test_svg_cases.py shows that each misses the GPU test's bound by far)."""
import numpy as np
from oracle import metrpo_oracle as O
from oracle.bptt_oracle import _cost_grads

WRONG = ('cost_at_next', 'clip_gate', 'gamma_t_plus_1', 'drop_last', 'divide_by_N')


def _act(name, z):
    return np.maximum(z, 0) if name == 'relu' else np.tanh(z) if name == 'tanh' else z


def _dact(name, h):
    """derivative of the activation, from its OUTPUT h"""
    return (h > 0).astype(h.dtype) if name == 'relu' else 1.0 - np.square(h) if name == 'tanh' else np.ones_like(h)


def dyn_jacobian(dm, k, s, a, dtype=np.float64):
    """F [L, ns, ns+na] of head k at the rows of s [L, ns], a [L, na]; also the hidden pre-activations (the relu kink sites)."""
    dm = dm.astype(dtype)
    s, a = s.astype(dtype), a.astype(dtype)
    ns, na, nd = dm.ns, dm.na, dm.n_drop
    h = ((np.concatenate([s, a], axis=1) - dm.in_mean) / dm.in_std)[:, nd:]
    hs, zs, L = [], [], len(dm.Ws)
    for l in range(L - 1):
        z = h @ dm.Ws[l][k] + dm.bs[l][k]
        h = _act(dm.acts[l], z)
        zs.append(z); hs.append(h)
    F = np.zeros((s.shape[0], ns, ns + na), dtype=dtype)
    for i in range(ns):
        d = np.broadcast_to(dm.diff_std[i] * dm.Ws[L - 1][k][:, i], (s.shape[0], dm.Ws[L - 1][k].shape[0])).copy()
        for l in range(L - 2, -1, -1):
            d = (d * _dact(dm.acts[l], hs[l])) @ dm.Ws[l][k].T
        F[:, i, nd:] = d / dm.in_std[nd:]
        F[:, i, i] += 1.0
    return F, zs


def pol_jacobian(theta, pdims, s, dtype=np.float64):
    """Pi [L, na, ns] of the tanh mean net at the rows of s; also the mean and the layer outputs (for the VJP)."""
    Ws, bs, _ = O.policy_unflatten(np.asarray(theta, dtype=dtype), pdims)
    mean, hs = O._policy_forward(Ws, bs, s.astype(dtype))
    na, ns = pdims[-1], pdims[0]
    Pi = np.zeros((s.shape[0], na, ns), dtype=dtype)
    for d_ in range(na):
        dh = np.broadcast_to(Ws[-1][:, d_], (s.shape[0], Ws[-1].shape[0])).copy()
        for l in range(len(Ws) - 2, -1, -1):
            dh = (dh * (1.0 - np.square(hs[l + 1]))) @ Ws[l].T
        Pi[:, d_, :] = dh
    return Pi, mean, (Ws, hs)


def cost_adjoints(env, s, a, dtype=np.float64):
    """(c_s [L, ns], c_a [L, na]) of cost(x_next = s, u = a)"""
    gu, gx = _cost_grads(env, a.astype(dtype), s.astype(dtype), np.ones(s.shape[0], dtype=dtype))
    return gx, gu


def svg_gradient(dm, theta, pdims, env, obs, act, lengths=None, model=0, gamma=1.0, dtype=np.float64, wrong=None, obs_next=None):
    """obs [n, T, ns], act [n, T, na], lengths [n] (None: T) -> dict(theta [P] with log_std slots 0, state [ns], mean_adj [n, T, na] = gamma^t q_t,
    dyn_jac [n, T, ns, ns+na], pol_jac [n, T, na, ns]); rows at or behind a length are zero and never read.  obs_next [n, T, ns]: s_t+1, read by
    wrong='cost_at_next' only."""
    assert wrong is None or wrong in WRONG
    n, T, ns = obs.shape
    na = act.shape[2]
    lengths = np.full(n, T, dtype=np.int64) if lengths is None else np.asarray(lengths)
    g_theta = np.zeros(O.policy_num_params(pdims))
    g_state = np.zeros(ns)
    GM = np.zeros((n, T, na)); Fo = np.zeros((n, T, ns, ns + na)); Po = np.zeros((n, T, na, ns))
    for r in range(n):
        Lr = int(lengths[r])
        s, a = obs[r, :Lr], act[r, :Lr]
        F, _ = dyn_jacobian(dm, model, s, a, dtype)
        Pi, mean, (Ws, hs) = pol_jacobian(theta, pdims, s, dtype)
        c_s, c_a = cost_adjoints(env, obs_next[r, :Lr] if wrong == 'cost_at_next' else s, a, dtype)
        F64, Pi64, c_s, c_a = F.astype(np.float64), Pi.astype(np.float64), c_s.astype(np.float64), c_a.astype(np.float64)
        lam = np.zeros(ns)
        q_all = np.zeros((Lr, na))
        for t in range(Lr - 1 - (1 if wrong == 'drop_last' else 0), -1, -1):
            q = c_a[t] + gamma * (lam @ F64[t][:, ns:])
            if wrong == 'clip_gate':
                q = q * ((mean[t] >= -1.0) & (mean[t] <= 1.0))
            lam = c_s[t] + q @ Pi64[t] + gamma * (lam @ F64[t][:, :ns])
            q_all[t] = (gamma ** (t + (1 if wrong == 'gamma_t_plus_1' else 0))) * q
        gm = q_all.astype(dtype)                                 # the mean adjoint the policy VJP reads
        gW, gb = O._backward(Ws, hs, gm)
        g_theta += O.policy_flatten([w.astype(np.float64) for w in gW], [b.astype(np.float64) for b in gb], np.zeros(na))
        g_state += lam
        GM[r, :Lr], Fo[r, :Lr], Po[r, :Lr] = gm, F, Pi
    den = float(lengths.sum()) if wrong == 'divide_by_N' else float(n)
    return dict(theta=g_theta / den, state=g_state / den, mean_adj=GM, dyn_jac=Fo, pol_jac=Po)


def svg_update(theta, grad_theta, lr):
    """svg_update (svg_utils.py:12-25): theta_vars += float32(-lr) * float32(grad) through assign_add on the W / b variables; the log_std slots of
    grad_theta are 0 and stay out (they are no theta_var).  float32 in, float32 out."""
    theta = np.asarray(theta, dtype=np.float32)
    step = np.float32(-lr) * np.asarray(grad_theta).astype(np.float32)          # (a zero slot adds -0.0: the bits of log_std stay)
    return (theta + step).astype(np.float32)
