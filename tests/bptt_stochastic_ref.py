"""Float64 restatement of the 'bptt-stochastic' policy update (model_based_rl.py:1188-1196) for the tests: the unrolled graph of
build_policy_graph (:106-151) with policy noise, u = clip(mean + eps * exp(log_std), -1, 1) (training.py:115-116, :128), differentiated by
torch autograd; and a NumPy restatement of the production draws (Philox4x32-10 + Box-Muller, csrc/device_common.h RNG_BPTT).

Anchored in tests/test_bptt_stochastic_ref.py: at eps = 0 it equals oracle/bptt_oracle.policy_costs_and_grad, and its log_std gradient
matches central finite differences."""
import numpy as np
import torch

RNG_BPTT = 4


def _policy_params(th, dims):
    Ws, bs, o = [], [], 0
    for i in range(len(dims) - 1):
        n = dims[i] * dims[i + 1]
        Ws.append(th[o:o + n].reshape(dims[i], dims[i + 1])); o += n
        bs.append(th[o:o + dims[i + 1]]); o += dims[i + 1]
    return Ws, bs, th[o:o + dims[-1]]


def _cost(env, u, xn):
    su2 = torch.sum(u * u, dim=1)
    if env == 'swimmer':
        return -(xn[:, 5] - 1e-2 * torch.mean(u * u, dim=1))
    if env == 'half_cheetah':
        inner = xn[:, 9] - 1e-1 * 0.5 * su2                      # tf.clip_by_value: gradient inside [min, max], bounds included
        keep = (inner >= -10) & (inner <= 10)
        return -torch.where(keep, inner, torch.clamp(inner, -10, 10).detach())
    if env == 'ant':
        return -(xn[:, 15] - 1e-2 * 0.5 * su2 + 0.05)
    if env == 'humanoid':
        return (xn[:, -1] - 1.5) ** 2 + 1e-2 * 1e-3 * su2
    if env == 'hopper':
        return -(xn[:, 5] - 0.01 * 0.5 * su2 - 10 * torch.clamp(0.45 - xn[:, 0], min=0) - 10 * torch.clamp(torch.abs(xn[:, 1]) - .2, min=0)
                 - torch.sum(torch.clamp(torch.abs(xn[:, 2:]) - 100, min=0), dim=1))
    if env == 'snake':
        return -(xn[:, 7] - 1e-2 * 0.5 * su2)
    raise KeyError(env)


def stochastic_costs_and_grad(dm, theta, dims, env, x0, T, gamma, eps):
    """-> (costs [K], grad [P] incl. the log_std slots, n_saturates [B, na] int) of mean_k costs[k] with the draws eps [K, T, B, na]."""
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    Ws, bs, log_std = _policy_params(th, dims)
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    in_mean, in_std, dmean, dstd = t64(dm.in_mean), t64(dm.in_std), t64(dm.diff_mean)[:dm.ns], t64(dm.diff_std)[:dm.ns]
    eps = t64(eps)
    B = x0.shape[0]
    nsat = np.zeros((B, dims[-1]), dtype=np.int64)
    costs = []
    for k in range(dm.K):
        x = t64(x0); cost = 0.0; dones = torch.zeros(B, dtype=torch.float64)
        for t in range(T):
            h = x
            for l in range(len(Ws) - 1):
                h = torch.tanh(h @ Ws[l] + bs[l])
            u_pre = h @ Ws[-1] + bs[-1] + eps[k, t] * torch.exp(log_std)
            inside = (u_pre >= -1.0) & (u_pre <= 1.0)                 # tf.clip_by_value passes the gradient at the bounds
            u = torch.where(inside, u_pre, torch.clamp(u_pre, -1.0, 1.0).detach())
            nsat += (torch.abs(u) == 1.0).numpy()
            z = ((torch.cat([x, u], dim=1) - in_mean) / in_std)[:, dm.n_drop:]
            for l in range(len(dm.Ws)):
                z = z @ t64(dm.Ws[l][k]) + t64(dm.bs[l][k])
                if l < len(dm.Ws) - 1:
                    z = {'relu': torch.relu, 'tanh': torch.tanh, 'identity': lambda v: v}[dm.acts[l]](z)
            xn = dmean + dstd * z + x
            c = _cost(env, u, xn)
            if env == 'ant':
                c = c * (1 - dones)
            cost = cost + (gamma ** t) * torch.mean(c)
            if env == 'ant':
                nd = (xn[:, 2] >= 0.2) & (xn[:, 2] <= 1.0) & torch.isfinite(xn).all(dim=1)
                dones = torch.maximum(dones, (~nd).to(torch.float64)).detach()
            x = xn
        costs.append(cost)
    total = torch.stack(costs).mean()
    total.backward()
    return np.array([float(c.detach()) for c in costs]), th.grad.numpy().copy(), nsat


# ---- production draws: Philox4x32-10 (Salmon et al. 2011) and the device's Box-Muller (normal4), restated in NumPy ----
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: 4 uint64 arrays holding 32-bit words; key: (k0, k1) ints.  Returns the 4 output words."""
    x, y, z, w = [np.asarray(c, dtype=np.uint64) for c in ctr]
    k0, k1 = np.uint64(key[0] & _MASK), np.uint64(key[1] & _MASK)
    m0, m1, mask = np.uint64(_M0), np.uint64(_M1), np.uint64(_MASK)
    for _ in range(10):
        p0, p1 = m0 * x, m1 * z
        x, y, z, w = (p1 >> np.uint64(32)) ^ y ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ w ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(_W0)) & mask, (k1 + np.uint64(_W1)) & mask
    return x, y, z, w


def bptt_noise(seed, K, T, B, na):
    """eps [K, T, B, na] of the documented mapping: the block with counter (b, i, t, RNG_BPTT << 16 | c), key = seed, gives the normals
    of action dims 4c .. 4c+3 of (model i, step t, env b) as r0 cos, r0 sin, r1 cos, r1 sin (r = sqrt(-2 ln u), u = (word + 1/2) 2^-32 in fp32)."""
    i, t, b = np.meshgrid(np.arange(K), np.arange(T), np.arange(B), indexing='ij')
    out = np.zeros((K, T, B, 4 * ((na + 3) // 4)))
    for c in range((na + 3) // 4):
        r = philox4x32_10((b.ravel(), i.ravel(), t.ravel(), np.full(b.size, (RNG_BPTT << 16) | c)), (seed & _MASK, (seed >> 32) & _MASK))
        u = [((np.asarray(v, dtype=np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)).astype(np.float64) for v in r]
        r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
        blk = np.stack([r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]), r1 * np.cos(2 * np.pi * u[3]), r1 * np.sin(2 * np.pi * u[3])], -1)
        out[..., 4 * c:4 * c + 4] = blk.reshape(K, T, B, 4)
    return out[..., :na]
