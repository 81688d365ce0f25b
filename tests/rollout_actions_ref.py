"""NumPy restatement of metrpo_rollout_actions (include/metrpo.h), float64 arithmetic on the fp32 inputs the device stores: the loop of
get_error_distribution(known_actions=True), env_helpers.py:216-222, kept step by step.

    actions = np.clip(actions, *bounds)                  # :216 (VecSimpleEnv.step does the same, :599)
    for t: o_next = dynamics(o, actions[t]); cost = cost_np_vec(o, actions[t], o_next); o = o_next       # :218-230

The ensemble forward is tests/model_error_ref.py's (the mean over the heads for model -1, the chosen head otherwise; here also a head per env,
eps_rand's cur_model_idx).  The restatement feeds its own state back and never resets: `done` is is_done(s', s') of every step, reported and ignored.
"""
import numpy as np

from oracle import metrpo_oracle as O
import model_error_ref as R


def forward(dm, model, s, a):
    """model: -1 (mean over the heads), a head, or an int array [B] with a head per env."""
    if np.ndim(model) == 0:
        return R.forward(dm, int(model), s, a)
    model = np.asarray(model)
    return O.dynamics_forward_all(dm, s, a)[model, np.arange(len(s))]


def rollout_actions(dm, env, init_obs, actions, model=-1):
    """init_obs [B, ns], actions [T, B, na] unclipped.  -> dict(obs [T+1, B, ns] with obs[0] = init_obs, rew [T, B], done [T, B] bool,
    clipped [T, B, na])."""
    s = np.asarray(init_obs, np.float64)
    a = np.clip(np.asarray(actions, np.float64), -1.0, 1.0)                               # :216
    T = a.shape[0]
    obs, rew, done = [s], [], []
    for t in range(T):                                                                    # :218
        with np.errstate(all='ignore'):
            nxt = forward(dm, model, s, a[t])                                             # :226-227
            rew.append(-O.cost_np_vec(env, s, a[t], nxt))                                 # :228 (reward = -cost, :601)
        done.append(np.asarray(O.is_done(env, nxt, nxt), bool))                           # :603
        obs.append(nxt)
        s = nxt                                                                           # :230 -- whatever `done` says
    return dict(obs=np.stack(obs), rew=np.stack(rew).reshape(T, -1), done=np.stack(done).reshape(T, -1), clipped=a)
