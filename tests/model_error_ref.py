"""NumPy restatement of the reference's model diagnostics, float64 arithmetic on the fp32 inputs the device stores:

  * evaluate_model_predictions, env_helpers.py:141-166 -- the loop over `timesteps`, restated line for line (the reference's line in the comment at
    the end of each statement);
  * get_error_distribution, env_helpers.py:214-233 -- the estimated-cost half (the real-simulator half :195-212 is the caller's data).

The policy and the model forward are oracle/metrpo_oracle.py's.  One rule is added to the reference's arithmetic, the library's (include/metrpo.h,
metrpo_model_error): a window stops serving a horizon once is_done fired at any step < h of its rollout -- only Ant can; the reference's diagnostic
never terminates, the library's rollout resets a finished env, so the state behind a done is no prediction.  `keep` carries the rule; with it all
True the arrays are the reference's.
"""
import numpy as np

from oracle import metrpo_oracle as O

STAT_KEYS = ('100%', '0%', '75%', '25%', '50%', 'avg', 'batch_size')      # env_helpers.py:112-129


def forward(dm, model, s, a):
    """dynamics_out of the call sites: avg_prediction = the mean over the heads (model_based_rl.py:626; model = -1), or training_models[model] (:638)."""
    if model < 0:
        return np.mean(O.dynamics_forward_all(dm, s, a), axis=0)
    return O.dynamics_forward(dm, model, s, a)


def horizon_errors(dm, theta, pdims, env, Os, Rs, timestep, model=-1, As=None, known_actions=False):
    """One pass of the loop body env_helpers.py:142-160 for `timestep`.  Os [n, T+1, ns], Rs [n, T], As [n, T, na] (recorded, unclipped).
    -> dict(state_diff [N, ns], cost_diff [N], keep [N] bool, pred [N, ns], step_costs [timestep, N], step_rewards [timestep, N], i, t)
    over ALL N = n (T + 1 - timestep) windows in the reference's order (trajectory-major)."""
    Os = np.asarray(Os, np.float64); Rs = np.asarray(Rs, np.float64)
    n, T1, n_states = Os.shape                                                            # :142
    max_timestep = T1 - 1
    assert Rs.shape == (n, max_timestep)                                                  # :139
    Xs = np.reshape(Os[:, :-timestep, :], (-1, n_states))                                 # :143
    Ys = np.reshape(Os[:, timestep:, :], (-1, n_states))                                  # :144
    costs = np.zeros(len(Xs))                                                             # :145
    rewards = np.zeros(len(Xs))                                                           # :146
    observations = Xs                                                                     # :147
    keep = np.ones(len(Xs), bool)
    step_costs, step_rewards = [], []
    for t in range(timestep):                                                             # :148
        if known_actions:
            actions = np.reshape(np.asarray(As, np.float64)[:, t:t + max_timestep + 1 - timestep], (-1, dm.na))    # :221, per window
        else:
            actions = O.policy_mean(theta, pdims, observations)                           # :149
        actions = np.clip(actions, -1.0, 1.0)                                             # :150 / :216
        with np.errstate(all='ignore'):
            next_observations = forward(dm, model, observations, actions)                 # :151-152
            c = O.cost_np_vec(env, observations, actions, next_observations)
        costs = costs + c                                                                 # :153
        r = np.reshape(Rs[:, t:t + max_timestep + 1 - timestep], -1)
        rewards = rewards + r                                                             # :154
        step_costs.append(c); step_rewards.append(r)
        keep &= ~np.asarray(O.is_done(env, next_observations, next_observations), bool)   # the library's rule: a done at a step < timestep
        observations = next_observations                                                  # :156
    with np.errstate(all='ignore'):
        state_diff = np.abs(Ys - observations)                                            # :159
        cost_diff = np.abs(costs + rewards)                                               # :160
    i, t = np.divmod(np.arange(len(Xs)), max_timestep + 1 - timestep)
    return dict(state_diff=state_diff, cost_diff=cost_diff, keep=keep, pred=observations, real=Ys, costs=costs, rewards=rewards,
                step_costs=np.array(step_costs), step_rewards=np.array(step_rewards), i=i, t=t)


def write_stats(d, data):
    """env_helpers.py:61-70."""
    for key, value in d.items():
        if '%' in key:
            value.append(np.percentile(data, int(key[:-1]), axis=0))
        elif key == 'avg':
            value.append(np.mean(data, axis=0))
        elif key == 'batch_size':
            value.append(len(data))
        else:
            assert False


def evaluate_model_predictions(dm, theta, pdims, env, Os, Rs, timesteps=(1, 3, 5, 7, 10, 12, 15, 18, 20, 100), model=-1, As=None,
                               known_actions=False):
    """env_helpers.py:108-166 without the csv files: the `errors` dict, statistics over the kept windows, plus `dropped` per horizon and the
    per-horizon arrays under 'per_h' (not in the reference's dict)."""
    errors = {'timesteps': timesteps, 'l2_sum': [], 'l1_sum': [], 'l1_state_cost': [],
              'state_diff': {k: [] for k in STAT_KEYS}, 'cost_diff': {k: [] for k in STAT_KEYS}, 'dropped': [], 'per_h': []}
    for timestep in timesteps:                                                            # :141
        e = horizon_errors(dm, theta, pdims, env, Os, Rs, timestep, model, As, known_actions)
        state_diff, cost_diff = e['state_diff'][e['keep']], e['cost_diff'][e['keep']]
        errors['l1_sum'].append(np.mean(np.sum(state_diff, axis=1)))                      # :162
        errors['l2_sum'].append(np.mean(np.sum(state_diff, axis=1)))                      # :163 (the reference fills l2_sum with l1_sum's expression)
        errors['l1_state_cost'].append(np.mean(state_diff[:, -1]))                        # :164
        write_stats(errors['state_diff'], state_diff)                                     # :165
        write_stats(errors['cost_diff'], cost_diff)                                       # :166
        errors['dropped'].append(int(np.sum(~e['keep'])))
        errors['per_h'].append(e)
    return errors


def get_error_distribution(dm, theta, pdims, env, initial_states, actions, real_costs, real_final_states, horizon, model=0, known_actions=False):
    """env_helpers.py:214-233.  actions [n, horizon, na] as recorded.  -> (e_cost, e_state, keep)."""
    o = np.asarray(initial_states, np.float64)                                            # :215
    actions = np.clip(np.asarray(actions, np.float64), -1, 1)                             # :216
    real_costs = np.asarray(real_costs, np.float64)
    estimated_costs = np.zeros_like(real_costs)                                           # :217
    keep = np.ones(len(o), bool)
    for t in range(horizon):                                                              # :218
        if known_actions:                                                                 # :220
            a = actions[:, t, :]                                                          # :221
        else:
            a = np.clip(O.policy_mean(theta, pdims, o), -1.0, 1.0)                        # :223-225
        with np.errstate(all='ignore'):
            o_next = forward(dm, model, o, a)                                             # :226-227
            estimated_costs = estimated_costs + O.cost_np_vec(env, o, a, o_next)          # :228
        keep &= ~np.asarray(O.is_done(env, o_next, o_next), bool)
        o = o_next                                                                        # :230
    e_cost = estimated_costs - real_costs                                                 # :232
    e_state = o - np.asarray(real_final_states, np.float64)                               # :233
    return e_cost, e_state, keep


# ---- shared synthetic "real" trajectories (tests only) ---------------------------------------------------------------------------------------------
def recorded_trajectories(dm, theta, pdims, env, pool, n, T, seed=0, noise=0.02):
    """Stand-in for sample_fixed_init_trajectories (env_helpers.py:132-137): n trajectories of T steps of a "real" system -- head 0 of the
    ensemble plus state noise, under the noisy policy -- rounded to fp32.  -> Os [n, T+1, ns], As [n, T, na] (unclipped), Rs [n, T]."""
    rng = np.random.RandomState(seed)
    s = np.asarray(pool[:n], np.float64).copy()
    Os, As, Rs = [s], [], []
    for t in range(T):
        a = O.policy_mean(theta, pdims, s) + 0.3 * rng.randn(n, dm.na)
        ac = np.clip(a, -1, 1)
        nxt = O.dynamics_forward(dm, 0, s, ac) + noise * rng.randn(n, dm.ns) * (np.arange(dm.ns) != 2 if env == 'ant' else 1.0)
        Rs.append(-O.cost_np_vec(env, s, ac, nxt)); As.append(a); Os.append(nxt)
        s = nxt
    f = lambda x: np.ascontiguousarray(np.asarray(x, np.float32))
    return f(np.stack(Os, 1)), f(np.stack(As, 1)), f(np.stack(Rs, 1))
