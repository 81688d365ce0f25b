"""The 'svg' branch of the reference's optimize_policy, on the device: value gradients along RECORDED rollouts.

    svg_utils.py:27-66            svg_gradient: per rollout, t = L-1 ... 0, the state adjoint lambda and the parameter gradient through the
                                  Jacobians of cost, policy mean and dynamics head at the recorded (s_t, a_t); the mean over the rollouts
    svg_utils.py:12-25            svg_update: theta_vars += float32(-lr) * float32(avg_grads['theta']) on the W / b of the mean network
    model_based_rl.py:797-805     collect_data: rollout_data = one list of (o[t], a[t], o[t+1]) triplets per recorded trajectory
    model_based_rl.py:381-389     setup_gradients on head 'model0'; :654-660 the learning rate; :1204-1206 the branch (training cost 0.0)

The three sess.run calls per recorded step of the reference (ns + na + 1 tf.gradients graphs on one-row batches) are one call here:
metrpo_svg_grad / metrpo_svg_update (csrc/svg.hip) form every Jacobian of every step at once and scan each rollout in float64.

DIVERGENCE, stated: the reference's loop discards its own updates.  model_based_rl.py:1280-1282 breaks unconditionally after the first
validation round and log_and_restore (:1400) then restores the checkpoint saved at entry (:1127-1129), so as written an 'svg' run leaves the
policy unchanged.  early_stop.optimize_policy runs an SVG object through the 'bptt' branch's loop instead: one svg_update on the same
rollout_data per iteration, training cost 0.0 (:1206), validation every log_every iterations, keep-or-restore.

from_params / shapes_from_params keep refusing 'algo': 'svg' (a params file carries no recorded rollouts): build an SVG by hand, as an LBFGS.
Ant has no 'svg': its cost_tf takes a fourth argument (com_ant_env.py:70) and the reference's cost_tf(None, a_in, s_in) raises."""
import numpy as np
import torch


def rollout_triplets(Os, As):
    """collect_data's rollout_data (model_based_rl.py:797-805): Os[i] [L_i + 1, ns] observations, As[i] [>= L_i, na] actions of trajectory i ->
    one list of (o[t], a[t], o[t+1]) per trajectory, t < L_i."""
    rollout_data = []
    for o, a in zip(Os, As):
        o, a = np.asarray(o), np.asarray(a)
        rollout_data.append([(o[t], a[t], o[t + 1]) for t in range(len(o) - 1)])
    return rollout_data


def pack_rollouts(rollout_data, ns=None, na=None):
    """The reference's list of lists of (s_t, a_t, s_t+1) triplets -> (obs [n, T, ns], act [n, T, na] float32, zero-padded to the longest
    rollout; lengths [n] int32).  s_t+1 is not packed: svg_gradient never reads it.  Raises ValueError for no rollout, an empty rollout, or a
    triplet whose state / action size differs from the first one's (or from ns / na when given)."""
    n = len(rollout_data)
    if n < 1:
        raise ValueError("pack_rollouts: no rollout")
    lengths = np.array([len(r) for r in rollout_data], dtype=np.int32)
    if lengths.min() < 1:
        raise ValueError("pack_rollouts: rollout %d is empty (svg_gradient needs at least one triplet per rollout)" % int(np.argmin(lengths)))
    s0, a0 = np.asarray(rollout_data[0][0][0]), np.asarray(rollout_data[0][0][1])
    ns = int(s0.size) if ns is None else int(ns)
    na = int(a0.size) if na is None else int(na)
    T = int(lengths.max())
    obs = np.zeros((n, T, ns), dtype=np.float32)
    act = np.zeros((n, T, na), dtype=np.float32)
    for i, r in enumerate(rollout_data):
        for t, trip in enumerate(r):
            s, a = np.asarray(trip[0]).reshape(-1), np.asarray(trip[1]).reshape(-1)
            if s.size != ns or a.size != na:
                raise ValueError("pack_rollouts: rollout %d step %d has a state of %d and an action of %d entries, expected %d and %d"
                                 % (i, t, s.size, a.size, ns, na))
            obs[i, t], act[i, t] = s, a
    return obs, act, lengths


def check_lengths(lengths, n, T):
    """Host-side validation of a lengths vector for [n, T, .] tensors (the device clamps into [1, T] and would hide a wrong one)."""
    lengths = np.asarray(lengths)
    if lengths.shape != (n,) or not np.issubdtype(lengths.dtype, np.integer):
        raise ValueError("lengths: expected %d integers, got shape %s dtype %s" % (n, lengths.shape, lengths.dtype))
    if lengths.min() < 1 or lengths.max() > T:
        raise ValueError("lengths: every rollout needs 1 ... T = %d steps, got min %d max %d" % (T, int(lengths.min()), int(lengths.max())))
    return lengths.astype(np.int32)


class SVG(object):
    """svg_gradient / svg_update over the engine's policy and dynamics head `model` (the reference: 0).  learning_rate: svg_update's lr
    (model_based_rl.py:654-660); gamma: svg_gradient's (the reference never passes one: 1.0)."""

    needs_init_pool = False        # early_stop's 'bptt' loop: this branch draws no reset states, its batch is the recorded rollout_data

    def __init__(self, engine, learning_rate, model=0, gamma=1.0):
        if getattr(engine, 'env_name', None) == 'ant':
            raise ValueError("'svg' is not defined on Ant: its cost_tf takes a fourth argument (com_ant_env.py:70) and the reference's "
                             "cost_tf(None, a_in, s_in) raises")
        self.engine, self.learning_rate, self.model, self.gamma = engine, float(learning_rate), int(model), float(gamma)
        self.rollout_data = None
        self._packed = (None, None)

    def _pack(self, rollout_data):
        if self._packed[0] is not rollout_data:                 # one host pass and one upload per rollout_data, however many updates follow
            obs, act, lengths = pack_rollouts(rollout_data, self.engine.ns, self.engine.na)
            lengths = check_lengths(lengths, obs.shape[0], obs.shape[1])
            dev = self.engine.device
            self._packed = (rollout_data, (torch.as_tensor(obs, device=dev), torch.as_tensor(act, device=dev), torch.as_tensor(lengths, device=dev)))
        return self._packed[1]

    def svg_gradient(self, rollout_data):
        """-> {'theta': [P] float64 device tensor in get_policy's layout (log_std slots 0), 'state': [ns] float64} = the reference's avg_grads."""
        obs, act, lengths = self._pack(rollout_data)
        g = self.engine.svg_grad(obs, act, lengths, model=self.model, gamma=self.gamma)
        return {'theta': g['theta'], 'state': g['state']}

    def svg_update(self, rollout_data):
        """svg_update (svg_utils.py:12-25): the gradient and theta += float32(-lr) * float32(grad) on the engine's policy; -> grads['theta']."""
        obs, act, lengths = self._pack(rollout_data)
        return self.engine.svg_update(obs, act, self.learning_rate, lengths, model=self.model, gamma=self.gamma)['theta']

    def optimize_policy_iteration(self, _=None):
        """:1204-1206: one svg_update on self.rollout_data (set it first; early_stop.optimize_policy does); training cost 0.0 as the reference's."""
        if self.rollout_data is None:
            raise ValueError("SVG.optimize_policy_iteration: set rollout_data (collect_data's list of triplet lists) first")
        self.svg_update(self.rollout_data)
        return 0.0
