#!/usr/bin/env python3
"""Golden vector for the 'svg' policy update, produced by the reference's OWN svg_gradient (svg_utils.py:27-66), imported in place and called
unmodified.

Build container only (reads the reference checkout; the .npz it writes is the committed fixture).  As in make_golden_tf.py, `tensorflow` is
tests/golden/tf_shim.py and the reference's closures policy_model (training.py:96-117), dynamics_model (:218-269) and the env's cost_tf come out
of training.train(variant) run up to its train_models call.

The shim has no tf.gradients, so setup_gradients (svg_utils.py:68-144) cannot run; the three callables svg_gradient is given are built here from
torch float64 autograd over those same closures, with setup_gradients' reductions (:81-121):
  cost_gradient(s, a)    gradients of cost_tf(None, a_in, s_in) w.r.t. [s_in, a_in]                          -> {'state' [1, ns], 'action' [1, na]}
  policy_gradient(s)     per action i, gradients of policy_out[:, i] w.r.t. [s_in] + theta_vars: np.sum(., axis=0) of the first, the rest
                         flattened and concatenated                                                           -> {'state' [na, ns], 'theta' [na, P']}
  model_gradient(s, a)   per state i, gradients of s_out[:, i] w.r.t. [s_in, a_in], each np.sum(., axis=0)  -> {'state' [ns, ns], 'action' [ns, na]}
theta_vars are get_policy_parameters' (svg_utils.py:7-10): the biases, then the weights, of the mean network; the fixture stores the result in
the flat order W0, b0, ..., Wout, bout, log_std (zeros).  The dynamics head is 'model0' (model_based_rl.py:382 passes variable_name '0', which
names no trained head; the models are 'model%d').

Usage:  python tests/golden/make_golden_svg.py        (from the repo root)"""
import sys
sys.dont_write_bytecode = True
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_tf as GT                                       # noqa: E402  (installs the shim, the stub finder and the reference imports)
import tf_shim                                                    # noqa: E402
import torch                                                      # noqa: E402
import svg_utils as ref_svg                                       # noqa: E402  the reference's module, unmodified
import utils as ref_utils                                         # noqa: E402

tf = GT.tf
MG = GT.MG


def main():
    env_name, K, dyn_hidden, pol_hidden = 'swimmer', 2, (16, 16), (8, 8)
    ns, na = GT.DIMS[env_name]
    tf.reset_default_graph()
    tf.get_default_session = tf_shim.get_default_session
    rng = np.random.RandomState(1234)
    cap = GT.capture_reference_closures(env_name, K, dyn_hidden, pol_hidden, 5, 1.0, 0.0, 10.0, 1234)
    dynamics_model, policy_model, cost_tf = cap['dynamics_model'], cap['policy_model'], cap['cost_tf']
    input_rms, diff_rms, params = cap['input_rms'], cap['diff_rms'], cap['params']
    sess = tf.get_default_session()
    scope, L = 'training_dynamics', len(dyn_hidden) + 1
    input_rms.update(rng.randn(150, ns + na) * rng.uniform(0.3, 2.0, size=ns + na) + rng.randn(ns + na) * 0.3)
    diff_rms.update(rng.randn(150, ns) * rng.uniform(0.05, 0.5, size=ns) + rng.randn(ns) * 0.02)
    in_mean, in_std = sess.run([input_rms.mean, input_rms.std])
    diff_mean, diff_std = sess.run([diff_rms.mean, diff_rms.std])
    probe = tf_shim._t(rng.randn(1, ns + na))
    for k in range(K):                                            # creates the heads' variables
        dynamics_model(probe, scope, 'model%d' % k)
    for v in tf.get_collection(tf.GraphKeys.TRAINABLE_VARIABLES, scope=scope + '/'):
        w = v.numpy() * (0.3 if '/layer%d/' % (L - 1) in v.name else 1.0)
        v.set(w.astype(np.float32).astype(np.float64))
    for v in tf.get_collection(tf.GraphKeys.TRAINABLE_VARIABLES, scope='training_policy'):
        if v.name.endswith('/b:0'):
            v.set(rng.randn(*v.tensor.shape) * 0.1)
        v.set(v.numpy().astype(np.float32).astype(np.float64))
    theta_vars = ref_utils.get_variables(scope='training_policy', filter='/b:')        # get_policy_parameters, svg_utils.py:7-10
    theta_vars.extend(ref_utils.get_variables(scope='training_policy', filter='/W:'))
    assert len(theta_vars) == 2 * (len(pol_hidden) + 1)

    def leaf(x):
        return tf_shim._t(np.asarray(x, dtype=np.float64)).clone().requires_grad_(True)

    def g(out, wrt):
        return [np.zeros(tuple(w.shape)) if r is None else r.detach().numpy().copy()
                for r, w in zip(torch.autograd.grad(out, wrt, allow_unused=True, retain_graph=True), wrt)]

    def cost_gradient(s, a):
        s_in, a_in = leaf(s), leaf(a)
        out = g(cost_tf(None, a_in, s_in), [s_in, a_in])          # "current state cost", svg_utils.py:123-125
        return dict(zip(['state', 'action'], out))

    def policy_gradient(s):
        s_in = leaf(s)
        policy_out = policy_model(s_in)
        wrt = [s_in] + [v.tensor for v in theta_vars]
        grads = [[], []]
        for i in range(na):
            out = g(policy_out[:, i].sum(), wrt)
            grads[0].append(np.sum(out[0], axis=0))
            grads[1].append(np.concatenate([np.reshape(t, [-1]) for t in out[1:]], axis=0))
        return dict(zip(['state', 'theta'], [np.array(x) for x in grads]))

    def model_gradient(s, a):
        s_in, a_in = leaf(s), leaf(a)
        s_out = dynamics_model(tf.concat([s_in, a_in], axis=1), scope, 'model0')
        grads = [[], []]
        for i in range(ns):
            out = g(s_out[:, i].sum(), [s_in, a_in])
            grads[0].append(np.sum(out[0], axis=0))
            grads[1].append(np.sum(out[1], axis=0))
        return dict(zip(['state', 'action'], [np.array(x) for x in grads]))

    # recorded rollouts: n = 3, padded to T = 5, ragged; float32-representable
    n, T, lens = 3, 5, [5, 3, 1]
    obs = (rng.randn(n, T + 1, ns) * 0.4).astype(np.float32).astype(np.float64)
    act = (rng.randn(n, T, na) * 0.8).astype(np.float32).astype(np.float64)
    rollouts = [[(obs[r, t], act[r, t], obs[r, t + 1]) for t in range(lens[r])] for r in range(n)]
    out = dict(env=np.array(env_name), K=np.array(K), dyn_hidden=np.array(dyn_hidden), pol_hidden=np.array(pol_hidden), dyn_act=np.array('relu'),
               pdims=np.array([ns] + list(pol_hidden) + [na]), in_mean=in_mean, in_std=in_std, diff_mean=diff_mean, diff_std=diff_std,
               n_drop=np.array(2 if params['dynamics_model'].get('ignore_xy_input') else 1 if params['dynamics_model'].get('ignore_x_input') else 0),
               theta=GT.policy_theta(), obs=obs[:, :T], act=act, lengths=np.array(lens, dtype=np.int32), gammas=np.array([1.0, 0.9]))
    out.update({k_: v_.astype(np.float32) for k_, v_ in GT.dyn_weights(scope, K, L).items()})
    names = [v.name[:-2] for v in theta_vars]
    sizes = [int(np.prod(v.tensor.shape)) for v in theta_vars]
    for j, gamma in enumerate(out['gammas']):
        avg = ref_svg.svg_gradient(rollouts, policy_gradient, model_gradient, cost_gradient) if gamma == 1.0 else \
            ref_svg.svg_gradient(rollouts, policy_gradient, model_gradient, cost_gradient, gamma=float(gamma))
        flat = np.squeeze(avg['theta'])
        by, o = {}, 0
        for nm, sz in zip(names, sizes):
            by[nm] = flat[o:o + sz]; o += sz
        hid = sorted([nm for nm in by if 'hidden_' in nm and nm.endswith('/W')], key=lambda s_: int(s_.split('hidden_')[1].split('/')[0]))
        parts = []
        for nm in hid:
            parts += [by[nm], by[nm[:-2] + '/b']]
        parts += [by['training_policy/mean_network/output/W'], by['training_policy/mean_network/output/b'], np.zeros(na)]
        out['grad_theta_%d' % j] = np.concatenate(parts)
        out['grad_state_%d' % j] = np.squeeze(avg['state'])
    MG.save('svg_swimmer', **out)


if __name__ == '__main__':
    main()
