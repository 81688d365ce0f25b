"""Wire / on-disk formats at the boundary of the inner loop, so that the accelerated loop can be driven by,
or compared against, artefacts of a reference run:

    new_rollouts_%d.pkl            pickle.dump((x_all, y_all))                                model_based_rl.py:810-811
    validation-init pickles        pickle of the list / array of reset states                 model_based_rl.py:444-487
    progress.csv                   rllab logger tabular output, one column per record_tabular  model_based_rl.py:590-733, 1037-1039, 1317-1320
    checkpoint names               policy-and-models-%d.ckpt, policy.ckpt, <scope>_<i>.ckpt    model_based_rl.py:728, 1128, 929

    policy-and-models-%d.ckpt      tf.train.Saver() of every global variable (:495-496, :728-729)   load/save_policy_and_models
    policy.ckpt                    the policy's trainable variables (:532, :1127-1129)               load/save_policy_checkpoint
    <scope>_<i>.ckpt               model i of the ensemble (:499-509, :927-930, recover_weights)     load/save_model_checkpoint
    params*.pkl                    joblib.dump of the rllab policy (training.py:378, 401; :549)      load_rllab_policy_pickle

The .ckpt bundles are read and written without TensorFlow by tf_checkpoint.py (tensor bundle V2; status there: format-spec-
pinned, reference-unpinned).  The rllab pickles are read without rllab by a restricted unpickler.  Dynamics / policy
parameters also cross the boundary as flat float32 vectors (`Engine.get_dynamics / get_policy`), stored as .npz with the TF
variable names of training.py:183-194 as keys."""
import csv
import math
import os
import pickle
import re
from collections import OrderedDict

import numpy as np

from . import tf_checkpoint

ROLLOUTS_FILE = 'new_rollouts_%d.pkl'                      # model_based_rl.py:810
POLICY_AND_MODELS_CKPT = 'policy-and-models-%d.ckpt'       # :728
POLICY_CKPT = 'policy.ckpt'                                # :1128
MODEL_CKPT = '%s_%d.ckpt'                                  # :929  (scope, model index)

# columns the outer loop records per iteration, in the order of the record_tabular calls
PROGRESS_COLUMNS_OUTER = ['collect_data_time', 'model_opt_time', 'policy_opt_time', 'MaxPolicyWeightDiff', 'MinPolicyWeightDiff',
                          'AvgPolicyWeightDiff', 'save_and_log_time', 'Time', 'ItrTime']


def progress_columns(model_scopes=('training_dynamics',), modes=('real', 'trpo_mean', 'estimated')):
    """All columns of one progress.csv row: outer loop (:590-733) + optimize_models (:1037-1039) + optimize_policy (:1317-1320)."""
    cols = ['collect_data_time', '# model updates'] + ['%s_min_sum_validation_loss' % s for s in model_scopes] + ['model_opt_time']
    cols += ['%s_policy_mean_min_validation_cost' % k for k in modes] + ['real_current_validation_cost', '# policy updates']
    cols += PROGRESS_COLUMNS_OUTER[2:]
    return cols


def save_rollouts(log_dir, count, x_all, y_all):
    """:809-811 -- x_all [n][ns+na] = (o_t, a_t), y_all [n][ns] = o_{t+1}."""
    path = os.path.join(log_dir, ROLLOUTS_FILE % count)
    with open(path, 'wb') as f:
        pickle.dump((np.asarray(x_all), np.asarray(y_all)), f)
    return path


def load_rollouts(path):
    with open(path, 'rb') as f:
        x_all, y_all = pickle.load(f)
    x_all, y_all = np.asarray(x_all), np.asarray(y_all)
    assert x_all.ndim == 2 and y_all.ndim == 2 and x_all.shape[0] == y_all.shape[0]
    return x_all, y_all


def save_validation_init(path, states):
    """:456-457 / :481-482 -- the reference pickles a python list of reset states (vip == vrip case) or an ndarray."""
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'wb') as f:
        pickle.dump(states, f)


def load_validation_init(path):
    """-> float32 [n][ns] array whatever container the reference pickled (:447-452)."""
    with open(path, 'rb') as f:
        v = pickle.load(f)
    return np.asarray(v, dtype=np.float32)


class TabularLog(object):
    """rllab logger's record_tabular / dump_tabular to progress.csv: header = keys of the first dumped row (insertion order),
    every later row must carry the same keys."""

    def __init__(self, path):
        self.path, self.row, self.header = path, OrderedDict(), None

    def record_tabular(self, key, val):
        self.row[str(key)] = val

    def dump_tabular(self):
        new = self.header is None
        if new:
            self.header = list(self.row.keys())
        assert list(self.row.keys()) == self.header, "progress.csv columns changed between iterations"
        with open(self.path, 'w' if new else 'a', newline='') as f:
            w = csv.DictWriter(f, fieldnames=self.header)
            if new:
                w.writeheader()
            w.writerow(self.row)
        self.row = OrderedDict()


def read_progress(path):
    """-> dict column -> float array (non-numeric cells become nan)."""
    with open(path, newline='') as f:
        rows = list(csv.DictReader(f))
    out = OrderedDict()
    for k in (rows[0].keys() if rows else []):
        col = []
        for r in rows:
            try:
                col.append(float(r[k]))
            except (TypeError, ValueError):
                col.append(np.nan)
        out[k] = np.array(col)
    return out


def dynamics_variable_names(n_layers, model):
    """TF variable names of one model's MLP (training.py:183-194): model%d/layer%d/weights, .../biases."""
    names = []
    for l in range(n_layers):
        names += ['model%d/layer%d/weights' % (model, l), 'model%d/layer%d/biases' % (model, l)]
    return names


def save_dynamics_npz(path, engine, input_rms=None, diff_rms=None, scope='training_dynamics'):
    """All K models AND the running normalisers under the reference's TF variable names -- the payload of the checkpoint the
    reference writes (model_based_rl.py:728; variables training.py:183-194 and running_mean_std.py:5-20):
        <scope>/model<k>/layer<l>/weights | biases,   input_rms/runningsum | runningsumsq | count,   diff_rms/...
    input_rms / diff_rms: dynamics_training.RunningMeanStd objects (their sums are what TF checkpoints hold); without them
    the file carries weights only and load_dynamics_npz needs the normalisers supplied."""
    flat = engine.get_dynamics().detach().cpu().numpy()
    dims = [engine.ns + engine.na - engine.n_drop] + list(engine.dyn_hidden) + [engine.ns]
    arrs, L = {}, len(dims) - 1
    for k in range(engine.K):
        o = 0
        for l in range(L):
            n = dims[l] * dims[l + 1]
            arrs['%s/model%d/layer%d/weights' % (scope, k, l)] = flat[k, o:o + n].reshape(dims[l], dims[l + 1]); o += n
            arrs['%s/model%d/layer%d/biases' % (scope, k, l)] = flat[k, o:o + dims[l + 1]]; o += dims[l + 1]
    for name, rms in (('input_rms', input_rms), ('diff_rms', diff_rms)):
        if rms is not None:
            arrs[name + '/runningsum'] = rms._sum.detach().cpu().numpy()
            arrs[name + '/runningsumsq'] = rms._sumsq.detach().cpu().numpy()
            arrs[name + '/count'] = np.array(rms._count, dtype=np.float64)
    np.savez(path, **arrs)


def rms_mean_std(rsum, rsumsq, count):
    """RunningMeanStd read-out (running_mean_std.py:22-27): mean = sum / count, std = sqrt(max(sumsq / count - mean^2, 1e-2)),
    in the dtype of the sums."""
    mean = rsum / count
    return mean, np.sqrt(np.maximum(rsumsq / count - mean * mean, 1e-2))


def _normalizer_stats(path, names, get, input_rms, diff_rms, used=None):
    """{'input_rms' | 'diff_rms': (mean, std)} from the stored running sums (restored into the given RunningMeanStd objects;
    mean = sum / count, std = sqrt(max(sumsq / count - mean^2, 1e-2)), running_mean_std.py:22-27), else from the given objects."""
    import torch
    stats = {}
    for name, rms in (('input_rms', input_rms), ('diff_rms', diff_rms)):
        keys = [name + '/runningsum', name + '/runningsumsq', name + '/count']
        if keys[0] in names:
            rsum, rsq, cnt = np.asarray(get(keys[0])), np.asarray(get(keys[1])), float(get(keys[2]))
            if used is not None:
                used.extend(keys)
            if rms is not None:
                if rsum.shape != tuple(rms._sum.shape) or rsq.shape != tuple(rms._sumsq.shape):
                    raise ValueError("%s: %s has shape %s, the RunningMeanStd holds %s" % (path, keys[0], rsum.shape, tuple(rms._sum.shape)))
                rms._sum.copy_(torch.as_tensor(rsum)); rms._sumsq.copy_(torch.as_tensor(rsq)); rms._count = cnt
            stats[name] = rms_mean_std(rsum, rsq, cnt)
        elif rms is not None:
            stats[name] = (rms.mean.cpu().numpy(), rms.std.cpu().numpy())
        else:
            raise KeyError("%s holds no %s statistics and none were supplied" % (path, name))
    return stats


def load_dynamics_npz(path, engine, input_rms=None, diff_rms=None, scope='training_dynamics'):
    """Inverse of save_dynamics_npz; works on a FRESH engine (one set_dynamics call with all K models and the normalisers).
    If the file holds the running sums they are restored into input_rms / diff_rms (when given) and mean/std (0.1 floor,
    running_mean_std.py:22-27) are derived from them; otherwise the given objects supply the normalisers."""
    import torch
    z = np.load(path)
    dims = [engine.ns + engine.na - engine.n_drop] + list(engine.dyn_hidden) + [engine.ns]
    L = len(dims) - 1
    pref = scope + '/' if ('%s/model0/layer0/weights' % scope) in z.files else ''      # files written before the scope prefix
    rows = []
    for k in range(engine.K):
        parts = []
        for l in range(L):
            parts += [z['%smodel%d/layer%d/weights' % (pref, k, l)].reshape(-1), z['%smodel%d/layer%d/biases' % (pref, k, l)].reshape(-1)]
        rows.append(np.concatenate(parts))
    stats = _normalizer_stats(path, z.files, z.__getitem__, input_rms, diff_rms)
    ns = engine.ns
    engine.set_dynamics(torch.as_tensor(np.stack(rows).astype(np.float32)), stats['input_rms'][0], stats['input_rms'][1],
                        stats['diff_rms'][0][:ns], stats['diff_rms'][1][:ns])


# ------------------------------------------------------------------------------------------------ TF checkpoints of the reference run
class OptimizerStateError(ValueError):
    """The Adam beta powers of a checkpoint do not describe one step count."""


def _dyn_dims(engine):
    return [engine.ns + engine.na - engine.n_drop] + list(engine.dyn_hidden) + [engine.ns]


def _dyn_tensors(scope, k, row, dims, suffix=''):
    """Model k's flat [dyn_param_count] row -> {<scope>/model<k>/layer<l>/weights (n_in, n_out) | biases (n_out,) + suffix}."""
    out, o = OrderedDict(), 0
    for l in range(len(dims) - 1):
        n = dims[l] * dims[l + 1]
        out['%s/model%d/layer%d/weights%s' % (scope, k, l, suffix)] = row[o:o + n].reshape(dims[l], dims[l + 1]); o += n
        out['%s/model%d/layer%d/biases%s' % (scope, k, l, suffix)] = row[o:o + dims[l + 1]]; o += dims[l + 1]
    return out


def _dyn_shapes(scope, k, dims):
    return [(n, (dims[l], dims[l + 1]) if n.endswith('weights') else (dims[l + 1],))
            for l in range(len(dims) - 1) for n in ('%s/model%d/layer%d/weights' % (scope, k, l), '%s/model%d/layer%d/biases' % (scope, k, l))]


def _policy_var_names(engine, policy_scope):
    """rllab GaussianMLPPolicy variables in get_param_values order (= the engine's theta order), with their shapes."""
    dims = engine.pol_dims
    out = []
    for l in range(len(dims) - 1):
        layer = 'hidden_%d' % l if l < len(dims) - 2 else 'output'
        out += [('%s/mean_network/%s/W' % (policy_scope, layer), (dims[l], dims[l + 1])),
                ('%s/mean_network/%s/b' % (policy_scope, layer), (dims[l + 1],))]
    out.append(('%s/output_std_param/param' % policy_scope, (engine.na,)))
    return out


def _match(names, regex, what):
    """The one name matching `regex`, None when none does; several matches are an error that lists them."""
    rx = re.compile(regex)
    hits = [n for n in names if rx.match(n)]
    if len(hits) > 1:
        raise KeyError("%s: %d variables match (%s)" % (what, len(hits), ', '.join(hits)))
    return hits[0] if hits else None


def _scope_rx(scope):
    return re.escape(scope) + r'(?:_\d+)?'                                  # TF uniquifies a reused scope as <scope>_1, ...


def _policy_var_rx(name, policy_scope):
    """Pattern (unanchored) of one policy variable: the scope may carry a _<n> suffix, the leaf too."""
    return _scope_rx(policy_scope) + '/' + re.escape(name[len(policy_scope) + 1:]) + r'(?:_\d+)?'


def _policy_rx(name, policy_scope):
    return '^' + _policy_var_rx(name, policy_scope) + '$'


def _slot_rx(opt_scope, var_rx, slot):
    return '^adam_' + _scope_rx(opt_scope) + '/(?:.*/)?' + var_rx + '/' + slot + '$'


def _beta_rx(opt_scope, which):
    return '^adam_' + _scope_rx(opt_scope) + '/(?:.*/)?beta%d_power(?:_\\d+)?$' % which


def _check_shape(path, name, arr, shape):
    if tuple(arr.shape) != tuple(shape):
        raise ValueError("%s: %s has shape %s, the engine expects %s" % (path, name, tuple(arr.shape), tuple(shape)))


def adam_step_from_powers(beta1_power, beta2_power, beta1=0.9, beta2=0.999, where=''):
    """Steps taken by a tf.train.AdamOptimizer from its beta powers.  TF creates beta1_power = beta1 and multiplies it by beta1
    after every step (adam.py _create_slots / _finish), so after t steps it holds beta1^(t+1): t = round(log_beta1(beta1_power)) - 1.
    beta2_power must agree; once beta1_power has underflowed float32 it is t that beta2_power alone gives."""
    b1p, b2p = float(beta1_power), float(beta2_power)
    if not (0.0 < b2p <= beta2 * (1 + 1e-6)) or not (0.0 <= b1p <= beta1 * (1 + 1e-6)):
        raise OptimizerStateError("%sbeta powers (%r, %r) are not powers of beta1 = %r, beta2 = %r" % (where, b1p, b2p, beta1, beta2))
    e2 = math.log(b2p) / math.log(beta2)
    if b1p < 1e-30:
        return int(round(e2)) - 1
    t = int(round(math.log(b1p) / math.log(beta1))) - 1
    if abs(e2 - (t + 1)) > 0.5:
        raise OptimizerStateError("%sbeta1_power = %r gives %d steps, beta2_power = %r gives %.2f" % (where, b1p, t, b2p, e2 - 1))
    return t


def _beta_powers(t, beta1, beta2):
    return np.float32(beta1 ** (t + 1)), np.float32(beta2 ** (t + 1))


def _load_adam(path, ck, used, missing, opt_scope, var_names, where, var_rx=re.escape):
    """-> (beta1_power name, beta2_power name, {var: (m slot name | None, v slot name | None)}) or None when the checkpoint holds
    no beta powers of adam_<opt_scope>."""
    names = list(ck)
    n1, n2 = _match(names, _beta_rx(opt_scope, 1), where + ' beta1_power'), _match(names, _beta_rx(opt_scope, 2), where + ' beta2_power')
    if n1 is None or n2 is None:
        missing.append('adam_%s/beta%d_power' % (opt_scope, 1 if n1 is None else 2))
        return None
    used += [n1, n2]
    return n1, n2, {v: (_match(names, _slot_rx(opt_scope, var_rx(v), 'Adam'), v + '/Adam'),
                        _match(names, _slot_rx(opt_scope, var_rx(v), 'Adam_1'), v + '/Adam_1')) for v in var_names}


def _report(ck, used, missing):
    u = set(used)
    return {'mapped': [n for n in ck if n in u], 'unmapped': [n for n in ck if n not in u], 'missing': list(missing)}


def _read_dyn_model(path, ck, used, scope, k, dims):
    parts = []
    for name, shape in _dyn_shapes(scope, k, dims):
        if name not in ck:
            raise KeyError("%s: no %s (variables of %s/model%d: %s)" % (path, name, scope, k, ', '.join(n for n in ck if n.startswith('%s/model%d/' % (scope, k))) or 'none'))
        _check_shape(path, name, ck[name], shape)
        parts.append(ck[name].astype(np.float32).reshape(-1)); used.append(name)
    return np.concatenate(parts)


def _read_policy(path, ck, used, engine, policy_scope):
    parts = []
    for name, shape in _policy_var_names(engine, policy_scope):
        hit = _match(ck, _policy_rx(name, policy_scope), name)
        if hit is None:
            raise KeyError("%s: no variable matches %s (variables under %s: %s)" % (path, name, policy_scope,
                           ', '.join(n for n in ck if n.startswith(policy_scope)) or 'none'))
        _check_shape(path, hit, ck[hit], shape)
        parts.append(ck[hit].astype(np.float32).reshape(-1)); used.append(hit)
    return np.concatenate(parts)


def _zeros_like_slots(path, ck, used, slots, shapes):
    """{var: (m, v)} resolved names -> flat float32 m, v in the variables' order; a slot TF never created reads as zeros."""
    ms, vs = [], []
    for var, shape in shapes:
        nm, nv = slots[var]
        for nme, out in ((nm, ms), (nv, vs)):
            if nme is None:
                out.append(np.zeros(int(np.prod(shape)), np.float32))
            else:
                _check_shape(path, nme, ck[nme], shape)
                out.append(ck[nme].astype(np.float32).reshape(-1)); used.append(nme)
    return np.concatenate(ms), np.concatenate(vs)


def load_policy_and_models(prefix, engine, input_rms=None, diff_rms=None, scope='training_dynamics', policy_scope='training_policy',
                           optimizer_state=True, beta1=0.9, beta2=0.999):
    """Restore what `saver.save(sess, policy-and-models-<n>.ckpt)` (model_based_rl.py:495-496, 728-729) holds onto a fresh or used
    engine: all K models, both RunningMeanStd triples (restored into input_rms / diff_rms when given), the policy and, with
    optimizer_state, the Adam state of the dynamics (adam_<scope>) and the BPTT policy (adam_<policy_scope>) optimizers.
    An optimizer whose beta powers are absent starts from zero state.  -> {mapped, unmapped, missing} lists of names."""
    ck = tf_checkpoint.read_checkpoint(prefix)
    path, used, missing = prefix, [], []
    dims = _dyn_dims(engine)
    rows = np.stack([_read_dyn_model(path, ck, used, scope, k, dims) for k in range(engine.K)])
    stats = _normalizer_stats(path, ck, ck.__getitem__, input_rms, diff_rms, used)
    for name in ('input_rms', 'diff_rms'):
        if name + '/runningsum' not in ck:
            missing.append(name + '/runningsum')
    theta = _read_policy(path, ck, used, engine, policy_scope)
    ns = engine.ns
    engine.set_dynamics(rows, stats['input_rms'][0], stats['input_rms'][1], stats['diff_rms'][0][:ns], stats['diff_rms'][1][:ns])
    engine.set_policy(theta)
    if optimizer_state:
        dvars = [ns_ for k in range(engine.K) for ns_ in _dyn_shapes(scope, k, dims)]
        got = _load_adam(path, ck, used, missing, scope, [n for n, _ in dvars], 'adam_%s' % scope)
        if got is None:
            engine.train_reset()
        else:
            n1, n2, slots = got
            t = adam_step_from_powers(ck[n1], ck[n2], beta1, beta2, '%s: adam_%s: ' % (path, scope))
            m, v = _zeros_like_slots(path, ck, used, slots, dvars)
            missing += [n + '/Adam' for n, _ in dvars if slots[n][0] is None] + [n + '/Adam_1' for n, _ in dvars if slots[n][1] is None]
            engine.set_train_adam(m.reshape(engine.K, -1), v.reshape(engine.K, -1), t)
        pvars = _policy_var_names(engine, policy_scope)
        got = _load_adam(path, ck, used, missing, policy_scope, [n for n, _ in pvars], 'adam_%s' % policy_scope,
                         lambda n: _policy_var_rx(n, policy_scope))
        if got is None:
            engine.policy_adam_reset()
        else:
            n1, n2, slots = got
            t = adam_step_from_powers(ck[n1], ck[n2], beta1, beta2, '%s: adam_%s: ' % (path, policy_scope))
            m, v = _zeros_like_slots(path, ck, used, slots, pvars)
            # output_std_param has no gradient in the BPTT graph, so TF creates no slot for it: not reported missing
            missing += [n + s for n, _ in pvars[:-1] for s, i in (('/Adam', 0), ('/Adam_1', 1)) if slots[n][i] is None]
            engine.set_policy_adam(m, v, t)
    return _report(ck, used, missing)


def _policy_tensors(engine, policy_scope, theta):
    out, o = OrderedDict(), 0
    for name, shape in _policy_var_names(engine, policy_scope):
        n = int(np.prod(shape))
        out[name] = theta[o:o + n].reshape(shape); o += n
    return out


def save_policy_and_models(log_dir, count, engine, input_rms, diff_rms, scope='training_dynamics', policy_scope='training_policy',
                           optimizer_state=True, beta1=0.9, beta2=0.999, block_size=262144):
    """Write log_dir/policy-and-models-<count>.ckpt under the reference's variable names (all float32, as TF holds them):
    <scope>/model<k>/layer<l>/{weights,biases}, {input_rms,diff_rms}/{runningsum,runningsumsq,count} (when the objects are
    given), <policy_scope>/mean_network/{hidden_<i>,output}/{W,b}, <policy_scope>/output_std_param/param and, with
    optimizer_state, adam_<scope>/<var>/Adam | Adam_1 + adam_<scope>/beta{1,2}_power for both optimizers (policy slots for the
    mean network only: TF creates none for output_std_param in the BPTT graph).  Returns the checkpoint prefix."""
    dims = _dyn_dims(engine)
    flat = engine.get_dynamics().detach().cpu().numpy()
    theta = engine.get_policy().detach().cpu().numpy()
    t = OrderedDict()
    for k in range(engine.K):
        t.update(_dyn_tensors(scope, k, flat[k], dims))
    for name, rms in (('input_rms', input_rms), ('diff_rms', diff_rms)):
        if rms is not None:
            t[name + '/runningsum'] = rms._sum.detach().cpu().numpy().astype(np.float32)
            t[name + '/runningsumsq'] = rms._sumsq.detach().cpu().numpy().astype(np.float32)
            t[name + '/count'] = np.array(rms._count, dtype=np.float32)
    pol = _policy_tensors(engine, policy_scope, theta)
    t.update(pol)
    if optimizer_state:
        m, v, step = (x.detach().cpu().numpy() if hasattr(x, 'detach') else x for x in engine.get_train_adam())
        for k in range(engine.K):
            for (name, a), (_, b) in zip(_dyn_tensors(scope, k, m[k], dims).items(), _dyn_tensors(scope, k, v[k], dims).items()):
                t['adam_%s/%s/Adam' % (scope, name)] = a; t['adam_%s/%s/Adam_1' % (scope, name)] = b
        t['adam_%s/beta1_power' % scope], t['adam_%s/beta2_power' % scope] = _beta_powers(step, beta1, beta2)
        m, v, step = (x.detach().cpu().numpy() if hasattr(x, 'detach') else x for x in engine.get_policy_adam())
        pm, pv = _policy_tensors(engine, policy_scope, m), _policy_tensors(engine, policy_scope, v)
        for name in list(pol)[:-1]:
            t['adam_%s/%s/Adam' % (policy_scope, name)] = pm[name]; t['adam_%s/%s/Adam_1' % (policy_scope, name)] = pv[name]
        t['adam_%s/beta1_power' % policy_scope], t['adam_%s/beta2_power' % policy_scope] = _beta_powers(step, beta1, beta2)
    prefix = os.path.join(log_dir, POLICY_AND_MODELS_CKPT % count)
    return tf_checkpoint.write_checkpoint(prefix, {n: np.asarray(a, dtype=np.float32) for n, a in t.items()}, block_size=block_size)


def save_policy_checkpoint(log_dir, engine, policy_scope='training_policy'):
    """log_dir/policy.ckpt: the policy's trainable variables (policy_saver, model_based_rl.py:532, 1127-1129)."""
    theta = engine.get_policy().detach().cpu().numpy()
    return tf_checkpoint.write_checkpoint(os.path.join(log_dir, POLICY_CKPT), _policy_tensors(engine, policy_scope, theta))


def load_policy_checkpoint(prefix, engine, policy_scope='training_policy'):
    """policy_saver.restore (model_based_rl.py:1400): the policy's trainable variables -> engine.set_policy."""
    ck = tf_checkpoint.read_checkpoint(prefix)
    used = []
    engine.set_policy(_read_policy(prefix, ck, used, engine, policy_scope))
    return _report(ck, used, [])


def save_model_checkpoint(log_dir, engine, k, scope='training_dynamics'):
    """log_dir/<scope>_<k>.ckpt: model k's weights (dynamics_savers[scope][k], model_based_rl.py:499-509, 927-930, 1002)."""
    if not 0 <= k < engine.K:
        raise ValueError("model index %d outside [0, %d)" % (k, engine.K))
    row = engine.get_dynamics()[k].detach().cpu().numpy()
    return tf_checkpoint.write_checkpoint(os.path.join(log_dir, MODEL_CKPT % (scope, k)), _dyn_tensors(scope, k, row, _dyn_dims(engine)))


def load_model_checkpoint(prefix, engine, k, scope='training_dynamics'):
    """recover_weights (model_based_rl.py:871-878): model k only, through metrpo_set_dynamics_model; the other models and the
    normalisers stay as they are (the engine's dynamics must have been set)."""
    if not 0 <= k < engine.K:
        raise ValueError("model index %d outside [0, %d)" % (k, engine.K))
    ck = tf_checkpoint.read_checkpoint(prefix)
    used = []
    engine.set_dynamics_model(k, _read_dyn_model(prefix, ck, used, scope, k, _dyn_dims(engine)))
    return _report(ck, used, [])


# ------------------------------------------------------------------------------------------------ rllab policy pickles
_PICKLE_ALLOWED = {
    ('numpy.core.multiarray', '_reconstruct'), ('numpy._core.multiarray', '_reconstruct'), ('numpy', 'ndarray'), ('numpy', 'dtype'),
    ('numpy.core.multiarray', 'scalar'), ('numpy._core.multiarray', 'scalar'), ('numpy.core.numeric', '_frombuffer'),
    ('numpy._core.numeric', '_frombuffer'),
    ('builtins', 'list'), ('builtins', 'dict'), ('builtins', 'tuple'), ('builtins', 'set'), ('builtins', 'frozenset'),
    ('builtins', 'object'), ('builtins', 'bytearray'), ('builtins', 'slice'), ('builtins', 'complex'), ('collections', 'OrderedDict'),
    ('copyreg', '_reconstructor'), ('_codecs', 'encode'),
}
_PICKLE_STUB_ROOTS = ('rllab.', 'sandbox.', 'tensorflow.')


class PickledStub(object):
    """Stands in for an rllab / sandbox / tensorflow object of a pickle: records constructor arguments and state, does nothing."""
    _pickled_name = None
    args, kwargs, state = (), {}, None                 # copyreg._reconstructor (protocol 0 / 1) bypasses __new__

    def __new__(cls, *args, **kwargs):
        obj = object.__new__(cls)
        obj.args, obj.kwargs, obj.state = args, kwargs, None
        return obj

    def __init__(self, *args, **kwargs):
        pass

    def __setstate__(self, state):
        self.state = state

    def __repr__(self):
        return '<pickled %s>' % self._pickled_name


_stub_classes = {}


def _stub(module, name):
    key = module + '.' + name
    if key not in _stub_classes:
        _stub_classes[key] = type(str(name), (PickledStub,), {'_pickled_name': key, '__module__': __name__})
    return _stub_classes[key]


# joblib's array container (joblib >= 0.10, what the reference's joblib 0.10.3 writes).  Its own read_array unpickles an
# object-dtype payload with a plain pickle.load, outside any find_class: the container is replaced by a subclass that reads
# such a payload through the restricted unpickler.  joblib <= 0.9's NDArrayWrapper (np.load of a side file the pickle names)
# is not accepted.
_JOBLIB_WRAPPER = ('joblib.numpy_pickle', 'NumpyArrayWrapper')
_safe_wrapper = []


def _safe_array_wrapper():
    if not _safe_wrapper:
        try:
            from joblib import numpy_pickle as jp
        except ImportError:
            raise pickle.UnpicklingError("the pickle holds joblib array containers: reading it needs joblib")

        class SafeNumpyArrayWrapper(jp.NumpyArrayWrapper):
            def read_array(self, unpickler, *args):
                if not isinstance(self.dtype, np.dtype) or self.subclass is not np.ndarray:
                    raise pickle.UnpicklingError("joblib array container with dtype %r / subclass %r refused" % (self.dtype, self.subclass))
                if not self.dtype.hasobject:
                    return super(SafeNumpyArrayWrapper, self).read_array(unpickler, *args)
                arr = _RestrictedUnpickler(unpickler.file_handle, encoding='latin1').load()
                if not isinstance(arr, np.ndarray):
                    raise pickle.UnpicklingError("joblib object-array payload is a %s, not an ndarray" % type(arr).__name__)
                return arr
        _safe_wrapper.append(SafeNumpyArrayWrapper)
    return _safe_wrapper[0]


def _restricted_find_class(module, name):
    if (module, name) == _JOBLIB_WRAPPER:
        return _safe_array_wrapper()
    if (module, name) in _PICKLE_ALLOWED:
        return getattr(__import__(module, fromlist=[name]), name)
    if (module + '.').startswith(_PICKLE_STUB_ROOTS):
        return _stub(module, name)
    raise pickle.UnpicklingError("refusing to load %s.%s from a policy pickle (only NumPy arrays, builtin containers and inert "
                                 "stand-ins for rllab / sandbox / tensorflow names are allowed)" % (module, name))


class _RestrictedUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        return _restricted_find_class(module, name)


def _unpickle(path):
    try:
        from joblib import numpy_pickle as jp
    except ImportError:
        jp = None
    with open(path, 'rb') as f:
        if jp is None:
            return _RestrictedUnpickler(f, encoding='latin1').load()

        class _JoblibRestricted(jp.NumpyUnpickler):
            def find_class(self, module, name):
                return _restricted_find_class(module, name)

        import inspect
        kw = {'ensure_native_byte_order': True} if 'ensure_native_byte_order' in inspect.signature(jp.NumpyUnpickler.__init__).parameters else {}
        opener = getattr(jp, '_read_fileobject', None)
        if opener is None:
            return _JoblibRestricted(path, f, **kw).load()
        with opener(f, path) as fobj:                          # joblib's compressed dumps are unwrapped here
            if isinstance(fobj, str):
                raise pickle.UnpicklingError("%s: a joblib cache directory entry, not a pickle" % path)
            up = _JoblibRestricted(path, fobj, **kw)
            up.encoding = 'latin1'                             # python-2 era numpy pickles
            return up.load()


def load_rllab_policy_pickle(path):
    """joblib.dump(training_policy, params*.pkl) (training.py:378, 401; model_based_rl.py:549) -> (theta float32, meta).
    rllab's Parameterized.__getstate__ stores {'__args', '__kwargs', 'params': get_param_values()}; theta is that flat vector,
    whose order is the engine's theta order (include/metrpo.h).  meta: hidden_sizes and init_std from __kwargs when present,
    plus the pickled class name.  Load it with GaussianMLPPolicy.set_param_values(theta) or engine.set_policy(theta)."""
    obj = _unpickle(path)
    state = obj.state if isinstance(obj, PickledStub) else obj
    if not isinstance(state, dict) or 'params' not in state:
        raise ValueError("%s: no rllab Parameterized state with a 'params' vector (got %s)" % (path, type(state).__name__))
    theta = np.asarray(state['params'], dtype=np.float32).reshape(-1)
    kwargs = state.get('__kwargs') or {}
    meta = {'class': getattr(obj, '_pickled_name', None)}
    if 'hidden_sizes' in kwargs:
        meta['hidden_sizes'] = tuple(int(h) for h in kwargs['hidden_sizes'])
    if 'init_std' in kwargs:
        meta['init_std'] = float(kwargs['init_std'])
    return theta, meta
