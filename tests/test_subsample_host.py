"""CPU tests of the host logic of subsampled Fisher-vector products (ConjugateGradientOptimizer(subsample_factor < 1), no GPU, no kernels):
argument validation, the draw, the params key, TRPO's pass-through, and -- with an injected evaluator that records which rows each call saw --
that gradient and line search see the whole batch while every product of the CG solve and the final Hx see the sub-batch."""
import json
import os

import numpy as np
import pytest
import torch
from oracle import metrpo_oracle as O
import metrpo_amd
from metrpo_amd.optimizer import ConjugateGradientOptimizer
from metrpo_amd.params import shapes_from_params
from test_host_logic import OracleEvaluator, make_update_problem
import subsample_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize('f', [0.0, -0.1, 1.0001, 2, float('nan')])
def test_subsample_factor_outside_unit_interval_raises(f):
    with pytest.raises(ValueError, match='subsample_factor'):
        ConjugateGradientOptimizer(subsample_factor=f)


def test_factor_one_is_accepted_and_draws_nothing():
    opt = ConjugateGradientOptimizer(subsample_factor=1.0)
    assert opt._subsample_factor == 1.0 and opt._gen is None


def test_empty_subsample_raises_naming_n_and_f():
    opt = ConjugateGradientOptimizer(subsample_factor=0.01)
    assert opt.subsample_size(100) == 1 and opt.subsample_size(250) == 2       # int(n * f), rllab's truncation
    with pytest.raises(ValueError) as e:
        opt.subsample_size(99)
    assert '99' in str(e.value) and '0.01' in str(e.value)


def test_draw_is_reproducible_from_seed_and_differs_by_rank_and_call():
    a, b = ConjugateGradientOptimizer(subsample_factor=0.25, seed=3), ConjugateGradientOptimizer(subsample_factor=0.25, seed=3)
    c = ConjugateGradientOptimizer(subsample_factor=0.25, seed=4)
    ia, ib, ic = a.draw_indices(1000), b.draw_indices(1000), c.draw_indices(1000)
    assert ia.dtype == torch.int32 and ia.numel() == 250 and torch.equal(ia, ib) and not torch.equal(ia, ic)
    assert len(set(ia.tolist())) == 250 and 0 <= int(ia.min()) and int(ia.max()) < 1000       # without replacement, inside the batch
    assert not torch.equal(a.draw_indices(1000), ia)                                           # one fresh draw per optimize() call
    assert torch.equal(a.draw_indices(1000), [b.draw_indices(1000), b.draw_indices(1000)][1])  # ... the same stream on both
    r1 = ConjugateGradientOptimizer(subsample_factor=0.25, seed=3).draw_indices(1000, rank=1)
    assert not torch.equal(r1, ia)


def test_params_key_default_and_value():
    p = json.load(open(os.path.join(HERE, 'golden', 'params_swimmer.json')))
    sh = shapes_from_params(p)
    assert sh['trpo_ext'] == dict(subsample_factor=1.0)
    assert sh['trpo'] == dict(step_size=0.01, discount=1.0, init_std=1.0, reset=True)          # the reference's keys are untouched
    p['policy_opt_params']['trpo']['subsample_factor'] = 0.1
    assert shapes_from_params(p)['trpo_ext'] == dict(subsample_factor=0.1)


class _Stub(object):
    vectorized = True
    engine = None


def test_trpo_forwards_optimizer_args():
    class NoSampler(object):
        def __init__(self, algo, **kw):
            pass
    algo = metrpo_amd.TRPO(env=None, policy=_Stub(), baseline=None, sampler_cls=NoSampler, step_size=0.02,
                           optimizer_args=dict(subsample_factor=0.2, seed=5, cg_iters=7))
    opt = algo.optimizer
    assert opt._subsample_factor == 0.2 and opt._seed == 5 and opt._cg_iters == 7 and opt._max_constraint_val == 0.02
    assert metrpo_amd.TRPO(env=None, policy=_Stub(), baseline=None, sampler_cls=NoSampler).optimizer._subsample_factor == 1.0


class RecordingEvaluator(OracleEvaluator):
    """OracleEvaluator that serves Hx from the rows it was told to subsample and writes down how many rows each call saw."""

    def __init__(self, *a):
        super(RecordingEvaluator, self).__init__(*a)
        self.seen, self.idx = [], None

    @property
    def n_samples(self):
        return len(self.d[0])

    def subsample(self, idx, comm=None):
        self.idx = np.asarray(idx).astype(np.int64)
        self.seen.append(('subsample', len(self.idx)))

    def loss_grad(self):
        self.seen.append(('loss_grad', len(self.d[0])))
        return super(RecordingEvaluator, self).loss_grad()

    def hvp(self, v):
        rows = self.d[0] if self.idx is None else self.d[0][self.idx]
        self.seen.append(('hvp', len(rows)))
        return torch.from_numpy(O.fisher_vector_product(self.theta, self.pdims, rows, np.asarray(v), reg_coeff=0.0))      # mean over the subsample

    def loss_constraint(self, theta):
        self.seen.append(('loss_constraint', len(self.d[0])))
        return super(RecordingEvaluator, self).loss_constraint(theta)


def test_host_loop_sends_only_the_products_to_the_sub_batch():
    theta, pdims, data = make_update_problem(N=400)
    N = len(data[0])
    ev = RecordingEvaluator(theta, pdims, data, N)
    opt = ConjugateGradientOptimizer(fused=False, subsample_factor=0.25, seed=1)
    opt.update_opt(leq_constraint=(None, 0.01))
    out = opt.optimize(ev)
    m = N // 4
    kinds = [k for k, _ in ev.seen]
    assert kinds[0] == 'subsample' and kinds.count('subsample') == 1 and ev.seen[0][1] == m        # one draw per call, before anything is evaluated
    assert kinds.count('loss_grad') == 1 and kinds.count('hvp') == 10 + 1                          # cg_iters products + the final Hx(descent_direction)
    assert all(n == m for k, n in ev.seen if k == 'hvp')
    assert all(n == N for k, n in ev.seen if k in ('loss_grad', 'loss_constraint'))
    assert kinds.count('loss_constraint') == out['n_backtrack'] + 1
    ref = R.cg_optimize_sub(theta, pdims, *data, idx=ev.idx)
    np.testing.assert_allclose(out['g'], ref['g'], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(out['d'], ref['d'], rtol=1e-9, atol=1e-12)
    assert abs(out['beta'] - ref['beta']) <= 1e-9 * ref['beta']
    assert out['n_backtrack'] == ref['n_backtrack'] and out['accepted'] == ref['accepted']
    full = O.cg_optimize(theta, pdims, *data, max_kl=0.01)
    assert np.linalg.norm(out['d'] - full['d']) > 1e-3 * np.linalg.norm(full['d'])                # it is not the whole-batch solve
    # subsample_indices overrides the draw (and works at subsample_factor = 1)
    ev2 = RecordingEvaluator(theta, pdims, data, N)
    opt2 = ConjugateGradientOptimizer(fused=False)
    opt2.update_opt(leq_constraint=(None, 0.01))
    out2 = opt2.optimize(ev2, subsample_indices=ev.idx)
    assert np.array_equal(ev2.idx, ev.idx) and np.array_equal(out2['d'], out['d'])


def test_factor_one_keeps_todays_host_path():
    theta, pdims, data = make_update_problem(N=300)
    ev = RecordingEvaluator(theta, pdims, data, len(data[0]))
    opt = ConjugateGradientOptimizer(fused=False, subsample_factor=1.0)
    opt.update_opt(leq_constraint=(None, 0.01))
    out = opt.optimize(ev)
    assert 'subsample' not in [k for k, _ in ev.seen]
    ref = O.cg_optimize(theta, pdims, *data, max_kl=0.01)
    np.testing.assert_allclose(out['d'], ref['d'], rtol=1e-9, atol=1e-12)


def test_evaluator_without_subsample_support_is_refused():
    theta, pdims, data = make_update_problem(N=300)
    opt = ConjugateGradientOptimizer(fused=False, subsample_factor=0.5)
    opt.update_opt(leq_constraint=(None, 0.01))
    with pytest.raises(TypeError, match='subsample'):
        opt.optimize(OracleEvaluator(theta, pdims, data, 300))


def test_reference_margin_rule():
    assert R.is_clear([(-0.05, 0.02), (-0.04, 0.008)], 0.0, 0.01)
    assert not R.is_clear([(-0.04, 0.00999)], 0.0, 0.01)            # accepted within the device's KL error of the bound
    assert not R.is_clear([(-0.05, 0.01001), (-0.04, 0.008)], 0.0, 0.01)


def test_clamp_is_in_the_kernel_source():
    """Code reading only (no out-of-range index goes to a device): the gather clamps an index into [0, N) before any row is read and raises the
    status cell the next status call reports."""
    src = open(os.path.join(ROOT, 'me-trpo_amd', 'csrc', 'subsample.hip')).read()
    body = src[src.index('__global__ void __launch_bounds__(SUB_ROWS) k_subsample'):]
    clamp, first_read = body.index('if (r < 0 || r >= k.N)'), body.index('k.valid[r]')
    assert clamp < first_read < body.index('gather_field(k.obs')
    assert 'r = (r < 0) ? 0 : k.N - 1;' in body and '*k.err = 1.0;' in body
    comm = open(os.path.join(ROOT, 'me-trpo_amd', 'csrc', 'comm.hip')).read()
    assert 'sub_err_cell(c)' in comm[comm.index('int32_t metrpo_comm_check'):]
