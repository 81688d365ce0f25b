"""The float64 restatement tests/svg_ref.py against the reference's OWN svg_gradient (svg_utils.py:27-66): the fixture tests/golden/svg_swimmer.npz
was written by tests/golden/make_golden_svg.py, which imports the reference's module in place and calls it unmodified on callables built by
float64 autograd over the reference's policy_model, dynamics_model and cost_tf closures (n = 3 rollouts padded to T = 5, lengths 5, 3, 1;
gamma = 1 and 0.9)."""
import numpy as np

from conftest import load_golden, dm_from_golden
import svg_ref as R


def fixture():
    d = load_golden('svg_swimmer')
    return d, dm_from_golden(d, 'swimmer'), [int(x) for x in d['pdims']]


def test_restatement_matches_the_reference_svg_gradient():
    d, dm, pdims = fixture()
    assert d['obs'].shape == (3, 5, 10) and d['act'].shape == (3, 5, 2) and list(d['lengths']) == [5, 3, 1]
    for j, gamma in enumerate(d['gammas']):
        got = R.svg_gradient(dm, d['theta'], pdims, 'swimmer', d['obs'], d['act'], d['lengths'], model=0, gamma=float(gamma))
        want_t, want_s = d['grad_theta_%d' % j], d['grad_state_%d' % j]
        assert np.linalg.norm(want_t) > 0 and np.all(want_t[-pdims[-1]:] == 0.0)
        np.testing.assert_allclose(got['theta'], want_t, rtol=1e-9, atol=1e-9 * np.abs(want_t).max())
        np.testing.assert_allclose(got['state'], want_s, rtol=1e-9, atol=1e-9 * np.abs(want_s).max())
    assert not np.allclose(d['grad_theta_0'], d['grad_theta_1'], rtol=1e-3)        # gamma reaches the result


def test_padding_rows_of_the_fixture_are_never_read():
    d, dm, pdims = fixture()
    obs, act = d['obs'].copy(), d['act'].copy()
    for r, L in enumerate(d['lengths']):
        obs[r, L:], act[r, L:] = np.nan, np.nan
    got = R.svg_gradient(dm, d['theta'], pdims, 'swimmer', obs, act, d['lengths'])
    np.testing.assert_allclose(got['theta'], d['grad_theta_0'], rtol=1e-9, atol=1e-9 * np.abs(d['grad_theta_0']).max())
