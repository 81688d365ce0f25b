"""The fused 2 x 32 policy-update kernels (csrc/policy_mfma.hip) reproduce, bit for bit, the outputs recorded in tests/golden/update_bits_gfx950.json
(tools/update_bits.py on an MI355X, with the library of the commit before the tile loops were made branch-free and unrolled over two input
buffers): gradient in both old-log_std forms with and without `valid`, FVP as a call of its own and inside a TRPO update's cached solve, loss / KL,
the VPG, PPO and PPO-KL heads (gate open and closed), and the VJP form through bptt_grad; every environment of update_cases.FUSED_ENVS at
N = 1, 17, 261, swimmer also at N = 300007.  "With `valid`" is valid[::7] = 0, and at N = 1 -- where that leaves nothing -- the one sample valid,
so that every size also goes through the `valid` pointer.  A change of those kernels that reorders no arithmetic keeps every hash; one that does has to say so
and regenerate the fixture.  The record is of gfx950 code: skipped on any other device."""
import json
import os
import sys

import pytest
import torch
import update_cases as U

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'update_bits_gfx950.json')
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tools'))


def _arch():
    return torch.cuda.get_device_properties(0).gcnArchName.split(':')[0] if torch.cuda.is_available() else None


@pytest.mark.parametrize('env', U.FUSED_ENVS)
def test_update_outputs_keep_their_bits(env):
    rec = json.load(open(FIXTURE))
    if _arch() != rec['arch']:
        pytest.skip('the recorded hashes are of %s code' % rec['arch'])
    import update_bits
    want = {k: v for k, v in rec['hashes'].items() if k.startswith(env + '/')}
    got = update_bits.env_hashes(env)
    assert sorted(got) == sorted(want)
    diff = sorted(k for k in want if got[k] != want[k])
    assert not diff, '%d of %d outputs changed: %s' % (len(diff), len(want), diff[:12])


def test_fixture_covers_the_issue_cases():
    rec = json.load(open(FIXTURE))
    keys = set(rec['hashes'])
    for env in U.FUSED_ENVS:
        for N in (1, 17, 261) + ((300007,) if env == 'swimmer' else ()):
            pre = '%s/N%d/' % (env, N)
            for m in ('none', 'seven' if N > 1 else 'ones'):
                for form in ('rows', 'bcast'):
                    for op in ('grad', 'losskl/old', 'losskl/trial', 'ppo', 'ppokl-open', 'ppokl-closed'):
                        assert pre + '%s/%s/%s' % (op, form, m) in keys
                for op in ('vpg', 'fvp', 'trpo/g', 'trpo/d', 'trpo/theta'):
                    assert pre + '%s/%s' % (op, m) in keys
        assert all('%s/vjp/B%d' % (env, b) in keys and rec['hashes']['%s/vjp/B%d/family' % (env, b)] == 'mfma' for b in (1, 5, 33))
