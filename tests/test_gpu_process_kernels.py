"""The process_samples kernels of process.hip against the float64 time-major restatement tests/process_ref.py, at every form the launch
rules dispatch to.  The entry points used here need no dynamics and no policy, so the widths the six envs do not have are reached with
Engine('humanoid', 1, (16, 16), (8, 8), ns=..., na=2) (humanoid's minimum state width is 1).

Dispatch table (process.hip; NS = the compile-time width, 0 = any width; case ids are the parametrize ids below):

  kernel / instantiation          launch rule (process.hip)                                    cases
  k_gae<NS,16> (10, 11, 14, 18)   :564 B <= 256 && T >= 128 && ns <= 18; with coefficients      b256_t128_every, params_swimmer, hopper_b100_t128,
                                  always pre_v (:567: nblk <= 4, T >= 16)                        hopper_b1_t200, snake_b128_t300, snake_b256_t129,
                                                                                                 cheetah_b17_t128, cheetah_params
  k_gae<NS,8> (10, 11, 14, 18)    :564 otherwise; no coefficients / pre_v (:567 nblk <= 32 &&    c1_swimmer, b257_t128, b256_t127_none, b2048_t16,
                                  T >= 16) / in-kernel predict (nblk > 32 or T < 16)             b2049_t16, b64_t15, hopper_b63_t5, hopper_b300_t40,
                                                                                                 hopper_b65_t16_none, snake_b2100_t20, snake_b500_t1,
                                                                                                 snake_b65_t64, cheetah_b257_t128, cheetah_b1000_t30,
                                                                                                 cheetah_b3000_t12
  k_gae<29,8>, k_gae<55,8>        :582 switch (ns), never wide; none / pre_v / in-kernel        c3_ant, ant_b2200_t16, ant_b63_t40_none, ant_b1_t5,
                                                                                                 c4_humanoid, c4_humanoid_straddle, humanoid_b2100_t8,
                                                                                                 humanoid_b65_t23_none
  k_gae<0,8>                      :582 default; in-kernel predict only while its staging fits   rt33_pre, rt56_kern, rt7_kern, rt40_none, rt57_pre,
                                  (:581: 4 * 8 * 64 * ns + 48 KB <= 160 KB, ns <= 56)            rt57_none; test_gae_runtime_width_too_wide (ns = 57)
  k_baseline_predict              :567 pre_v (coefficients, nblk <= 32, T >= 16)                 every *_pre / params / c3 / c4 case above
  k_gram_mfma<2>, <3>, <4>        :740-742 nfb = ceil((2 ns + 5) / 16) <= 2, 3, 4                g2_*, g3_*, g4_*
  k_gram_mfma_wide<5> ... <8>     :743-746 nfb = 5 (ns 30..37), 6 (38..45), 7 (46..53), 8       w5_*, w6_*, w7_*, w8_*
                                  (54..61); <5> and <6>: 15 / 21 block pairs over 4 waves
  k_gram                          :747 nfb >= 9 (ns >= 62)                                        gen62_*, gen69_*
  k_gram_final                    after every Gram kernel                                         every gram case
  k_baseline_solve_wave<FT>       :726 F = 24, 26, 32, 40, 62                                     test_solve_* ns 10, 11, 14, 18, 29
  k_baseline_solve                :727-731 other F while F (F + 1) + F doubles fit 160 KB        test_solve_* ns 33 (F 70), 55 (F 114), 69 (F 142);
                                  (F <= 142)                                                     test_solve_too_wide (F 144: unsupported)
  k_center                        launch_center: grid min(ceil(N / 256), 8 n_sm); grid-stride   center_* (N = 6 250 000 > 8 * 256 * 256)
  k_path_counts, k_stop_scan      launch_sampler_progress                                         test_sampler_progress_*

Bounds: GAE (adv, ret) within TOL.GAE_ULP fp32 ulp of the float64 scan (floor TOL.GAE_FLOOR x max |ref|), valid bit for bit, the count exact, the
sums within 1e-12 of sum |a| (sum a^2: relative); the normal equations under TOL.NORMAL_EQ; solve coefficients within F kappa u64 (norm-wise) of
np.linalg.solve and lstsq(rcond=-1) on SPD systems; centring under TOL.ADVANTAGE_CENTRED against the two-pass float64 centring; sampler counts and
stop steps exact.  Every kernel also repeats bit for bit and accumulates into a caller's buffer where the ABI says it accumulates.
profiles/r07_process_coverage.txt lists the kernels this module launches.
"""
import numpy as np
import pytest
import torch
import tolerances as TOL
import process_ref as R

U64 = np.finfo(np.float64).eps / 2
GL = [(1.0, 1.0), (0.99, 0.95), (0.995, 1.0), (0.9, 0.0)]
ENV_NS = (10, 11, 14, 18, 29, 55)


def cpu(t):
    return t.detach().cpu().numpy()


_ENG = {}


def engine(ns):
    import metrpo_amd
    if ns not in _ENG:
        _ENG[ns] = metrpo_amd.Engine('humanoid', 1, (16, 16), (8, 8), ns=ns, na=2)
    return _ENG[ns]


def gae_form(ns, B, T, coef):
    """launch_gae's choice (process.hip:564-582) -> (NS, NW, 'none' | 'pre_v' | 'kernel')."""
    wide = B <= 256 and T >= 128 and ns <= 18
    nblk = (B + 63) // 64
    mode = 'none' if not coef else ('pre_v' if (nblk <= 32 and T >= 16) else 'kernel')
    return (ns if ns in ENV_NS else 0), (16 if wide else 8), mode


# (id, ns, B, T, coefficients, done pattern, (gamma, lam) index, reward scale, t_offset)
GAE_CASES = [
    ('c1_swimmer', 10, 5000, 100, True, 'single', 1, 1.0, 0),
    ('params_swimmer', 10, 100, 500, True, 'straddle', 2, 1.0, 0),
    ('b256_t128_every', 10, 256, 128, False, 'every', 0, 1e3, 0),
    ('b257_t128', 10, 257, 128, True, 'ant', 3, 1e3, 0),
    ('b256_t127_none', 10, 256, 127, False, 'none', 1, 1.0, 0),
    ('b2048_t16', 10, 2048, 16, True, 'straddle', 1, 1.0, 50),
    ('b2049_t16', 10, 2049, 16, True, 'straddle', 1, 1.0, 50),
    ('b64_t15', 10, 64, 15, True, 't0', 0, 1.0, 0),
    ('hopper_b100_t128', 11, 100, 128, True, 'straddle', 1, 1e3, 300),
    ('hopper_b1_t200', 11, 1, 200, False, 'ant', 2, 1.0, 0),
    ('hopper_b63_t5', 11, 63, 5, True, 'every', 1, 1.0, 0),
    ('hopper_b300_t40', 11, 300, 40, True, 't0', 3, 1.0, 0),
    ('hopper_b65_t16_none', 11, 65, 16, False, 'straddle', 0, 1.0, 0),
    ('snake_b128_t300', 14, 128, 300, True, 'ant', 1, 1.0, 500),
    ('snake_b256_t129', 14, 256, 129, False, 'straddle', 2, 1e3, 0),
    ('snake_b2100_t20', 14, 2100, 20, True, 'ant', 1, 1.0, 0),
    ('snake_b500_t1', 14, 500, 1, False, 'every', 1, 1.0, 0),
    ('snake_b65_t64', 14, 65, 64, True, 'straddle', 3, 1e3, 0),
    ('cheetah_b17_t128', 18, 17, 128, False, 'single', 0, 1.0, 0),
    ('cheetah_params', 18, 100, 500, True, 'straddle', 1, 1.0, 0),
    ('cheetah_b257_t128', 18, 257, 128, False, 't0', 1, 1.0, 0),
    ('cheetah_b1000_t30', 18, 1000, 30, True, 'ant', 2, 1e3, 0),
    ('cheetah_b3000_t12', 18, 3000, 12, True, 'straddle', 1, 1.0, 0),
    ('c3_ant', 29, 300, 500, True, 'ant', 1, 1.0, 0),
    ('ant_b2200_t16', 29, 2200, 16, True, 'ant', 0, 1.0, 0),
    ('ant_b63_t40_none', 29, 63, 40, False, 'straddle', 3, 1.0, 0),
    ('ant_b1_t5', 29, 1, 5, True, 'every', 1, 1.0, 0),
    ('c4_humanoid', 55, 64, 1000, True, 'single', 1, 1.0, 0),
    ('c4_humanoid_straddle', 55, 65, 1000, True, 'straddle', 2, 1e3, 0),
    ('humanoid_b2100_t8', 55, 2100, 8, True, 'straddle', 1, 1.0, 0),
    ('humanoid_b65_t23_none', 55, 65, 23, False, 'ant', 0, 1.0, 0),
    ('rt33_pre', 33, 100, 50, True, 'straddle', 1, 1.0, 0),
    ('rt56_kern', 56, 130, 12, True, 't0', 2, 1.0, 0),
    ('rt7_kern', 7, 3000, 10, True, 'ant', 1, 1.0, 0),
    ('rt40_none', 40, 70, 33, False, 'straddle', 3, 1.0, 0),
    ('rt57_pre', 57, 100, 20, True, 'ant', 1, 1.0, 0),
    ('rt57_none', 57, 70, 9, False, 'every', 0, 1.0, 0),
]


def test_gae_cases_reach_every_dispatched_form():
    """The case table above reaches every cell the launch rule can produce (CPU: a restatement of the rule, not a launch)."""
    want = set()
    for NS in (10, 11, 14, 18):
        want |= {(NS, 16, 'none'), (NS, 16, 'pre_v'), (NS, 8, 'none'), (NS, 8, 'pre_v'), (NS, 8, 'kernel')}
    for NS in (29, 55, 0):
        want |= {(NS, 8, 'none'), (NS, 8, 'pre_v'), (NS, 8, 'kernel')}
    got = {gae_form(c[1], c[2], c[3], c[4]) for c in GAE_CASES}
    assert got == want, (sorted(want - got), sorted(got - want))
    assert {c[5] for c in GAE_CASES} == set(R.DONE_PATTERNS) and {c[6] for c in GAE_CASES} == set(range(len(GL)))
    # the boundaries of each rule sit on both sides
    shapes = {(c[2], c[3]) for c in GAE_CASES}
    assert {(256, 128), (257, 128), (256, 127), (2048, 16), (2049, 16), (64, 15)} <= shapes
    assert {1, 5} <= {c[3] for c in GAE_CASES} and {1, 63, 65} <= {c[2] for c in GAE_CASES}


def _traj(eng, obs, rew, done, tpath):
    from metrpo_amd.engine import Trajectory
    T, B, ns = obs.shape
    dev = eng.device
    return Trajectory(torch.as_tensor(obs, device=dev), torch.zeros(T, B, eng.na, device=dev), torch.as_tensor(rew, device=dev),
                      torch.zeros(T, B, eng.na, device=dev), torch.as_tensor(done, device=dev), torch.as_tensor(tpath, device=dev),
                      torch.zeros(B, ns, device=dev), B, T, 1)


def frac_of(got, ref, bound):
    """|got - ref| / bound element by element (a zero bound demands equality).  The call sites assert it <= 1 with assert_allclose against 0,
    atol 1, so that a METRPO_TOL_REPORT run records the fraction of each bound used, per call site."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))


def _ulp_bound(ref):
    ref = np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    return TOL.GAE_ULP * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + TOL.GAE_FLOOR * scale


def _gae_inputs(ns, B, T, coef, pattern, rscale, t_offset, nw, seed):
    rng = np.random.RandomState(seed)
    done, tpath = R.make_done(pattern, T, B, rng, nw=nw, t_offset=t_offset)
    obs = (rng.randn(T, B, ns) * 3.0).astype(np.float32)                   # some entries beyond the +-10 clip of the features
    obs[rng.rand(T, B, ns) < 0.02] *= 5.0
    rew = (rng.randn(T, B) * rscale).astype(np.float32)                     # mixed signs
    coeffs = rng.randn(2 * ns + 4) * 0.05 * rscale if coef else None
    return obs, rew, done, tpath, coeffs


@pytest.mark.gpu
@pytest.mark.parametrize('case', GAE_CASES, ids=[c[0] for c in GAE_CASES])
def test_gae_matches_float64_scan(case):
    cid, ns, B, T, coef, pattern, gi, rscale, t_off = case
    gamma, lam = GL[gi]
    NS, NW, mode = gae_form(ns, B, T, coef)
    obs, rew, done, tpath, coeffs = _gae_inputs(ns, B, T, coef, pattern, rscale, t_off, NW, seed=GAE_CASES.index(case))
    V = R.baseline_values(obs, tpath, coeffs) if coef else None
    ra, rr, rv = R.gae(rew, done, gamma, lam, V)
    eng = engine(ns)
    traj = _traj(eng, obs, rew, done, tpath)
    cd = torch.as_tensor(coeffs, dtype=torch.float64, device=eng.device) if coef else None
    adv, ret, valid, st = eng.gae(traj, cd, gamma, lam)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cpu(valid).astype(bool), rv)
    np.testing.assert_allclose(frac_of(cpu(adv), ra, _ulp_bound(ra)), 0.0, rtol=0, atol=1.0, err_msg='adv')
    np.testing.assert_allclose(frac_of(cpu(ret), rr, _ulp_bound(rr)), 0.0, rtol=0, atol=1.0, err_msg='ret')
    want = R.stats(ra, rv)
    s = cpu(st)
    assert s[2] == want[2] == rv.sum()
    np.testing.assert_allclose(s[0], want[0], rtol=0, atol=1e-12 * np.abs(ra[rv]).sum())
    np.testing.assert_allclose(s[1], want[1], rtol=1e-12, atol=0)
    if pattern == 'none':
        assert not rv.any() and (s == 0).all()
    # a second call: bit for bit the first, statistics ADDED to what the caller's buffer holds
    acc = torch.tensor([0.5, -1.25, 3.0], dtype=torch.float64, device=eng.device)
    a2, r2, v2, st2 = eng.gae(traj, cd, gamma, lam, stats=acc)
    torch.cuda.synchronize()
    assert st2 is acc and torch.equal(a2, adv) and torch.equal(r2, ret) and torch.equal(v2, valid)
    np.testing.assert_array_equal(cpu(acc), np.array([0.5, -1.25, 3.0]) + s)


@pytest.mark.gpu
def test_gae_runtime_width_too_wide():
    """k_gae<0,8>'s in-kernel predict stages 8 waves x 64 rows x ns floats: ns = 57 needs more than 160 KB with the kernel's own LDS -> the call
    reports METRPO_EUNSUPPORTED (the pre_v and no-coefficient forms of the same width run: cases rt57_pre, rt57_none)."""
    from metrpo_amd._lib import MetrpoError
    ns, B, T = 57, 70, 9
    assert gae_form(ns, B, T, True) == (0, 8, 'kernel')
    obs, rew, done, tpath, coeffs = _gae_inputs(ns, B, T, True, 'every', 1.0, 0, 8, seed=5)
    eng = engine(ns)
    with pytest.raises(MetrpoError, match='unsupported'):
        eng.gae(_traj(eng, obs, rew, done, tpath), torch.as_tensor(coeffs, device=eng.device), 0.99, 0.95)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------- Gram
# (id, ns, N, valid: 'null' | 'all' | 'tiles', largest path time)
GRAM_CASES = [
    ('g2_n1', 10, 1, 'all', 999), ('g2_n15', 10, 15, 'tiles', 999), ('g2_n2e6', 10, 2000003, 'tiles', 999),
    ('g3_n16', 14, 16, 'null', 500), ('g3_n17', 18, 17, 'tiles', 999),
    ('g4_n4099', 29, 4099, 'tiles', 999), ('g4_n70001', 29, 70001, 'null', 499),
    ('w5_n17', 33, 17, 'tiles', 999), ('w5_n70001', 33, 70001, 'tiles', 999),
    ('w6_n4099', 41, 4099, 'tiles', 999), ('w6_n70001', 41, 70001, 'null', 999),
    ('w7_n70001', 49, 70001, 'tiles', 999),
    ('w8_n1', 55, 1, 'all', 999), ('w8_n4099', 55, 4099, 'tiles', 999),
    ('gen62_n4099', 62, 4099, 'tiles', 999), ('gen69_n15', 69, 15, 'null', 999), ('gen69_n70001', 69, 70001, 'tiles', 999),
]


def gram_form(ns):
    nfb = (2 * ns + 4 + 1 + 15) // 16
    return ('mfma', max(nfb, 2)) if nfb <= 4 else (('wide', nfb) if nfb <= 8 else ('generic', nfb))


def test_gram_cases_reach_every_form():
    got = {gram_form(c[1]) for c in GRAM_CASES}
    assert got == {('mfma', 2), ('mfma', 3), ('mfma', 4), ('wide', 5), ('wide', 6), ('wide', 7), ('wide', 8), ('generic', 9)}
    assert {c[1] for c in GRAM_CASES if gram_form(c[1])[0] == 'generic'} == {62, 69}
    assert {1, 15, 16, 17, 4099, 70001} <= {c[2] for c in GRAM_CASES} and max(c[2] for c in GRAM_CASES) >= 2000000


def _gram_inputs(ns, N, vkind, tmax, seed):
    rng = np.random.RandomState(seed)
    obs = (rng.randn(N, ns) * 3.0).astype(np.float32)
    obs[rng.rand(N, ns) < 0.02] *= 6.0                                       # beyond the +-10 clip
    ret = (rng.randn(N) * 30.0 + 5.0).astype(np.float32)
    tpath = rng.randint(0, tmax + 1, size=N).astype(np.int32)
    tpath[:min(N, 4)] = tmax
    valid = None
    if vkind == 'all':
        valid = np.ones(N, np.uint8)
    elif vkind == 'tiles':
        valid = (rng.rand(N) >= 0.1).astype(np.uint8)
        nt = (N + 15) // 16
        for t in np.nonzero(rng.rand(nt) < 0.2)[0]:
            valid[16 * t:16 * t + 16] = 0                                   # whole invalid 16-sample tiles
        if N >= 4099:
            valid[128:128 + 64 * 3] = 0                                     # and whole 64-sample tiles of the generic kernel
        valid[-1] = 1
    return obs, ret, tpath, valid


@pytest.mark.gpu
@pytest.mark.parametrize('case', GRAM_CASES, ids=[c[0] for c in GRAM_CASES])
def test_gram_matches_float64_normal_equations(case):
    cid, ns, N, vkind, tmax = case
    obs, ret, tpath, valid = _gram_inputs(ns, N, vkind, tmax, seed=GRAM_CASES.index(case) + 100)
    G, b = R.normal_equations(obs, ret, tpath, valid)
    F = 2 * ns + 4
    eng = engine(ns)
    dev = eng.device
    args = (torch.as_tensor(obs, device=dev), torch.as_tensor(ret, device=dev), torch.as_tensor(tpath, device=dev),
            torch.as_tensor(valid, device=dev) if valid is not None else None)
    out = torch.zeros(F * F + F, dtype=torch.float64, device=dev)
    eng.baseline_gram(*args, out=out)
    torch.cuda.synchronize()
    g = cpu(out)
    AtA, Aty = g[:F * F].reshape(F, F), g[F * F:]
    d = np.sqrt(np.diag(G))
    np.testing.assert_allclose(frac_of(AtA, G, TOL.NORMAL_EQ * np.outer(d, d)), 0.0, rtol=0, atol=1.0, err_msg='AtA')
    y = ret.astype(np.float64) if valid is None else ret.astype(np.float64)[valid.astype(bool)]
    np.testing.assert_allclose(frac_of(Aty, b, TOL.NORMAL_EQ * d * np.sqrt(y @ y)), 0.0, rtol=0, atol=1.0, err_msg='Aty')
    assert np.array_equal(AtA, AtA.T)                                       # exactly symmetric (the solve assumes it)
    # accumulates into the caller's buffer, and a repeat is bit for bit
    base = np.random.RandomState(1).randn(F * F + F)
    base[:F * F] = (base[:F * F].reshape(F, F) + base[:F * F].reshape(F, F).T).reshape(-1)
    acc = torch.as_tensor(base, device=dev)
    eng.baseline_gram(*args, out=acc)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cpu(acc), base + g)
    again = torch.zeros_like(out)
    eng.baseline_gram(*args, out=again)
    torch.cuda.synchronize()
    assert torch.equal(again, out)


# ------------------------------------------------------------------------------------------------------------------------------- solve
SOLVE_NS = [10, 11, 14, 18, 29, 33, 55, 69]                                    # F = 24, 26, 32, 40, 62 (one wave); 70, 114, 142 (workgroup)


def _spd(F, kappa, rng):
    Q, _ = np.linalg.qr(rng.randn(F, F))
    s = 1e3 * kappa * np.logspace(0, -np.log10(kappa), F)                    # eigenvalues 1e3 ... 1e3 kappa: reg = 1e-5 barely moves them
    A = (Q * s) @ Q.T
    return 0.5 * (A + A.T)


def _solve(eng, A, b, reg):
    F = A.shape[0]
    gram = torch.tensor(np.concatenate([A.reshape(-1), b]), dtype=torch.float64, device=eng.device)
    x = cpu(eng.baseline_solve(gram, reg_coeff=reg))
    torch.cuda.synchronize()
    return x


@pytest.mark.gpu
@pytest.mark.parametrize('kappa', [1e2, 1e5, 1e8])
@pytest.mark.parametrize('ns', SOLVE_NS)
def test_solve_spd_coefficients(ns, kappa):
    """Well-conditioned SPD systems: the coefficients themselves against np.linalg.solve and against the reference's lstsq(rcond=-1), norm-wise
    within F kappa u64 (kappa = cond(A + reg I) of the case) -- elimination without pivoting is backward stable on SPD matrices."""
    F = 2 * ns + 4
    rng = np.random.RandomState(ns * 7 + int(np.log10(kappa)))
    A = _spd(F, kappa, rng)
    b = A @ rng.randn(F)
    reg = 1e-5
    Ar = A + reg * np.eye(F)
    k = np.linalg.cond(Ar)
    x = _solve(engine(ns), A, b, reg)
    bound = F * k * U64
    for want in (np.linalg.solve(Ar, b), np.linalg.lstsq(Ar, b, rcond=-1)[0]):
        np.testing.assert_allclose(np.linalg.norm(x - want) / np.linalg.norm(want), 0.0, rtol=0, atol=bound)


@pytest.mark.gpu
@pytest.mark.parametrize('ns', SOLVE_NS)
def test_solve_production_rank_deficient(ns):
    """A Gram of the shape every run starts from: all paths of one length (the time features repeat per path), a saturated and a duplicated
    observation column (exact null space, positive definite only through reg).  The predictions and the regularised residual against lstsq(-1)."""
    rng = np.random.RandomState(ns)
    H, npath = 40, 60
    obs = np.clip(rng.randn(H * npath, ns) * 2.0, -10, 10).astype(np.float32)
    obs[:, 1] = 0.75
    obs[:, ns - 1] = obs[:, 0]
    tpath = np.tile(np.arange(H), npath).astype(np.int32)
    Fm = R.features(obs, tpath)
    y = rng.randn(H * npath) * 3.0 + Fm[:, 0]
    A, b, reg = Fm.T @ Fm, Fm.T @ y, 1e-5
    F = A.shape[0]
    x = _solve(engine(ns), A, b, reg)
    want = np.linalg.lstsq(A + reg * np.eye(F), b, rcond=-1)[0]
    assert np.isfinite(x).all() and np.abs(x).max() <= 10.0 * max(1.0, np.abs(want).max())
    np.testing.assert_allclose(Fm @ x, Fm @ want, rtol=0, atol=1e-6 * max(1.0, np.abs(Fm @ want).max()))
    Ar = A + reg * np.eye(F)
    assert np.linalg.norm(Ar @ x - b) <= 1e-8 * max(1.0, np.linalg.norm(b)) + 1e-6 * np.linalg.norm(Ar @ want - b)


@pytest.mark.gpu
@pytest.mark.parametrize('ns', SOLVE_NS)
def test_solve_regulariser_escalation(ns):
    """An exactly singular A + reg I (pivot 0 is -reg + reg = 0.0): the first attempt fails, the second solves (A + 10 reg I) x = b."""
    F = 2 * ns + 4
    rng = np.random.RandomState(ns + 1)
    M = rng.randn(4 * F, F)
    A = M.T @ M / (4 * F)
    b = rng.randn(F)
    reg = 1e-5
    A[0, :] = 0.0; A[:, 0] = 0.0; A[0, 0] = -reg
    x = _solve(engine(ns), A, b, reg)
    want = np.linalg.solve(A + 10 * reg * np.eye(F), b)
    np.testing.assert_allclose(x, want, rtol=1e-7, atol=1e-9 * np.abs(want).max())


@pytest.mark.gpu
def test_solve_too_wide():
    """F = 144 (ns = 70): F (F + 1) + F doubles exceed 160 KB of LDS -> METRPO_EUNSUPPORTED (F = 142 runs: test_solve_* ns = 69)."""
    from metrpo_amd._lib import MetrpoError
    ns = 70
    F = 2 * ns + 4
    A = _spd(F, 10.0, np.random.RandomState(0))
    with pytest.raises(MetrpoError, match='unsupported'):
        _solve(engine(ns), A, np.ones(F), 1e-5)


# ------------------------------------------------------------------------------------------------------------------------------- centring
# (id, N, valid: None | 'mask' | 'none', data: 'normal' | 'const' | 'offset')
CENTER_CASES = [
    ('grid_stride_null', 6250000, None, 'normal'), ('grid_stride_masked', 6250000, 'mask', 'normal'),
    ('n_odd_masked', 1000003, 'mask', 'normal'), ('n77_null', 77, None, 'normal'),
    ('std0', 100003, 'mask', 'const'), ('mean_over_std_1e4', 2000001, 'mask', 'offset'), ('count0', 5003, 'none', 'normal'),
]


@pytest.mark.gpu
@pytest.mark.parametrize('case', CENTER_CASES, ids=[c[0] for c in CENTER_CASES])
def test_center_matches_two_pass(case):
    cid, N, vkind, data = case
    rng = np.random.RandomState(CENTER_CASES.index(case))
    if data == 'normal':
        adv = (rng.randn(N) * 2.0 + 0.3).astype(np.float32)
    elif data == 'const':
        adv = np.full(N, 0.3, np.float32)
    else:
        adv = (1e4 + rng.randn(N)).astype(np.float32)
    valid = None if vkind is None else ((rng.rand(N) >= 0.25) if vkind == 'mask' else np.zeros(N, bool)).astype(np.uint8)
    if data == 'const':
        adv[valid == 0] = rng.randn(int((valid == 0).sum())).astype(np.float32)     # only the valid samples are constant
    ref = R.center(adv, valid)
    st = R.stats(adv, np.ones(N, bool) if valid is None else valid)
    eng = engine(10)
    dev = eng.device
    a = torch.as_tensor(adv, device=dev)
    eng.center_advantages(a, torch.as_tensor(valid, device=dev) if valid is not None else None, torch.as_tensor(st, device=dev))
    torch.cuda.synchronize()
    got = cpu(a)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, **TOL.ADVANTAGE_CENTRED)
    if valid is not None:
        assert (got[valid == 0] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------- sampler progress
def _progress(eng, done, tpath, t0, batch, counts, state, stop):
    dev = eng.device
    eng.sampler_progress(torch.as_tensor(done, device=dev), torch.as_tensor(tpath, device=dev), t0, batch, counts, state, stop)
    torch.cuda.synchronize()


def _progress_buffers(eng, T):
    dev = eng.device
    return (torch.full((T,), -7.0, dtype=torch.float64, device=dev), torch.tensor([0.0, -1.0], dtype=torch.float64, device=dev),
            torch.zeros(1, dtype=torch.int32, device=dev))


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 300, 1000])
@pytest.mark.parametrize('how', ['exact', 'crossed', 'never'])
def test_sampler_progress_stop_step(B, how):
    """k_path_counts / k_stop_scan: per-step completed-path samples exactly, the first step whose running total reaches batch_size."""
    T = 40
    done, tpath = R.make_done('ant', T, B, np.random.RandomState(B), t_offset=30)
    done[T // 2] = 1                                                         # at least one completion
    tpath = tpath.copy()
    counts_ref = R.path_counts(done, tpath)
    cum = np.cumsum(counts_ref)
    t_star = int(np.nonzero(counts_ref > 0)[0][len(np.nonzero(counts_ref > 0)[0]) // 2])
    prev = cum[t_star - 1] if t_star > 0 else 0.0
    assert counts_ref[t_star] >= 2
    batch = int({'exact': cum[t_star], 'crossed': prev + 1, 'never': cum[-1] + 1}[how])     # crossed: the total jumps over batch_size at t_star
    ref_cum, ref_stop = R.stop_step(done, tpath, 0, batch)
    eng = engine(10)
    counts, state, stop = _progress_buffers(eng, T)
    _progress(eng, done, tpath, 0, batch, counts, state, stop)
    np.testing.assert_array_equal(cpu(counts), counts_ref)
    s = cpu(state)
    if how == 'never':
        assert ref_stop is None and int(cpu(stop)[0]) == 0 and s[1] == -1.0 and s[0] == cum[-1]
    else:
        assert ref_stop == t_star and int(cpu(stop)[0]) == 1 and s[1] == t_star and s[0] == ref_cum


@pytest.mark.gpu
def test_sampler_progress_carries_across_chunks_and_stops():
    """A 90-step rollout in chunks of 30 (t0 = 0, 30, 60): the running total carries in state[0], the stop step is global, and a chunk
    processed after the stop changes nothing (counts untouched, state unchanged)."""
    T, B, Tc = 90, 257, 30
    done, tpath = R.make_done('t0', T, B, np.random.RandomState(3))
    counts_ref = R.path_counts(done, tpath)
    cum = np.cumsum(counts_ref)
    t_star = 44                                                               # inside the second chunk
    batch = int(cum[t_star])
    assert cum[t_star - 1] < batch
    eng = engine(18)
    counts, state, stop = _progress_buffers(eng, Tc)
    _progress(eng, done[:Tc], tpath[:Tc], 0, batch, counts, state, stop)
    np.testing.assert_array_equal(cpu(counts), counts_ref[:Tc])
    assert int(cpu(stop)[0]) == 0 and cpu(state)[0] == cum[Tc - 1] and cpu(state)[1] == -1.0
    _progress(eng, done[Tc:2 * Tc], tpath[Tc:2 * Tc], Tc, batch, counts, state, stop)
    np.testing.assert_array_equal(cpu(counts), counts_ref[Tc:2 * Tc])
    assert int(cpu(stop)[0]) == 1 and cpu(state)[1] == t_star and cpu(state)[0] == cum[t_star]
    assert R.stop_step(done, tpath, 0, batch) == (cum[t_star], t_star)
    before = (cpu(counts).copy(), cpu(state).copy())
    _progress(eng, done[2 * Tc:], tpath[2 * Tc:], 2 * Tc, batch, counts, state, stop)     # after the stop: a no-op
    np.testing.assert_array_equal(cpu(counts), before[0])
    np.testing.assert_array_equal(cpu(state), before[1])
    assert int(cpu(stop)[0]) == 1
