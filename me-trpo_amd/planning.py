"""Planning by shooting through the learned ensemble: candidate action sequences are scored by every head in ONE device call
(Engine.score_actions / metrpo_score_actions) and the planner loop -- sample, score, top-k, refit -- is a few lines of torch on device tensors.
Nothing here reads a device tensor back inside a loop (no .item(), no .cpu()); the caller synchronises once, when it uses a result.

Every function takes `scorer=` in place of the engine's own: any callable (actions [T, B, na], init [S, ns]) -> ret [K, B] with candidate b starting
from init[b // (B // S)].  With a scorer the engine may be None and the logic runs on whatever device the states live on (then pass na=).

Layouts: states [S, ns]; a batch of candidates is [S, N, T, na] towards the caller (trajectory-major, as open_loop_predictions) and [T, S * N, na]
towards the device, candidate b = s * N + n.

First-order refinement (Grad-CEM / CEM-GD style): Engine.score_actions_grad / metrpo_score_actions_grad gives the gradient of every head's return with
respect to the candidates in one call; refine_actions runs projected gradient ascent on a batch of candidates with it, plan_cem_gd refines CEM's elites
(or all candidates) before each refit.  These take `grad_scorer=` as the others take `scorer=`: any callable
(actions [T, B, na], init [S, ns]) -> (ret [K, B], grad [K, T, B, na]).

The same in NOISE space around the policy: Engine.score_policy_actions_grad / metrpo_score_policy_actions_grad gives dR / d noise with the policy path
included; refine_noise is refine_actions there (projection clamp(+-noise_clip)), plan_cem_policy_gd refines plan_cem_policy's elites (or all) before
each refit, and ShootingController(policy_prior=True, noise_grad_steps=n) plans with it.

Structure: one loop, two spaces, optional refinement.  _cem is the CEM iteration, written once; plan_cem, plan_cem_gd, plan_cem_policy and
plan_cem_policy_gd check their arguments (_check_cem), resolve their scorers (_resolve, _resolve_pair), call it once and name the result.  The two spaces
differ in the clamp bound (1 / noise_clip), in the planted delta = 0 candidate and in the scorers; refinement is one _refine call before or behind the
top-k.  A batch of supplied candidates goes through _candidates (score_*_sequences, refine_*).

A value behind the horizon: Engine.set_terminal_value / metrpo_set_terminal_value adds gamma^T alive_T V(s_T) to every return above and seeds the
gradients to match.  The scorers are closures over the engine, so every planner here has it without a signature change: set it, plan, clear it.
baseline_terminal_value forms V from a LinearFeatureBaseline fit; ShootingController(terminal_value=baseline) does the setting and clearing.
The value's second form is a two-layer tanh net (Engine.set_terminal_value_mlp): ValueMLP holds and fits one, value_targets forms its fit targets, and
ShootingController(terminal_value=ValueMLP) plans with it."""
import numpy as np
import torch


def engine_scorer(engine, gamma=1.0, stop_at_done=True, force_generic=False):
    """The engine's own scorer: (actions [T, B, na], init [S, ns]) -> ret [K, B], one metrpo_score_actions call, nothing synchronised."""
    def scorer(actions, init):
        return engine.score_actions(init, actions, gamma=gamma, stop_at_done=stop_at_done, force_generic=force_generic)['ret']
    return scorer


def aggregate_heads(ret, aggregate='mean'):
    """ret [K, B] -> [B]: 'mean' over the heads, 'min' (the worst head), or ('pessimistic', beta): mean - beta * population std over the heads."""
    if isinstance(aggregate, str):
        if aggregate == 'mean':
            return ret.mean(dim=0)
        if aggregate == 'min':
            return ret.min(dim=0).values
        raise ValueError("aggregate: %r is none of 'mean', 'min', ('pessimistic', beta)" % (aggregate,))
    if isinstance(aggregate, (tuple, list)) and len(aggregate) == 2 and aggregate[0] == 'pessimistic':
        return ret.mean(dim=0) - float(aggregate[1]) * ret.std(dim=0, unbiased=False)
    raise ValueError("aggregate: %r is none of 'mean', 'min', ('pessimistic', beta)" % (aggregate,))


def engine_grad_scorer(engine, gamma=1.0, stop_at_done=True, force_generic=False):
    """The engine's own gradient scorer: (actions [T, B, na], init [S, ns]) -> (ret [K, B], grad [K, T, B, na]), one metrpo_score_actions_grad call,
    nothing synchronised."""
    def grad_scorer(actions, init):
        out = engine.score_actions_grad(init, actions, gamma=gamma, stop_at_done=stop_at_done, want=('grad', 'ret'), force_generic=force_generic)
        return out['ret'], out['grad']
    return grad_scorer


def aggregate_heads_grad(ret, grad, aggregate='mean'):
    """ret [K, B], grad [K, T, B, na] (grad[k] the gradient of ret[k]) -> [T, B, na]: the gradient of aggregate_heads(ret, aggregate) with respect to
    the candidates.  'mean': the head mean; 'min': the argmin head's gradient; ('pessimistic', beta): sum_k (1/K - beta (r_k - mean) / (K std)) g_k,
    the std term dropped where std = 0."""
    K = ret.shape[0]
    if isinstance(aggregate, str):
        if aggregate == 'mean':
            return grad.mean(dim=0)
        if aggregate == 'min':
            idx = ret.argmin(dim=0)
            return grad.gather(0, idx.view(1, 1, -1, 1).expand(1, grad.shape[1], grad.shape[2], grad.shape[3]))[0]
        raise ValueError("aggregate: %r is none of 'mean', 'min', ('pessimistic', beta)" % (aggregate,))
    if isinstance(aggregate, (tuple, list)) and len(aggregate) == 2 and aggregate[0] == 'pessimistic':
        dev = ret - ret.mean(dim=0, keepdim=True)
        sd = ret.std(dim=0, unbiased=False, keepdim=True)
        coef = 1.0 / K - float(aggregate[1]) * torch.where(sd > 0, dev / (K * torch.where(sd > 0, sd, torch.ones_like(sd))), torch.zeros_like(dev))
        return (coef.unsqueeze(1).unsqueeze(-1) * grad).sum(dim=0)
    raise ValueError("aggregate: %r is none of 'mean', 'min', ('pessimistic', beta)" % (aggregate,))


def _resolve(engine, given, factory, what, *args):
    """The scorer (what = 'scorer') or gradient scorer ('grad_scorer') a call uses: the one given, else factory(engine, *args)"""
    if given is not None:
        return given
    if engine is None:
        raise ValueError("an engine or a %s is needed" % what)
    return factory(engine, *args)


def _resolve_pair(engine, scorer, grad_scorer, factory, grad_factory, grad_steps, *args):
    """(scorer, grad_scorer) of a _gd planner.  No gradient scorer is built where none is used (grad_steps = 0 with an engine or a scorer); with neither
    scorer nor engine the scorer is the gradient scorer's first output."""
    derived = scorer is None and engine is None
    if grad_steps > 0 or derived:
        grad_scorer = _resolve(engine, grad_scorer, grad_factory, 'grad_scorer', *args)
    if derived:
        return (lambda a, init: grad_scorer(a, init)[0]), grad_scorer
    return _resolve(engine, scorer, factory, 'scorer', *args), grad_scorer


def _states(engine, states, na):
    """-> (states [S, ns] float32 contiguous on the engine's device, na): the engine's na, else the one passed"""
    dev = engine.device if engine is not None else None
    states = torch.as_tensor(states, device=dev).to(torch.float32)
    if states.dim() == 1:
        states = states.unsqueeze(0)
    ns = engine.ns if engine is not None else states.shape[-1]
    if states.dim() != 2 or states.shape[1] != ns or states.shape[0] < 1:
        raise ValueError("states: expected [S, %d] with S >= 1, got %s" % (ns, tuple(states.shape)))
    if engine is not None:
        na = engine.na
    if na is None or int(na) < 1:
        raise ValueError("na is needed when there is no engine")
    return states.contiguous(), int(na)


def _device_major(cand):
    """[S, N, T, na] -> [T, S * N, na], candidate b = s * N + n"""
    S, N, T, na = cand.shape
    return cand.permute(2, 0, 1, 3).reshape(T, S * N, na).contiguous()


def _from_device_major(x, S, N):
    """[T, S * N, na] -> [S, N, T, na]"""
    T, _, na = x.shape
    return x.reshape(T, S, N, na).permute(1, 2, 0, 3).contiguous()


def _candidates(engine, states, x, name):
    """Supplied candidates x (a tensor: [S, N, T, na], or [S, T, na] = one per state; `name` is the word for them in the message) with their states
    -> (states [S, ns], the candidates device-major [T, S * N, na], S, N, single: whether x was the 3-D form)"""
    states, na = _states(engine, states, x.shape[-1] if x.dim() >= 1 else None)
    cand = x.to(device=states.device, dtype=torch.float32)
    S = states.shape[0]
    single = cand.dim() == 3
    if single:
        cand = cand.unsqueeze(1)
    if cand.dim() != 4 or cand.shape[0] != S or cand.shape[3] != na or cand.shape[1] < 1 or cand.shape[2] < 1:
        raise ValueError("%s: expected [%d, N, T, %d] or [%d, T, %d], got %s" % (name, S, na, S, na, tuple(x.shape)))
    return states, _device_major(cand), S, cand.shape[1], single


def _score_candidates(engine, states, x, name, scorer, aggregate):
    """score_action_sequences / score_noise_sequences behind the scorer's resolution"""
    states, cand, S, N, single = _candidates(engine, states, x, name)
    scores = aggregate_heads(scorer(cand, states), aggregate).reshape(S, N)
    return scores[:, 0] if single else scores


def score_action_sequences(engine, states, actions, gamma=1.0, stop_at_done=True, aggregate='mean', scorer=None):
    """Score supplied action sequences: states [S, ns], actions [S, N, T, na] (N candidates per state) or [S, T, na] (one each), trajectory-major
    and unclipped (clipped on the device).  -> scores [S, N] (or [S]): the heads' discounted returns folded by `aggregate`.  A device tensor."""
    act = torch.as_tensor(actions)
    scorer = _resolve(engine, scorer, engine_scorer, 'scorer', gamma, stop_at_done)
    return _score_candidates(engine, states, act, 'actions', scorer, aggregate)


def _check_counts(horizon, n_candidates):
    if int(horizon) < 1 or int(n_candidates) < 1:
        raise ValueError("horizon and n_candidates must be positive, got %r and %r" % (horizon, n_candidates))
    return int(horizon), int(n_candidates)


def plan_random_shooting(engine, states, horizon, n_candidates, generator=None, gamma=1.0, stop_at_done=True, aggregate='mean', scorer=None, na=None):
    """Random shooting: per state, n_candidates sequences of `horizon` actions drawn uniformly from [-1, 1], scored in one call, the best taken.
    -> dict(actions [S, T, na] the best sequence, score [S] its score, scores [S, N] all of them), device tensors."""
    T, N = _check_counts(horizon, n_candidates)
    scorer = _resolve(engine, scorer, engine_scorer, 'scorer', gamma, stop_at_done)
    states, na = _states(engine, states, na)
    S, dev = states.shape[0], states.device
    cand = torch.rand(T, S, N, na, generator=generator, device=dev, dtype=torch.float32) * 2.0 - 1.0
    scores = aggregate_heads(scorer(cand.reshape(T, S * N, na), states), aggregate).reshape(S, N)
    score, best = scores.max(dim=1)
    idx = best.view(1, S, 1, 1).expand(T, S, 1, na)
    return dict(actions=cand.gather(2, idx)[:, :, 0].permute(1, 0, 2).contiguous(), score=score, scores=scores)


def _time_major_param(x, T, S, na, dev, name):
    """a scalar, [T, na] or [S, T, na] -> [T, S, 1, na]"""
    x = torch.as_tensor(x, device=dev, dtype=torch.float32)
    if x.dim() == 0:
        return x.expand(T, S, 1, na).clone()
    if tuple(x.shape) == (T, na):
        return x.view(T, 1, 1, na).expand(T, S, 1, na).clone()
    if tuple(x.shape) == (S, T, na):
        return x.permute(1, 0, 2).reshape(T, S, 1, na).clone()
    raise ValueError("%s: expected a scalar, [%d, %d] or [%d, %d, %d], got %s" % (name, T, na, S, T, na, tuple(x.shape)))


def _check_cem(horizon, n_candidates, n_elites, n_iters, alpha, grad_steps=0, grad_lr=0.05, optimizer='adam', refine='elites'):
    """The CEM family's argument check -> (T, N, E, n_iters, grad_steps) as ints.  The plain planners leave the refinement arguments at values that pass."""
    T, N = _check_counts(horizon, n_candidates)
    E, n_iters = int(n_elites), int(n_iters)
    grad_steps = _check_refine(grad_steps, grad_lr, optimizer)
    if refine not in ('elites', 'all'):
        raise ValueError("refine: %r is neither 'elites' nor 'all'" % (refine,))
    if not (1 <= E <= N):
        raise ValueError("n_elites must be in 1 ... n_candidates = %d, got %r" % (N, n_elites))
    if n_iters < 1:
        raise ValueError("n_iters must be positive, got %r" % (n_iters,))
    if not (0.0 <= float(alpha) < 1.0):
        raise ValueError("alpha must be in [0, 1), got %r" % (alpha,))
    return T, N, E, n_iters, grad_steps


def _cem(scorer, states, na, T, N, E, n_iters, init_mean, init_std, alpha, min_std, aggregate, generator, bound, plant_zero,
         grad_scorer=None, grad_steps=0, refine='elites', refine_args=()):
    """The CEM loop of the four planners, over candidates clamped to +-bound (1 for actions, noise_clip for noise around the policy).
    plant_zero: candidate 0 of every state is set to 0 in every iteration (plan_cem_policy's include_policy) and its DRAWN score in iteration 0 is kept.
    grad_steps > 0: _refine with refine_args = (lr, optimizer, betas, eps), on all candidates before the top-k (refine = 'all') or on the elites behind it.
    One randn(T, S, N, na) per iteration; nothing is read back.
    -> (mean [S, T, na], std [S, T, na], best [S, T, na], best_score [S], history [n_iters, S], elites [S, E], policy_score [S] or None)"""
    S, dev = states.shape[0], states.device
    mean = _time_major_param(0.0 if init_mean is None else init_mean, T, S, na, dev, 'init_mean')
    std = _time_major_param(init_std, T, S, na, dev, 'init_std')
    alpha, min_std = float(alpha), float(min_std)
    best_score = torch.full((S,), float('-inf'), device=dev, dtype=torch.float32)
    best = torch.zeros(T, S, na, device=dev, dtype=torch.float32)
    history = torch.empty(n_iters, S, device=dev, dtype=torch.float32)
    policy_score = None
    for it in range(n_iters):
        eps = torch.randn(T, S, N, na, generator=generator, device=dev, dtype=torch.float32)
        a = torch.clamp(mean + std * eps, -bound, bound)
        if plant_zero:
            a[:, :, 0] = 0.0                                                              # the policy itself rides along in every iteration
        if grad_steps > 0 and refine == 'all':
            ref_a, ref_s, _, _, first = _refine(grad_scorer, states, a.reshape(T, S * N, na), grad_steps, *refine_args, aggregate, bound)
            a, scores, drawn = ref_a.reshape(T, S, N, na), ref_s.reshape(S, N), first.reshape(S, N)
        else:
            scores = drawn = aggregate_heads(scorer(a.reshape(T, S * N, na), states), aggregate).reshape(S, N)
        if plant_zero and it == 0:
            policy_score = drawn[:, 0].clone()
        vals, idx = torch.topk(scores, E, dim=1)                                          # sorted: column 0 is the iteration's best
        elites = a.gather(2, idx.view(1, S, E, 1).expand(T, S, E, na))
        if grad_steps > 0 and refine == 'elites':
            ref_a, ref_s = _refine(grad_scorer, states, elites.reshape(T, S * E, na), grad_steps, *refine_args, aggregate, bound)[:2]
            vals, order = torch.topk(ref_s.reshape(S, E), E, dim=1)                       # sorted again: refinement may reorder the elites
            elites = ref_a.reshape(T, S, E, na).gather(2, order.view(1, S, E, 1).expand(T, S, E, na))
        elites = elites.double()
        e_mean = elites.sum(dim=2, keepdim=True) / E
        e_std = torch.sqrt(((elites - e_mean) ** 2).sum(dim=2, keepdim=True) / E)
        mean = alpha * mean + (1.0 - alpha) * e_mean.float()
        std = torch.clamp(alpha * std + (1.0 - alpha) * e_std.float(), min=min_std)
        better = vals[:, 0] > best_score
        best_score = torch.where(better, vals[:, 0], best_score)
        best = torch.where(better.view(1, S, 1), elites[:, :, 0].float(), best)
        history[it] = vals.mean(dim=1)
    tm = lambda x: x.permute(1, 0, 2).contiguous()
    return tm(mean[:, :, 0]), tm(std[:, :, 0]), tm(best), best_score, history, idx, policy_score


def plan_cem(engine, states, horizon, n_candidates, n_elites, n_iters, init_mean=None, init_std=1.0, alpha=0.0, min_std=0.0, gamma=1.0,
             aggregate='mean', generator=None, stop_at_done=True, scorer=None, na=None):
    """Cross-entropy method over action sequences, per state.  Each iteration: eps = randn(T, S, N, na); a = clip(mean + std * eps, -1, 1); one scoring
    call for all S * N candidates; the n_elites best per state (topk); elite mean and population std (ddof 0) of the CLIPPED elites, formed in float64
    and rounded to fp32; mean <- alpha * mean + (1 - alpha) * elite_mean, the same for std, floored at min_std.
    init_mean / init_std: a scalar, [T, na] or [S, T, na] (None: zeros).
    -> dict(actions [S, T, na] the final mean, std [S, T, na], best_actions [S, T, na] / best_score [S] the best candidate seen in any iteration,
    history [n_iters, S] the elites' mean score per iteration, elites [S, n_elites] the candidate indices of the LAST iteration's elites, best first),
    device tensors; nothing is read back."""
    T, N, E, n_iters, _ = _check_cem(horizon, n_candidates, n_elites, n_iters, alpha)
    scorer = _resolve(engine, scorer, engine_scorer, 'scorer', gamma, stop_at_done)
    states, na = _states(engine, states, na)
    mean, std, best, best_score, history, elites, _ = _cem(scorer, states, na, T, N, E, n_iters, init_mean, init_std, alpha, min_std, aggregate, generator,
                                                           bound=1.0, plant_zero=False)
    return dict(actions=mean, std=std, best_actions=best, best_score=best_score, history=history, elites=elites)


def _refine(grad_scorer, states, a, n_steps, lr, optimizer, betas, eps, aggregate, bound=1.0):
    """refine_actions on device-major candidates a [T, B, na] -> (best [T, B, na], best_score [B], last [T, B, na], last_score [B], first_score [B]).
    bound: the projection is clamp(-bound, bound) -- 1 for actions, noise_clip for noise around the policy (refine_noise)"""
    lr, b1, b2, eps, bound = float(lr), float(betas[0]), float(betas[1]), float(eps), float(bound)
    m = v = None
    best = best_score = first_score = None
    for it in range(n_steps + 1):
        ret, grad = grad_scorer(a, states)
        score = aggregate_heads(ret, aggregate)
        if it == 0:
            best, best_score, first_score = a, score, score
        else:
            better = score > best_score
            best_score = torch.where(better, score, best_score)
            best = torch.where(better.view(1, -1, 1), a, best)
        if it == n_steps:
            break
        g = aggregate_heads_grad(ret, grad, aggregate)
        if optimizer == 'sgd':
            step = lr * g
        else:                                                                             # Adam, ascent: written out in torch ops
            m = (1.0 - b1) * g if m is None else b1 * m + (1.0 - b1) * g
            v = (1.0 - b2) * g * g if v is None else b2 * v + (1.0 - b2) * g * g
            step = lr * (m / (1.0 - b1 ** (it + 1))) / (torch.sqrt(v / (1.0 - b2 ** (it + 1))) + eps)
        a = torch.clamp(a + step, -bound, bound)
    return best, best_score, a, score, first_score


def _check_refine(n_steps, lr, optimizer):
    if int(n_steps) < 0:
        raise ValueError("n_steps must not be negative, got %r" % (n_steps,))
    if not (float(lr) > 0.0 and np.isfinite(float(lr))):
        raise ValueError("lr must be positive and finite, got %r" % (lr,))
    if optimizer not in ('adam', 'sgd'):
        raise ValueError("optimizer: %r is neither 'adam' nor 'sgd'" % (optimizer,))
    return int(n_steps)


def _check_noise_clip(noise_clip):
    noise_clip = float(noise_clip)
    if not (noise_clip > 0.0 and np.isfinite(noise_clip)):
        raise ValueError("noise_clip must be positive and finite, got %r" % (noise_clip,))
    return noise_clip


def _refine_candidates(engine, states, x, name, grad_scorer, n_steps, lr, optimizer, betas, eps, aggregate, bound):
    """refine_actions / refine_noise behind their checks: _refine on supplied candidates (_candidates' x and name) -> the result dict, its first key `name`"""
    states, cand, S, N, single = _candidates(engine, states, x, name)
    best, best_score, last, last_score, first = _refine(grad_scorer, states, cand, n_steps, lr, optimizer, betas, eps, aggregate, bound)
    res = {name: _from_device_major(best, S, N), 'score': best_score.reshape(S, N), 'last': _from_device_major(last, S, N),
           'last_score': last_score.reshape(S, N), 'initial_score': first.reshape(S, N)}
    return {k: v[:, 0] for k, v in res.items()} if single else res


def refine_actions(engine, states, actions, n_steps, lr, optimizer='adam', betas=(0.9, 0.999), eps=1e-8, gamma=1.0, stop_at_done=True, aggregate='mean',
                   grad_scorer=None):
    """Projected gradient ASCENT on candidate action sequences: states [S, ns], actions [S, N, T, na] (or [S, T, na]: one each).  n_steps times
    a <- clip(a + step, -1, 1) with step = lr * g ('sgd') or Adam's lr * m_hat / (sqrt(v_hat) + eps) ('adam', moments per candidate entry), g =
    aggregate_heads_grad of one gradient call; n_steps + 1 calls in all (the last iterate is scored too).  Keep-best: `actions` / `score` are the
    best-scoring iterate seen per candidate, so the result is never worse than the input.
    -> dict(actions [S, N, T, na], score [S, N], last / last_score the final iterate, initial_score [S, N]), device tensors; nothing is read back."""
    n_steps = _check_refine(n_steps, lr, optimizer)
    grad_scorer = _resolve(engine, grad_scorer, engine_grad_scorer, 'grad_scorer', gamma, stop_at_done)
    return _refine_candidates(engine, states, torch.as_tensor(actions), 'actions', grad_scorer, n_steps, lr, optimizer, betas, eps, aggregate, 1.0)


def plan_cem_gd(engine, states, horizon, n_candidates, n_elites, n_iters, grad_steps, grad_lr=0.05, refine='elites', optimizer='adam', betas=(0.9, 0.999),
                eps=1e-8, init_mean=None, init_std=1.0, alpha=0.0, min_std=0.0, gamma=1.0, aggregate='mean', generator=None, stop_at_done=True,
                scorer=None, grad_scorer=None, na=None):
    """plan_cem with gradient refinement before the refit (Grad-CEM / CEM-GD): each iteration draws and clips as plan_cem does, then
    refine='elites': scores all candidates (one scoring call), takes the n_elites best and refines THEM by refine_actions' grad_steps steps;
    refine='all': refines every candidate (no separate scoring call) and takes the n_elites best of the refined ones.
    The refit uses the refined elites (keep-best: never worse than the ones drawn).  grad_steps = 0 returns plan_cem's tensors bit for bit for the
    same generator state.  -> plan_cem's dict; `elites` indexes the drawn candidates."""
    T, N, E, n_iters, grad_steps = _check_cem(horizon, n_candidates, n_elites, n_iters, alpha, grad_steps, grad_lr, optimizer, refine)
    scorer, grad_scorer = _resolve_pair(engine, scorer, grad_scorer, engine_scorer, engine_grad_scorer, grad_steps, gamma, stop_at_done)
    states, na = _states(engine, states, na)
    mean, std, best, best_score, history, elites, _ = _cem(scorer, states, na, T, N, E, n_iters, init_mean, init_std, alpha, min_std, aggregate, generator,
                                                           bound=1.0, plant_zero=False, grad_scorer=grad_scorer, grad_steps=grad_steps, refine=refine,
                                                           refine_args=(grad_lr, optimizer, betas, eps))
    return dict(actions=mean, std=std, best_actions=best, best_score=best_score, history=history, elites=elites)


# ---------------------------------------------------------------------- planning in noise space around the policy (POPLIN-A)
def engine_policy_scorer(engine, gamma=1.0, stop_at_done=True, noise_in_std=False, force_generic=False):
    """The engine's closed-loop scorer: (noise [T, B, na], init [S, ns]) -> ret [K, B] of a_t = clip(policy mean(s_t) + noise_t), one
    metrpo_score_policy_actions call, nothing synchronised.  The `scorer=` signature of the other planners."""
    def scorer(noise, init):
        return engine.score_policy_actions(init, noise, gamma=gamma, stop_at_done=stop_at_done, noise_in_std=noise_in_std, force_generic=force_generic)['ret']
    return scorer


def score_noise_sequences(engine, states, noise, gamma=1.0, stop_at_done=True, aggregate='mean', noise_in_std=False, scorer=None):
    """score_action_sequences' counterpart in noise space: states [S, ns], noise [S, N, T, na] (N candidates per state) or [S, T, na] (one each),
    trajectory-major; every candidate is the closed loop a_t = clip(policy mean(s_t) + noise_t) on each head (noise_in_std: noise in units of the
    policy's std).  -> scores [S, N] (or [S]): the heads' discounted returns folded by `aggregate`.  A device tensor."""
    nz = torch.as_tensor(noise)
    scorer = _resolve(engine, scorer, engine_policy_scorer, 'scorer', gamma, stop_at_done, noise_in_std)
    return _score_candidates(engine, states, nz, 'noise', scorer, aggregate)


def plan_cem_policy(engine, states, horizon, n_candidates, n_elites, n_iters, init_mean=None, init_std=0.5, noise_clip=2.0, alpha=0.0, min_std=0.0,
                    gamma=1.0, aggregate='mean', generator=None, stop_at_done=True, scorer=None, na=None, include_policy=True):
    """Cross-entropy method over NOISE sequences around the policy, per state (POPLIN-A): a candidate is delta [T, na] and stands for the closed loop
    a_t = clip(policy mean(s_t) + delta_t) on every head; delta = 0 is the policy itself.  plan_cem's loop over delta: eps = randn(T, S, N, na);
    delta = clamp(mean + std * eps, -noise_clip, noise_clip) (2.0 spans the whole action range from any mean); one scoring call; the n_elites best per
    state; elite mean and population std of the clamped elites in float64; the same mixing with alpha and floor at min_std.
    include_policy: candidate 0 of every state in every iteration is delta = 0, so the best candidate seen is never worse than the policy under the
    scorer.  scorer: (noise [T, B, na], init [S, ns]) -> ret [K, B] (None: engine_policy_scorer).
    -> dict(noise [S, T, na] the final mean, std [S, T, na], best_noise [S, T, na] / best_score [S] the best candidate seen in any iteration, history
    [n_iters, S], elites [S, n_elites] of the last iteration, policy_score [S] the score of delta = 0 in the first iteration (None without
    include_policy)), device tensors; nothing is read back."""
    T, N, E, n_iters, _ = _check_cem(horizon, n_candidates, n_elites, n_iters, alpha)
    noise_clip = _check_noise_clip(noise_clip)
    scorer = _resolve(engine, scorer, engine_policy_scorer, 'scorer', gamma, stop_at_done)
    states, na = _states(engine, states, na)
    mean, std, best, best_score, history, elites, policy_score = _cem(scorer, states, na, T, N, E, n_iters, init_mean, init_std, alpha, min_std, aggregate,
                                                                      generator, bound=noise_clip, plant_zero=include_policy)
    return dict(noise=mean, std=std, best_noise=best, best_score=best_score, history=history, elites=elites, policy_score=policy_score)


def engine_policy_grad_scorer(engine, gamma=1.0, stop_at_done=True, noise_in_std=False, force_generic=False):
    """The engine's closed-loop gradient scorer: (noise [T, B, na], init [S, ns]) -> (ret [K, B], grad [K, T, B, na] = d ret / d noise, the policy path
    included), one metrpo_score_policy_actions_grad call, nothing synchronised.  The `grad_scorer=` signature of the other planners."""
    def grad_scorer(noise, init):
        out = engine.score_policy_actions_grad(init, noise, gamma=gamma, stop_at_done=stop_at_done, noise_in_std=noise_in_std, want=('grad', 'ret'),
                                               force_generic=force_generic)
        return out['ret'], out['grad']
    return grad_scorer


def refine_noise(engine, states, noise, n_steps, lr, noise_clip=2.0, optimizer='adam', betas=(0.9, 0.999), eps=1e-8, gamma=1.0, stop_at_done=True,
                 aggregate='mean', noise_in_std=False, grad_scorer=None):
    """refine_actions in noise space: projected gradient ASCENT on candidate noise sequences around the policy, states [S, ns], noise [S, N, T, na] (or
    [S, T, na]: one each).  n_steps times delta <- clamp(delta + step, -noise_clip, noise_clip) with refine_actions' steps, g = aggregate_heads_grad of
    one closed-loop gradient call (d ret / d noise with the policy path included); n_steps + 1 calls in all.  Keep-best: `noise` / `score` are the
    best-scoring iterate seen per candidate, so the result is never worse than the input.
    -> dict(noise [S, N, T, na], score [S, N], last / last_score the final iterate, initial_score [S, N]), device tensors; nothing is read back."""
    n_steps = _check_refine(n_steps, lr, optimizer)
    noise_clip = _check_noise_clip(noise_clip)
    grad_scorer = _resolve(engine, grad_scorer, engine_policy_grad_scorer, 'grad_scorer', gamma, stop_at_done, noise_in_std)
    return _refine_candidates(engine, states, torch.as_tensor(noise), 'noise', grad_scorer, n_steps, lr, optimizer, betas, eps, aggregate, noise_clip)


def plan_cem_policy_gd(engine, states, horizon, n_candidates, n_elites, n_iters, grad_steps, grad_lr=0.05, refine='elites', optimizer='adam',
                       betas=(0.9, 0.999), eps=1e-8, init_mean=None, init_std=0.5, noise_clip=2.0, alpha=0.0, min_std=0.0, gamma=1.0, aggregate='mean',
                       generator=None, stop_at_done=True, scorer=None, grad_scorer=None, na=None, include_policy=True):
    """plan_cem_policy with gradient refinement before the refit, as plan_cem_gd is plan_cem's: each iteration draws and clamps as plan_cem_policy does
    (include_policy still plants delta = 0 as candidate 0), then
    refine='elites': scores all candidates (one scoring call), takes the n_elites best and refines THEM by refine_noise's grad_steps steps;
    refine='all': refines every candidate (no separate scoring call) and takes the n_elites best of the refined ones.
    The refit uses the refined elites (keep-best: never worse than the ones drawn, so the best candidate seen is still never worse than the policy).
    grad_steps = 0 returns plan_cem_policy's tensors bit for bit for the same generator state.  -> plan_cem_policy's dict; `elites` indexes the drawn
    candidates; policy_score is the score of delta = 0 itself, before any refinement."""
    T, N, E, n_iters, grad_steps = _check_cem(horizon, n_candidates, n_elites, n_iters, alpha, grad_steps, grad_lr, optimizer, refine)
    noise_clip = _check_noise_clip(noise_clip)
    scorer, grad_scorer = _resolve_pair(engine, scorer, grad_scorer, engine_policy_scorer, engine_policy_grad_scorer, grad_steps, gamma, stop_at_done)
    states, na = _states(engine, states, na)
    mean, std, best, best_score, history, elites, policy_score = _cem(scorer, states, na, T, N, E, n_iters, init_mean, init_std, alpha, min_std, aggregate,
                                                                      generator, bound=noise_clip, plant_zero=include_policy, grad_scorer=grad_scorer,
                                                                      grad_steps=grad_steps, refine=refine, refine_args=(grad_lr, optimizer, betas, eps))
    return dict(noise=mean, std=std, best_noise=best, best_score=best_score, history=history, elites=elites, policy_score=policy_score)


def baseline_terminal_value(baseline, t_index, ns):
    """(w1 [ns], w2 [ns], bias) for Engine.set_terminal_value from a LinearFeatureBaseline fit (or its coefficient vector
    [o, o^2, al, al^2, al^3, 1], length 2 ns + 4) with the time features evaluated at path step t_index, al = t_index / 100:
    w1 = c[:ns], w2 = c[ns:2 ns], bias = c[2 ns] al + c[2 ns + 1] al^2 + c[2 ns + 2] al^3 + c[2 ns + 3] -- LinearFeatureBaseline.predict at row t_index.
    t_index is a scalar (bias a scalar) or [S] (bias [S]: one per start state).  Coefficients that live on the device stay there: nothing is read back."""
    c = getattr(baseline, 'coeffs_for_kernel', baseline)
    if c is None:
        raise ValueError("baseline_terminal_value: the baseline has not been fitted")
    ns = int(ns)
    if torch.is_tensor(c):
        c = c.to(torch.float64).reshape(-1)
        al = torch.as_tensor(t_index, device=c.device).to(torch.float64) / 100.0
    else:
        c = np.asarray(c, dtype=np.float64).reshape(-1)
        al = np.asarray(t_index, dtype=np.float64) / 100.0
    if c.shape[0] != 2 * ns + 4:
        raise ValueError("baseline_terminal_value: %d coefficients, expected 2 * %d + 4" % (c.shape[0], ns))
    if al.ndim > 1:
        raise ValueError("baseline_terminal_value: t_index is a scalar or [S]")
    bias = c[2 * ns] * al + c[2 * ns + 1] * al ** 2 + c[2 * ns + 2] * al ** 3 + c[2 * ns + 3]
    return c[:ns], c[ns:2 * ns], bias


class ValueMLP(object):
    """A two-layer tanh value net for Engine.set_terminal_value_mlp (include/metrpo.h: metrpo_set_terminal_value_mlp): a plain container of the six
    arrays W0 [ns, h1], b0 [h1], W1 [h1, h2], b1 [h2], W2 [h2], b2 [1] (float64 tensors, weights in-major) and an input normaliser mean, std [ns]:
        o = clip(s, -10, 10);  x = (o - mean) / std;  V = b2 + W2 . tanh(W1^T tanh(W0^T x + b0) + b1)
    The clip acts on the raw state, so packed() folds the normaliser into W0 / b0 exactly and the library never sees it.  `bias` (a scalar, or [S]:
    one per start state of the scoring call) is what ShootingController hands on with the net; predict() adds it only when it is a scalar.
    Fitting is torch autograd (plumbing, not a hot path); value_targets below forms the targets."""

    def __init__(self, ns, hidden=(32, 32), generator=None):
        self.ns, self.hidden = int(ns), tuple(int(h) for h in hidden)
        if len(self.hidden) != 2 or min(self.hidden) < 1 or max(self.hidden) > 32:
            raise ValueError("ValueMLP: hidden = %r must be two widths in 1 .. 32" % (hidden,))
        h1, h2 = self.hidden
        draw = lambda *shape: torch.randn(*shape, dtype=torch.float64, generator=generator)
        self.W0, self.b0 = draw(self.ns, h1) / np.sqrt(self.ns), torch.zeros(h1, dtype=torch.float64)
        self.W1, self.b1 = draw(h1, h2) / np.sqrt(h1), torch.zeros(h2, dtype=torch.float64)
        self.W2, self.b2 = draw(h2) / np.sqrt(h2), torch.zeros(1, dtype=torch.float64)
        self.mean, self.std = torch.zeros(self.ns, dtype=torch.float64), torch.ones(self.ns, dtype=torch.float64)
        self.bias = 0.0

    def arrays(self):
        return [self.W0, self.b0, self.W1, self.b1, self.W2, self.b2]

    @staticmethod
    def _forward(arrays, mean, std, states):
        W0, b0, W1, b1, W2, b2 = arrays
        x = (torch.clamp(states, -10.0, 10.0) - mean) / std
        return torch.tanh(torch.tanh(x @ W0 + b0) @ W1 + b1) @ W2 + b2

    def predict(self, states):
        """V of states [N, ns] (tensor or array) -> [N] float64 tensor on the states' device"""
        s = torch.as_tensor(states).to(torch.float64)
        dev = s.device
        v = self._forward([a.to(dev) for a in self.arrays()], self.mean.to(dev), self.std.to(dev), s.reshape(-1, self.ns))
        return v + float(self.bias) if np.ndim(self.bias) == 0 else v

    def fit(self, states, targets, n_steps, lr, normalise=True):
        """Adam on the mean squared error of V(states) against targets [N], n_steps full-batch steps from the current arrays, on the states' device
        (hand it tensors on the engine's device).  normalise: mean / std of the CLIPPED states first (std floored at 1e-6).  -> the losses [n_steps + 1],
        before the first step and behind every step."""
        s = torch.as_tensor(states).to(torch.float64).reshape(-1, self.ns)
        dev = s.device
        y = torch.as_tensor(targets).to(device=dev, dtype=torch.float64).reshape(-1)
        if y.shape[0] != s.shape[0]:
            raise ValueError("ValueMLP.fit: %d targets for %d states" % (y.shape[0], s.shape[0]))
        if normalise:
            o = torch.clamp(s, -10.0, 10.0)
            self.mean, self.std = o.mean(dim=0), torch.clamp(o.std(dim=0, unbiased=False), min=1e-6)
        mean, std = self.mean.to(dev), self.std.to(dev)
        par = [a.detach().to(dev).clone().requires_grad_(True) for a in self.arrays()]
        opt = torch.optim.Adam(par, lr=lr)
        losses = []
        for _ in range(int(n_steps)):
            opt.zero_grad()
            loss = torch.mean((self._forward(par, mean, std, s) - y) ** 2)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        with torch.no_grad():
            losses.append(torch.mean((self._forward(par, mean, std, s) - y) ** 2))
        self.W0, self.b0, self.W1, self.b1, self.W2, self.b2 = (p.detach() for p in par)
        return torch.stack(losses).cpu().numpy()

    def packed(self):
        """The library's d_params, float32: W0' | b0' | W1 | b1 | W2 | b2 with the normaliser folded in, W0' = W0 / std[:, None], b0' = b0 - (mean / std) @ W0"""
        dev = self.W0.device
        mean, std = self.mean.to(dev), self.std.to(dev)
        W0 = self.W0 / std[:, None]
        b0 = self.b0 - (mean / std) @ self.W0
        return torch.cat([W0.reshape(-1), b0, self.W1.reshape(-1), self.b1, self.W2, self.b2]).to(torch.float32)


def value_targets(engine, baseline, paths, gamma):
    """Fit targets for ValueMLP.fit from recorded or imagined paths (dicts with 'observations' [L, ns] and 'rewards' [L], the baseline's own form):
    every row's discounted return-to-go  G_t = sum_{u >= t} gamma^(u - t) r_u.  A path that was cut off rather than ended (path['truncated'] set) and a
    fitted baseline: the last row's own reward is replaced by the baseline's prediction there, so the tail behind the cut is the baseline's estimate,
    G_t = sum_{t <= u < L - 1} gamma^(u - t) r_u + gamma^(L - 1 - t) V_b(row L - 1).  baseline None: nothing is bootstrapped.
    -> (states [N, ns], targets [N]) float64 tensors on the engine's device, rows of all paths in order."""
    states, targets = [], []
    for path in paths:
        obs = np.asarray(path['observations'], dtype=np.float64)
        r = np.asarray(path['rewards'], dtype=np.float64).reshape(-1).copy()
        if obs.ndim != 2 or obs.shape[0] != r.shape[0]:
            raise ValueError("value_targets: observations %s do not go with %d rewards" % (obs.shape, r.shape[0]))
        if baseline is not None and path.get('truncated', False) and r.shape[0] > 0:
            r[-1] = float(np.asarray(baseline.predict(path))[-1])
        g, acc = np.zeros_like(r), 0.0
        for t in range(r.shape[0] - 1, -1, -1):
            acc = r[t] + gamma * acc
            g[t] = acc
        states.append(obs); targets.append(g)
    dev = engine.device if engine is not None else torch.device('cpu')
    return (torch.as_tensor(np.concatenate(states, axis=0), dtype=torch.float64, device=dev),
            torch.as_tensor(np.concatenate(targets, axis=0), dtype=torch.float64, device=dev))


class ShootingController(object):
    """Model-predictive control by CEM with a warm start, with the policy's call shape: get_actions(obs [S, ns]) -> (actions [S, na], {}).
    Every call plans `horizon` steps ahead from obs, returns the first action of the plan's mean and keeps the rest: the next call starts from the
    previous mean shifted by one step, its last row reset to init_mean's last row (std starts from init_std every time).
    The action comes back as float64 NumPy, as GaussianMLPPolicy.get_actions gives it -- one read-back per call, behind the planner.
    grad_steps > 0 plans with plan_cem_gd (grad_lr, refine, grad_scorer) instead.
    policy_prior=True plans with plan_cem_policy (noise_clip) around the engine's policy instead: the warm start is the noise mean shifted by one step,
    its last row reset to 0, and the action is clip(policy mean(obs) + noise mean[0]).
    policy_prior=True with noise_grad_steps > 0 plans with plan_cem_policy_gd (noise_grad_lr, refine, noise_grad_scorer): gradients with respect to the
    NOISE, the policy path included.
    terminal_value=baseline (a fitted LinearFeatureBaseline, or its coefficient vector) plans with a value behind the horizon: the controller counts
    every env's path steps (one per get_actions call, zeroed by reset), and around each plan sets the engine's terminal value to the baseline at
    path step counter + horizon -- one bias per env -- and clears it again.  None: nothing is set, cleared or counted.
    terminal_value=ValueMLP: the net is set around each plan in the same way (Engine.set_terminal_value_mlp) with the net's own `bias`: a scalar unless
    the caller made it [S]."""

    def __init__(self, engine, horizon, n_candidates, n_elites, n_iters, init_mean=None, init_std=1.0, alpha=0.0, min_std=0.0, gamma=1.0,
                 aggregate='mean', generator=None, stop_at_done=True, scorer=None, na=None, grad_steps=0, grad_lr=0.05, refine='elites', grad_scorer=None,
                 policy_prior=False, noise_clip=2.0, noise_grad_steps=0, noise_grad_lr=0.05, noise_grad_scorer=None, terminal_value=None):
        self.engine, self.horizon, self.scorer, self.na = engine, int(horizon), scorer, (engine.na if engine is not None else na)
        # grad_steps > 0: plan_cem_gd with these settings in plan_cem's place (0: plan_cem, as before)
        self.grad_steps, self.grad_kw = _check_refine(grad_steps, grad_lr, 'adam'), dict(grad_lr=grad_lr, refine=refine, grad_scorer=grad_scorer)
        if refine not in ('elites', 'all'):
            raise ValueError("refine: %r is neither 'elites' nor 'all'" % (refine,))
        # policy_prior: plan_cem_policy over noise around the engine's policy; the warm start is the shifted NOISE mean, its last row reset to 0
        self.policy_prior, self.noise_clip = bool(policy_prior), float(noise_clip)
        if self.policy_prior and self.grad_steps > 0:
            raise ValueError("policy_prior=True plans in noise space; grad_steps > 0 (gradients with respect to open-loop actions) cannot be combined with it")
        if self.policy_prior and engine is None:
            raise ValueError("policy_prior=True needs an engine (its policy_actions gives the mean the noise is added to)")
        # noise_grad_steps > 0 (with policy_prior): plan_cem_policy_gd in plan_cem_policy's place
        self.noise_grad_steps = _check_refine(noise_grad_steps, noise_grad_lr, 'adam')
        self.noise_grad_kw = dict(grad_lr=noise_grad_lr, refine=refine, grad_scorer=noise_grad_scorer)
        if self.noise_grad_steps > 0 and not self.policy_prior:
            raise ValueError("noise_grad_steps > 0 refines noise around the policy: it needs policy_prior=True (grad_steps refines open-loop actions)")
        self.init_mean, self.init_std = init_mean, init_std
        self.kw = dict(n_candidates=n_candidates, n_elites=n_elites, n_iters=n_iters, alpha=alpha, min_std=min_std, gamma=gamma, aggregate=aggregate,
                       generator=generator, stop_at_done=stop_at_done)
        self._mean = None                                                                 # [S, T, na]: the warm start of the next call
        self.last_plan = None
        # terminal_value: the baseline whose value at path step counter + horizon is the engine's terminal value during a plan
        self.terminal_value = terminal_value
        if terminal_value is not None and engine is None:
            raise ValueError("terminal_value needs an engine (the value is set on it around each plan)")
        self._steps = None                                                                # [S] int64: path steps taken since the env's last reset

    def reset(self, dones=None):
        """Forget the warm start: of every env (dones None) or of the envs whose entry of dones is set.  Their step counters start from 0 again."""
        if self._steps is not None:
            if dones is None:
                self._steps = None
            else:
                d = np.asarray(dones).astype(bool).reshape(-1)
                # another number of envs than the counter was made for: every counter starts afresh, as get_actions does with the warm start
                self._steps = np.where(d, 0, self._steps) if d.shape[0] == self._steps.shape[0] else None
        if dones is None or self._mean is None:
            self._mean = None
            return
        d = torch.as_tensor(np.asarray(dones).astype(bool), device=self._mean.device)
        if d.numel() != self._mean.shape[0]:                                              # another number of envs: get_actions would drop the warm start too
            self._mean = None
            return
        self._mean = torch.where(d.view(-1, 1, 1), self._fresh(self._mean.shape[0], self._mean.device), self._mean)

    def _fresh(self, S, dev):
        m = _time_major_param(0.0 if self.init_mean is None else self.init_mean, self.horizon, S, self.na, dev, 'init_mean')
        return m[:, :, 0].permute(1, 0, 2).contiguous()

    def shifted(self, mean):
        """[S, T, na] -> the same one step on: row t <- row t + 1, the last row <- init_mean's last row"""
        fresh = self._fresh(mean.shape[0], mean.device)
        return torch.cat([mean[:, 1:], fresh[:, -1:]], dim=1)

    def shifted_noise(self, noise):
        """[S, T, na] -> the same one step on: row t <- row t + 1, the last row <- 0 (the policy itself)"""
        return torch.cat([noise[:, 1:], torch.zeros_like(noise[:, -1:])], dim=1)

    def get_actions(self, observations):
        obs = torch.as_tensor(np.asarray(observations) if not torch.is_tensor(observations) else observations)
        S = obs.shape[0] if obs.dim() == 2 else 1
        if self.terminal_value is None:
            return self._plan(obs, S)
        if self._steps is None or self._steps.shape[0] != S:
            self._steps = np.zeros(S, dtype=np.int64)
        if isinstance(self.terminal_value, ValueMLP):
            self.engine.set_terminal_value_mlp(self.terminal_value.packed(), self.terminal_value.hidden, self.terminal_value.bias)
        else:
            self.engine.set_terminal_value(*baseline_terminal_value(self.terminal_value, self._steps + self.horizon, self.engine.ns))
        try:
            out = self._plan(obs, S)
        finally:
            self.engine.clear_terminal_value()
        self._steps = self._steps + 1
        return out

    def _plan(self, obs, S):
        start = self._mean if (self._mean is not None and self._mean.shape[0] == S) else self.init_mean
        kw = dict(self.kw, init_mean=start, init_std=self.init_std, scorer=self.scorer, na=self.na)
        if self.policy_prior:
            planners, steps, grad_kw = (plan_cem_policy, plan_cem_policy_gd), self.noise_grad_steps, self.noise_grad_kw
            kw['noise_clip'] = self.noise_clip
        else:
            planners, steps, grad_kw = (plan_cem, plan_cem_gd), self.grad_steps, self.grad_kw
        if steps > 0:
            kw.update(grad_kw, grad_steps=steps)
        plan = self.last_plan = planners[steps > 0](self.engine, obs, self.horizon, **kw)
        if self.policy_prior:
            self._mean = self.shifted_noise(plan['noise'])
            obs2 = obs.reshape(S, -1).to(device=plan['noise'].device, dtype=torch.float32)
            pmean = self.engine.policy_actions(obs2)[1]                                   # one policy forward, not a second scoring call
            return torch.clamp(pmean + plan['noise'][:, 0], -1.0, 1.0).double().cpu().numpy(), {}
        self._mean = self.shifted(plan['actions'])
        return plan['actions'][:, 0].double().cpu().numpy(), {}


    def get_action(self, observation):
        a, info = self.get_actions(np.asarray(observation)[None])
        return a[0], info
