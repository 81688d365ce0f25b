"""NumPy restatement of the rollout's production draws: the Philox4x32-10 stream documented in csrc/device_common.h (counter = (env lo, env hi, t,
purpose << 16 | chunk), key = seed) turned into the five draw tensors of helpers.draws, so that a rollout that drew for itself can be replayed by
the float64 oracle (helpers.oracle_rollout) and by the device in parity mode (Engine.rollout(**draws)).

The specification is the comment block above `enum { RNG_STEP ... }` in device_common.h and k_rollout_generic (rollout_generic.hip); env index
genv = stream_offset + b as a 64-bit value, global step t0 + t:
  RNG_STEP block (genv, t0 + t, chunk c):  .x, .y -> normal2 = eps[t, b, 2c], eps[t, b, 2c + 1].  Chunk 0 also carries
      .z -> model_idx[t, b] = (.z K) >> 32 (step_rand head of step t) and reset_model[t + 1, b] = ((.z & 0xFFFF) K) >> 16,
      .w -> reset_idx[t + 1, b] = (.w n_pool) >> 32   (the reset that FOLLOWS step t).
  RNG_SELNOISE block (genv, t0 + t, chunk c): normal4 = sel_noise[t, b, 4c .. 4c + 3].
  RNG_RESET block (genv, 0, chunk 0): .x -> reset_idx[0, b], .y -> reset_model[0, b], both by the 32-bit rule (the initial vec_env.reset()).
Row 0 of a continuation chunk (t0 > 0) is the reset that follows step t0 - 1, so a chunk is a slice of one long call.

Uniforms as on the device, (float32(word) + 0.5f) 2^-32 rounded in fp32; logarithm, square root, sine and cosine in float64 (the device's
__logf / __sincosf are what tests/tolerances.py PHILOX_NORMAL bounds).  One copy of Philox: tests/bptt_stochastic_ref.py."""
import numpy as np
from bptt_stochastic_ref import philox4x32_10

RNG_STEP, RNG_SELNOISE, RNG_RESET = 1, 2, 3
_MASK = 0xFFFFFFFF


def uniform32(word):
    """The device's uniform of a 32-bit word: (float)word + 0.5f, times 2^-32, every operation rounded to fp32.  Lies in (0, 1]."""
    w = np.asarray(word, dtype=np.uint64).astype(np.float32)
    return ((w + np.float32(0.5)) * np.float32(2.0 ** -32)).astype(np.float64)


def radius(word):
    """Box-Muller radius sqrt(-2 ln u) of a word; 0 (not NaN, not -0) at the words whose uniform rounds to 1."""
    return np.sqrt(-2.0 * np.log(uniform32(word))) + 0.0


def normal2(wa, wb):
    """device_common.h normal2: (r cos, r sin, r) with r from the first word and the angle 2 pi u from the second."""
    r, ang = radius(wa), 2.0 * np.pi * uniform32(wb)
    return r * np.cos(ang), r * np.sin(ang), r


def index32(word, n):
    """rng_index: (word n) >> 32."""
    return ((np.asarray(word, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def index16(word, n):
    """rng_index16: ((word & 0xFFFF) n) >> 16, n <= 65535."""
    return (((np.asarray(word, dtype=np.uint64) & np.uint64(0xFFFF)) * np.uint64(n)) >> np.uint64(16)).astype(np.int64)


def counters(stream_offset, t0, B, T, ns, na):
    """Every Philox block one rollout(B, T) call at (stream_offset, t0) reads, as (name, genv [n], t [n], purpose, chunk) with n = T B
    ((t, b) in C order) for the per-step blocks and n = B for the reset blocks ('reset0': row 0 of reset_idx / reset_model)."""
    genv = np.uint64(stream_offset) + np.arange(B, dtype=np.uint64)
    tt, gg = np.meshgrid(np.arange(t0, t0 + T, dtype=np.uint64), genv, indexing='ij')
    tt, gg = tt.ravel(), gg.ravel()
    out = [('step', gg, tt, RNG_STEP, c) for c in range(max(1, (na + 1) // 2))]
    out += [('sel', gg, tt, RNG_SELNOISE, c) for c in range((ns + 3) // 4)]
    if t0 == 0:
        out.append(('reset0', genv, np.zeros(B, dtype=np.uint64), RNG_RESET, 0))
    else:
        out.append(('reset0', genv, np.full(B, t0 - 1, dtype=np.uint64), RNG_STEP, 0))
    return out


def draw_block(seed, genv, t, purpose, chunk):
    """rng_draw: the four output words of block (genv lo, genv hi, t, purpose << 16 | chunk) under key (seed lo, seed hi)."""
    genv = np.asarray(genv, dtype=np.uint64)
    ctr = (genv & np.uint64(_MASK), genv >> np.uint64(32), np.asarray(t, dtype=np.uint64) & np.uint64(_MASK),
           np.full(genv.shape, (purpose << 16) | chunk, dtype=np.uint64))
    return philox4x32_10(ctr, (int(seed) & _MASK, (int(seed) >> 32) & _MASK))


def rollout_draws(seed, stream_offset, t0, B, T, K, n_pool, ns, na):
    """-> (draws, radii): draws = dict(eps [T,B,na], model_idx [T,B], sel_noise [T,B,ns], reset_idx [T+1,B], reset_model [T+1,B]) as helpers.draws
    lays them out; radii = dict(eps [T,B,na], sel_noise [T,B,ns]): the Box-Muller radius behind every normal."""
    eps, eps_r = np.zeros((T, B, 2 * ((na + 1) // 2))), np.zeros((T, B, 2 * ((na + 1) // 2)))
    sel, sel_r = np.zeros((T, B, 4 * ((ns + 3) // 4))), np.zeros((T, B, 4 * ((ns + 3) // 4)))
    model_idx = np.zeros((T, B), np.int64)
    reset_idx, reset_model = np.zeros((T + 1, B), np.int64), np.zeros((T + 1, B), np.int64)
    for name, genv, t, purpose, c in counters(stream_offset, t0, B, T, ns, na):
        x, y, z, w = draw_block(seed, genv, t, purpose, c)
        if name == 'step':
            n0, n1, r = normal2(x, y)
            if 2 * c < eps.shape[2]:
                eps[:, :, 2 * c], eps[:, :, 2 * c + 1] = n0.reshape(T, B), n1.reshape(T, B)
                eps_r[:, :, 2 * c] = eps_r[:, :, 2 * c + 1] = r.reshape(T, B)
            if c == 0:
                model_idx[:] = index32(z, K).reshape(T, B)
                reset_model[1:] = index16(z, K).reshape(T, B)
                reset_idx[1:] = index32(w, n_pool).reshape(T, B)
        elif name == 'sel':
            for j, (wa, wb) in enumerate(((x, y), (z, w))):
                n0, n1, r = normal2(wa, wb)                                # normal4 = two Box-Muller pairs: (.x, .y) and (.z, .w)
                sel[:, :, 4 * c + 2 * j], sel[:, :, 4 * c + 2 * j + 1] = n0.reshape(T, B), n1.reshape(T, B)
                sel_r[:, :, 4 * c + 2 * j] = sel_r[:, :, 4 * c + 2 * j + 1] = r.reshape(T, B)
        elif t0 == 0:
            reset_idx[0], reset_model[0] = index32(x, n_pool), index32(y, K)
        else:
            reset_idx[0], reset_model[0] = index32(w, n_pool), index16(z, K)
    draws = dict(eps=eps[:, :, :na].copy(), model_idx=model_idx, sel_noise=sel[:, :, :ns].copy(), reset_idx=reset_idx, reset_model=reset_model)
    return draws, dict(eps=eps_r[:, :, :na].copy(), sel_noise=sel_r[:, :, :ns].copy())
