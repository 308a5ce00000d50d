"""NumPy restatement of the adaptive sampler's noise estimate and stopping rule, operation for operation.

A pixel with k = 64 m samples holds exactly m samples in each of its 64 lane sums S_l (tests/accum_model.py: sample s belongs to lane s % 64), so
the lane sums are 64 equally weighted, independent estimates of m times the pixel.  In FP64, in this order, with no fused multiply-add:

    v_l = S_l.r + S_l.g + S_l.b          T = sum of v_l by the xor butterfly 32, 16, ... 1       mu = T * (1.0 / 64)
    d_l = v_l - mu                       Q = sum of d_l * d_l by the same butterfly
    se  = sqrt(Q * (1.0 / 63) * (1.0 / 64)) * (1.0 / m)                                            I  = mu * (1.0 / m)
    err = se / (I + dark_floor)          exactly 0 where Q == 0 (all lanes equal), +inf where T is not finite

se is the standard error of the mean of the channel sum, err that error relative to the channel sum itself.  After each pass a pixel stays active iff
err > threshold and its count + step <= max; a pixel that stopped never restarts.
"""
import numpy as np

import accum_model as am

DARK_FLOOR = 0.01


def standard_error(partial, count):
    """(se, I) of lane sums partial[..., 64, 3] holding `count` (a positive multiple of 64; scalar or per-pixel array) samples each"""
    partial = np.asarray(partial, dtype=np.float64)
    count = np.asarray(count)
    assert partial.shape[-2:] == (am.LANES, 3) and (count > 0).all() and (count % am.LANES == 0).all()
    with np.errstate(all="ignore"):
        v = ((partial[..., 0] + partial[..., 1]) + partial[..., 2])[..., None]     # [..., lane, 1]: accum_model's butterfly sums along axis -2
        T = am.butterfly(v)                                                       # [..., 1]
        mu = T * (1.0 / 64)
        d = v - mu[..., None, :]
        Q = am.butterfly(d * d)
        inv_m = 1.0 / (count // am.LANES).astype(np.float64)
        se = np.sqrt(Q * (1.0 / 63) * (1.0 / 64))[..., 0] * inv_m
        I = mu[..., 0] * inv_m
    return se, I, T[..., 0], Q[..., 0]


def error(partial, count, dark_floor=DARK_FLOOR):
    """the noise estimate of every pixel of partial[..., 64, 3]"""
    se, I, T, Q = standard_error(partial, count)
    with np.errstate(all="ignore"):
        err = se / (I + dark_floor)
    err = np.where(Q == 0.0, 0.0, err)
    return np.where(np.isfinite(T), err, np.inf)


def adaptive(samples, min_samples, max_samples, step_samples, threshold, dark_floor=DARK_FLOOR):
    """The adaptive loop over samples[..., n >= max_samples, 3] (sample s of every pixel at index s): returns (frame, counts, history) where history
    lists, per pass, (count of the active pixels after the pass, active mask before it, error map after it)."""
    samples = np.asarray(samples, dtype=np.float64)
    for c in (min_samples, max_samples, step_samples):
        assert c > 0 and c % am.LANES == 0
    assert min_samples <= max_samples <= samples.shape[-2]
    shape = samples.shape[:-2]
    partial = np.zeros(shape + (am.LANES, 3))
    counts = np.zeros(shape, dtype=np.int32)
    active = np.ones(shape, dtype=bool)
    history = []
    now = 0
    while active.any():
        target = min_samples if now == 0 else now + step_samples
        # only the active pixels get the pass's samples: the others' sums stay as they were when they stopped
        partial[active] = am.lane_partials(now, samples[active][..., now:target, :], partial[active])
        counts[active] = target
        err = error(partial, np.maximum(counts, am.LANES), dark_floor)
        before = active.copy()
        active = before & (err > threshold) & (target + step_samples <= max_samples)
        history.append((target, before, err))
        now = target
    frame = am.butterfly(partial) * (1.0 / counts)[..., None]
    return frame, counts, history
