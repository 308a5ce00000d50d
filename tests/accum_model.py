"""NumPy restatement of the order in which a frame's samples are summed, operation for operation.

A pixel's samples are summed in 64 lanes: sample s belongs to lane s % 64 and a lane adds its samples in increasing s, starting from 0.0.
The lanes are then combined by an xor butterfly (every lane adds the lane `m` away, for a fixed sequence of m) and the total is multiplied
by 1.0 / n.  The streaming pipeline and the fused kernel pair lanes 32, 16, ... 1 apart; the pixel-group kernel sums over L = lanes_for(n)
lanes and pairs them 1, 2, ... L/2 apart, which over 64 lanes is the steps 32 ... L first and then 1 ... L/2 (`asc_lanes = L`).

IEEE-754 double addition is commutative, so `v + v[partner]` gives every lane the value the device's lanes hold.
"""
import numpy as np

LANES = 64


def lanes_for(n):
    """lanes of a wave that share a pixel in the pixel-group kernel: the largest power of two <= n, at most 64"""
    lanes = LANES
    while lanes > n:
        lanes >>= 1
    return lanes


def lane_partials(first, samples, partial=None):
    """adds samples[..., k, :] (the samples first + k, k = 0 .. n-1) to partial[..., lane, :] in increasing k; returns the partials"""
    samples = np.asarray(samples, dtype=np.float64)
    if partial is None:
        partial = np.zeros(samples.shape[:-2] + (LANES, samples.shape[-1]), dtype=np.float64)
    for k in range(samples.shape[-2]):
        partial[..., (first + k) % LANES, :] += samples[..., k, :]
    return partial


def butterfly(partial, asc_lanes=1):
    """the xor butterfly over the 64 lanes: steps 32 ... asc_lanes, then 1 ... asc_lanes / 2; returns lane 0's total"""
    v = np.array(partial, dtype=np.float64)
    idx = np.arange(LANES)
    m = 32
    while m >= asc_lanes:
        v = v + v[..., idx ^ m, :]
        m >>= 1
    m = 1
    while m < asc_lanes:
        v = v + v[..., idx ^ m, :]
        m <<= 1
    return v[..., 0, :]


def resolve(partial, n, asc_lanes=1):
    """the mean of the n samples the partials hold"""
    return butterfly(partial, asc_lanes) * (1.0 / n)


def frame(samples, first=0, splits=None, asc_lanes=1):
    """the frame of samples[..., n, 3] accumulated in consecutive batches of the sizes in `splits` (default: one batch)"""
    samples = np.asarray(samples, dtype=np.float64)
    n = samples.shape[-2]
    splits = list(splits) if splits is not None else [n]
    assert sum(splits) == n
    partial, at = None, 0
    for b in splits:
        partial = lane_partials(first + at, samples[..., at:at + b, :], partial)
        at += b
    return resolve(partial, n, asc_lanes)
