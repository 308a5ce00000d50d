"""NumPy restatement of the firefly-robust resolve (include/zr_capi.h: zr_accum_resolve_robust), operation for operation in the order the
header states (raytracer_project_amd/csrc/zr_robust.hip is compiled without multiply-add contraction).  All FP64.

A pixel with count = 64 m samples holds m samples in each of its 64 lane sums S_l = (x, y, z).  `sum` below is accum_model's xor butterfly 32, 16, ... 1.

    key       v_l = (S_l.x + S_l.y) + S_l.z;  a lane is bad when v_l is not finite;  k_l = v_l, or +inf for a bad lane
    rank      r_l = #{ j : k_j < k_l, or k_j == k_l and j < l }  (IEEE < and ==: -0.0 ties with 0.0) — counted here, literally
    Gini      K = the key of the good lane of highest rank (rank 63 - n_bad), 0.0 if every lane is bad;  k^_l = k_l, or K for a bad lane
              T = sum k^_l;  A = sum (double)(2 r_l - 63) * k^_l
              g = 1.0 if T or A is not finite, else 0.0 if T <= 0.0, else q = A / (64.0 * T), q < 0.0 -> 0.0, q > 1.0 -> 1.0
    trim      GINI: x = strength * g, x > 1.0 -> 1.0, t = min((int)floor(x * 32.0), 31);  FIXED: t = trim;  then t = max(t, min(n_bad, 31))
              lane l is kept iff t <= r_l <= 63 - t;  n_k = 64 - 2 t
    colour    Tk = sum (kept ? S_l.c : 0.0);  out_c = Tk * (1.0 / (double)(m * n_k))
    variance  mu = Tk * (1.0 / n_k);  d_l = kept ? S_l.c - mu : 0.0;  Q = sum d_l * d_l
              var = Q * (1.0 / (n_k - 1)) * (1.0 / n_k) * inv_m * inv_m, inv_m = 1.0 / m;  +inf where Tk is not finite
    n_bad >= 32: colour and variance +inf, t = 31
"""
import numpy as np

import accum_model as am

GINI, FIXED = 0, 1
DEFAULT_STRENGTH = 1.0


def wave_total(v):
    """the xor butterfly 32, 16, ... 1 over v[..., 64]: the total every lane ends with"""
    return am.butterfly(np.asarray(v, dtype=np.float64)[..., None])[..., 0]


def keys(partial):
    """(k, bad): the rank keys [..., 64] of lane sums partial[..., 64, 3] and which lanes are bad"""
    with np.errstate(all="ignore"):
        v = (partial[..., 0] + partial[..., 1]) + partial[..., 2]
    bad = ~np.isfinite(v)
    return np.where(bad, np.inf, v), bad


def ranks(k):
    """the stable rank of every lane of k[..., 64] (no NaN), by counting"""
    lane = np.arange(am.LANES)
    kj, kl = k[..., None, :], k[..., :, None]                       # [..., l, j]
    before = (kj < kl) | ((kj == kl) & (lane[None, :] < lane[:, None]))
    return before.sum(axis=-1)


def gini(k, bad, r):
    """(g, T, A) of keys k[..., 64] with ranks r"""
    n_bad = bad.sum(axis=-1)
    top = (r == (63 - n_bad)[..., None]) & ~bad                     # one lane per pixel, none when every lane is bad
    K = np.where(top.any(axis=-1), np.where(top, k, -np.inf).max(axis=-1), 0.0)   # (that one lane's key, bits and all)
    kh = np.where(bad, K[..., None], k)
    with np.errstate(all="ignore"):
        T = wave_total(kh)
        A = wave_total((2 * r - 63).astype(np.float64) * kh)
        q = A / (64.0 * T)
    q = np.where(q < 0.0, 0.0, q)
    q = np.where(q > 1.0, 1.0, q)
    g = np.where(~np.isfinite(T) | ~np.isfinite(A), 1.0, np.where(T <= 0.0, 0.0, q))
    return g, T, A


def trim_of(g, n_bad, mode=GINI, trim=0, strength=DEFAULT_STRENGTH):
    if mode == GINI:
        with np.errstate(all="ignore"):
            x = np.float64(strength) * g
        x = np.where(x > 1.0, 1.0, x)
        t = np.minimum(np.floor(x * 32.0).astype(np.int64), 31)
    else:
        t = np.full(np.shape(g), int(trim), dtype=np.int64)
    return np.maximum(t, np.minimum(n_bad, 31))


def resolve_robust(partial, count, mode=GINI, trim=0, strength=DEFAULT_STRENGTH, details=False):
    """zr_accum_resolve_robust of lane sums partial[..., 64, 3] holding `count` (a positive multiple of 64; scalar or per-pixel array) samples each:
    (colour [..., 3], variance [..., 3], t [...] int32); details: also a dict of g, T, A, r, kept"""
    partial = np.asarray(partial, dtype=np.float64)
    count = np.broadcast_to(np.asarray(count), partial.shape[:-2])
    assert partial.shape[-2:] == (am.LANES, 3) and (count > 0).all() and (count % am.LANES == 0).all()
    assert mode in (GINI, FIXED) and 0 <= trim <= 31 and strength >= 0 and np.isfinite(strength)
    m = count // am.LANES
    k, bad = keys(partial)
    n_bad = bad.sum(axis=-1)
    r = ranks(k)
    g, T, A = gini(k, bad, r)
    t = trim_of(g, n_bad, mode, trim, strength)
    kept = (t[..., None] <= r) & (r <= 63 - t[..., None])
    n_k = 64 - 2 * t
    with np.errstate(all="ignore"):
        Tk = am.butterfly(np.where(kept[..., None], partial, 0.0))                 # [..., 3]
        col = Tk * (1.0 / (m * n_k).astype(np.float64))[..., None]
        mu = Tk * (1.0 / n_k.astype(np.float64))[..., None]
        d = np.where(kept[..., None], partial - mu[..., None, :], 0.0)
        Q = am.butterfly(d * d)
        inv_m = (1.0 / m.astype(np.float64))[..., None]
        var = Q * (1.0 / (n_k - 1).astype(np.float64))[..., None] * (1.0 / n_k.astype(np.float64))[..., None] * inv_m * inv_m
    var = np.where(np.isfinite(Tk), var, np.inf)
    lost = (n_bad >= 32)[..., None]
    col = np.where(lost, np.inf, col); var = np.where(lost, np.inf, var)
    out = (col, var, t.astype(np.int32))
    return out + (dict(g=g, T=T, A=A, r=r, kept=kept, n_bad=n_bad),) if details else out
