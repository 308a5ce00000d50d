"""NumPy restatement of the dual-buffer non-local-means denoiser: zr_accum_halves in FP64 on top of accum_model's lanes, and zr_denoise_nlm
(raytracer_project_amd/csrc/zr_nlm.hip) in FP32 on top of denoise_model — operation for operation in the kernels' order (they are compiled without
multiply-add contraction); only exp / exp2 / log2 come from a different library.  The model knows no tiles.

The half images.  A pixel with k = 64 m samples: the xor butterfly 32, 16, 8, 4, 2 over its 64 lane sums leaves T_A (the even lanes) in lane 0 and T_B (the
odd lanes) in lane 1;  A = T_A * (1.0 / (k / 2)),  B = T_B * (1.0 / (k / 2)).

The filter.  Cleaning, normal decoding and the albedo divisor a' are denoise_model's.  uA = clean(A) / a', uB = clean(B) / a',
Vh = 2 max(clean(variance), 0) / (a' a'), V^ = its 3 x 3 Gaussian per channel (denoise_guided_model's stencil rules).  With clamp() to the nearest frame
pixel, for every offset D (dy outer, dx inner), per buffer u, with vs = V^_s.c and vt = V^_t.c, t = clamp(s + D):

    canc = alpha (vs + min(vt, vs))      id = 1 / (eps + kk (vs + vt)), kk = k k      delta_c = ((u_s.c - u_t.c)^2 - canc) id
    e_D(s) = ((delta_x + delta_y) + delta_z) (1/3)
    D_D(p) = (sum over tau_y, tau_x in [-f, f] of e_D(clamp(p + tau)), from 0) inv_np,  inv_np = 1 / (2f + 1)^2
    w_u = exp(-(max(D_D(p), 0) + |a_p - a_q|^2 inv_a)) w_n   for q = p + D inside the frame;  1 at the centre
    fB = sum w_uA uB_q / sum w_uA      fA = sum w_uB uA_q / sum w_uB
    out = ((fA + fB) 0.5) a'           out_error = (((fA - fB) 0.5) a')^2
"""
import numpy as np

import accum_model as am
import denoise_guided_model as gm
import denoise_model as dm

F = np.float32


def accum_halves(partial, count):
    """zr_accum_halves of lane sums partial[..., 64, 3] holding `count` (a positive multiple of 64; scalar or per-pixel array) samples each: (A, B), [..., 3]"""
    v = np.array(partial, dtype=np.float64)
    count = np.asarray(count)
    assert v.shape[-2:] == (am.LANES, 3) and (count > 0).all() and (count % am.LANES == 0).all()
    idx = np.arange(am.LANES)
    with np.errstate(all="ignore"):
        for m in (32, 16, 8, 4, 2):
            v = v + v[..., idx ^ m, :]
        scale = (1.0 / (count // 2).astype(np.float64))[..., None]
        return v[..., 0, :] * scale, v[..., 1, :] * scale


def prepare(half_a, half_b, variance, albedo, normal, demodulate):
    """nlm_pack + nlm_smooth: (uA, uB, V^, albedo, n, n_valid, a'), float32"""
    uA, a, _, n, valid = dm.prepare(half_a, albedo, normal, None, demodulate)
    div = dm.albedo_divisor(a, demodulate)
    uB = dm.clean(half_b) / div
    with np.errstate(over="ignore"):
        Vh = (F(2) * gm.clean_variance(variance) / (div * div)).astype(np.float32)
        Vs = np.stack([gm.smoothed_spread(Vh[..., c]) for c in range(3)], axis=-1)
    return uA.astype(np.float32), uB.astype(np.float32), Vs, a, n, valid, div


def _edge(x, m):
    """x with m pixels of its own edge around it: index [m + y, m + x] is x at clamp(y, x)"""
    return np.pad(x, ((m, m), (m, m)) + ((0, 0),) * (x.ndim - 2), mode="edge")


def denoise_nlm(half_a, half_b, variance, albedo, normal, search_radius=7, patch_radius=1, demodulate_albedo=False, k=0.7, alpha=1.0, sigma_normal=64.0,
                sigma_albedo=0.25, epsilon=1e-10, return_weights=False):
    """zr_denoise_nlm on (H, W, 3) frames: (out, out_error), both (H, W, 3) float64; with return_weights also the ((2r+1)^2, H, W) weights of uA and of uB"""
    uA, uB, V, a, n, valid, div = prepare(half_a, half_b, variance, albedo, normal, demodulate_albedo)
    H, W = uA.shape[:2]
    r, f = int(search_radius), int(patch_radius)
    kk = F(k) * F(k); al = F(alpha); eps = F(epsilon)
    inv_a = F(1) / (F(sigma_albedo) * F(sigma_albedo)); s_n = F(sigma_normal)
    inv_np = F(1) / F((2 * f + 1) * (2 * f + 1))
    third = F(1.0) / F(3.0)
    pA, pB, pV = _edge(uA, r), _edge(uB, r), _edge(V, r)
    inside = np.ones((H, W), bool)
    numA = np.zeros((H, W, 3), np.float32); swB = np.zeros((H, W), np.float32)   # sum w_uB uA_q, sum w_uB
    numB = np.zeros((H, W, 3), np.float32); swA = np.zeros((H, W), np.float32)   # sum w_uA uB_q, sum w_uA
    wsA, wsB = [], []
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ok = dm._shift(inside, dy, dx, False)
                if dy == 0 and dx == 0:
                    wa = np.ones((H, W), np.float32); wb = wa
                else:
                    At, Bt, Vt = (x[r + dy:r + dy + H, r + dx:r + dx + W] for x in (pA, pB, pV))   # at t = clamp(s + D)
                    canc = al * (V + np.minimum(Vt, V))
                    idn = F(1) / (eps + kk * (V + Vt))
                    da = uA - At; db = uB - Bt
                    dA = (da * da - canc) * idn; dB = (db * db - canc) * idn
                    eA = ((dA[..., 0] + dA[..., 1]) + dA[..., 2]) * third
                    eB = ((dB[..., 0] + dB[..., 1]) + dB[..., 2]) * third
                    DA = np.zeros((H, W), np.float32); DB = np.zeros((H, W), np.float32)
                    peA, peB = _edge(eA, f), _edge(eB, f)
                    for ty in range(-f, f + 1):
                        for tx in range(-f, f + 1):
                            DA = DA + peA[f + ty:f + ty + H, f + tx:f + tx + W]; DB = DB + peB[f + ty:f + ty + H, f + tx:f + tx + W]
                    DA = DA * inv_np; DB = DB * inv_np
                    aq, nq, vq = (dm._shift(x, dy, dx) for x in (a, n, valid))
                    b = a - aq
                    arg_a = (b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1] + b[..., 2] * b[..., 2]) * inv_a
                    dot = n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1] + n[..., 2] * nq[..., 2]
                    wn = np.where(valid & vq, np.exp2(s_n * np.log2(np.maximum(F(0), dot))), F(1)).astype(np.float32)
                    wa = np.exp(-(np.fmax(DA, F(0)) + arg_a)) * wn
                    wb = np.exp(-(np.fmax(DB, F(0)) + arg_a)) * wn
                wa = np.where(ok, wa, F(0)).astype(np.float32); wb = np.where(ok, wb, F(0)).astype(np.float32)
                Aq, Bq = dm._shift(uA, dy, dx), dm._shift(uB, dy, dx)
                numB = numB + wa[..., None] * Bq; swA = swA + wa
                numA = numA + wb[..., None] * Aq; swB = swB + wb
                if return_weights:
                    wsA.append(wa); wsB.append(wb)
        fA = numA / swB[..., None]; fB = numB / swA[..., None]
        out = ((fA + fB) * F(0.5)) * div
        e = ((fA - fB) * F(0.5)) * div
        err = e * e
    res = (out.astype(np.float64), err.astype(np.float64))
    return res + (np.stack(wsA), np.stack(wsB)) if return_weights else res


def nlm_params(p):
    """keyword arguments of denoise_nlm() from a capi.DenoiseNlmParams"""
    return dict(search_radius=p.search_radius, patch_radius=p.patch_radius, demodulate_albedo=bool(p.demodulate_albedo), k=p.k, alpha=p.alpha,
                sigma_normal=p.sigma_normal, sigma_albedo=p.sigma_albedo, epsilon=p.epsilon)
