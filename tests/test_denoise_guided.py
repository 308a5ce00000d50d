"""Variance-guided denoising: zr_accum_variance (the variance of every pixel's mean from the accumulator's lane sums, FP64, bit-exact
against tests/denoise_guided_model.py), zr_denoise_guided (the a-trous filter of zr_denoise with the colour weight driven by that variance, FP32,
against the same model), zr_accum_denoise (the two without the host round trip) and camera::denoise_variance_guided of the drop-in.  CPU tests check
the ABI surface, the refusals and the model's properties; GPU tests check the device against the model, the state rules, edge behaviour, quality on
real renders against zr_denoise on the same frames, and the drop-in."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import accum_model as am
import denoise_guided_model as gm
import denoise_model as dm
from conftest import ROOT, demo_scene


# ---- CPU: ABI surface ----------------------------------------------------------------------------------------------------------------------

GUIDED_SYMBOLS = ["zr_accum_variance", "zr_denoise_guided", "zr_accum_denoise"]


def test_guided_params_mirror_matches_c_struct(built):
    from raytracer_project_amd import capi
    s = capi.load_scenes()
    s.zrs_sizeof.restype = C.c_size_t
    s.zrs_sizeof.argtypes = [C.c_int]
    assert s.zrs_sizeof(18) == C.sizeof(capi.DenoiseGuidedParams) == 28


def test_guided_entry_points_exported(built):
    from raytracer_project_amd import capi
    lib = capi.load()
    for name in GUIDED_SYMBOLS:
        assert hasattr(lib, name) and name in capi.CAPI_SYMBOLS
    assert hasattr(capi.load_scenes(), "zrs_render_dropin_denoise_guided")
    assert lib.zr_abi_version() == 3


def test_guided_defaults_match_header(built):
    from raytracer_project_amd import capi
    txt = open(os.path.join(ROOT, "include", "zr_capi.h")).read()
    want = {k.lower(): float(np.float32(v.rstrip("f"))) for k, v in re.findall(r"#define ZR_DENOISE_GUIDED_DEFAULT_(\w+) ([0-9.e-]+f?)", txt)}
    assert len(want) == 6
    p = capi.DenoiseGuidedParams.defaults()
    assert want == {"iterations": p.iterations, "demodulate": p.demodulate_albedo, "sigma_variance": p.sigma_variance, "sigma_normal": p.sigma_normal,
                    "sigma_albedo": p.sigma_albedo, "epsilon": p.epsilon}
    assert p.sigma_depth == 0.0
    assert gm.guided_params(p) == dict(iterations=p.iterations, demodulate_albedo=bool(p.demodulate_albedo), sigma_variance=p.sigma_variance, sigma_normal=64.0,
                                       sigma_albedo=0.25, sigma_depth=0.0, epsilon=float(np.float32(1e-8)))
    with pytest.raises(AttributeError):
        capi.DenoiseGuidedParams.defaults(sigma_color=1.0)


def test_guided_refuses_bad_arguments_without_a_device(built):
    """Argument checks come before any device call: NULL context / accumulator / pointers, sizes, levels, sigmas and epsilon give ZR_E_INVALID."""
    from raytracer_project_amd import capi
    lib = capi.load()
    f = np.zeros((2, 3, 3))
    p = capi.DenoiseGuidedParams.defaults()
    ptr = f.ctypes.data
    assert lib.zr_denoise_guided(None, C.byref(p), ptr, ptr, ptr, ptr, None, 3, 2, ptr, ptr) == capi.ZR_E_INVALID
    assert b"null" in lib.zr_last_error()
    assert lib.zr_accum_variance(None, ptr) == capi.ZR_E_INVALID
    assert lib.zr_accum_denoise(None, C.byref(p), ptr, ptr, None, ptr, ptr) == capi.ZR_E_INVALID
    fake = C.c_void_p(1)   # never dereferenced: every call below fails its argument checks first
    assert lib.zr_accum_variance(fake, None) == capi.ZR_E_INVALID
    for args in ((None, ptr, ptr, ptr), (ptr, None, ptr, ptr), (ptr, ptr, None, ptr), (ptr, ptr, ptr, None)):      # colour, variance, albedo, normal
        assert lib.zr_denoise_guided(fake, C.byref(p), *args, None, 3, 2, ptr, ptr) == capi.ZR_E_INVALID
    assert lib.zr_denoise_guided(fake, None, ptr, ptr, ptr, ptr, None, 3, 2, ptr, ptr) == capi.ZR_E_INVALID
    assert lib.zr_denoise_guided(fake, C.byref(p), ptr, ptr, ptr, ptr, None, 3, 2, None, ptr) == capi.ZR_E_INVALID
    assert lib.zr_denoise_guided(fake, C.byref(p), ptr, ptr, ptr, ptr, None, 0, 2, ptr, ptr) == capi.ZR_E_INVALID
    assert lib.zr_denoise_guided(fake, C.byref(p), ptr, ptr, ptr, ptr, None, 1 << 16, 1 << 16, ptr, ptr) == capi.ZR_E_INVALID
    for args in ((None, ptr, ptr), (ptr, None, ptr), (ptr, ptr, None)):                                              # albedo, normal, out
        assert lib.zr_accum_denoise(fake, C.byref(p), args[0], args[1], None, args[2], None) == capi.ZR_E_INVALID
    assert lib.zr_accum_denoise(fake, None, ptr, ptr, None, ptr, None) == capi.ZR_E_INVALID
    bad = [dict(iterations=-1), dict(iterations=9), dict(sigma_variance=0.0), dict(sigma_variance=-1.0), dict(sigma_variance=np.inf), dict(sigma_variance=np.nan),
           dict(sigma_normal=0.0), dict(sigma_normal=np.inf), dict(sigma_albedo=0.0), dict(sigma_albedo=np.nan), dict(sigma_depth=-0.5), dict(sigma_depth=np.nan),
           dict(sigma_depth=np.inf), dict(epsilon=0.0), dict(epsilon=-1e-8), dict(epsilon=np.inf), dict(epsilon=np.nan)]
    for kw in bad:
        q = capi.DenoiseGuidedParams.defaults(**kw)
        assert lib.zr_denoise_guided(fake, C.byref(q), ptr, ptr, ptr, ptr, None, 3, 2, ptr, ptr) == capi.ZR_E_INVALID, kw
        assert lib.zr_accum_denoise(fake, C.byref(q), ptr, ptr, None, ptr, None) == capi.ZR_E_INVALID, kw


# ---- CPU: the model ------------------------------------------------------------------------------------------------------------------------

def _synthetic(w, h, seed, plant=True):
    """tests/test_denoise.py's synthetic frame (noisy HDR colour over an albedo step and a normal step, NaN / Inf planted in every input) and a variance
    frame with values in roughly 1e-3 ... 10 and planted NaN / Inf / negative entries"""
    rng = np.random.default_rng(seed)
    i = np.arange(w)[None, :, None]
    j = np.arange(h)[:, None, None]
    albedo = np.where(i < w // 2, np.array([0.7, 0.2, 0.1]), np.array([0.1, 0.5, 0.8])) * np.ones((h, w, 3))
    albedo = albedo + rng.uniform(-0.02, 0.02, albedo.shape)
    albedo[rng.random((h, w)) < 0.02] = 0.0                       # black material: the divisor falls back to 1
    normal = np.where(j < h // 3, np.array([0.5, 0.5, 1.0]), np.array([1.0, 0.5, 0.5])) * np.ones((h, w, 3))
    normal = normal + rng.normal(0, 0.03, normal.shape)
    normal[rng.random((h, w)) < 0.02] = 0.5                       # encodes the zero vector: no information
    base = albedo * np.where(j < h // 3, 0.8, 2.0)
    color = base * rng.exponential(1.0, (h, w, 1))
    color[rng.random((h, w)) < 0.005] *= 60.0                     # fireflies
    zdepth = np.repeat(np.clip(0.3 + 0.5 * i / max(w, 1) + rng.normal(0, 0.01, (h, w, 1)), 0, 1), 3, axis=2)
    variance = 10.0 ** rng.uniform(-3, 1, (h, w, 3))
    if plant:
        for a, vals in ((albedo, (np.nan, np.inf)), (normal, (np.nan, -np.inf)), (color, (np.nan, np.inf)), (zdepth, (np.nan, np.inf)),
                        (variance, (np.nan, np.inf, -np.inf, -1.0))):
            m = rng.random(a.shape) < 0.003
            a[m] = rng.choice(vals, size=int(m.sum()))
    return color, variance, albedo, normal, zdepth


def test_model_one_pixel_frame():
    """1 x 1: only the centre tap — out = input and V' = V up to the FP32 conversion of the inputs and two roundings (w d / w, w^2 V / w^2)"""
    c = np.array([[[0.3, 1.7, 0.05]]]); v = np.array([[[0.2, 3.0, 1e-3]]])
    a = np.array([[[0.6, 0.5, 0.4]]]); n = np.array([[[0.5, 0.5, 1.0]]])
    for demod in (False, True):
        out, var = gm.denoise_guided(c, v, a, n, iterations=5, demodulate_albedo=demod)
        assert np.allclose(out, c, rtol=1e-6, atol=0) and np.allclose(var, v, rtol=2e-6, atol=0)


def test_model_zero_iterations_is_the_identity():
    c, v, a, n, _ = _synthetic(17, 11, 3)
    out, var = gm.denoise_guided(c, v, a, n, iterations=0, demodulate_albedo=False)
    assert np.array_equal(out, dm.clean(c).astype(np.float64))
    assert np.array_equal(var, np.maximum(dm.clean(v), 0).astype(np.float64))
    # demodulated and remodulated: the variance comes back up to the roundings of / a^2 and * a^2
    out, var = gm.denoise_guided(c, v, a, n, iterations=0, demodulate_albedo=True)
    assert np.allclose(out, dm.clean(c), rtol=2.5e-7, atol=0)
    assert np.allclose(var, np.maximum(dm.clean(v), 0), rtol=2.5e-7, atol=0)


def test_model_constant_frame_one_level():
    """constant colour, guides and variance: an interior pixel keeps its colour and V' = V (sum h^2)^2 = V 4900 / 65536 of the B3 taps"""
    h, w = 9, 11
    c = np.full((h, w, 3), 0.3) * np.array([1.0, 2.0, 0.5])
    v = np.full((h, w, 3), 0.04) * np.array([1.0, 3.0, 0.5])
    a = np.full((h, w, 3), 0.6); n = np.full((h, w, 3), [0.5, 0.5, 1.0]); z = np.full((h, w, 3), 0.4)
    for demod in (False, True):
        out, var = gm.denoise_guided(c, v, a, n, z, iterations=1, demodulate_albedo=demod, sigma_depth=0.1)
        assert np.allclose(out, c, rtol=1e-6, atol=0)
        assert np.allclose(var[2:-2, 2:-2], v[2:-2, 2:-2] * (4900.0 / 65536.0), rtol=1e-6, atol=0)


def test_model_weights_are_normalised():
    """Every level is a convex combination of its taps: weights non-negative, the centre tap's positive, taps off the frame weigh nothing (the 5 x 5
    and the 3 x 3), and the output stays within the input's range channel by channel."""
    c, v, a, n, z = _synthetic(21, 13, 5, plant=False)
    d, V, aa, zz, nn, valid = gm.prepare(c, v, a, n, z, True)
    for level in (0, 1, 3):
        out, vout, w = gm.atrous_level(d, V, aa, zz, nn, valid, level, 2.0, 64.0, 0.1, 0.05, True, return_weights=True)
        assert w.shape == (25,) + d.shape[:2] and (w >= 0).all() and (w[12] > 0).all()
        assert (w[:, 0, 0].reshape(5, 5)[:2, :] == 0).all() and (w[:, 0, 0].reshape(5, 5)[:, :2] == 0).all()   # corner: up / left taps off
        wn = w / w.sum(axis=0)
        taps = np.stack([dm._shift(d, ky << level, kx << level) for ky in range(-2, 3) for kx in range(-2, 3)]).astype(np.float64)
        assert np.allclose(out, np.einsum("thw,thwc->hwc", wn.astype(np.float64), taps), rtol=1e-5, atol=1e-6)
        lo, hi = d.min(axis=(0, 1)), d.max(axis=(0, 1))
        assert (out >= lo * (1 - 1e-6)).all() and (out <= hi * (1 + 1e-6)).all()
        assert (vout >= 0).all() and (vout <= V.max(axis=(0, 1)) * (1 + 1e-6)).all()      # sum w^2 V / (sum w)^2 <= max V
    s = gm.spread(V, dm.tone_r(d))
    sm, g = gm.smoothed_spread(s, return_weights=True)
    assert (g >= 0).all() and (g[4] == 0.25).all()
    assert (g[:, 0, 0].reshape(3, 3)[0, :] == 0).all() and (g[:, 0, 0].reshape(3, 3)[:, 0] == 0).all() and g[:, 0, 0].sum() == 0.5625
    assert (g[:, 5, 5].sum() == 1.0) and (sm >= s.min()).all() and (sm <= s.max() * (1 + 1e-6)).all()


def test_model_converged_pixels_pass_through():
    """a two-colour checker with zero variance comes back unchanged: with the denominator epsilon a differing neighbour's weight underflows"""
    h, w = 12, 16
    ij = np.add.outer(np.arange(h), np.arange(w)) % 2
    c = np.where(ij[..., None] == 0, np.array([0.2, 0.5, 0.1]), np.array([0.6, 0.1, 0.9])) * np.ones((h, w, 3))
    a = np.full((h, w, 3), 0.5); n = np.full((h, w, 3), [0.5, 0.5, 1.0])
    out, var = gm.denoise_guided(c, np.zeros_like(c), a, n, iterations=5)
    assert np.allclose(out, c, rtol=1e-6, atol=0) and not var.any()


def test_model_bad_variance_behaves_as_zero():
    c, v, a, n, _ = _synthetic(19, 9, 8, plant=False)
    bad = v.copy()
    rng = np.random.default_rng(1)
    m = rng.random(v.shape) < 0.2
    bad[m] = rng.choice([np.nan, np.inf, -np.inf, -2.0], size=int(m.sum()))
    zeroed = np.where(m, 0.0, v)
    for demod in (False, True):
        x = gm.denoise_guided(c, bad, a, n, iterations=3, demodulate_albedo=demod)
        y = gm.denoise_guided(c, zeroed, a, n, iterations=3, demodulate_albedo=demod)
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
        assert np.isfinite(x[0]).all() and np.isfinite(x[1]).all()


def test_variance_model_agrees_with_numpy():
    """against np.var(lanes, ddof=1) / 64 / m^2 to 1e-12 relative on random lane sums, for a scalar count and for per-pixel counts"""
    rng = np.random.default_rng(4)
    lanes = rng.exponential(3.0, (5, 7, 64, 3)) * rng.uniform(0.1, 10, (5, 7, 1, 3))
    for count in (64, 192, 64 * rng.integers(1, 5, (5, 7))):
        got = gm.accum_variance(lanes, count)
        m = (np.asarray(count) // 64).astype(np.float64)
        want = np.var(lanes, axis=-2, ddof=1) / 64 / (m * m)[..., None]
        assert got.shape == (5, 7, 3) and np.allclose(got, want, rtol=1e-12, atol=0)
    flat = np.full((2, 64, 3), 0.7)
    flat[1, 5, 2] = np.inf
    got = gm.accum_variance(flat, 64)
    assert (got[0] == 0).all() and got[1, 2] == np.inf and (got[1, :2] == 0).all()


def _region_noise_frame(w=96, h=64, seed=21):
    """a frame whose illumination detail the guides cannot see (a soft shadow edge, fine stripes, a bright blob over constant albedo and normals) with
    noise of relative size 0.05 in the left half and 1.5 in the right: 64 lane estimates per pixel -> (truth, mean, variance of the mean, albedo, normal)"""
    rng = np.random.default_rng(seed)
    x = np.arange(w)[None, :] / w; y = np.arange(h)[:, None] / h
    light = 0.25 + 0.75 / (1 + np.exp(-(x - 0.3 - 0.2 * y) * 40)) + 0.15 * np.sin(x * w * 2 * np.pi / 6) + 2.0 * np.exp(-((x - 0.7) ** 2 + (y - 0.4) ** 2) * 300)
    truth = light[..., None] * np.array([0.9, 0.7, 0.5])
    rel = np.where(x < 0.5, 0.05, 1.5) * np.ones((h, w))
    lanes = truth[:, :, None, :] * (1 + rel[:, :, None, None] * rng.normal(0, 1, (h, w, 64, 3)) * 8.0)     # a lane estimate: 8 x the mean's noise
    mean = lanes.mean(axis=2)
    var = gm.accum_variance(lanes, 64)
    return truth, mean, var, np.full((h, w, 3), 0.5), np.full((h, w, 3), [0.5, 0.5, 1.0])


def test_model_guided_beats_plain_on_region_dependent_noise():
    truth, mean, var, a, n = _region_noise_frame()
    plain = dm.denoise(mean, a, n)
    guided, _ = gm.denoise_guided(mean, var, a, n)
    mse = lambda f: float(((f - truth) ** 2).mean())
    print(f"synthetic frame: MSE noisy {mse(mean):.4e}, plain model {mse(plain):.4e}, guided model {mse(guided):.4e}")
    assert mse(guided) < mse(plain) and mse(guided) < mse(mean)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(built):
    from raytracer_project_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _plan_order(W, H, rect, ts=32):
    """(ys, xs) of the plan's pixels in plan order: the tiles row-major, a tile's pixels of the region row-major"""
    x0, y0, w, h = rect if rect else (0, 0, W, H)
    ys, xs = [], []
    for ty in range(y0 // ts, (y0 + h - 1) // ts + 1):
        for tx in range(x0 // ts, (x0 + w - 1) // ts + 1):
            for y in range(max(ty * ts, y0), min(ty * ts + ts, y0 + h)):
                for x in range(max(tx * ts, x0), min(tx * ts + ts, x0 + w)):
                    ys.append(y); xs.append(x)
    return np.array(ys), np.array(xs)


def _model_variance_frame(acc, H, W, rect, count):
    """the model on the accumulator's own lane sums, scattered to the frame (zeros elsewhere)"""
    ys, xs = _plan_order(W, H, rect)
    sums = acc.lane_sums()
    assert sums.shape == (len(ys), 3, 64)
    want = np.zeros((H, W, 3))
    want[ys, xs] = gm.accum_variance(sums.transpose(0, 2, 1), count if np.isscalar(count) else count[ys, xs])
    return want


# the fused route and the lean pipeline, on 40 x 12 tiles that straddle a tile boundary; a single pixel
VARIANCE_TILES = [("cfg5", (250, 300, 40, 12)), ("cfg2", (600, 300, 40, 12)), ("cfg5", (263, 301, 1, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,rect", VARIANCE_TILES, ids=["cfg5-fused", "cfg2-lean", "one-pixel"])
def test_accum_variance_matches_model_bit_for_bit(name, rect, ctx):
    from raytracer_project_amd import capi
    ds = demo_scene(name)
    sc = capi.Scene(ctx, ds.desc)
    cam = ds.camera.copy()
    W, H = cam.image_width, cam.image_height
    acc = capi.Accumulator(ctx, W, H, capi.Region(*rect, 0, 0, 0, 0))
    try:
        out = np.zeros((H, W, 3))
        assert ctx.lib.zr_accum_variance(acc._a, out.ctypes.data) == capi.ZR_E_STATE          # nothing rendered
        for done in (64, 128):
            acc.accumulate(sc, cam, ds.env, ds.seed, 64)
            got = acc.variance()
            assert got.tobytes() == _model_variance_frame(acc, H, W, rect, done).tobytes(), done
            assert np.isfinite(got).all() and (got >= 0).all() and (got.any() or rect[2] * rect[3] == 1)
        acc.reset(0)
        acc.accumulate(sc, cam, ds.env, ds.seed, 65)
        assert acc.state()["done"] == 65
        assert ctx.lib.zr_accum_variance(acc._a, out.ctypes.data) == capi.ZR_E_STATE          # 65 is no multiple of 64
    finally:
        acc.close(); sc.close()


@pytest.mark.gpu
def test_accum_variance_after_an_adaptive_run(ctx):
    """a non-uniform accumulator uses each pixel's own count"""
    from raytracer_project_amd import capi
    name, rect = VARIANCE_TILES[0]
    ds = demo_scene(name)
    sc = capi.Scene(ctx, ds.desc)
    cam = ds.camera.copy()
    W, H = cam.image_width, cam.image_height
    acc = capi.Accumulator(ctx, W, H, capi.Region(*rect, 0, 0, 0, 0))
    try:
        acc.accumulate(sc, cam, ds.env, ds.seed, 64)
        ys, xs = _plan_order(W, H, rect)
        thr = float(np.median(acc.error()[ys, xs]))
        acc.render_adaptive(sc, cam, ds.env, ds.seed, capi.AdaptiveParams.defaults(min_samples=64, max_samples=256, step_samples=64, threshold=thr))
        counts = acc.sample_counts()
        assert len(np.unique(counts[ys, xs])) > 1
        assert acc.variance().tobytes() == _model_variance_frame(acc, H, W, rect, counts).tobytes()
    finally:
        acc.close(); sc.close()


def _bounds(dev, model, vmax):
    """colour: |dev - model| <= 2e-5 |model| + 1e-6 per channel (the project's bound: same FP32 operations in the same order, only expf / exp2f / log2f
    differ by an ulp or two); variance: 2e-5 |model| + 1e-6 max(input variance).  Returns (channels outside, worst ratio to the bound) for each."""
    ec = np.abs(dev[0] - model[0]); lc = 2e-5 * np.abs(model[0]) + 1e-6
    ev = np.abs(dev[1] - model[1]); lv = 2e-5 * np.abs(model[1]) + 1e-6 * vmax
    return (int((ec > lc).sum()), float((ec / lc).max())), (int((ev > lv).sum()), float((ev / lv).max()))


def _check_against_model(ctx, p, c, v, a, n, z):
    dev = ctx.denoise_guided(p, c, v, a, n, z)
    model = gm.denoise_guided(c, v, a, n, z, **gm.guided_params(p))
    assert np.isfinite(dev[0]).all() and np.isfinite(dev[1]).all() and (dev[1] >= 0).all()
    (bad_c, worst_c), (bad_v, worst_v) = _bounds(dev, model, float(np.maximum(dm.clean(v), 0).max()))
    print(f"guided device vs model {c.shape[1]}x{c.shape[0]} it={p.iterations} demod={p.demodulate_albedo} depth={z is not None}: "
          f"worst colour {worst_c:.3f} x the bound, worst variance {worst_v:.3f} x the bound")
    assert bad_c == 0, f"{bad_c} colour channels outside the bound (worst {worst_c:.2f} x the bound)"
    assert bad_v == 0, f"{bad_v} variance channels outside the bound (worst {worst_v:.2f} x the bound)"


MODEL_CASES = [(w, h, demod, depth) for (w, h) in [(1, 1), (7, 5), (333, 77)] for demod in (True, False) for depth in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,demod,depth", MODEL_CASES)
def test_device_matches_model(w, h, demod, depth, ctx):
    from raytracer_project_amd import capi
    c, v, a, n, z = _synthetic(w, h, 2000 + w + h)
    p = capi.DenoiseGuidedParams.defaults(demodulate_albedo=int(demod), sigma_depth=0.05 if depth else 0.0)
    _check_against_model(ctx, p, c, v, a, n, z if depth else None)


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [0, 1, 8])
def test_device_matches_model_level_counts(iterations, ctx):
    """at level 7 the step of 128 puts most taps of a 129 x 65 frame off it"""
    from raytracer_project_amd import capi
    c, v, a, n, z = _synthetic(129, 65, 78)
    p = capi.DenoiseGuidedParams.defaults(iterations=iterations, sigma_variance=1.3, sigma_albedo=0.3, sigma_normal=16.0, epsilon=1e-6)
    _check_against_model(ctx, p, c, v, a, n, None)


@pytest.mark.gpu
@pytest.mark.parametrize("guide", ["albedo", "normal"])
def test_edges_hold(guide, ctx):
    """tests/test_denoise.py's edge test with a large uniform variance: the variance term lets every colour difference through, the guides' edges
    must still hold — after five levels every left pixel stays < 1e-3 and every right pixel > 1 - 1e-3"""
    from raytracer_project_amd import capi
    w, h = 64, 48
    left = np.arange(w)[None, :, None] < w // 2
    c = np.where(left, 0.0, 1.0) * np.ones((h, w, 3))
    if guide == "albedo":
        a = np.where(left, 0.2, 0.8) * np.ones((h, w, 3)); n = np.full((h, w, 3), [0.5, 0.5, 1.0])
    else:
        a = np.full((h, w, 3), 0.5); n = np.where(left, np.array([0.5, 0.5, 1.0]), np.array([1.0, 0.5, 0.5])) * np.ones((h, w, 3))
    out, var = ctx.denoise_guided(capi.DenoiseGuidedParams.defaults(), c, np.full((h, w, 3), 10.0), a, n)
    assert out[:, : w // 2].max() < 1e-3
    assert out[:, w // 2:].min() > 1.0 - 1e-3
    assert (var < 10.0).all() and (var > 0).all()


@pytest.mark.gpu
def test_deterministic_and_in_place(ctx):
    from raytracer_project_amd import capi
    c, v, a, n, z = _synthetic(333, 77, 12)
    p = capi.DenoiseGuidedParams.defaults(sigma_depth=0.05)
    x = ctx.denoise_guided(p, c, v, a, n, z)
    y = ctx.denoise_guided(p, c, v, a, n, z)
    assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
    ci = np.ascontiguousarray(c).copy(); vi = np.ascontiguousarray(v).copy()
    ctx.denoise_guided(p, ci, vi, a, n, z, out=ci, out_variance=vi)
    assert ci.tobytes() == x[0].tobytes() and vi.tobytes() == x[1].tobytes()
    # out_variance is optional
    only = np.zeros_like(c)
    assert ctx.lib.zr_denoise_guided(ctx._c, C.byref(p), np.ascontiguousarray(c).ctypes.data, np.ascontiguousarray(v).ctypes.data,
                                     np.ascontiguousarray(a).ctypes.data, np.ascontiguousarray(n).ctypes.data, np.ascontiguousarray(z).ctypes.data, 333, 77,
                                     only.ctypes.data, None) == 0
    assert only.tobytes() == x[0].tobytes()


# ---- real renders: 64-spp accumulators of tests/test_denoise.py's quality scenes, truth at 4096 spp (its own variance is 1/64 of the input's) ----------

QUALITY_SIZE = {"cfg5": (300, 300), "mix0": (384, 256)}
_sets = {}


def _quality_set(ctx, name):
    """rendered once per scene and shared, unchanged: the 64-spp frame and variance, the guides, the truth — and for cfg5 the adaptive frame (min 64,
    step 64, max 256, threshold = the median of the 64-spp error map) with its variance.  The accumulators stay open for zr_accum_denoise."""
    if name in _sets:
        return _sets[name]
    from raytracer_project_amd import capi
    ds = demo_scene(name)
    cam = ds.camera.copy()
    cam.image_width, cam.image_height = QUALITY_SIZE[name]
    cam.samples_per_pixel = 64
    sc = capi.Scene(ctx, ds.desc)
    s = dict(scene=sc, cam=cam)
    acc = capi.Accumulator(ctx, cam.image_width, cam.image_height)
    acc.accumulate(sc, cam, ds.env, ds.seed, 64)
    s["acc"], s["noisy"], s["variance"] = acc, acc.resolve(), acc.variance()
    s["albedo"], s["normal"], _ = sc.render_aov(cam, ds.seed, 1.0)
    tc = cam.copy(); tc.samples_per_pixel = 4096
    s["truth"] = sc.render(tc, ds.env, ds.seed, None)
    if name == "cfg5":
        ad = capi.Accumulator(ctx, cam.image_width, cam.image_height)
        thr = float(np.median(acc.error()))
        ad.render_adaptive(sc, cam, ds.env, ds.seed, capi.AdaptiveParams.defaults(min_samples=64, max_samples=256, step_samples=64, threshold=thr))
        s["ad_acc"], s["ad_noisy"], s["ad_variance"], s["ad_counts"] = ad, ad.resolve(), ad.variance(), ad.sample_counts()
    _sets[name] = s
    return s


@pytest.fixture(scope="module", autouse=True)
def _close_sets():
    yield
    for s in _sets.values():
        for k in ("acc", "ad_acc", "scene"):
            if k in s:
                s[k].close()
    _sets.clear()


# F = MSE(noisy) / MSE(filtered) of the guided filter with its defaults, measured on the MI355X, less 5 %: renders and filter are
# deterministic, the margin absorbs libm or compiler drift only
QUALITY_PINS = {"cfg5": 2.09, "mix0": 1.91, "cfg5-adaptive": 1.69}     # measured: 2.201, 2.011, 1.781


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(QUALITY_PINS))
def test_quality_on_real_renders(case, ctx):
    from raytracer_project_amd import capi
    name = case.split("-")[0]
    s = _quality_set(ctx, name)
    noisy, var = (s["ad_noisy"], s["ad_variance"]) if case.endswith("adaptive") else (s["noisy"], s["variance"])
    if case.endswith("adaptive"):
        assert len(np.unique(s["ad_counts"])) > 1
    guided, _ = ctx.denoise_guided(capi.DenoiseGuidedParams.defaults(), noisy, var, s["albedo"], s["normal"])
    plain = ctx.denoise(capi.DenoiseParams.defaults(), noisy, s["albedo"], s["normal"])
    mse = lambda f: float(((f - s["truth"]) ** 2).mean())
    f_guided, f_plain = mse(noisy) / mse(guided), mse(noisy) / mse(plain)
    print(f"guided denoise quality {case}: MSE noisy {mse(noisy):.4e}, F_guided {f_guided:.3f}, F_plain {f_plain:.3f}")
    assert f_guided >= f_plain, (f_guided, f_plain)
    assert f_guided >= QUALITY_PINS[case], (f_guided, QUALITY_PINS[case])


@pytest.mark.gpu
@pytest.mark.parametrize("adaptive", [False, True], ids=["uniform", "adaptive"])
def test_accum_denoise_equals_the_host_route_bit_for_bit(adaptive, ctx):
    from raytracer_project_amd import capi
    s = _quality_set(ctx, "cfg5")
    acc, noisy, var = (s["ad_acc"], s["ad_noisy"], s["ad_variance"]) if adaptive else (s["acc"], s["noisy"], s["variance"])
    _, _, z = s["scene"].render_aov(s["cam"], demo_scene("cfg5").seed, 1.0)
    for p, depth in ((capi.DenoiseGuidedParams.defaults(), None), (capi.DenoiseGuidedParams.defaults(demodulate_albedo=1, sigma_depth=0.05, iterations=3), z)):
        got = acc.denoise(p, s["albedo"], s["normal"], depth)
        want = ctx.denoise_guided(p, noisy, var, s["albedo"], s["normal"], depth)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert np.abs(got[0] - noisy).max() > 0


@pytest.mark.gpu
def test_accum_denoise_refusals(ctx):
    """a region accumulator (tile_mod = 2, or a rectangle) is refused with ZR_E_INVALID whatever it holds; a whole-frame one follows zr_accum_variance's
    state rules"""
    from raytracer_project_amd import capi
    ds = demo_scene("cfg5")
    sc = capi.Scene(ctx, ds.desc)
    cam = ds.camera.copy()
    cam.image_width, cam.image_height = 64, 40
    g = np.full((40, 64, 3), 0.5); out = np.zeros((40, 64, 3))
    p = capi.DenoiseGuidedParams.defaults()
    call = lambda acc: ctx.lib.zr_accum_denoise(acc._a, C.byref(p), g.ctypes.data, g.ctypes.data, None, out.ctypes.data, None)
    try:
        for reg in (capi.Region(0, 0, 0, 0, 0, 2, 1, 0), capi.Region(8, 8, 16, 16, 0, 0, 0, 0)):
            acc = capi.Accumulator(ctx, 64, 40, reg)
            assert call(acc) == capi.ZR_E_INVALID
            acc.accumulate(sc, cam, ds.env, ds.seed, 64)
            assert call(acc) == capi.ZR_E_INVALID
            acc.close()
        acc = capi.Accumulator(ctx, 64, 40)
        assert call(acc) == capi.ZR_E_STATE                 # nothing rendered
        acc.accumulate(sc, cam, ds.env, ds.seed, 65)
        assert call(acc) == capi.ZR_E_STATE                 # 65 is no multiple of 64
        acc.reset(0)
        acc.accumulate(sc, cam, ds.env, ds.seed, 64)
        assert call(acc) == 0 and out.any()
        acc.close()
    finally:
        sc.close()


# ---- drop-in: camera::render with use_denoiser and denoise_variance_guided -----------------------------------------------------------------------

DROPIN = [("mix0", (0, 0), 128, 0.05), ("cfg5", (160, 160), 128, 0.05)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,size,spp,thr", DROPIN, ids=[d[0] for d in DROPIN])
def test_dropin_variance_guided(name, size, spp, thr, ctx):
    from raytracer_project_amd import capi
    ds = demo_scene(name)
    w, h = size
    got = ds.render_dropin_denoise_guided(thr, width=w, height=h, spp=spp)
    plain, counts, _, _ = ds.render_dropin_adaptive(thr, width=w, height=h, spp=spp)
    assert got["guided"] and len(np.unique(counts)) > 1
    assert got["render_accumulator"].tobytes() == plain.tobytes()             # the raw frame is the adaptive render's without the denoiser
    cam = ds.camera.copy()
    cam.image_width, cam.image_height = w or cam.image_width, h or cam.image_height
    cam.samples_per_pixel = spp
    sc = capi.Scene(ctx, ds.desc)
    acc = capi.Accumulator(ctx, cam.image_width, cam.image_height)
    try:
        acc.render_adaptive(sc, cam, ds.env, ds.seed, capi.AdaptiveParams.defaults(min_samples=64, max_samples=spp, step_samples=64, threshold=thr))
        assert acc.resolve().tobytes() == plain.tobytes()
        var = acc.variance()
        assert got["variance_buffer"].tobytes() == var.tobytes()
        a, n, _ = sc.render_aov(cam, ds.seed, 1.0)
        want, _ = ctx.denoise_guided(capi.DenoiseGuidedParams.defaults(), plain, var, a, n)
        assert got["denoise_buffer"].tobytes() == want.tobytes()
        # with the flag off every buffer is what it is today: the plain filter's output, no variance
        off = ds.render_dropin_denoise_guided(thr, guided=False, width=w, height=h, spp=spp)
        assert not off["guided"] and (off["variance_buffer"] == -1).all()
        assert off["render_accumulator"].tobytes() == plain.tobytes()
        assert off["denoise_buffer"].tobytes() == ctx.denoise(capi.DenoiseParams.defaults(), plain, a, n).tobytes()
        assert off["denoise_buffer"].tobytes() != got["denoise_buffer"].tobytes()
    finally:
        acc.close(); sc.close()


@pytest.mark.gpu
def test_dropin_variance_guided_progressive_and_one_shot(ctx, capfd):
    """samples_per_pass with a multiple-of-64 total has a variance too; a one-shot render (or another total) has none: a warning, and the plain filter"""
    from raytracer_project_amd import capi
    ds = demo_scene("cfg5")
    w = h = 96
    today = ds.render_dropin_denoise(w, h, 8)
    capfd.readouterr()
    got = ds.render_dropin_denoise_guided(0.0, width=w, height=h, spp=8)
    assert "denoise_variance_guided ignored" in capfd.readouterr().err
    assert not got["guided"] and (got["variance_buffer"] == -1).all()
    assert got["render_accumulator"].tobytes() == today["render_accumulator"].tobytes()
    assert got["denoise_buffer"].tobytes() == today["denoise_buffer"].tobytes()
    got = ds.render_dropin_denoise_guided(0.0, samples_per_pass=40, width=w, height=h, spp=72)     # 72 is no multiple of 64
    assert "denoise_variance_guided ignored" in capfd.readouterr().err and not got["guided"]
    assert got["denoise_buffer"].tobytes() == ds.render_dropin_denoise(w, h, 72)["denoise_buffer"].tobytes()
    got = ds.render_dropin_denoise_guided(0.0, samples_per_pass=48, width=w, height=h, spp=128)
    assert "ignored" not in capfd.readouterr().err and got["guided"]
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel = w, h, 128
    sc = capi.Scene(ctx, ds.desc)
    acc = capi.Accumulator(ctx, w, h)
    try:
        acc.accumulate(sc, cam, ds.env, ds.seed, 128)
        assert got["render_accumulator"].tobytes() == acc.resolve().tobytes()
        assert got["variance_buffer"].tobytes() == acc.variance().tobytes()
        a, n, _ = sc.render_aov(cam, ds.seed, 1.0)
        assert got["denoise_buffer"].tobytes() == acc.denoise(capi.DenoiseGuidedParams.defaults(), a, n)[0].tobytes()
    finally:
        acc.close(); sc.close()
