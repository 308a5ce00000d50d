"""The denoiser behind camera::use_denoiser (camera.hpp:268-291): zr_denoise, an edge-avoiding a-trous filter guided by albedo
and normals (NOT OIDN: its contract is the NumPy restatement in tests/denoise_model.py), and zr_sharpen_frame,
post_processor::apply_sharpening on its own.  CPU tests check the ABI surface and the model's properties; GPU tests check the
device against the model, the filter's edge behaviour and quality on real renders, and the drop-in's use_denoiser path."""
import ctypes as C

import numpy as np
import pytest

import denoise_model as dm
from conftest import demo_scene


# ---- CPU: ABI surface --------------------------------------------------------------------------------------------------

def test_denoise_params_mirror_matches_c_struct(built):
    from raytracer_project_amd import capi
    s = capi.load_scenes()
    s.zrs_sizeof.restype = C.c_size_t
    s.zrs_sizeof.argtypes = [C.c_int]
    assert s.zrs_sizeof(14) == C.sizeof(capi.DenoiseParams) == 24


def test_denoise_entry_points_exported(built):
    from raytracer_project_amd import capi
    lib = capi.load()
    for name in ("zr_denoise", "zr_sharpen_frame"):
        assert hasattr(lib, name) and name in capi.CAPI_SYMBOLS
    s = capi.load_scenes()
    assert hasattr(s, "zrs_render_dropin_denoise")


def test_denoise_defaults_match_header(built):
    import os
    import re
    from conftest import ROOT
    from raytracer_project_amd import capi
    txt = open(os.path.join(ROOT, "include", "zr_capi.h")).read()
    want = {k.lower(): float(np.float32(v.rstrip("f"))) for k, v in re.findall(r"#define ZR_DENOISE_DEFAULT_(\w+) ([0-9.]+f?)", txt)}
    assert len(want) == 5
    p = capi.DenoiseParams.defaults()
    assert want == {"iterations": p.iterations, "demodulate": p.demodulate_albedo, "sigma_color": p.sigma_color, "sigma_normal": p.sigma_normal,
                    "sigma_albedo": p.sigma_albedo}
    assert p.sigma_depth == 0.0
    assert dm.denoise_params(p) == dict(iterations=5, demodulate_albedo=False, sigma_color=1.5, sigma_normal=64.0, sigma_albedo=0.25, sigma_depth=0.0)


def test_denoise_refuses_bad_arguments_without_a_device(built):
    """Argument checks come before any device call: NULL context / pointers, sizes, levels and sigmas give ZR_E_INVALID."""
    from raytracer_project_amd import capi
    lib = capi.load()
    f = np.zeros((2, 3, 3))
    p = capi.DenoiseParams.defaults()
    ptr = f.ctypes.data
    assert lib.zr_denoise(None, C.byref(p), ptr, ptr, ptr, None, 3, 2, ptr) == -1
    assert b"null" in lib.zr_last_error()
    assert lib.zr_sharpen_frame(None, ptr, 3, 2, 0.2, ptr) == -1
    fake = C.c_void_p(1)   # never dereferenced: every call below fails its argument checks first
    assert lib.zr_denoise(fake, C.byref(p), ptr, None, ptr, None, 3, 2, ptr) == -1
    assert lib.zr_denoise(fake, C.byref(p), ptr, ptr, ptr, None, 0, 2, ptr) == -1
    assert lib.zr_denoise(fake, C.byref(p), ptr, ptr, ptr, None, 1 << 16, 1 << 16, ptr) == -1
    for kw in (dict(iterations=-1), dict(iterations=9), dict(sigma_color=0.0), dict(sigma_normal=0.0), dict(sigma_albedo=0.0),
               dict(sigma_albedo=-1.0), dict(sigma_depth=-0.5)):
        q = capi.DenoiseParams.defaults(**kw)
        assert lib.zr_denoise(fake, C.byref(q), ptr, ptr, ptr, None, 3, 2, ptr) == -1, kw
    assert lib.zr_sharpen_frame(fake, ptr, 0, 2, 0.2, ptr) == -1
    assert lib.zr_sharpen_frame(fake, ptr, 3, 2, 0.2, None) == -1


# ---- CPU: properties of the model --------------------------------------------------------------------------------------

def _synthetic(w, h, seed, plant=True):
    """noisy HDR colour over an albedo step (vertical) and a normal step (horizontal); NaN / Inf planted in every input"""
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
    if plant:
        for a, vals in ((albedo, (np.nan, np.inf)), (normal, (np.nan, -np.inf)), (color, (np.nan, np.inf)), (zdepth, (np.nan, np.inf))):
            m = rng.random(a.shape) < 0.003
            a[m] = rng.choice(vals, size=int(m.sum()))
    return color, albedo, normal, zdepth


def test_model_constant_frame_is_unchanged():
    h, w = 19, 23
    c = np.full((h, w, 3), 0.3) * np.array([1.0, 2.0, 0.5])
    a = np.full((h, w, 3), 0.6)
    n = np.full((h, w, 3), [0.5, 0.5, 1.0])
    z = np.full((h, w, 3), 0.4)
    for demod in (True, False):
        out = dm.denoise(c, a, n, z, iterations=5, demodulate_albedo=demod, sigma_depth=0.1)
        assert np.allclose(out, c, rtol=4e-7, atol=0), np.abs(out - c).max()


def test_model_zero_iterations_is_the_identity():
    c, a, n, _ = _synthetic(17, 11, 3, plant=False)
    for demod in (True, False):
        out = dm.denoise(c, a, n, iterations=0, demodulate_albedo=demod)
        want = c.astype(np.float32).astype(np.float64)
        assert np.allclose(out, want, rtol=2.5e-7, atol=0)


def test_model_weights_are_normalised():
    """Every level is a convex combination of its taps: the normalised weights sum to one, the centre tap's is positive, taps
    off the frame weigh nothing, and the output stays within the inputs' range channel by channel."""
    c, a, n, z = _synthetic(21, 13, 5, plant=False)
    d, aa, zz, nn, valid = dm.prepare(c, a, n, z, True)
    for level in (0, 1, 3):
        out, w = dm.atrous_level(d, aa, zz, nn, valid, level, 0.5, 64.0, 0.1, 0.05, True, return_weights=True)
        assert w.shape == (25,) + d.shape[:2] and (w >= 0).all() and (w[12] > 0).all()
        wn = w / w.sum(axis=0)
        assert np.allclose(wn.sum(axis=0), 1.0, atol=1e-6)
        assert (w[:, 0, 0].reshape(5, 5)[:2, :] == 0).all() and (w[:, 0, 0].reshape(5, 5)[:, :2] == 0).all()   # corner: up / left taps off
        want = np.einsum("thw,thwc->hwc", wn.astype(np.float64), np.stack([dm._shift(d, ky << level, kx << level) for ky in range(-2, 3)
                                                                          for kx in range(-2, 3)]).astype(np.float64))
        assert np.allclose(out, want, rtol=1e-5, atol=1e-6)
        lo, hi = d.min(axis=(0, 1)), d.max(axis=(0, 1))
        assert (out >= lo * (1 - 1e-6)).all() and (out <= hi * (1 + 1e-6)).all()


def test_model_sharpen_matches_the_reference_loop():
    rng = np.random.default_rng(9)
    f = rng.random((6, 7, 3))
    out = dm.sharpen(f, 0.3)
    want = f.copy()
    for y in range(1, 5):
        for x in range(1, 6):
            s = f[y, x] * 5.0
            s = s - f[y - 1, x]; s = s - f[y + 1, x]; s = s - f[y, x - 1]; s = s - f[y, x + 1]
            want[y, x] = f[y, x] * (1.0 - 0.3) + s * 0.3
    assert np.array_equal(out, want)
    assert np.array_equal(dm.sharpen(f, 0.0), f)


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(built):
    from raytracer_project_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _bound(dev, model):
    """|dev - model| <= 2e-5 |model| + 1e-6 per channel.  The kernel and the model perform the same FP32 operations in the same
    order (no contraction on either side); they differ only in expf / powf, which are within a few ulp of each other — ~1e-7
    relative on a weight, far inside the bound even after five levels."""
    err = np.abs(dev - model)
    lim = 2e-5 * np.abs(model) + 1e-6
    return int((err > lim).sum()), float((err / lim).max())


# every size with and without demodulation and the depth guide (1080p: three settings cover both switches; the model takes seconds there)
MODEL_CASES = [(w, h, demod, depth) for (w, h) in [(1, 1), (7, 5), (333, 77)] for demod in (True, False) for depth in (False, True)] + \
              [(1920, 1080, True, False), (1920, 1080, False, True), (1920, 1080, True, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,demod,depth", MODEL_CASES)
def test_device_matches_model(w, h, demod, depth, ctx):
    from raytracer_project_amd import capi
    c, a, n, z = _synthetic(w, h, 1000 + w + h)
    p = capi.DenoiseParams.defaults(demodulate_albedo=int(demod), sigma_depth=0.05 if depth else 0.0)
    dev = ctx.denoise(p, c, a, n, z if depth else None)
    model = dm.denoise(c, a, n, z if depth else None, **dm.denoise_params(p))
    assert np.isfinite(dev).all()
    bad, worst = _bound(dev, model)
    assert bad == 0, f"{bad} channels outside the bound (worst {worst:.2f} x the bound)"


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [0, 1, 8])
def test_device_matches_model_level_counts(iterations, ctx):
    from raytracer_project_amd import capi
    c, a, n, z = _synthetic(129, 65, 77)
    p = capi.DenoiseParams.defaults(iterations=iterations, sigma_color=1.3, sigma_albedo=0.3, sigma_normal=16.0)
    bad, worst = _bound(ctx.denoise(p, c, a, n), dm.denoise(c, a, n, **dm.denoise_params(p)))
    assert bad == 0, (bad, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("guide", ["albedo", "normal"])
def test_edges_hold(guide, ctx):
    """Colour 0 left and 1 right of a vertical edge, the albedo (or normal) differs across it: after five levels every left
    pixel stays < 1e-3 — a right tap's weight underflows (albedo: exp(-|da|^2 / sigma_a^2)) or is exactly 0 (normals at 90
    degrees: max(0, n.n)^sigma_n)."""
    from raytracer_project_amd import capi
    w, h = 64, 48
    left = np.arange(w)[None, :, None] < w // 2
    c = np.where(left, 0.0, 1.0) * np.ones((h, w, 3))
    if guide == "albedo":
        a = np.where(left, 0.2, 0.8) * np.ones((h, w, 3)); n = np.full((h, w, 3), [0.5, 0.5, 1.0])
    else:
        a = np.full((h, w, 3), 0.5); n = np.where(left, np.array([0.5, 0.5, 1.0]), np.array([1.0, 0.5, 0.5])) * np.ones((h, w, 3))
    out = ctx.denoise(capi.DenoiseParams.defaults(), c, a, n)
    assert out[:, : w // 2].max() < 1e-3
    assert out[:, w // 2:].min() > 1.0 - 1e-3


@pytest.mark.gpu
def test_deterministic_and_in_place(ctx):
    from raytracer_project_amd import capi
    c, a, n, z = _synthetic(333, 77, 11)
    p = capi.DenoiseParams.defaults(sigma_depth=0.05)
    x = ctx.denoise(p, c, a, n, z)
    y = ctx.denoise(p, c, a, n, z)
    assert x.tobytes() == y.tobytes()
    inplace = np.ascontiguousarray(c).copy()
    ctx.denoise(p, inplace, a, n, z, out=inplace)
    assert inplace.tobytes() == x.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (7, 5), (333, 77)])
@pytest.mark.parametrize("amount", [0.2, 0.75, 0.0, -1.0])
def test_sharpen_is_exact(w, h, amount, ctx):
    rng = np.random.default_rng(w * 31 + h)
    f = rng.exponential(1.0, (h, w, 3))
    out = ctx.sharpen(f, amount)
    assert out.tobytes() == dm.sharpen(f, amount).tobytes()
    g = f.copy()
    ctx.sharpen(g, amount, out=g)
    assert g.tobytes() == out.tobytes()


# Quality on real renders: 8 spp denoised vs 8 spp noisy, against 1024 spp of the same camera.  Measured on the MI355X (see
# DESIGN §9): the pins below keep a margin under the measurements; 3x is the bar the feature was asked to clear.
QUALITY = {"cfg5": dict(size=(300, 300), pin=3.5), "mix0": dict(size=(384, 256), pin=3.0)}


def _render_set(ctx, name, spp):
    from conftest import demo_scene
    from raytracer_project_amd import capi
    ds = demo_scene(name)
    cam = ds.camera.copy()
    cam.image_width, cam.image_height = QUALITY[name]["size"]
    cam.samples_per_pixel = spp
    sc = capi.Scene(ctx, ds.desc)
    frame = sc.render(cam, ds.env, ds.seed, None)
    a, n, _ = sc.render_aov(cam, ds.seed, 1.0)
    return frame, a, n


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(QUALITY))
def test_quality_on_real_renders(name, ctx):
    from raytracer_project_amd import capi
    noisy, a, n = _render_set(ctx, name, 8)
    truth, _, _ = _render_set(ctx, name, 1024)
    den = ctx.denoise(capi.DenoiseParams.defaults(), noisy, a, n)
    mse_noisy = float(((noisy - truth) ** 2).mean())
    mse_den = float(((den - truth) ** 2).mean())
    factor = mse_noisy / mse_den
    print(f"denoise quality {name}: MSE noisy {mse_noisy:.4e}, denoised {mse_den:.4e}, factor {factor:.2f}")
    assert factor >= QUALITY[name]["pin"], factor


# ---- drop-in: camera::render with use_denoiser -------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name,size,spp", [("mix0", (0, 0), 8), ("cfg5", (160, 160), 8)])
def test_dropin_use_denoiser(name, size, spp, ctx):
    from raytracer_project_amd import capi
    ds = demo_scene(name)
    w, h = size
    got = ds.render_dropin_denoise(w, h, spp)
    plain, _ = ds.render_dropin(w, h, spp)
    assert got["render_accumulator"].tobytes() == plain.tobytes()            # the raw frame is left exactly as without the flag
    cam = ds.camera.copy()
    cam.image_width, cam.image_height = w or cam.image_width, h or cam.image_height
    cam.samples_per_pixel = spp
    sc = capi.Scene(ctx, ds.desc)
    a, n, _ = sc.render_aov(cam, ds.seed, 1.0)                                 # post_processor's z_depth_max_dist default
    want = ctx.denoise(capi.DenoiseParams.defaults(), plain, a, n)
    assert got["denoise_buffer"].tobytes() == want.tobytes()
    assert not got["albedo_buffer"].any() and not got["normal_buffer"].any()  # public AOV buffers untouched with their flags off
    assert not got["reflection_buffer"].any() and not got["refraction_buffer"].any()
    assert np.abs(got["denoise_buffer"] - plain).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("sharpening", [False, True])
def test_dropin_use_denoiser_passes(sharpening, ctx):
    """With use_reflection / use_refraction the pass frames are denoised in place, then sharpened when post.use_sharpening is
    set (camera.hpp:277-290)."""
    from raytracer_project_amd import capi
    ds = demo_scene("mix0")
    spp = 8
    got = ds.render_dropin_denoise(0, 0, spp, passes=True, sharpening=sharpening)
    cam = ds.camera.copy(); cam.samples_per_pixel = spp
    sc = capi.Scene(ctx, ds.desc)
    beauty, refl, refr = sc.render_passes(cam, ds.env, ds.seed, None)
    a, n, _ = sc.render_aov(cam, ds.seed, 1.0)
    assert got["render_accumulator"].tobytes() == beauty.tobytes()
    p = capi.DenoiseParams.defaults()
    assert got["denoise_buffer"].tobytes() == ctx.denoise(p, beauty, a, n).tobytes()
    for key, raw in (("reflection_buffer", refl), ("refraction_buffer", refr)):
        want = ctx.denoise(p, raw, a, n)
        if sharpening:
            want = ctx.sharpen(want, 0.2)   # post_processor::sharpen_amount default
        assert got[key].tobytes() == want.tobytes(), key
        assert raw.any()
