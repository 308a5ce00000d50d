"""The sky pre-pass (raytracer_project_amd/csrc/zr_sky.hip, zr_device.h camera_ray_escapes): before the streaming pipeline starts, a pixel whose every camera
ray provably sees only the environment is finished by one wave — begin_sample's ray, the MISS stage's background, stream_reduce's sum — and never becomes a
work unit.  Only certain misses are resolved there, by the arithmetic that resolves them anyway, so NOTHING may change: the frame is the frame with the pre-pass
switched off (ZR_SKY_PREPASS=0, read per render), bit for bit, and the frame of the counting render, which never takes the pre-pass; small hand-built worlds
still match the CPU oracle.  Context.presolved_pixels() says how many pixels took the short way."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import demo_scene
from test_render_paths import World, _check, _small_camera

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    d = a != b
    assert not d.any(), (what, int(d.sum()), float(np.abs(a - b).max()))


def _three(ctx, sc, cam, env, seed, reg, monkeypatch):
    """(frame with the pre-pass, pixels it resolved, frame without it, frame of the counting render); the last two must report no presolved pixel"""
    on = sc.render(cam, env, seed, reg)
    presolved = ctx.presolved_pixels()
    assert ctx.counters().path == 2
    monkeypatch.setenv("ZR_SKY_PREPASS", "0")
    try:
        off = sc.render(cam, env, seed, reg)
        assert ctx.presolved_pixels() == 0
    finally:
        monkeypatch.delenv("ZR_SKY_PREPASS")
    counted = sc.render(cam, env, seed, reg, count=True)
    assert ctx.presolved_pixels() == 0
    ctr = ctx.counters()
    assert ctr.path == 2 and ctr.escaped + ctr.shade_lanes == ctr.segments
    return on, presolved, off, counted


# ---- cfg3 with the reduced mesh --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cfg3(built):
    from raytracer_project_amd import capi
    ds = demo_scene("cfg3", (200, 20, 256, 128))
    ctx = capi.Context(0)
    sc = capi.Scene(ctx, ds.desc)
    assert sc.kernels()["shade_lean"] == 1
    yield ds, ctx, sc
    sc.close()
    ctx.close()


def _cfg3_camera(ds, spp):
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel = 480, 270, spp
    return cam


@pytest.mark.parametrize("spp", [16, 80])
def test_cfg3_frame_is_the_frame_without_the_prepass(spp, cfg3, monkeypatch):
    """480 x 270 at 16 spp (lanes with no sample) and 80 spp (uneven lane loads): bit-equal to the pre-pass switched off and to the counting render, and at least
    10 % of the pixels are resolved (the CPU estimate from pixel centres is 17.2 %; the margin is for the pixels the horizon runs through)"""
    ds, ctx, sc = cfg3
    cam = _cfg3_camera(ds, spp)
    on, presolved, off, counted = _three(ctx, sc, cam, ds.env, ds.seed, None, monkeypatch)
    n = cam.image_width * cam.image_height
    print(f"cfg3 {spp} spp: presolved {presolved} of {n} pixels ({presolved / n:.4f})")
    _same(on, off, "pre-pass on against off")
    _same(on, counted, "pre-pass on against the counting render")
    assert float(on.sum()) > 0
    assert presolved >= 0.10 * n, (presolved, n)


def test_tile_shards(cfg3, monkeypatch):
    """every other tile of the frame, as multi.tile_region deals them to rank 0 of 2: the shard's pixels bit-equal, the others untouched"""
    from raytracer_project_amd import capi, multi
    ds, ctx, sc = cfg3
    cam = _cfg3_camera(ds, 16)
    shares = []
    for rank in (0, 1):
        reg = multi.tile_region(capi, rank, 2)
        on, presolved, off, counted = _three(ctx, sc, cam, ds.env, ds.seed, reg, monkeypatch)
        _same(on, off, f"rank {rank}: pre-pass on against off")
        _same(on, counted, f"rank {rank}: pre-pass on against the counting render")
        assert presolved > 0
        shares.append((on, presolved))
    whole = sc.render(cam, ds.env, ds.seed, None)
    total = ctx.presolved_pixels()
    print(f"tile shards: presolved {shares[0][1]} + {shares[1][1]} of the frame's {total}")
    assert shares[0][1] + shares[1][1] == total
    _same(shares[0][0] + shares[1][0], whole, "the two shards against the whole frame")   # (a shard leaves the other's pixels at zero)


def test_polled_render(cfg3, monkeypatch):
    """keep_going set and never cleared: the polled round loop (samples[] zeroed, previews possible) over the compacted list gives the same frame"""
    from raytracer_project_amd import capi
    ds, ctx, sc = cfg3
    cam = _cfg3_camera(ds, 16)
    plain = sc.render(cam, ds.env, ds.seed, None)
    want = ctx.presolved_pixels()
    keep_going = C.c_uint8(1)
    polled = np.zeros_like(plain)
    capi._check(ctx.lib.zr_render(ctx._c, sc._s, C.byref(cam), C.byref(ds.env), C.c_uint64(ds.seed), None, 0, polled.ctypes.data,
                                  C.cast(C.byref(keep_going), C.c_void_p), None))
    assert ctx.presolved_pixels() == want > 0
    _same(polled, plain, "polled against plain")
    monkeypatch.setenv("ZR_SKY_PREPASS", "0")
    off = np.zeros_like(plain)
    capi._check(ctx.lib.zr_render(ctx._c, sc._s, C.byref(cam), C.byref(ds.env), C.c_uint64(ds.seed), None, 0, off.ctypes.data,
                                  C.cast(C.byref(keep_going), C.c_void_p), None))
    assert ctx.presolved_pixels() == 0
    _same(polled, off, "polled: pre-pass on against off")


# ---- small worlds against the CPU oracle ---------------------------------------------------------------------------------------------------------------

GROUND = ((0.0, -500.0, 0.0), 498.5)   # its top is y = -1.5
HUGE = ((3000.0, -1.5 - math.sqrt(1e10 - 9e6), 0.0), 100000.0)   # test_shade_escape.py: world_huge_ground


def _ball():
    w = World()
    w.sphere((0.0, 0.3, 0.0), 2.0, w.lambertian((0.7, 0.3, 0.2)))
    return w


def _ground(sphere=GROUND):
    w = World()
    w.sphere(sphere[0], sphere[1], w.lambertian((0.5, 0.5, 0.5)))
    return w


def _look(cam, lookfrom, lookat, vfov=None):
    for c in range(3):
        cam.lookfrom[c] = lookfrom[c]
        cam.lookat[c] = lookat[c]
    if vfov is not None:
        cam.vfov = vfov


# name: (world, sphere of a one-sphere world or None, camera set-up)
#  single_ball      most rays miss every box
#  horizon          the ground's horizon in frame (7.2 degrees below the horizontal, the frame's top 11.6 above it): the rows above it pass the sphere overhead
#  grazing          the camera 0.06 above the ground, looking along it at the sphere's top: the horizon (0.1 to 0.3 degrees down; a pixel row is 1.4) runs
#                   through the row below the frame's centre
#  ground_fills     the camera looks down with a narrow field of view: no sky in frame
#  empty_sky        the camera looks away from the only object: every pixel is sky and the pipeline does not run at all
#  huge_ground      a ground sphere of radius 1e5
SMALL = {
    "single_ball": (_ball, ((0.0, 0.3, 0.0), 2.0), lambda cam: None),
    "horizon": (_ground, GROUND, lambda cam: None),
    "grazing": (_ground, GROUND, lambda cam: _look(cam, (0.0, -1.49, 7.0), (0.0, -1.49, 0.0))),
    "ground_fills": (_ground, GROUND, lambda cam: _look(cam, (6.0, 2.5, 7.0), (0.0, -1.5, 0.0), 20)),
    "empty_sky": (_ball, ((0.0, 0.3, 0.0), 2.0), lambda cam: _look(cam, (6.0, 2.5, 7.0), (12.0, 8.0, 14.0))),
    "huge_ground": (lambda: _ground(HUGE), None, lambda cam: None),
}


def _sky_pixels(ctx, cam, seed, sphere):
    """of a one-sphere world: (pixels whose every camera ray misses the sphere, pixels with rays on both sides), from the rays the device makes (zr_kat_camera_rays)
    and the sphere's discriminant in extended precision — no ray of these frames comes within 1e-9 (relative) of the horizon, far outside the predicate's 2^-36"""
    W, H, spp = cam.image_width, cam.image_height, cam.samples_per_pixel
    req = np.array([(x, y, s) for y in range(H) for x in range(W) for s in range(spp)], dtype=np.int32)
    rays = ctx.kat_camera_rays(cam, seed, req).astype(np.longdouble)
    o, d = rays[:, 0:3], rays[:, 3:6]
    oc = np.array(sphere[0], dtype=np.longdouble) - o
    a, h = (d * d).sum(1), (d * oc).sum(1)
    c = (oc * oc).sum(1) - np.longdouble(sphere[1]) ** 2
    disc = h * h - a * c
    rel = disc / (a * ((oc * oc).sum(1) + np.longdouble(sphere[1]) ** 2))
    assert float(np.abs(rel).min()) > 1e-9, float(np.abs(rel).min())
    assert (c > 0).all()   # the camera is outside
    miss = ((disc < 0) | (h < 0)).reshape(H * W, spp)
    return int(miss.all(1).sum()), int((miss.any(1) & ~miss.all(1)).sum())


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_world_matches_oracle(name, built, monkeypatch):
    """64 x 36, 4 spp, through the pipeline (ZR_FUSED=0): radiance within the render tests' tolerance of the CPU oracle, the frame bit-equal to the pre-pass
    switched off and to the counting render — and what each world is there for.  In a one-sphere world the resolved pixels are exactly those whose every
    camera ray misses the sphere: a pixel the horizon runs through stays with the pipeline."""
    from oracle import zr_oracle_py as zo
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_FUSED", "0")
    make, sphere, aim = SMALL[name]
    world = make()
    cam, env = _small_camera()
    cam.image_width, cam.image_height, cam.samples_per_pixel = 64, 36, 4
    aim(cam)
    seed = 1433 + len(name)
    n = cam.image_width * cam.image_height
    ctx = capi.Context(0)
    try:
        sc = capi.Scene(ctx, world.desc)
        try:
            assert sc.kernels()["shade_lean"] == 1
            on, presolved, off, counted = _three(ctx, sc, cam, env, seed, None, monkeypatch)
            sky, straddling = _sky_pixels(ctx, cam, seed, sphere) if sphere else (None, None)
        finally:
            sc.close()
    finally:
        ctx.close()
    ref, _, _, _ = zo.OracleScene(world.desc).render(cam, env, seed, None)
    print(f"{name}: presolved {presolved} of {n} pixels ({presolved / n:.3f}); pixels whose every ray misses the sphere {sky}, with rays on both sides {straddling}")
    _check(on, ref, name)
    _same(on, off, name + ": pre-pass on against off")
    _same(on, counted, name + ": pre-pass on against the counting render")
    assert float(ref.sum()) > 0
    if sphere:
        assert presolved == sky, (presolved, sky)
    if name in ("single_ball", "horizon"):
        assert 0 < presolved < n and straddling > 0
    elif name == "grazing":
        # the 18 rows above the frame's centre are sky; the row below it holds the horizon, and only its pixels whose four rays all happen to pass above it are sky
        assert straddling > 0 and 18 * 64 <= presolved < 18 * 64 + 32, (presolved, straddling)
    elif name == "ground_fills":
        assert presolved == 0
    elif name == "empty_sky":
        assert presolved == n
