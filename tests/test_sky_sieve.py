"""The one-ray sieve in front of the sky pre-pass (zr_sky.hip sky_sieve): a thread per pixel asks of the pixel's first camera ray what the pre-pass asks of all of
them, and only pixels whose first ray escapes get the pre-pass's wave.  A pixel is sky only if every ray escapes, so the sieve can only remove pixels the
pre-pass would have kept for the pipeline: with the sieve on (ZR_SKY_SIEVE=1, read per render) and off (the default: it gains less than a frame's run-to-run
spread, profiles/r25_round_loop_ab.txt) the frames are equal bit for bit and the pre-pass resolves the same number of pixels.

A progressive batch with sample0 != 0 is not here: a batch of an accumulator renders into per-sample radiance (no frame to write a sky pixel's mean into, its own
pixel list), and render_stream runs the pre-pass only for a frame it reduces itself, which always starts at sample 0.  The sieve still takes sample0 as the
pre-pass does, so that the two agree on which ray is a pixel's first."""
import numpy as np
import pytest

import frame_edge_worlds as fw
from conftest import demo_scene

pytestmark = pytest.mark.gpu


def _on_off(ctx, sc, cam, env, seed, monkeypatch, what):
    monkeypatch.setenv("ZR_SKY_SIEVE", "1")
    try:
        on = sc.render(cam, env, seed, None)
        n_on = ctx.presolved_pixels()
        assert ctx.counters().path == 2
        monkeypatch.setenv("ZR_SKY_SIEVE", "0")
        off = sc.render(cam, env, seed, None)
        n_off = ctx.presolved_pixels()
    finally:
        monkeypatch.delenv("ZR_SKY_SIEVE")
    default = sc.render(cam, env, seed, None)
    assert np.array_equal(default, off) and ctx.presolved_pixels() == n_off, f"{what}: the default is the pre-pass without the sieve"
    monkeypatch.setenv("ZR_SKY_PREPASS", "0")
    try:
        walked = sc.render(cam, env, seed, None)
        assert ctx.presolved_pixels() == 0
    finally:
        monkeypatch.delenv("ZR_SKY_PREPASS")
    n = cam.image_width * cam.image_height
    print(f"{what}: pre-solved {n_on} of {n} pixels with the sieve, {n_off} without")
    assert np.array_equal(on, off), f"{what}: sieve on against off"
    assert np.array_equal(on, walked), f"{what}: against the frame without the pre-pass"
    assert n_on == n_off, (what, n_on, n_off)
    return n_on, n


@pytest.fixture(scope="module")
def cfg3(built):
    from raytracer_project_amd import capi
    ds = demo_scene("cfg3", (200, 20, 256, 128))
    ctx = capi.Context(0)
    sc = capi.Scene(ctx, ds.desc)
    yield ds, ctx, sc
    sc.close()
    ctx.close()


@pytest.mark.parametrize("spp", [16, 80])
def test_cfg3(spp, cfg3, monkeypatch):
    """the reduced-mesh cfg3 of test_sky_prepass.py at 480 x 270: sky, mesh and the horizon between them, where a pixel's first ray may escape and a later one stay"""
    ds, ctx, sc = cfg3
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel = 480, 270, spp
    n_sky, n = _on_off(ctx, sc, cam, ds.env, ds.seed, monkeypatch, f"cfg3 {spp} spp")
    assert 0.10 * n <= n_sky < n


CELLS = [
    fw.all_sky_cell(),   # every pixel a candidate; n_walk == 0
    # no sky pixel: looking down at the ground sphere, no pixel is a candidate
    fw.Cell("no_sky_7x5", "open", fw.open_camera(7, 5, fw.SHAPE_SPP, fw.SHAPE_DEPTH, lookat=(0.0, -20.0, 0.0)), 7011),
    # all sky and more candidates (33 667) than the candidates' grid has waves (32 768): the stride of sky_prepass_candidates; 131 rows of 257: no whole block
    fw.Cell("sky_257x131", "open", fw.open_camera(257, 131, fw.SHAPE_SPP, fw.SHAPE_DEPTH, lookat=(0.0, 20.0, 0.0)), 7013),
]


@pytest.mark.parametrize("cell", [pytest.param(c, id=c.name) for c in CELLS])
def test_small_worlds(cell, built, monkeypatch):
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_FUSED", "0")
    ctx = capi.Context(0)
    sc = capi.Scene(ctx, cell.world.scene_desc)
    try:
        n_sky, n = _on_off(ctx, sc, cell.cam, fw.solid_env(), cell.seed, monkeypatch, cell.name)
    finally:
        sc.close(); ctx.close()
    assert n_sky == (0 if cell.name.startswith("no_sky") else n), (cell.name, n_sky, n)
