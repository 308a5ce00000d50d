"""Lean SHADE's escape stage (zr_stream.hip stream_shade, zr_device.h ray_escapes): a scattered ray that provably leaves the world ends its path in the
round that made it instead of travelling through EXTEND.  Only certain misses are resolved there, by the arithmetic that resolves them anyway, so
NOTHING may change: the frame is the frame with the stage switched off (ZR_SHADE_ESCAPE=0, read at commit), bit for bit, the counters are the same, and
small hand-built worlds still match the CPU oracle.  zr_counters::escaped says how many segments took the short way; zr_counters::shade_lanes counts, from
SHADE's side, the segments EXTEND traced, so escaped + shade_lanes == segments ties the two kernels' books together."""
import math

import numpy as np
import pytest

from conftest import demo_scene
from test_render_paths import World, _check, _small_camera

pytestmark = pytest.mark.gpu


def _render(ctx, desc, cam, env, seed, reg, escape, monkeypatch):
    """(frame of the product build, frame of the counting build, counters) with the stage on / off"""
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_SHADE_ESCAPE", "1" if escape else "0")
    sc = capi.Scene(ctx, desc)
    try:
        assert sc.kernels()["shade_lean"] == 1
        plain = sc.render(cam, env, seed, reg)
        counted = sc.render(cam, env, seed, reg, count=True)
        ctr = ctx.counters()
        assert ctr.path == 2
        return plain, counted, ctr, sc.tree_boxes()
    finally:
        sc.close()
        monkeypatch.delenv("ZR_SHADE_ESCAPE")


def _books(ctr):
    return (ctr.primary_samples, ctr.segments, ctr.rng_draws, ctr.hits)


def _same(a, b, what):
    d = a != b
    assert not d.any(), (what, int(d.sum()), float(np.abs(a - b).max()))


@pytest.mark.parametrize("name,args,spp", [("cfg3", (200, 20, 256, 128), 16), ("cfg2", (), 4)])
def test_switch_on_equals_switch_off(name, args, spp, built, monkeypatch):
    """cfg3 with the reduced mesh and cfg2's 640x360 region (the shapes of test_lean_shade_build_renders_the_general_builds_image): frames bit-equal,
    (primary_samples, segments, rng_draws, hits) equal, and with the stage on some segments did escape and the two kernels' counts add up"""
    from raytracer_project_amd import capi
    ds = demo_scene(name, args)
    cam = ds.camera.copy(); cam.samples_per_pixel = spp
    reg = capi.Region(0, 0, 640, 360, 0, 0, 0, 0) if name == "cfg2" else None
    ctx = capi.Context(0)
    try:
        on_plain, on_counted, on, _ = _render(ctx, ds.desc, cam, ds.env, ds.seed, reg, True, monkeypatch)
        off_plain, off_counted, off, _ = _render(ctx, ds.desc, cam, ds.env, ds.seed, reg, False, monkeypatch)
    finally:
        ctx.close()
    print(f"{name}: segments {on.segments}, escaped {on.escaped} ({on.escaped / on.segments:.3f}), rounds {on.rounds} against {off.rounds}")
    _same(on_plain, off_plain, name + ": product build")
    _same(on_counted, off_counted, name + ": counting build")
    _same(on_plain, on_counted, name + ": counting against product build")
    assert float(on_plain.sum()) > 0
    assert _books(on) == _books(off), (name, _books(on), _books(off))
    assert on.nodes_tested == off.nodes_tested, (name, on.nodes_tested, off.nodes_tested)   # an escaped segment's root boxes are counted where they are tested
    assert off.escaped == 0 and on.escaped > 0, (name, on.escaped, off.escaped)
    assert on.escaped + on.shade_lanes == on.segments, (name, on.escaped, on.shade_lanes, on.segments)
    assert off.shade_lanes == off.segments, (name, off.shade_lanes, off.segments)


# ---- small worlds against the CPU oracle ---------------------------------------------------------------------------------------------------------------

def _grey(w):
    return w.lambertian((0.5, 0.5, 0.5))


def world_ground_alone():
    """a ground sphere alone: the world is one leaf of one sphere, and every scattered ray leaves it"""
    w = World()
    w.sphere((0.0, -500.0, 0.0), 498.5, _grey(w))
    return w


def world_ground_and_glass():
    """a ground sphere and a glass sphere: rays are made INSIDE the glass, and inside is where a sphere may never be ruled out"""
    w = World()
    w.sphere((0.0, -500.0, 0.0), 498.5, _grey(w))
    w.sphere((0.0, 0.0, 0.0), 1.5, w.material(2, w.solid((1, 1, 1)), 1.5))
    return w


def world_single_ball():
    """one small sphere: a root with a single child and three empty ones, most camera rays miss its box"""
    w = World()
    w.sphere((0.0, 0.3, 0.0), 2.0, w.lambertian((0.7, 0.3, 0.2)))
    return w


def world_triangle_floor():
    """16 x 16 x 2 triangles and no sphere: every child of the root is an inner node, so only the box test can let a ray go.  A hit point lies inside the
    box of its own subtree, so a ray escapes only where the surface IS the box's face: the floor is flat at the top of the root boxes (a scattered ray starts
    0.0001 above it, the boxes are padded by one float ulp) with dents below it, whose rays start inside a box and stay with EXTEND"""
    w = World()
    m = w.lambertian((0.4, 0.6, 0.3))
    n, s = 16, 0.5
    for i in range(n):
        for j in range(n):
            x0, z0 = (i - n / 2) * s, (j - n / 2) * s
            y = [-1.5 - (0.3 if (3 * a + 5 * b) % 7 == 0 else 0.0) for a, b in ((i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1))]   # one vertex in seven is a dent
            p = [(x0, y[0], z0), (x0 + s, y[1], z0), (x0, y[2], z0 + s), (x0 + s, y[3], z0 + s)]
            w.add_triangle([p[0], p[2], p[1]], m)
            w.add_triangle([p[1], p[2], p[3]], m)
    return w


def world_huge_ground():
    """a ground sphere of radius 1e5: |oc|^2 2^-44 = 5.7e-4 is above the margin 2.5e-7 |d|^2 for every direction a scatter makes (|d| <= 2), so the guard
    of sphere_miss_certain refuses and only the box test is left — which no ray from the ground passes, because it starts inside the ground's box: the
    sphere's top, where the box ends, lies 3000 to the side and 45 above the part of the surface the camera sees (which passes through (0, -1.5, 0))"""
    w = World()
    w.sphere((3000.0, -1.5 - math.sqrt(1e10 - 9e6), 0.0), 100000.0, _grey(w))
    return w


SMALL = {"ground_alone": world_ground_alone, "ground_and_glass": world_ground_and_glass, "single_ball": world_single_ball,
         "triangle_floor": world_triangle_floor, "huge_ground": world_huge_ground}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_world_matches_oracle(name, built, monkeypatch):
    """64 x 36, 4 spp, through the pipeline (ZR_FUSED=0): radiance within the render tests' tolerance of the CPU oracle, (segments, draws, hits) exactly the
    oracle's, the frame bit-equal to the stage switched off — and what each world is there for"""
    from oracle import zr_oracle_py as zo
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_FUSED", "0")
    world = SMALL[name]()
    cam, env = _small_camera()
    cam.image_width, cam.image_height, cam.samples_per_pixel = 64, 36, 4
    seed = 977 + len(name)
    ctx = capi.Context(0)
    try:
        on_plain, on_counted, on, boxes = _render(ctx, world.desc, cam, env, seed, None, True, monkeypatch)
        off_plain, _, off, _ = _render(ctx, world.desc, cam, env, seed, None, False, monkeypatch)
    finally:
        ctx.close()
    ref, rctr, _, _ = zo.OracleScene(world.desc).render(cam, env, seed, None)
    top = boxes[(boxes["tree"] == 0) & (boxes["depth"] <= 2)]
    print(f"{name}: segments {on.segments}, hits {on.hits}, escaped {on.escaped}; boxes to depth 2 (depth, leaf, kind, count): "
          f"{[(int(b['depth']), int(b['leaf']), int(b['kind']), int(b['count'])) for b in top]}")
    leaves = top[top["leaf"] == 1]
    one_sphere_world = len(top) == 2 and len(leaves) == 1 and leaves[0]["kind"] == 0 and leaves[0]["count"] == 1   # the root's box and its only child
    _check(on_plain, ref, name)
    _same(on_plain, off_plain, name + ": on against off")
    _same(on_plain, on_counted, name + ": counting against product build")
    assert (on.segments, on.rng_draws, on.hits) == (rctr.segments, rctr.rng_draws, rctr.hits), (name, _books(on), (rctr.segments, rctr.rng_draws, rctr.hits))
    assert _books(on) == _books(off)
    assert on.escaped + on.shade_lanes == on.segments and off.escaped == 0
    assert float(ref.sum()) > 0 and on.hits > 0
    if name == "ground_alone":
        # every hit is a camera ray's, its scattered ray points out of the sphere, and it escapes unless the guard refuses: |n + u|^2 = 2 + 2 cos(theta) below
        # |oc|^2 2^-44 / 2.5e-7 = 0.0565, a share of 1.4 % of the directions; those few go to EXTEND and miss there
        assert one_sphere_world
        assert 0.97 * on.hits <= on.escaped <= on.hits, (on.escaped, on.hits)
        assert on.segments == on.primary_samples + on.hits
    elif name == "ground_and_glass":
        assert (leaves["kind"] == 0).all() and int(leaves["count"].sum()) == 2
        assert on.escaped > 0
    elif name == "single_ball":
        assert one_sphere_world
        assert 0 < on.escaped <= on.hits
    elif name == "triangle_floor":
        assert len(top) >= 7 and not top["leaf"].any(), "a root child is a leaf"
        assert on.escaped > 0
    elif name == "huge_ground":
        assert one_sphere_world
        assert on.escaped == 0, on.escaped
