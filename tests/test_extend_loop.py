"""The lean EXTEND's loop (zr_stream.hip stream_extend<., 0>): the phase of an iteration is chosen on the scalar unit, the three phases are separate wave-uniform
ifs, and while every slot of a pool is active (the pool's control word CTL_INACTIVE is 0) FETCH asks for a slot's ray without reading its meta word first.  None of
it may change a result: with the skip switched off (ZR_EXTEND_ALL_ACTIVE=0, read per render) the frame, the books and the traced hits are the same bit for bit; a
pool with slots that never get a unit, a hand-out that ends in the middle of a SHADE launch, the drain pool and pools of one chunk or of a ragged last chunk
render what the CPU oracle renders, with exactly its number of segments: a slot without a path that was walked would be a segment too many.
Context.extend_fetches() says how the counting render's EXTEND fetched its slots: (meta word tested, meta word skipped)."""
import numpy as np
import pytest

from conftest import demo_scene
from test_render_paths import _check, _small_camera
from test_shade_in_place import GROUND, _oracle, _same, _triangles, world_ground_and_ball

gpu = pytest.mark.gpu

BOOKS = ("primary_samples", "segments", "nodes_tested", "spheres_tested", "triangles_tested", "cubes_tested", "media_tested", "hits", "rng_draws", "node_execs",
         "node_lanes", "leaf_execs", "leaf_lanes", "shade_execs", "shade_lanes", "rounds", "path", "escaped")   # every field of zr_counters but the three times
# node_execs and leaf_execs count a wave's iterations, and those depend on which rays share a wave: on which wave's atomic drew which chunk of slots, i.e. on timing.
# Two renders of one frame differ in them whatever the switch says (575341 against 574977 NODE iterations on the reduced cfg3 here; the lane-steps, node_lanes
# and leaf_lanes, are sums over rays and equal).  They are compared where one wave draws every slot: a pool of a single chunk.
SCHEDULE = ("node_execs", "leaf_execs")


def world_mixed():
    """ground sphere, a ball and a strip of 40 triangles above the ground, ONE lambertian: both leaf kinds of the lean build"""
    w = _triangles(40)()
    m = 0
    w.sphere(GROUND[0], GROUND[1] - 1.0, m)
    w.sphere((0.0, 0.3, 0.0), 1.2, m)
    return w


def _render_both(ctx, sc, cam, env, seed, monkeypatch, skip):
    """(product frame, counting frame, counters, (checked, skipped)) with the all-active FETCH on or off"""
    if not skip:
        monkeypatch.setenv("ZR_EXTEND_ALL_ACTIVE", "0")
    try:
        plain = sc.render(cam, env, seed, None)
        counted = sc.render(cam, env, seed, None, count=True)
        ctr = ctx.counters()
        fetches = ctx.extend_fetches()
        assert ctr.path == 2
        return plain, counted, ctr, fetches
    finally:
        if not skip:
            monkeypatch.delenv("ZR_EXTEND_ALL_ACTIVE")


def _on_off(ctx, sc, cam, env, seed, monkeypatch, what, one_chunk=False):
    """both settings: frames bit-equal (product, counting, one against the other), every counter equal (SCHEDULE's two in a pool of one chunk only), the same
    number of slots fetched, none of them skipped with the switch off.  Returns the switch-on (frame, counters, fetches)."""
    on_plain, on_counted, on, on_f = _render_both(ctx, sc, cam, env, seed, monkeypatch, True)
    off_plain, off_counted, off, off_f = _render_both(ctx, sc, cam, env, seed, monkeypatch, False)
    print(f"{what}: segments {on.segments}, rounds {on.rounds}; slots fetched (checked, skipped): on {on_f}, off {off_f}")
    _same(on_plain, off_plain, what + ": product build, on against off")
    _same(on_counted, off_counted, what + ": counting build, on against off")
    _same(on_plain, on_counted, what + ": counting against product build")
    for f in BOOKS:
        if f in SCHEDULE and not one_chunk:
            continue
        assert getattr(on, f) == getattr(off, f), (what, f, getattr(on, f), getattr(off, f))
    assert off_f[1] == 0 and off_f[0] == on_f[0] + on_f[1], (what, on_f, off_f)
    return on_plain, on, on_f


def _lean_scene(capi, ctx, desc):
    sc = capi.Scene(ctx, desc)
    k = sc.kernels()
    assert k["extend_level"] == 0 and k["shade_lean"] == 1, k
    return sc


# ---- 1: the switch changes nothing ---------------------------------------------------------------------------------------------------------------------------

@gpu
def test_switch_on_equals_switch_off_cfg3(built, monkeypatch):
    """cfg3 with the reduced mesh at 480 x 270, 16 spp: most rounds regenerate in place, so most slots are fetched without their meta word"""
    from raytracer_project_amd import capi
    ds = demo_scene("cfg3", (200, 20, 256, 128))
    cam = ds.camera.copy(); cam.samples_per_pixel = 16
    cam.image_width, cam.image_height = 480, 270
    ctx = capi.Context(0)
    try:
        sc = _lean_scene(capi, ctx, ds.desc)
        try:
            frame, ctr, fetches = _on_off(ctx, sc, cam, ds.env, ds.seed, monkeypatch, "cfg3 16 spp")
        finally:
            sc.close()
    finally:
        ctx.close()
    assert float(frame.sum()) > 0 and ctr.hits > 0
    assert fetches[0] > 0 and fetches[1] > 0, fetches   # the rounds that regenerate in place skip the word, the rounds after the hand-out test it


@gpu
@pytest.mark.parametrize("n", [1, 64, 1000, 1024, 4097])
def test_traced_hits_equal_with_the_switch_off(n, built, monkeypatch):
    """zr_trace through EXTEND (stream_load_rays, stream_extend, stream_hits_out): n a multiple of 64 makes every slot active (the word stays 0), any other n
    leaves slots beyond the rays (stream_load_rays sets it).  The hit records — t, point, normal, material of the primitive that answered — are the same bytes."""
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_TRACE_ENGINE", "extend")
    world = world_mixed()
    rng = np.random.default_rng(900 + n)
    rays = np.empty((n, 6))
    rays[:, :3] = np.array([6.0, 2.5, 7.0]) + rng.normal(0, 0.5, (n, 3))
    rays[:, 3:] = np.array([-6.0, -2.6, -7.0]) + rng.normal(0, 2.5, (n, 3))
    ctx = capi.Context(0)
    try:
        sc = _lean_scene(capi, ctx, world.desc)
        try:
            on = sc.trace(rays)
            monkeypatch.setenv("ZR_EXTEND_ALL_ACTIVE", "0")
            off = sc.trace(rays)
        finally:
            sc.close()
    finally:
        ctx.close()
    assert on.tobytes() == off.tobytes(), (n, int((on["t"] != off["t"]).sum()))
    hit = on["mat"] != 0xFFFFFFFF
    if n >= 64:
        assert hit.any() and not hit.all(), (n, int(hit.sum()))


# ---- 2 - 5: pools with inactive slots, against the CPU oracle -----------------------------------------------------------------------------------------------

def _against_oracle(capi, key, world, cam, env, seed, monkeypatch, what, one_chunk=False):
    """renders with the switch on and off; radiance within the render tests' tolerance of the oracle, (segments, draws, hits) exactly the oracle's"""
    ref, rbooks = _oracle(key, world, cam, env, seed)
    ctx = capi.Context(0)
    try:
        sc = _lean_scene(capi, ctx, world.desc)
        try:
            frame, ctr, fetches = _on_off(ctx, sc, cam, env, seed, monkeypatch, what, one_chunk)
            loop = ctx.round_loop()
        finally:
            sc.close()
    finally:
        ctx.close()
    _check(frame, ref, what)
    assert (ctr.segments, ctr.rng_draws, ctr.hits) == rbooks, (what, (ctr.segments, ctr.rng_draws, ctr.hits), rbooks)
    assert ctr.primary_samples == cam.image_width * cam.image_height * cam.samples_per_pixel
    return frame, ctr, fetches, loop


@gpu
@pytest.mark.parametrize("shape", [(16, 8), (15, 7), (1, 1)], ids=["16x8", "15x7", "1x1"])
def test_fewer_units_than_slots(shape, built, monkeypatch):
    """1 spp.  15 x 7 and 1 x 1: the pool is rounded up to whole waves (128 and 64 slots for 105 units and 1), stream_init leaves the slots behind the units
    inactive and sets the word, so no slot is ever fetched unchecked.  16 x 8: 128 units in 128 slots, the first round skips the word for all of them."""
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_FUSED", "0")
    monkeypatch.setenv("ZR_SKY_PREPASS", "0")   # every pixel through the pool
    world = world_mixed()
    cam, env = _small_camera()
    cam.image_width, cam.image_height, cam.samples_per_pixel = shape[0], shape[1], 1
    units = shape[0] * shape[1]
    what = f"{shape[0]}x{shape[1]} at 1 spp"
    _, ctr, fetches, _ = _against_oracle(capi, ("extend_loop_units", shape), world, cam, env, 7001 + units, monkeypatch, what, one_chunk=True)
    slots = (units + 63) // 64 * 64
    if slots > units:
        assert fetches[1] == 0 and fetches[0] >= slots, (what, fetches, slots)
    else:
        assert fetches[1] == slots and fetches[0] > 0, (what, fetches, slots)   # the first launch only: the first SHADE ends paths and has no unit to give them


@gpu
def test_units_run_out_in_the_middle_of_a_shade_launch(built, monkeypatch):
    """96 x 64 at 3 spp on a pool capped at 16384 slots (ZR_STREAM_SLOTS, read when the context is made): 2048 units are left for the first SHADE launch, fewer
    than the paths it ends, so lanes of one launch get the last units and others none.  The EXTEND launches before it skip the word, the ones after it test
    it; the frame is the one the uncapped pool renders."""
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_FUSED", "0")
    monkeypatch.setenv("ZR_SKY_PREPASS", "0")
    world = world_mixed()
    cam, env = _small_camera()
    cam.image_width, cam.image_height, cam.samples_per_pixel = 96, 64, 3
    seed = 7301
    ctx = capi.Context(0)
    try:
        sc = _lean_scene(capi, ctx, world.desc)
        try:
            uncapped = sc.render(cam, env, seed, None)
        finally:
            sc.close()
    finally:
        ctx.close()
    monkeypatch.setenv("ZR_STREAM_SLOTS", "16384")
    frame, ctr, fetches, _ = _against_oracle(capi, "extend_loop_mid_launch", world, cam, env, seed, monkeypatch, "capped pool")
    _same(frame, uncapped, "capped against uncapped pool")
    assert fetches[1] == 16384 and fetches[0] >= 16384, fetches   # the first launch skipped the word, every later one tested it: the units ran out in the first SHADE


@gpu
def test_drain_pool(built, monkeypatch):
    """The frame of test_shade_in_place's small pool (16384 slots, 64 x 48 at 16 spp, depth 50): the last paths are finished on the drain pool, whose slots behind
    the survivors stream_compact_pad leaves inactive.  The frame is the one rendered without the drain pool (ZR_STREAM_DRAIN_POOL=0) and the oracle's."""
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_FUSED", "0")
    monkeypatch.setenv("ZR_SKY_PREPASS", "0")
    monkeypatch.setenv("ZR_STREAM_SLOTS", "16384")
    world = world_ground_and_ball()
    cam, env = _small_camera()
    cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth = 64, 48, 16, 50
    seed = 5107
    frame, ctr, fetches, loop = _against_oracle(capi, "small_pool", world, cam, env, seed, monkeypatch, "drain pool")
    assert loop[0] > 0, loop   # the survivors did move
    monkeypatch.setenv("ZR_STREAM_DRAIN_POOL", "0")
    ctx = capi.Context(0)
    try:
        sc = _lean_scene(capi, ctx, world.desc)
        try:
            no_drain = sc.render(cam, env, seed, None)
            assert ctx.round_loop()[0] == 0
        finally:
            sc.close()
    finally:
        ctx.close()
    _same(frame, no_drain, "drain pool against none")
    assert fetches[0] > 0 and fetches[1] > 0, fetches


@gpu
@pytest.mark.parametrize("shape,spp", [((7, 1), 1), ((16, 8), 2), ((20, 20), 1), ((33, 31), 3)], ids=["64", "256", "448", "3072+"])
def test_one_chunk_and_ragged_pools(shape, spp, built, monkeypatch):
    """pools of one wave (64 slots), of exactly one chunk (256), of a chunk and a ragged one (448 = 256 + 192) and of twelve chunks less 59 slots (3069 units in
    3072 slots: the last wave has inactive slots)"""
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_FUSED", "0")
    monkeypatch.setenv("ZR_SKY_PREPASS", "0")
    world = world_mixed()
    cam, env = _small_camera()
    cam.image_width, cam.image_height, cam.samples_per_pixel = shape[0], shape[1], spp
    units = shape[0] * shape[1] * spp
    what = f"{shape[0]}x{shape[1]} at {spp} spp"
    slots = (units + 63) // 64 * 64
    _, ctr, fetches, _ = _against_oracle(capi, ("extend_loop_pool", shape, spp), world, cam, env, 7501 + units, monkeypatch, what, one_chunk=slots <= 256)
    assert fetches[1] == (slots if slots == units else 0) and fetches[0] >= slots, (what, fetches, slots)   # all units are dealt at initialisation
