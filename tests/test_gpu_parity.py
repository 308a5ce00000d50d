"""Parity tests proper: the HIP path (through the C ABI, libzr_hip.so) against
  (a) golden fixtures produced by the genuine reference arithmetic (tests/golden/*.npz), and
  (b) the CPU oracle on the same seeded inputs,
plus size-independent properties at BASELINE.json's full sizes.

Bar (BASELINE.json north_star): radiance within 1e-4 relative per channel on identical RNG seeds; integer
pixel indexing, segment counts and RNG-draw counts bit-exact.  The device computes in FP64 like the reference
but with FMA contraction, so individual values differ from the reference in the last bits (~1e-15 relative);
REL_TOL below is the north-star bound, not a fudge factor."""
import os

import numpy as np
import pytest

from conftest import demo_scene, load_golden, rel_err

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4      # north_star: "within 1e-4 relative per-channel"
ABS_FLOOR = 1e-7    # radiance below this is treated as 0 for the relative comparison

TILE_FIXTURES = ["cfg1_full", "cfg1_tile", "cfg2_tile", "cfg2_tile_b", "cfg3_small", "cfg3_full", "cfg5_tile",
                 "cfg5_tile_b", "mix0_full", "mix1_full", "mix2_full", "mix0_tile", "mesh0_full", "inst0_full", "inst1_full", "inst2_full", "demo_tile", "demo_tile_b", "cfg3w_small"]


@pytest.fixture(scope="module")
def ctx(built):
    from raytracer_project_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


_gpu_scenes = {}


BUILDERS = ["host", "device"]   # zr_bvh.cpp's binned-SAH builder and zr_build.hip's PLOC builder: every fixture through both trees


def gpu_scene(ctx, name, args=(), builder=None):
    """the committed scene, cached; builder = "host" | "device" forces ZR_BVH_BUILD for the commit (None: the library's default)"""
    from raytracer_project_amd import capi
    key = (name, tuple(args), builder)
    if key not in _gpu_scenes:
        old = os.environ.get("ZR_BVH_BUILD")
        if builder:
            os.environ["ZR_BVH_BUILD"] = builder
            os.environ["ZR_BUILD_CHECK"] = "1"   # the device builder checks its object boxes against the host's (zr_entry.h chain_box) and fails the commit on a difference
        try:
            sc = capi.Scene(ctx, demo_scene(name, args).desc)
        finally:
            if builder:
                del os.environ["ZR_BUILD_CHECK"]
                if old is None:
                    del os.environ["ZR_BVH_BUILD"]
                else:
                    os.environ["ZR_BVH_BUILD"] = old
        if builder:
            assert sc.stats()["builder"].startswith(builder), (name, builder, sc.stats()["builder"])
        _gpu_scenes[key] = sc
    return _gpu_scenes[key]


def _check(tile, want, what):
    err = rel_err(tile, want, ABS_FLOOR)
    bad = err > REL_TOL
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} channels exceed {REL_TOL} "
                           f"(max rel err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)})")
    return float(err.max())


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("count", [False, True], ids=["timed", "counting"])
@pytest.mark.parametrize("name", TILE_FIXTURES)
def test_radiance_matches_reference(name, count, builder, ctx):
    """GPU radiance vs the genuine reference's, same scene / camera / seed / spp — through BOTH instantiations of the
    pipeline kernels: the uninstrumented one bench.py times (`count=False`) and the counting one, whose segment and
    RNG-draw totals must equal the reference's exactly."""
    from raytracer_project_amd import capi
    fx = load_golden(name)
    m = fx["meta"]
    ds = demo_scene(m["scene"], m["scene_args"])
    cam = ds.camera.copy()
    cam.samples_per_pixel = m["spp"]
    reg = capi.Region(m["x0"], m["y0"], m["w"], m["h"], 0, 0, 0, 0)
    sc = gpu_scene(ctx, m["scene"], m["scene_args"], builder)
    out = sc.render(cam, ds.env, ds.seed, reg, count=count)
    ctr = ctx.counters()
    tile = out[m["y0"]:m["y0"] + m["h"], m["x0"]:m["x0"] + m["w"]]
    worst = _check(tile, fx["mean"], name)
    if count:
        # integer work accounting is bit-exact: same number of closest-hit queries and of RNG draws
        assert ctr.primary_samples == m["w"] * m["h"] * m["spp"]
        assert ctr.segments == m["segments"], (ctr.segments, m["segments"])
        assert ctr.rng_draws == m["draws"], (ctr.rng_draws, m["draws"])
    # pixels outside the region are untouched (integer pixel indexing)
    mask = np.ones(out.shape[:2], bool)
    mask[m["y0"]:m["y0"] + m["h"], m["x0"]:m["x0"] + m["w"]] = False
    assert not out[mask].any()
    print(f"{name}: max rel err {worst:.3e}, segments {ctr.segments}")


@pytest.mark.parametrize("engine", ["extend", "pairs"])
@pytest.mark.parametrize("name", ["trace_mix0", "trace_cfg2", "trace_cfg5", "trace_cfg3_small", "trace_mesh0", "trace_inst0", "trace_inst1", "trace_inst2", "trace_demo", "trace_cfg3w_small",
                                  "trace_adv_mix0", "trace_adv_cfg2", "trace_adv_cfg3_small"])
@pytest.mark.parametrize("builder", BUILDERS)
def test_hit_records_match_reference(name, engine, builder, ctx, monkeypatch):
    """world.hit() known answers on the device (zr_trace) vs the genuine reference's hit records, through both
    traversal engines: the streaming pipeline's EXTEND kernel (4-wide quantised tree) and the pair-BVH walk."""
    monkeypatch.setenv("ZR_TRACE_ENGINE", engine)
    fx = load_golden(name)
    m = fx["meta"]
    sc = gpu_scene(ctx, m["scene"], m["scene_args"], builder)
    rays, recs = fx["rays"], fx["recs"]
    hits = sc.trace(rays, seed=m["seed"], pixel=m["stream_pixel"], bounce=0)
    ref_hit = recs[:, 0] > 0
    got_hit = hits["mat"] != 0xFFFFFFFF
    assert np.array_equal(ref_hit, got_hit), f"{int((ref_hit != got_hit).sum())} rays disagree on hit/miss"
    tol = 1e-9
    assert np.all(rel_err(hits["t"][ref_hit], recs[ref_hit, 1], 1e-12) < tol)
    h = ref_hit.copy()
    if m.get("adversarial"):
        # class 6 of the adversarial rays starts 4096 scene sizes away: o + t d then carries |o| 2^-53 ~ 1e-11 of absolute
        # error per operation and a sphere's discriminant cancels 1e9:1, so p and the normal are compared for the other
        # classes only (hit/miss, t and the material are compared for all)
        h[np.arange(len(h)) % 8 == 6] = False
    assert np.all(np.abs(hits["p"][h] - recs[h, 2:5]) <= tol * (1 + np.abs(recs[h, 2:5])))
    assert np.all(np.abs(hits["normal"][h] - recs[h, 5:8]) < 1e-7)
    assert np.array_equal(hits["front_face"][h], recs[h, 8].astype(np.uint32))
    wrote_uv = np.any(hits["tangent"] != 0, axis=1) & h
    du = np.abs(hits["u"][wrote_uv] - recs[wrote_uv, 9])
    dv = np.abs(hits["v"][wrote_uv] - recs[wrote_uv, 10])
    # cfg5's walls overlap in the box corners, so a few rays hit two coincident coplanar faces at the same t; which
    # cube wins is the reference's traversal order (same point, normal and material, different face u/v): allow 2
    uv_bad = (du > 1e-9) | (dv > 1e-9)
    assert uv_bad.sum() <= 2, (int(uv_bad.sum()), du.max(), dv.max())
    assert np.all(np.abs(hits["tangent"][wrote_uv] - recs[wrote_uv, 11:14]) < 1e-7)
    pairs = set(zip(recs[h, 14].astype(int).tolist(), hits["mat"][h].tolist()))
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})


@pytest.mark.parametrize("engine", ["extend", "pairs"])
def test_known_answers_on_hand_placed_inputs(engine, ctx, monkeypatch):
    """Per-function known answers (tests/golden/kat_kat0.npz, generated by the genuine reference functions): sphere / triangle /
    cube / medium ::hit at their edge cases (poles, tangent rays, edge and vertex hits, t == ray_t.min / max with each
    primitive's own open / closed reading, origin inside the cube, the parallel threshold, a negative radius), material::scatter
    + emitted on those hits (fuzz-0 metal, total internal reflection, both faces, absorbed metal, light, failed texture load),
    texture::value at and beyond the unit square, get_background_color in every mode (disc edge, poles, seam), and get_ray at the
    corners of the frame — on the device, through zr_trace / zr_kat_*.  Decisions and draw counts exact, values to 1e-12."""
    from test_oracle_golden import kat_env, kat_trace
    from oracle import zr_oracle_py as zo
    monkeypatch.setenv("ZR_TRACE_ENGINE", engine)
    fx = load_golden("kat_kat0")
    m = fx["meta"]["hits"]
    ds = demo_scene("kat0")
    sc = gpu_scene(ctx, "kat0")
    rays, recs, scat = fx["rays"], fx["recs"], fx["scat"]
    if engine == "extend":   # the EXTEND kernel answers the render interval only
        keep = (rays[:, 6] == 0.001) & np.isinf(rays[:, 7])
        hits = np.zeros(len(rays), dtype=sc.trace(rays[:1, :6]).dtype)
        hits[:] = sc.trace(rays[:, :6], 0.001, float("inf"), seed=m["seed"], pixel=m["stream_pixel"], bounce=0)
    else:
        keep = np.ones(len(rays), bool)
        hits = kat_trace(lambda r, a, b: sc.trace(r, a, b, seed=m["seed"], pixel=m["stream_pixel"], bounce=0), rays)
    ref_hit = recs[:, 0] > 0
    got_hit = hits["mat"] != 0xFFFFFFFF
    assert np.array_equal(ref_hit[keep], got_hit[keep]), np.flatnonzero(keep & (ref_hit != got_hit))
    h = ref_hit & keep
    tol = 1e-12

    def close(a, b, what, tol=tol):
        err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
        assert err.max() <= tol, f"{what}: max error {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    close(hits["t"][h], recs[h, 1], "t"); close(hits["p"][h], recs[h, 2:5], "p"); close(hits["normal"][h], recs[h, 5:8], "normal")
    assert np.array_equal(hits["front_face"][h], recs[h, 8].astype(np.uint32))
    close(hits["u"][h], recs[h, 9], "u"); close(hits["v"][h], recs[h, 10], "v"); close(hits["tangent"][h], recs[h, 11:14], "tangent")
    pairs = set(zip(recs[h, 14].astype(int).tolist(), hits["mat"][h].tolist()))
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
    keys = np.array([zo.stream_key(m["seed"], m["stream_pixel"], k) for k in range(len(rays))], dtype=np.uint64)
    so = sc.kat_scatter(rays[h, :6], hits[h], keys[h])
    assert np.array_equal(so["scattered"], scat[h, 0].astype(np.uint32))
    assert np.array_equal(so["draws"], scat[h, 13].astype(np.uint32))
    close(so["attenuation"], scat[h, 1:4], "attenuation"); close(so["origin"], scat[h, 4:7], "scattered origin")
    close(so["direction"], scat[h, 7:10], "scattered direction"); close(so["emitted"], scat[h, 10:13], "emitted")
    if engine == "pairs":   # the remaining entry points do not depend on the traversal engine
        tin = fx["tex_in"]
        for t in range(6):
            sel = tin[:, 0] == t
            close(sc.kat_texture(ds.kat_textures[t], tin[sel, 1:6]), fx["tex_rgb"][sel], f"texture {t}")
        bin_ = fx["bg_in"]
        for env_row in {tuple(r[:16]) for r in bin_}:
            sel = np.all(bin_[:, :16] == np.array(env_row), axis=1)
            # the edge of the sun disc is a smoothstep over 2e-4 of cos(angle): last-bit differences (FMA) are amplified 5000 x there
            close(sc.kat_background(kat_env(env_row, ds.env.hdr_texture), bin_[sel, 16:19]), fx["bg_rgb"][sel], f"environment {env_row[:5]}", 1e-10)
        for scene in ("kat0", "cfg1"):
            d2 = demo_scene(scene)
            got = ctx.kat_camera_rays(d2.camera, d2.seed, fx[f"cam_req_{scene}"])
            close(got[:, :6], fx[f"cam_rays_{scene}"][:, :6], f"get_ray {scene}")
            assert np.array_equal(got[:, 6], fx[f"cam_rays_{scene}"][:, 6])


def kat1_entry_of(p):
    """the world-list entry of scene "kat1" a hit point belongs to: its cell (scenes/zr_scenes_mix.inc: pitch 8, cell k at (8 (k % 10) - 36, 8 (k // 10) - 28, .))
    and from the cell the order in which zr_build_kat1 adds the objects; the cube at the origin is entry 90"""
    col, row = np.rint((p[:, 0] + 36.0) / 8.0).astype(int), np.rint((p[:, 1] + 28.0) / 8.0).astype(int)
    cell = row * 10 + col
    entry = np.select([cell <= 16, cell <= 64, cell <= 84, cell <= 92, cell <= 99], [cell, cell - 3, cell - 3, cell - 3, cell - 2], cell - 2)
    return np.where(np.all(np.abs(p) < 1.5, axis=1), 90, entry)


@pytest.mark.parametrize("bake", ["1", "0"])
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("engine", ["extend", "pairs"])
def test_wrapper_chains_at_their_edges(engine, builder, bake, ctx, monkeypatch):
    """Wrapper chains at their edges (tests/golden/kat_kat1.npz, the genuine reference's answers on the hand-placed rays of make_golden.py kat1_inputs()) on the
    device, in every stored form: ZR_BAKE_TRIANGLES=1 stores the objects as test_kat1_objects_land_in_their_stored_forms lists them (baked triangles and spheres,
    placed cubes, material-only chains, instances, the op-list interpreter for the rest), =0 sends every wrapped object through the interpreter.  Hit / miss,
    front_face, the material, the scatter decision and the draw count are exact for every ray — the face-normal ties, where dot(d, normal) is exactly 0 and a
    translate or rotate_y calls set_face_normal a second time, among them.  Values: what the interpreter and the placed cube compute in the reference's own
    operation order to kat0's 1e-12 of max(1, |value|); baked triangles and spheres, evaluated in world space, to the trace fixtures' 1e-9 (t, p) and 1e-7.
    What it found (DESIGN, parity section): the baked forms answered front_face = true on the 20 ties of the fixture (now zr_device.h reface()), a baked sphere
    made its tangent from the refreshed normal, and a metal on a tie scattered or not by the sign of a fused multiply-add's rounding error (now dot_rn)."""
    from test_oracle_golden import KAT1_FORMS, kat_trace
    from oracle import zr_oracle_py as zo
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_TRACE_ENGINE", engine)
    monkeypatch.setenv("ZR_BVH_BUILD", builder)
    monkeypatch.setenv("ZR_BUILD_CHECK", "1")
    monkeypatch.setenv("ZR_BAKE_TRIANGLES", bake)   # read at commit: a scene of this cell's own
    fx = load_golden("kat_kat1")
    m = fx["meta"]["hits"]
    sc = capi.Scene(ctx, demo_scene("kat1").desc)
    try:
        assert sc.stats()["builder"].startswith(builder)
        rays, recs, scat = fx["rays"], fx["recs"], fx["scat"]
        if engine == "extend":   # the EXTEND kernel answers the render interval only
            keep = (rays[:, 6] == 0.001) & np.isinf(rays[:, 7])
            hits = np.zeros(len(rays), dtype=sc.trace(rays[:1, :6]).dtype)
            hits[:] = sc.trace(rays[:, :6], 0.001, float("inf"), seed=m["seed"], pixel=m["stream_pixel"], bounce=0)
        else:
            keep = np.ones(len(rays), bool)
            hits = kat_trace(lambda r, a, b: sc.trace(r, a, b, seed=m["seed"], pixel=m["stream_pixel"], bounce=0), rays)
        ref_hit = recs[:, 0] > 0
        got_hit = hits["mat"] != 0xFFFFFFFF
        assert np.array_equal(ref_hit[keep], got_hit[keep]), np.flatnonzero(keep & (ref_hit != got_hit))
        h = ref_hit & keep
        assert h.sum() > 500
        wrong = np.flatnonzero(h & (hits["front_face"] != recs[:, 8].astype(np.uint32)))
        assert wrong.size == 0, f"front_face differs on rays {wrong.tolist()}"
        pairs = set(zip(recs[h, 14].astype(int).tolist(), hits["mat"][h].tolist()))
        assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
        # each hit's bound by the stored form of the object it is on
        forms = np.array(KAT1_FORMS)[kat1_entry_of(recs[:, 2:5])]
        world_space = h & (bake == "1") & np.isin(forms, ["baked triangle", "baked sphere"])
        assert world_space.sum() > (100 if bake == "1" else -1) and (h & ~world_space).sum() > 300

        def close(a, b, what, tol):
            err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
            print(f"kat1 {engine} {builder} bake={bake}: {what} max error {err.max() if err.size else 0.0:.3e} (bound {tol:g})")
            assert not err.size or err.max() <= tol, f"{what}: max error {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
        for sel, tol_tp, tol_n, tag in ((h & ~world_space, 1e-12, 1e-12, "chain order"), (world_space, 1e-9, 1e-7, "world space")):
            close(hits["t"][sel], recs[sel, 1], f"t ({tag})", tol_tp); close(hits["p"][sel], recs[sel, 2:5], f"p ({tag})", tol_tp)
            close(hits["normal"][sel], recs[sel, 5:8], f"normal ({tag})", tol_n); close(hits["tangent"][sel], recs[sel, 11:14], f"tangent ({tag})", tol_n)
            close(hits["u"][sel], recs[sel, 9], f"u ({tag})", tol_tp); close(hits["v"][sel], recs[sel, 10], f"v ({tag})", tol_tp)
        keys = np.array([zo.stream_key(m["seed"], m["stream_pixel"], k) for k in range(len(rays))], dtype=np.uint64)
        so = sc.kat_scatter(rays[h, :6], hits[h], keys[h])
        assert np.array_equal(so["scattered"], scat[h, 0].astype(np.uint32)), np.flatnonzero(h)[so["scattered"] != scat[h, 0]]
        assert np.array_equal(so["draws"], scat[h, 13].astype(np.uint32)), np.flatnonzero(h)[so["draws"] != scat[h, 13]]
    finally:
        sc.close()


def test_dropin_virtuals_are_callable(ctx):
    """hittable::hit (hittable.hpp:29-36) and material::scatter / emitted (material.hpp:7-31) of the drop-in's built-in classes
    stay callable: bvh_node(world).hit(r, interval, rec) and rec.mat->scatter(...) called from C++ against include/zenith/zenith.hpp
    — each call one ray through the device — reproduce the genuine reference's answers on the hand-placed inputs."""
    fx = load_golden("kat_kat0")
    m = fx["meta"]["hits"]
    ds = demo_scene("kat0")
    rays, recs, scat = fx["rays"], fx["recs"], fx["scat"]
    got_r, got_s = ds.dropin_virtuals(rays, m["seed"], m["stream_pixel"])
    h = recs[:, 0] > 0
    # the four rays aimed at the constant_medium (make_golden.py kat_inputs): constant_medium::hit draws its distance off-stream,
    # and the callable hit() keys that draw by the host stream position, so whether and where they hit differs by design
    medium = np.zeros(len(rays), bool)
    medium[[58, 59, 60, 61]] = True
    assert np.all(rays[medium][:, 2] <= -3) and recs[58, 5] == 1 and recs[58, 9] == 0
    assert np.array_equal((got_r[:, 0] > 0)[~medium], h[~medium])
    x = h & ~medium
    err = np.abs(got_r[x, 1:14] - recs[x, 1:14]) / np.maximum(1.0, np.abs(recs[x, 1:14]))
    assert err.max() <= 1e-12, err.max()
    pairs = set(zip(recs[x, 14].astype(int).tolist(), got_r[x, 14].astype(int).tolist()))
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
    assert np.array_equal(got_s[x, 0], scat[x, 0]) and np.array_equal(got_s[x, 13], scat[x, 13])   # scattered flag, draws consumed
    err = np.abs(got_s[x, 1:13] - scat[x, 1:13]) / np.maximum(1.0, np.abs(scat[x, 1:13]))
    assert err.max() <= 1e-12, err.max()


@pytest.mark.parametrize("name", ["cfg3_small", "cfg2", "mix0"])
def test_extend_adversarial_rays(name, ctx, monkeypatch):
    """EXTEND's box tests are FP32, quantised and conservative; the pair walk uses plain FP32 boxes and the oracle FP64
    ones.  Rays chosen to stress the conservative arithmetic — axis-aligned directions (zero components, both signs of
    zero), origins on box planes and far away, tiny and huge direction scales — must give the same closest hit on all
    three (the hit is decided by the FP64 primitive tests alone)."""
    from oracle import zr_oracle_py as zo
    scene, args = {"cfg3_small": ("cfg3", (200, 20, 256, 128))}.get(name, (name, ()))   # 8 000-triangle knot
    ds = demo_scene(scene, args)
    sc = gpu_scene(ctx, scene, args)
    rng = np.random.default_rng(20260417)
    n = 6000
    o = rng.uniform(-6, 6, (n, 3))
    d = rng.normal(size=(n, 3))
    k = n // 6
    for a in range(3):                       # one or two exactly-zero components, +0 and -0
        d[a * k:(a + 1) * k, a] = 0.0
        d[a * k:a * k + k // 2, a] = -0.0
        d[a * k:a * k + k // 4, (a + 1) % 3] = 0.0
    d[3 * k:4 * k] *= 1e-12                  # un-normalised directions, both extremes (t scales with 1/|d|)
    d[4 * k:5 * k] *= 1e9
    o[5 * k:5 * k + k // 2] *= 1e4           # far origins looking back at the scene
    d[5 * k:5 * k + k // 2] = -o[5 * k:5 * k + k // 2] + rng.normal(size=(k // 2, 3))
    o[5 * k + k // 2:] = np.round(o[5 * k + k // 2:] * 4) / 4   # origins on round coordinates (often on box planes)
    rays = np.concatenate([o, d], axis=1)
    monkeypatch.setenv("ZR_TRACE_ENGINE", "extend")
    he = sc.trace(rays, seed=5, pixel=77, bounce=0)
    monkeypatch.setenv("ZR_TRACE_ENGINE", "pairs")
    hp = sc.trace(rays, seed=5, pixel=77, bounce=0)
    ho = zo.OracleScene(ds.desc).trace(rays, seed=5, pixel=77, bounce=0)
    assert (ho["mat"] != 0xFFFFFFFF).sum() > n // 20, "the probe rays barely hit the scene"
    for got, tag in ((he, "extend"), (hp, "pairs")):
        assert np.array_equal(got["mat"], ho["mat"]), f"{tag}: {(got['mat'] != ho['mat']).sum()} rays differ from the oracle"
        h = ho["mat"] != 0xFFFFFFFF
        assert np.all(rel_err(got["t"][h], ho["t"][h], 1e-300) < 1e-9), tag
        near = h.copy()
        near[5 * k:5 * k + k // 2] = False   # far origins: the sphere's discriminant cancels ~1e9:1 there, so fused and
        assert np.all(np.abs(got["normal"][near] - ho["normal"][near]) < 1e-7), tag   # unfused FP64 differ at 1e-5 in p / r


@pytest.mark.parametrize("count", [False, True], ids=["timed", "counting"])
@pytest.mark.parametrize("name,region", [("cfg1", None), ("mix0", None), ("mix1", None), ("mix2", None),
                                         ("cfg2", (512, 256, 64, 32)), ("cfg5", (200, 380, 32, 16))])
def test_radiance_matches_oracle(name, region, count, ctx):
    """GPU vs the CPU oracle on more pixels than the committed fixtures cover (oracle-sized regions)."""
    from oracle import zr_oracle_py as zo
    from raytracer_project_amd import capi
    ds = demo_scene(name)
    cam = ds.camera.copy()
    if name in ("cfg2", "cfg5"):
        cam.samples_per_pixel = 64  # keeps the CPU side in seconds; full-spp tiles are in the golden fixtures
    reg = capi.Region(*region, 0, 0, 0, 0) if region else None
    gpu = gpu_scene(ctx, name).render(cam, ds.env, ds.seed, reg, count=count)
    gctr = ctx.counters()
    cpu, cctr, _, _ = _oracle_render(name, region, cam, ds, reg)
    _check(gpu, cpu, name)
    if count:
        assert (gctr.segments, gctr.rng_draws, gctr.hits) == (cctr.segments, cctr.rng_draws, cctr.hits)


_oracle_cache = {}


def _oracle_render(name, region, cam, ds, reg):
    """the CPU side of test_radiance_matches_oracle, computed once per (scene, region)"""
    from oracle import zr_oracle_py as zo
    key = (name, region, cam.samples_per_pixel)
    if key not in _oracle_cache:
        _oracle_cache[key] = zo.OracleScene(ds.desc).render(cam, ds.env, ds.seed, reg)
    return _oracle_cache[key]


@pytest.mark.parametrize("builder", BUILDERS)
def test_empty_and_degenerate_scenes(builder, ctx, monkeypatch):
    """Empty world, a single primitive, two and three primitives: edge cases of the flattened layout, through both tree builders
    (an empty world has no tree to build: the host path answers whatever ZR_BVH_BUILD says)."""
    import ctypes as C
    monkeypatch.setenv("ZR_BVH_BUILD", builder)
    monkeypatch.setenv("ZR_BUILD_CHECK", "1")
    from oracle import zr_oracle_py as zo
    from raytracer_project_amd import capi
    ds = demo_scene("cfg1")
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel = 40, 24, 4
    # (1) empty world: every sample is background
    d = capi.SceneDesc()
    C.memmove(C.byref(d), C.byref(ds.desc), C.sizeof(d))
    d.n_spheres = 0
    d.n_objects = 0
    sc = capi.Scene(ctx, d)
    out = sc.render(cam, ds.env, 7, None, count=True)
    ctr = ctx.counters()
    assert ctr.hits == 0 and ctr.segments == ctr.primary_samples == 40 * 24 * 4
    cpu, _, _, _ = zo.OracleScene(d).render(cam, ds.env, 7, None)
    _check(out, cpu, "empty world")
    # (2) one sphere only (root pair with an empty second child)
    objs = (capi.Object * 1)(capi.Object(0, 1, 0, 0))
    d.n_spheres = 3
    d.objects = C.cast(objs, C.c_void_p)
    d.n_objects = 1
    sc = capi.Scene(ctx, d)
    assert sc.stats()["builder"].startswith(builder)
    out = sc.render(cam, ds.env, 7, None)
    cpu, _, _, _ = zo.OracleScene(d).render(cam, ds.env, 7, None)
    _check(out, cpu, "single sphere")
    # (3) two and three spheres: the smallest trees with an inner node (a one-pair tree; a root with a leaf and a pair)
    for n in (2, 3):
        objs_n = (capi.Object * n)(*[capi.Object(0, k, 0, 0) for k in range(n)])
        d.objects = C.cast(objs_n, C.c_void_p)
        d.n_objects = n
        sc = capi.Scene(ctx, d)
        assert sc.stats()["builder"].startswith(builder)
        out = sc.render(cam, ds.env, 7, None, count=True)
        ctr = ctx.counters()
        cpu, oc, _, _ = zo.OracleScene(d).render(cam, ds.env, 7, None)
        assert (ctr.segments, ctr.rng_draws, ctr.hits) == (oc.segments, oc.rng_draws, oc.hits)
        _check(out, cpu, f"{n} spheres")
        # the frame above came from the fused small-scene kernel; the tree itself answers through both traversal engines
        rng = np.random.default_rng(n)
        o = rng.uniform(-3, 3, (512, 3)); rays = np.concatenate([o, rng.uniform(-1, 1, (512, 3)) - o * 0.5], axis=1)
        want = zo.OracleScene(d).trace(rays)
        for engine in ("extend", "pairs"):
            monkeypatch.setenv("ZR_TRACE_ENGINE", engine)
            got = sc.trace(rays)
            assert np.array_equal(got["mat"], want["mat"]), (n, engine)
        monkeypatch.delenv("ZR_TRACE_ENGINE")


@pytest.mark.parametrize("builder", BUILDERS)
def test_deep_tree_sizes_the_traversal_stack(builder, ctx, monkeypatch):
    """A world built to need a deep traversal stack: 600 concentric spherical shells, every one a leaf of its own, all of them
    overlapping every ray through the centre.  The committed scene reports its exact worst-case stack demand
    (zr_scene_traversal_stack), the per-wave spill slabs are sized from it, and EXTEND's answers equal the pair walk's and the
    oracle's — no push can leave the slab (the round-1 kernel assumed 48 entries)."""
    import ctypes as C
    from oracle import zr_oracle_py as zo
    from raytracer_project_amd import capi
    n = 600
    sph = np.zeros((n, 4)); sph[:, 3] = 1.0 * 1.01 ** np.arange(n)         # same centre, radii 1 ... 390
    mats = np.zeros(n, dtype=np.uint32)
    mat = (capi.Material * 1)(capi.Material(0, 0, capi.NO_TEXTURE, 0, 0.0, 1.0, (C.c_double * 3)(1, 1, 1)))
    tex = (capi.Texture * 1)(capi.Texture(0, 0, 0, 0, 0, 0, 0, 1.0, (C.c_double * 3)(0.5, 0.5, 0.5)))
    d = capi.SceneDesc()
    d.spheres = sph.ctypes.data; d.sphere_mat = mats.ctypes.data; d.n_spheres = n
    d.materials = C.cast(mat, C.c_void_p); d.n_materials = 1
    d.textures = C.cast(tex, C.c_void_p); d.n_textures = 1
    monkeypatch.setenv("ZR_BVH_MAX_LEAF", "1")
    # through both builders: 600 concentric boxes are the worst case for a bottom-up merger too (every cluster overlaps every
    # other); should the device tree come out deeper than the traversal stack allows, the commit falls back to the host builder
    # and says so — either way the answers below must hold
    monkeypatch.setenv("ZR_BVH_BUILD", builder)
    monkeypatch.setenv("ZR_BUILD_CHECK", "1")
    sc = capi.Scene(ctx, d)
    assert sc.stats()["builder"].startswith(("host", "device"))
    if builder == "host":
        assert sc.stats()["builder"].startswith("host")
    demand = sc.stats()["traversal_stack"]
    assert demand > 12, demand      # more than the LDS part of the stack: the HBM slab is in use
    rng = np.random.default_rng(3)
    o = rng.normal(size=(4000, 3)); o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(0.0, 500.0, (4000, 1))
    rays = np.concatenate([o, -o + rng.normal(scale=0.05, size=(4000, 3))], axis=1)   # towards the centre: through every shell
    want = zo.OracleScene(d).trace(rays)
    for engine in ("extend", "pairs"):
        monkeypatch.setenv("ZR_TRACE_ENGINE", engine)
        got = sc.trace(rays)
        assert np.array_equal(got["mat"], want["mat"]), engine
        h = want["mat"] != 0xFFFFFFFF
        assert h.sum() > 3000 and np.all(rel_err(got["t"][h], want["t"][h], 1e-300) < 1e-9), engine
    sc.close()


def test_tile_sharding_is_exact(ctx):
    """Pixel tiles rendered by different 'ranks' (tile_mod / tile_rem) reassemble to the single-GPU image bit for bit,
    so the multi-GPU reduce (sum with zeros) is exact."""
    from raytracer_project_amd import capi
    ds = demo_scene("cfg2")
    cam = ds.camera.copy()
    cam.samples_per_pixel = 8
    sc = gpu_scene(ctx, "cfg2")
    full = sc.render(cam, ds.env, ds.seed, None)
    again = sc.render(cam, ds.env, ds.seed, None)
    assert np.array_equal(full, again), "render is not bit-reproducible"
    for skew in (0, 2):   # the row-major rule t % 3 and the lattice (tx + 2 ty) % 3 (zr_region::tile_skew)
        acc = np.zeros_like(full)
        for rank in range(3):
            part = sc.render(cam, ds.env, ds.seed, capi.Region(0, 0, 0, 0, 32, 3, rank, skew))
            assert not (acc != 0)[part != 0].any(), "tiles overlap between ranks"
            acc += part
        assert np.array_equal(acc, full), skew
    assert np.isfinite(full).all() and (full >= 0).all() and 0.1 < full.mean() < 2.0


def test_smallest_slot_pool_renders_the_same_image(built, monkeypatch):
    """ZR_STREAM_SLOTS below 64 SHADE blocks used to leave the work units of unserved shards unrendered; the pool is now clamped
    to 64 x 256 slots, and the image does not depend on the pool size (every sample is written once, reduced in a fixed order)."""
    from raytracer_project_amd import capi
    ds = demo_scene("mix0")
    cam = ds.camera.copy()
    cam.samples_per_pixel = 64
    frames = []
    for slots in ("4096", "1048576"):
        monkeypatch.setenv("ZR_STREAM_SLOTS", slots)
        c = capi.Context(0)
        try:
            sc = capi.Scene(c, ds.desc)
            frames.append(sc.render(cam, ds.env, ds.seed, None, count=True))
            assert c.counters().primary_samples == cam.image_width * cam.image_height * 64
            sc.close()
        finally:
            c.close()
    assert np.array_equal(frames[0], frames[1])


def test_unit_order_does_not_change_the_image(built, monkeypatch):
    """Work units are handed out bottom-up (the frame's drain is as long as the paths started last, and the top rows are where
    the one-segment sky samples are); top-down must give the same bits, counters included."""
    from raytracer_project_amd import capi
    ds = demo_scene("mix0")
    cam = ds.camera.copy()
    cam.samples_per_pixel = 32
    frames, segs = [], []
    c = capi.Context(0)
    try:
        sc = capi.Scene(c, ds.desc)
        for order in ("1", "0"):
            monkeypatch.setenv("ZR_STREAM_BOTTOM_UP", order)
            frames.append(sc.render(cam, ds.env, ds.seed, None, count=True))
            k = c.counters()
            segs.append((k.segments, k.rng_draws, k.primary_samples))
        sc.close()
    finally:
        c.close()
    assert np.array_equal(frames[0], frames[1]) and segs[0] == segs[1]


@pytest.mark.parametrize("var,values", [("ZR_STREAM_POOLS", ("1", "2", "3")), ("ZR_EXTEND_LEVEL", ("-1", "2"))])
def test_pipeline_shape_does_not_change_the_image(var, values, built, monkeypatch):
    """Sub-pools on separate HIP streams (the default for a rank's share of a sharded frame) and the build of the traversal
    kernel chosen for a scene (lean / cubes-and-media / everything) are scheduling and code-size choices: same bits, same counters.
    Every frame is the streaming pipeline's (ZR_FUSED=0: cfg5 would otherwise take the fused kernel); cfg5 compares EXTEND's level-1
    build with its level-2 build."""
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_FUSED", "0")
    for name in ("mix0", "cfg5" if var == "ZR_EXTEND_LEVEL" else "mix1"):
        ds = demo_scene(name)
        cam = ds.camera.copy()
        cam.samples_per_pixel = min(cam.samples_per_pixel, 48)
        frames, ctrs, levels = [], [], []
        for v in values:
            monkeypatch.setenv(var, v)
            monkeypatch.setenv("ZR_STREAM_SLOTS", "262144")   # a pool small enough to be split
            c = capi.Context(0)
            try:
                sc = capi.Scene(c, ds.desc)
                frames.append(sc.render(cam, ds.env, ds.seed, None, count=True))
                k = c.counters()
                assert k.path == 2, (name, var, v, k.path)
                ctrs.append((k.segments, k.rng_draws, k.primary_samples, k.hits))
                levels.append(sc.kernels()["extend_level"])
                sc.close()
            finally:
                c.close()
        if name == "cfg5":
            assert levels == [1, 2], levels
        for f, k in zip(frames[1:], ctrs[1:]):
            assert np.array_equal(frames[0], f) and ctrs[0] == k, (name, var)


def test_shared_mesh_is_stored_once(built, monkeypatch):
    """Two-level BVH: inst0 places one 960-triangle mesh 36 times and a 13-triangle one 8 times.  Flattened with groups the world
    list has 46 entries and the device holds each mesh once; with ZR_GROUPS=0 every placement is a baked copy of every triangle.
    Same picture (the two differ in the last bits only: a ray mapped into the mesh's space against vertices mapped out of it)."""
    from raytracer_project_amd import capi
    frames, sizes, entries = [], [], []
    for groups in ("1", "0"):
        monkeypatch.setenv("ZR_GROUPS", groups)
        ds = capi.DemoScene("inst0")
        entries.append((ds.desc.n_objects, ds.desc.n_groups, ds.desc.n_tris))
        c = capi.Context(0)
        try:
            sc = capi.Scene(c, ds.desc)
            sizes.append(sc.stats()["device_bytes"])
            frames.append(sc.render(ds.camera, ds.env, ds.seed, None, count=True))
            k = c.counters()
            assert k.primary_samples == ds.camera.image_width * ds.camera.image_height * ds.camera.samples_per_pixel
            sc.close()
        finally:
            c.close()
    assert entries[0] == (46, 2, 973) and entries[1][1] == 0 and entries[1][0] == 2 + 36 * 960 + 8 * 13
    assert sizes[0] * 8 < sizes[1], sizes
    err = rel_err(frames[0], frames[1])
    assert (err > REL_TOL).sum() == 0, float(err.max())


def test_many_groups_go_to_the_host_builder(built, monkeypatch):
    """A group's tree is a build of its own on the device (~1 ms however small the run): beyond ZR_BVH_DEVICE_MAX_GROUPS groups the commit is the
    host builder's even when the device build is asked for.  Same picture either way."""
    from raytracer_project_amd import capi
    ds = capi.DemoScene("inst2", 6)
    monkeypatch.setenv("ZR_BVH_BUILD", "device")
    frames = []
    for limit, want in (("1", "host"), ("256", "device")):
        monkeypatch.setenv("ZR_BVH_DEVICE_MAX_GROUPS", limit)
        c = capi.Context(0)
        try:
            sc = capi.Scene(c, ds.desc)
            assert sc.stats()["builder"].startswith(want), (limit, sc.stats()["builder"])
            frames.append(sc.render(ds.camera, ds.env, ds.seed, None))
            sc.close()
        finally:
            c.close()
    err = rel_err(frames[0], frames[1])
    assert (err > REL_TOL).sum() == 0, float(err.max())


def test_composite_prefab_shares_its_triangles(built, monkeypatch):
    """inst2: a prefab that holds a mesh (itself a shared model under a translate: a group inside a group), a glass sphere, a placed
    cube and a pedestal of six triangles, placed N times under scale / material_instance / rotate_z / translate; the mesh also
    placed by itself.  The drop-in flattens the prefab into a template: the triangles are stored once whatever N is (two zr_groups),
    a placement adds four small world entries; with ZR_GROUPS=0 every placement copies every triangle.  Same picture."""
    from raytracer_project_amd import capi
    shapes, sizes, frames = [], [], []
    for n, groups in ((6, "1"), (18, "1"), (6, "0")):
        monkeypatch.setenv("ZR_GROUPS", groups)
        ds = capi.DemoScene("inst2", n)
        shapes.append((ds.desc.n_objects, ds.desc.n_groups, ds.desc.n_tris))
        c = capi.Context(0)
        try:
            sc = capi.Scene(c, ds.desc)
            sizes.append(sc.stats()["device_bytes"])
            if n == 6:
                frames.append(sc.render(ds.camera, ds.env, ds.seed, None))
            sc.close()
        finally:
            c.close()
    assert shapes[0] == (1 + 4 * 6 + 3 + 2, 2, 487) and shapes[1] == (1 + 4 * 18 + 3 + 2, 2, 487), shapes   # triangles: independent of N
    assert shapes[2][1] == 0 and shapes[2][2] == 6 * 486 + 3 * 480 + 1, shapes
    # three times the placements: a few hundred bytes each (entry, wrapper ops, the placed sphere / cube records), no triangle
    assert sizes[1] - sizes[0] < 12 * 4 * 1024 and sizes[2] > 4 * sizes[0], sizes
    err = rel_err(frames[0], frames[1])
    assert (err > REL_TOL).sum() == 0, float(err.max())


def test_bench_line_contract(built):
    """bench.py --full on the reference's own CPU-sized case: one JSON line with the driver's keys, the roofline object (incl. the
    random-record rate the traversal kernel runs against) and a CPU baseline whose port reproduces the reference's counts."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "cfg1", "--steps", "2", "--warmup", "1", "--full"],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["dtype"] == "f64" and "workload" in d["config"]
    rf = d["roofline"]
    for key in ("bound", "bound_why", "bound_source", "achieved", "peak", "unit", "frac", "traffic", "frac_traffic", "l2_hit_rate", "fp64_valu_frac", "frac_layout",
                "random_record_rate_G_per_s", "frac_random_records", "kernel", "kernel_ms", "launches_timed", "model"):
        assert key in rf, key
    # cfg1 is three spheres: the fused small-scene kernel renders it, and what bounds that kernel is FP64 vector issue, not HBM
    # ("valu-issue" when a counter pass of the current kernel source is committed: frac is then the measured share of the issue rate; "fp64-valu" by construction without one)
    assert rf["bound"] in ("fp64-valu", "valu-issue") and rf["kernel"] == "fused_render"
    assert d["config"]["render_path"] == "fused small-scene kernel" and d["config"]["bvh_builder"].startswith(("host", "device"))
    assert d["config"]["bvh_build_upload_s"] >= 0 and d["config"]["bvh_build_upload_first_s"] >= 0
    # a register-resident kernel is not under the HBM ceiling: `frac` is its share of the chip's vector issue rate (from the counter file of the current kernel
    # source: null without one — never a fraction of a ceiling the kernel is not under), the HBM-model figure stays beside it
    assert rf["unit"] == "G wave-instructions/s" and abs(rf["peak"] - 614.4) < 1e-6 and "76 B per hit" in rf["model"] and "NOT" in rf["model"]
    assert rf["frac"] is None or (0 < rf["frac"] <= 1.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4)
    assert abs(rf["frac_hbm_model"] - rf["achieved_hbm_model"] / 8000.0) < 1e-4 and rf["kernel_ms"] > 0 and rf["launches_timed"] > 0
    assert rf["co_running"] is False and d["per_rank_ms_per_step"]["min"] > 0
    cb = d["cpu_baseline"]
    assert cb["value"] and cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("reference", "port") and cb["sample"]
    if cb["kind"] == "reference":   # the reference's best thread count (at most 16), median of three runs; the all-cores figure beside it
        assert cb["port"]["value"] > 0 and cb["port_matches_reference"] is True
        assert cb["cores"] <= 16 and len(cb["runs"]) == 3 and sorted(cb["runs"])[1] == cb["value"] and "reference_on_all_cores" in cb


def test_plain_bench_line_leaves_out_what_full_adds(built):
    """A plain bench.py run does only what its headline needs: the same line without the CPU baseline and without the restart commit
    (`bvh_build_upload_s` is null), both of which --full adds.  It renders what the --full run renders: same path, segments and frame."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "cfg1", "--steps", "1", "--warmup", "0"] + extra,
                           capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines[mode] = json.loads(out[0])
    plain, full = lines["plain"], lines["full"]
    assert "cpu_baseline" not in plain and "cpu_baseline" not in full
    assert plain["config"]["bvh_build_upload_s"] is None and plain["config"]["bvh_build_upload_first_s"] >= 0
    assert full["config"]["bvh_build_upload_s"] >= 0 and full["config"]["bvh_build_upload_first_s"] >= 0
    for key in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup"):
        assert plain[key] == full[key], key
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and set(plain["roofline"]) == set(full["roofline"])
    for key in ("render_path", "segments_per_step", "primary_per_step", "frame_checksum"):
        assert plain["config"][key] == full["config"][key], key


def test_bench_dumps_the_frame_of_its_last_step(ctx, tmp_path):
    """bench.py --dump-outputs DIR writes the frame the timed path computed (DIR/radiance.npy: the (H, W, 3) float64 mean radiance); it is
    the frame a caller of the C ABI gets for the same workload.  --steps sets the number of timed steps: K steps launch K times the render
    kernels of one step."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    launches = {}
    for steps in (1, 2):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "cfg1", "--steps", str(steps), "--warmup", "0", "--no-cpu-baseline",
                            "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert d["steps"] == steps
        launches[steps] = d["roofline"]["launches_timed"]
    assert launches[1] >= 1 and launches[2] == 2 * launches[1], launches
    assert sorted(os.listdir(tmp_path / "out")) == ["radiance.npy"]
    frame = np.load(tmp_path / "out" / "radiance.npy")
    assert frame.dtype == np.float64 and frame.shape == (225, 400, 3) and np.isfinite(frame).all() and frame.sum() > 0
    ds = demo_scene("cfg1")
    _check(frame, gpu_scene(ctx, "cfg1").render(ds.camera, ds.env, ds.seed), "bench.py --dump-outputs frame")


@pytest.mark.parametrize("workload", ["cfg2", "cfg3", "cfg5", "demo"])
def test_bench_line_names_its_bound_from_counters(built, workload):
    """for every workload the bench can name, `roofline.bound` comes from a counter pass of the CURRENT kernel source
    (profiles/r*_<workload>_traffic.json, keyed by bench.py --kernel-src-sha; scripts/profile_round.sh makes it) and `frac` is a fraction (<= 1) of the
    ceiling the dominant kernel is under: the HBM peak for worlds beyond the L2s, the chip's vector issue rate for worlds that sit in cache or registers
    (round 3 printed 1.10 of the HBM peak for cfg2).  A kernel change without a new counter pass fails here — by design."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", workload, "--steps", "1", "--warmup", "0", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rf = d["roofline"]
    assert rf["bound_source"].startswith("counters: profiles/r") and f"_{workload}_traffic.json" in rf["bound_source"], rf["bound_source"]
    assert rf["frac"] is not None and 0 < rf["frac"] <= 1.0, rf["frac"]
    assert rf["valu_issue_frac"] is not None and rf["l2_hit_rate"] is not None and rf["traffic"] and rf["traffic"] > 0
    if workload in ("cfg2", "cfg5", "demo"):   # in cache / in registers: vector issue, with the HBM-model figure beside it
        assert rf["bound"] == "valu-issue" and rf["unit"] == "G wave-instructions/s" and rf["frac_hbm_model"] > 0
    else:                                       # a million triangles: beyond the L2s, the SURVEY 8(d) model against the HBM peak
        assert rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["frac_hbm_model"]) < 1e-9


def test_lean_shade_build_renders_the_general_builds_image(ctx, monkeypatch):
    """SHADE's lean build (zr_device.h lean_rec / lean_shade: worlds of bare triangles and spheres over solid-colour lambertian / metal / dielectric / light
    materials, chosen at commit) leaves code out, not arithmetic: the frame equals the general build's bit for bit, on cfg3 (lambertian) and on the sphere
    scene cfg2 at reduced size, and the two sub-pools the lean pair runs on change nothing either.  The one arithmetic difference, a dielectric's Schlick
    weight as x^5 by three multiplications instead of pow (within 2 ulp), only meets a comparison with a random number: a different last bit would flip a
    scatter decision (~1e-16 per dielectric hit), not move a value by 1e-12, so there is no tolerance to allow.  Both builds render through the pipeline
    (test_render_paths.py checks the general build's cfg2 tiles against the reference fixtures)."""
    from raytracer_project_amd import capi
    for name, args, spp in (("cfg3", (200, 20, 256, 128), 16), ("cfg2", (), 4)):
        ds = demo_scene(name, args)
        cam = ds.camera.copy(); cam.samples_per_pixel = spp
        reg = capi.Region(0, 0, 640, 360, 0, 0, 0, 0) if name == "cfg2" else None
        frames = {}
        for lean in ("1", "0"):
            monkeypatch.setenv("ZR_SHADE_LEAN", lean)
            sc = capi.Scene(ctx, ds.desc)
            frames[lean] = sc.render(cam, ds.env, ds.seed, reg)
            assert (ctx.counters().path, sc.kernels()["shade_lean"]) == (2, int(lean)), (name, lean)
            sc.close()
        monkeypatch.delenv("ZR_SHADE_LEAN")
        d = frames["1"] != frames["0"]
        assert not d.any(), (name, int(d.sum()), rel_err(frames["1"], frames["0"], 1e-6).max())
        assert float(frames["1"].sum()) > 0


def test_device_builder_lays_the_tree_out_the_same_way_every_time(built):
    """the device builder numbered its 4-wide nodes with an atomic counter — same tree, same frame, but a node array whose layout changed from commit
    to commit (cache behaviour, a few per cent of timing noise).  Quads are now renumbered by the binary node they are rooted at (zr_build.hip: k_qmap): the committed
    node array is byte-identical commit after commit (ZR_COMMIT_HASH prints an FNV hash of the device arrays)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from raytracer_project_amd import capi\n"
            "ctx = capi.Context(0)\n"
            "for name, args in (('cfg3', (300, 40, 64, 32)), ('inst0', ())):\n"
            "    ds = capi.DemoScene(name, *args)\n"
            "    for k in range(4):\n"
            "        sc = capi.Scene(ctx, ds.desc); sc.close()\n") % root
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZR_COMMIT_HASH="1", ZR_BVH_BUILD="device"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stderr.splitlines() if "commit hash (device" in l]
    assert len(lines) == 8, r.stderr[-2000:]
    assert len(set(lines[:4])) == 1 and len(set(lines[4:])) == 1, lines


def test_dropin_cpp_api_renders(ctx):
    """camera::render(world, env, post, flag) of include/zenith/zenith.hpp end to end equals the C-ABI render — on the pipeline
    (mix0) and on the fused small-scene kernel (cfg5: the drop-in always passes render_flag and lines_rendered, so its frame comes
    in sixteen polled launches; the C-ABI call below renders it in one)."""
    ds = demo_scene("mix0")
    a, ctr = ds.render_dropin()
    b = gpu_scene(ctx, "mix0").render(ds.camera, ds.env, ds.seed, None)
    assert np.array_equal(a, b)
    ds = demo_scene("cfg5")
    a, ctr = ds.render_dropin(spp=8)
    cam = ds.camera.copy(); cam.samples_per_pixel = 8
    b = gpu_scene(ctx, "cfg5").render(cam, ds.env, ds.seed, None)
    assert ctr.path == (2 if os.environ.get("ZR_FUSED") == "0" else 3) and np.array_equal(a, b)   # (ZR_FUSED=0: the suite's sweep of non-default settings)


def test_dropin_renders_from_successive_threads_share_one_context(ctx):
    """The reference starts a fresh thread per render (main.cpp:1520-1531).  The drop-in keeps its device contexts in a
    process-wide pool: three renders from three successive threads create no context beyond the one the first render made, and the
    frames equal the C-ABI render."""
    ds = demo_scene("mix0")
    _, before = ds.render_dropin_threads(1, spp=4)
    a, after = ds.render_dropin_threads(3, spp=4)
    assert after == before, (before, after)
    cam = ds.camera.copy(); cam.samples_per_pixel = 4
    assert np.array_equal(a, gpu_scene(ctx, "mix0").render(cam, ds.env, ds.seed, None))


@pytest.mark.parametrize("name", ["cfg2", "cfg3", "cfg5"])
def test_full_size_properties(name, ctx):
    """BASELINE.json's full sizes (cfg2 1280x720x256, cfg3 1M triangles 1920x1080x512, cfg5 600x600x1024 depth 50) are far
    beyond what the CPU oracle can check in a test, so the full frames are checked through size-independent properties:
    bit-reproducibility, exact reassembly from interleaved tile shards (the multi-GPU decomposition), agreement of a
    sub-rectangle render with the same pixels of the full frame (pixel independence / integer indexing), segment
    conservation, and agreement of the embedded golden tile (which IS checked against the reference) with the frame."""
    from raytracer_project_amd import capi
    ds = demo_scene(name)
    cam = ds.camera
    sc = gpu_scene(ctx, name)
    full = sc.render(cam, ds.env, ds.seed, None, count=True)
    c_full = ctx.counters()
    assert np.isfinite(full).all() and (full >= 0).all()
    assert c_full.primary_samples == cam.image_width * cam.image_height * cam.samples_per_pixel
    # (1) reassembly from 2 interleaved shards, and segment conservation across shards
    acc = np.zeros_like(full)
    segs = 0
    for rank in range(2):
        part = sc.render(cam, ds.env, ds.seed, capi.Region(0, 0, 0, 0, 32, 2, rank, 0), count=True)
        segs += ctx.counters().segments
        acc += part
    assert np.array_equal(acc, full), "tile shards do not reassemble to the full frame bit for bit"
    assert segs == c_full.segments
    # (2) a sub-rectangle rendered alone equals the same pixels of the full frame
    x0, y0, w, h = cam.image_width // 3 + 5, cam.image_height // 2 - 7, 37, 19
    sub = sc.render(cam, ds.env, ds.seed, capi.Region(x0, y0, w, h, 0, 0, 0, 0))
    assert np.array_equal(sub[y0:y0 + h, x0:x0 + w], full[y0:y0 + h, x0:x0 + w])
    # (3) the golden tiles (reference-checked at full spp) are the same pixels of this frame
    for fx_name in {"cfg2": ["cfg2_tile", "cfg2_tile_b"], "cfg3": ["cfg3_full"], "cfg5": ["cfg5_tile"]}[name]:
        fx = load_golden(fx_name)
        m = fx["meta"]
        _check(full[m["y0"]:m["y0"] + m["h"], m["x0"]:m["x0"] + m["w"]], fx["mean"], fx_name + " inside the full frame")


@pytest.mark.parametrize("name", ["aov_mix0", "aov_mix1", "aov_cfg2", "aov_mesh0", "aov_inst0", "aov_inst2"])
def test_aov_passes_match_reference(name, ctx):
    """zr_render_aov (albedo / camera-space normal / z-depth of the primary hits) vs the genuine reference."""
    from raytracer_project_amd import capi
    fx = load_golden(name)
    m = fx["meta"]
    ds = demo_scene(m["scene"], m["scene_args"])
    reg = capi.Region(m["x0"], m["y0"], m["w"], m["h"], 0, 0, 0, 0)
    a, n, z = gpu_scene(ctx, m["scene"], m["scene_args"]).render_aov(ds.camera, ds.seed, m["zmax"], reg)
    sl = (slice(m["y0"], m["y0"] + m["h"]), slice(m["x0"], m["x0"] + m["w"]))
    _check(a[sl], fx["albedo"], name + " albedo")
    _check(n[sl], fx["normal"], name + " normal")
    _check(z[sl], fx["zdepth"], name + " z-depth")
    outside = np.ones(a.shape[:2], bool)
    outside[sl] = False
    assert not a[outside].any() and not n[outside].any() and not z[outside].any()


@pytest.mark.parametrize("name", ["passes_mix0", "passes_mix2", "passes_cfg2", "passes_cfg5", "passes_inst0"])
def test_reflection_refraction_passes_match_reference(name, ctx):
    """zr_render_passes (beauty + reflection / refraction split, camera.hpp:490-517) vs the genuine reference; segment and
    RNG-draw counts of both paths bit-exact; the beauty frame equals zr_render's image bit for bit."""
    from raytracer_project_amd import capi
    fx = load_golden(name)
    m = fx["meta"]
    ds = demo_scene(m["scene"], m["scene_args"])
    cam = ds.camera.copy()
    cam.samples_per_pixel = m["spp"]
    reg = capi.Region(m["x0"], m["y0"], m["w"], m["h"], 0, 0, 0, 0)
    sc = gpu_scene(ctx, m["scene"], m["scene_args"])
    b, r, f = sc.render_passes(cam, ds.env, ds.seed, reg)
    ctr = ctx.counters()
    sl = (slice(m["y0"], m["y0"] + m["h"]), slice(m["x0"], m["x0"] + m["w"]))
    _check(b[sl], fx["beauty"], name + " beauty")
    _check(r[sl], fx["reflection"], name + " reflection")
    _check(f[sl], fx["refraction"], name + " refraction")
    assert (ctr.primary_samples, ctr.segments, ctr.rng_draws) == (m["w"] * m["h"] * m["spp"], m["segments"], m["draws"])
    outside = np.ones(b.shape[:2], bool)
    outside[sl] = False
    assert not b[outside].any() and not r[outside].any() and not f[outside].any()
    plain = sc.render(cam, ds.env, ds.seed, reg)
    _check(b[sl], plain[sl], name + " beauty vs zr_render")


@pytest.mark.parametrize("name", ["mix0", "mix1", "mix2", "cfg2", "cfg5", "mesh0", "demo", "inst0", "inst1", "inst2"])
def test_path_records_match_oracle(name, ctx):
    """zr_trace_paths: every segment of 3000 primary samples — ray, hit, material, scatter decision, attenuation, emission
    and the number of RNG draws consumed — against the CPU oracle walking the same samples.  This is the device-side
    known-answer test of material::scatter / emitted and of the integrator's bookkeeping, segment by segment."""
    from oracle import zr_oracle_py as zo
    ds = demo_scene(name)
    cam = ds.camera.copy()
    sc = gpu_scene(ctx, name)
    rng = np.random.default_rng(11)
    n = 3000
    req = np.stack([rng.integers(0, cam.image_width, n), rng.integers(0, cam.image_height, n), rng.integers(0, cam.samples_per_pixel, n)], axis=1)
    nseg = min(cam.max_depth, 24)
    g = sc.trace_paths(cam, ds.seed, req, nseg)
    o = zo.OracleScene(ds.desc).trace_paths(cam, ds.seed, req, nseg)
    # decisions and counts are exact: hit flag, material, scattered flag, draws
    for col, what in ((6, "hit flag"), (8, "material"), (9, "scatter decision"), (16, "RNG draws")):
        bad = np.argwhere(g[:, :, col] != o[:, :, col])
        assert len(bad) == 0, f"{what}: {len(bad)} segments differ, first at request {req[bad[0][0]]} segment {bad[0][1]}"
    tol = 1e-7   # last-bit differences (fused multiply-add, libm) grow along a path of up to 24 refractions; decisions stay exact
    if name.startswith("inst"):
        tol = 1e-6   # ... and faster between the curved fuzz-0 mirrors of the instanced knots (1.5e-7 seen after eight bounces)
    for cols, what in ((slice(0, 6), "ray"), (slice(7, 8), "t"), (slice(10, 13), "attenuation"), (slice(13, 16), "emission")):
        err = np.abs(g[:, :, cols] - o[:, :, cols]) / np.maximum(1.0, np.abs(o[:, :, cols]))
        assert err.max() < tol, f"{what}: max error {err.max():.3e}"
    assert (o[:, :, 6] > 0).sum() > n, "the requests barely hit anything"


@pytest.mark.parametrize("variant", [0])
@pytest.mark.parametrize("name", ["cfg1_tile", "cfg2_tile_b", "cfg3_small", "cfg5_tile_b", "mix0_full", "mix1_full", "mesh0_full", "inst0_full", "inst1_full", "inst2_full", "demo_tile_b"])
def test_other_kernel_variants_match_reference(name, variant, built, monkeypatch):
    """ZR_KERNEL=0, the pixel-group megakernel that renders frames beyond the streaming pipeline's packing limits, shares the device
    arithmetic with the pipeline but walks the pair BVH and integrates in registers: same fixtures, same bar."""
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_KERNEL", str(variant))
    c = capi.Context(0)
    try:
        fx = load_golden(name)
        m = fx["meta"]
        ds = demo_scene(m["scene"], m["scene_args"])
        cam = ds.camera.copy()
        cam.samples_per_pixel = m["spp"]
        reg = capi.Region(m["x0"], m["y0"], m["w"], m["h"], 0, 0, 0, 0)
        sc = capi.Scene(c, ds.desc)
        out = sc.render(cam, ds.env, ds.seed, reg, count=True)
        ctr = c.counters()
        _check(out[m["y0"]:m["y0"] + m["h"], m["x0"]:m["x0"] + m["w"]], fx["mean"], f"{name} (variant {variant})")
        assert (ctr.primary_samples, ctr.segments, ctr.rng_draws) == (m["w"] * m["h"] * m["spp"], m["segments"], m["draws"])
        sc.close()
    finally:
        c.close()


def test_frames_beyond_the_streaming_limits_fall_back(ctx):
    """The streaming pipeline packs the bounce counter into 8 bits (max_depth <= 250); a deeper camera is rendered by the
    pixel-group megakernel automatically — same image contract, checked against the oracle (mix2: grey sky, long paths).
    Its paths end long before 250; tests/test_frame_edges.py has paths that run 250 segments, the switch at 251 and a side of 65536."""
    from oracle import zr_oracle_py as zo
    from raytracer_project_amd import capi
    ds = demo_scene("mix2")
    cam = ds.camera.copy()
    cam.max_depth, cam.samples_per_pixel = 300, 4
    reg = capi.Region(20, 12, 40, 24, 0, 0, 0, 0)
    gpu = gpu_scene(ctx, "mix2").render(cam, ds.env, ds.seed, reg, count=True)
    gctr = ctx.counters()
    cpu, cctr, _, _ = zo.OracleScene(ds.desc).render(cam, ds.env, ds.seed, reg)
    _check(gpu, cpu, "mix2 at max_depth 300")
    assert (gctr.segments, gctr.rng_draws, gctr.hits) == (cctr.segments, cctr.rng_draws, cctr.hits)
    assert gctr.rounds == 0, "expected the megakernel fallback, not the streaming pipeline"


@pytest.mark.parametrize("scene,spp", [("cfg2", 16), ("cfg5", 32)], ids=["pipeline", "fused"])
def test_cancellation_and_progress(scene, spp, ctx):
    """render_flag / lines_rendered of camera::render (camera.hpp:441, 548-552, 576-578) through the C ABI: *keep_going == 0
    stops the render with ZR_E_CANCELLED and leaves only finished work in the image; a completed render reports every row;
    passing the two pointers does not change the image.  On the streaming pipeline (cfg2) and on the fused small-scene kernel
    (cfg5), which renders a polled frame in sixteen launches."""
    import ctypes as C
    from raytracer_project_amd import capi
    ds = demo_scene(scene)
    cam = ds.camera.copy()
    cam.samples_per_pixel = spp
    sc = gpu_scene(ctx, scene)
    h, w = cam.image_height, cam.image_width
    plain = sc.render(cam, ds.env, ds.seed, None)
    lib = ctx.lib
    out = np.full((h, w, 3), -1.0)
    flag = C.c_uint8(1); rows = C.c_int(-5)
    rc = lib.zr_render(ctx._c, sc._s, C.byref(cam), C.byref(ds.env), C.c_uint64(ds.seed), None, 0, out.ctypes.data,
                       C.cast(C.byref(flag), C.c_void_p), C.cast(C.byref(rows), C.c_void_p))
    assert rc == 0 and rows.value == h
    assert np.array_equal(out, plain)
    # cancelled before it starts: error code, message, nothing but finished (= no) work written, progress short of the frame
    out2 = np.zeros((h, w, 3))
    flag = C.c_uint8(0); rows = C.c_int(-5)
    rc = lib.zr_render(ctx._c, sc._s, C.byref(cam), C.byref(ds.env), C.c_uint64(ds.seed), None, 0, out2.ctypes.data,
                       C.cast(C.byref(flag), C.c_void_p), C.cast(C.byref(rows), C.c_void_p))
    assert rc == -4 and b"cancel" in lib.zr_last_error().lower()
    assert 0 <= rows.value < h
    assert np.isfinite(out2).all() and (out2 >= 0).all() and out2.sum() < plain.sum()
    # the context is still usable
    assert np.array_equal(sc.render(cam, ds.env, ds.seed, None), plain)


def test_progress_and_preview_during_render(ctx, monkeypatch):
    """camera::lines_rendered advances WHILE the frame renders and the caller's accumulator shows the partial frame
    (camera.hpp:548-552, main.cpp:1576): a second thread watches rows_done and out_rgb during a zr_render call."""
    import ctypes as C
    import threading
    import time
    monkeypatch.setenv("ZR_PREVIEW_PERIOD_S", "0.02")
    ds = demo_scene("cfg2")
    cam = ds.camera.copy()
    cam.samples_per_pixel = 256
    sc = gpu_scene(ctx, "cfg2")
    h, w = cam.image_height, cam.image_width
    plain = sc.render(cam, ds.env, ds.seed, None)
    out = np.zeros((h, w, 3))
    flag = C.c_uint8(1); rows = C.c_int(0)
    seen, partial_sums = [], []
    done = threading.Event()

    def watch():
        while not done.is_set():
            seen.append(rows.value)
            partial_sums.append(float(out[::16, ::16].sum()))
            time.sleep(0.002)
    t = threading.Thread(target=watch); t.start()
    try:
        rc = ctx.lib.zr_render(ctx._c, sc._s, C.byref(cam), C.byref(ds.env), C.c_uint64(ds.seed), None, 0, out.ctypes.data,
                               C.cast(C.byref(flag), C.c_void_p), C.cast(C.byref(rows), C.c_void_p))
    finally:
        done.set(); t.join()
    assert rc == 0 and rows.value == h
    assert np.array_equal(out, plain), "the preview must not change the final image"
    mid = [r for r in seen if 0 < r < h]
    assert len(set(mid)) >= 3, f"rows_done did not advance during the render: {sorted(set(seen))[:10]}"
    assert seen == sorted(seen), "rows_done went backwards"
    final = float(plain[::16, ::16].sum())
    assert any(0.02 * final < p < 0.98 * final for p in partial_sums), "no partial frame was seen in the caller's buffer"


def test_cxx_host_collective_single_rank(ctx):
    """zr_comm_*: the RCCL reduce entry points a C++ host uses.  With one rank the reduce is the identity; this checks the
    lazy librccl.so binding, communicator creation on the context's device and an in-place ncclReduce of doubles."""
    import ctypes as C
    import torch
    from raytracer_project_amd import capi
    lib = ctx.lib
    uid = (C.c_ubyte * 128)()
    assert lib.zr_comm_unique_id(uid) == 0, lib.zr_last_error()
    comm = lib.zr_comm_create(ctx._c, 1, 0, uid)
    assert comm, lib.zr_last_error()
    frame = torch.arange(3 * 64 * 48, dtype=torch.float64, device="cuda").reshape(48, 64, 3) * 0.25
    want = frame.clone()
    assert lib.zr_comm_reduce_frame(comm, C.c_void_p(frame.data_ptr()), frame.numel(), 0, None) == 0, lib.zr_last_error()
    torch.cuda.synchronize()
    assert torch.equal(frame, want)
    # the packed-tile exchange (pack own tiles -> send to the root -> scatter there): with one rank the frame comes back as it was
    for tile in (0, 20):   # default 32-pixel tiles; 20-pixel tiles leave clipped tiles at both edges of the 64 x 48 frame
        reg = capi.Region(0, 0, 0, 0, tile, 0, 0, 0)
        assert lib.zr_comm_gather_frame(comm, C.c_void_p(frame.data_ptr()), 64, 48, C.byref(reg), 0, None) == 0, lib.zr_last_error()
        torch.cuda.synchronize()
        assert torch.equal(frame, want)
    # a region that is not the partition the exchange assumes is refused, not "gathered"
    bad = capi.Region(0, 0, 0, 0, 32, 2, 1, 0)
    assert lib.zr_comm_gather_frame(comm, C.c_void_p(frame.data_ptr()), 64, 48, C.byref(bad), 0, None) == capi.ZR_E_INVALID
    part = capi.Region(8, 8, 16, 16, 32, 0, 0, 0)
    assert lib.zr_comm_gather_frame(comm, C.c_void_p(frame.data_ptr()), 64, 48, C.byref(part), 0, None) == capi.ZR_E_INVALID
    lib.zr_comm_destroy(comm)


def test_cxx_host_exchange_through_rccl_on_one_rank(ctx):
    """zr_comm_gather_frame's whole exchange — pack -> ncclSend / ncclRecv (one group) -> unpack — executed on a one-GPU box: with
    ZR_COMM_SELF_EXCHANGE the single rank sends its packed tiles to itself through RCCL; the frame is poisoned between pack and unpack."""
    import ctypes as C
    import torch
    from raytracer_project_amd import capi
    lib = ctx.lib
    uid = (C.c_ubyte * 128)()
    assert lib.zr_comm_unique_id(uid) == 0, lib.zr_last_error()
    comm = lib.zr_comm_create(ctx._c, 1, 0, uid)
    assert comm, lib.zr_last_error()
    os.environ["ZR_COMM_SELF_EXCHANGE"] = "1"
    try:
        for (W, H, tile) in ((64, 48, 0), (70, 50, 20), (1920, 1080, 32)):
            frame = (torch.arange(3 * W * H, dtype=torch.float64, device="cuda").reshape(H, W, 3) + 1) * 0.25
            want = frame.clone()
            reg = capi.Region(0, 0, 0, 0, tile, 0, 0, 0)
            assert lib.zr_comm_gather_frame(comm, C.c_void_p(frame.data_ptr()), W, H, C.byref(reg), 0, None) == 0, lib.zr_last_error()
            torch.cuda.synchronize()
            assert torch.equal(frame, want), (W, H, tile)
    finally:
        del os.environ["ZR_COMM_SELF_EXCHANGE"]
        lib.zr_comm_destroy(comm)


def test_multi_exchange_on_the_nccl_backend_world_of_one():
    """multi.gather_frame / reduce_frame as bench.py --gpus N runs them — torch.distributed on the `nccl` backend (= RCCL), device
    tensors — executed on a one-GPU box: a process group of one rank, the `world <= 1` early-outs bypassed (`_force`).  Runs in a child process
    (a process group is process-wide state)."""
    import subprocess
    import sys
    import tempfile
    from conftest import ROOT
    worker = r'''
import os, sys
sys.path.insert(0, os.environ["ZR_ROOT"])
os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1")
import torch, torch.distributed as dist
from raytracer_project_amd import multi
assert "HSA_ENABLE_IPC_MODE_LEGACY" not in os.environ
rank, local, world = multi.init_distributed()          # before anything has touched the GPU: it must put the dmabuf-IPC setting into the environment
assert (rank, world) == (0, 1) and os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
torch.cuda.set_device(0)
dist.init_process_group(backend="nccl", rank=0, world_size=1)
assert dist.get_backend() == "nccl"
for (H, W, tile) in ((48, 64, 32), (50, 70, 16), (1080, 1920, 32)):
    full = (torch.arange(H * W * 3, dtype=torch.float64, device="cuda").reshape(H, W, 3) + 1) * 0.5
    acc = full.clone()
    multi.gather_frame(acc, 1, 0, tile, _force=True)
    torch.cuda.synchronize()
    assert torch.equal(acc, full), ("gather", H, W, tile)
    acc = full.clone()
    multi.reduce_frame(acc, 1, 0, _force=True)
    torch.cuda.synchronize()
    assert torch.equal(acc, full), ("reduce", H, W)
vals = multi.all_reduce_values([1.5, 2.5], 1, torch.device("cuda", 0))
assert vals == [1.5, 2.5]
dist.destroy_process_group()
print("nccl world-of-one ok")
'''
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "w.py")
        open(f, "w").write(worker)
        env = dict(os.environ, ZR_ROOT=ROOT, MASTER_PORT="29553")
        env.pop("HSA_ENABLE_IPC_MODE_LEGACY", None)   # init_distributed must set it itself
        p = subprocess.run([sys.executable, f], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "nccl world-of-one ok" in p.stdout, p.stdout + p.stderr


def test_cxx_host_collective_two_ranks():
    """zr_comm_gather_frame / zr_comm_reduce_frame between two processes on two GPUs (ids exchanged over a gloo group).  Needs a
    node with at least two devices: skipped on the one-GPU test box."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL refuses two ranks on one device)")
    import os
    import subprocess
    import sys
    import tempfile
    from conftest import ROOT
    worker = r'''
import ctypes as C, os, sys
import torch, torch.distributed as dist
sys.path.insert(0, os.environ["ZR_ROOT"])
from raytracer_project_amd import capi, multi
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
torch.cuda.set_device(rank)
ctx = capi.Context(rank); lib = ctx.lib
uid = (C.c_ubyte * 128)()
if rank == 0:
    assert lib.zr_comm_unique_id(uid) == 0
t = torch.tensor(list(uid), dtype=torch.uint8); dist.broadcast(t, 0)
uid = (C.c_ubyte * 128)(*t.tolist())
comm = lib.zr_comm_create(ctx._c, world, rank, uid)
assert comm, lib.zr_last_error()
H, W, T = 50, 70, 16
full = (torch.arange(H * W * 3, dtype=torch.float64, device="cuda").reshape(H, W, 3) + 1) * 0.5
own = multi.owned_pixels(H, W, world, full.device, T)
for mode in ("gather", "reduce"):
    frame = torch.zeros_like(full)
    frame.view(-1, 3)[own[rank]] = full.view(-1, 3)[own[rank]]
    if mode == "gather":
        reg = multi.tile_region(capi, rank, world, T)
        rc = lib.zr_comm_gather_frame(comm, C.c_void_p(frame.data_ptr()), W, H, C.byref(reg), 0, None)
    else: rc = lib.zr_comm_reduce_frame(comm, C.c_void_p(frame.data_ptr()), frame.numel(), 0, None)
    assert rc == 0, lib.zr_last_error()
    torch.cuda.synchronize()
    if rank == 0: assert torch.equal(frame, full), mode
lib.zr_comm_destroy(comm)
print("rank", rank, "ok")
'''
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "w.py")
        open(f, "w").write(worker)
        p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                            "--master-port", "29547", f], env=dict(os.environ, ZR_ROOT=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.count("ok") == 2, p.stdout + p.stderr


def test_affine_unit_handout_is_bit_identical(ctx):
    """ZR_STREAM_AFFINE=1 (work units dealt to the shards in screen-space chunks, zr_stream.hip st_unit_of) changes which slot
    renders which sample and nothing else: the frame equals the striped hand-out's bit for bit, whole and sharded."""
    from raytracer_project_amd import capi
    ds = demo_scene("mix0")
    sc = gpu_scene(ctx, "mix0")
    cam = ds.camera.copy(); cam.samples_per_pixel = 24
    outs = {}
    for aff in ("0", "1"):
        os.environ["ZR_STREAM_AFFINE"] = aff
        try:
            outs[aff] = (sc.render(cam, ds.env, ds.seed), sc.render(cam, ds.env, ds.seed, capi.Region(0, 0, 0, 0, 16, 3, 1, 0)))
        finally:
            del os.environ["ZR_STREAM_AFFINE"]
    assert np.array_equal(outs["0"][0], outs["1"][0])
    assert np.array_equal(outs["0"][1], outs["1"][1])
    assert float(outs["1"][0].sum()) > 0


def test_released_scene_is_not_rearmed_by_a_table_setter(ctx):
    """After a borrowed commit the geometry views are gone: zr_scene_set_materials alone must not make the scene committable
    again (it would build an empty world); giving every geometry array again does."""
    import ctypes as C
    from raytracer_project_amd import capi
    ds = demo_scene("cfg1")
    lib = ctx.lib
    s = lib.zr_scene_create(ctx._c)
    assert lib.zr_scene_set_all_borrowed(s, C.byref(ds.desc)) == 0 and lib.zr_scene_commit(s) == 0, lib.zr_last_error()
    assert lib.zr_scene_commit(s) == capi.ZR_E_STATE
    assert lib.zr_scene_set_materials(s, ds.desc.materials, ds.desc.n_materials) == 0
    assert lib.zr_scene_commit(s) == capi.ZR_E_STATE, "a table setter re-armed a released scene"
    assert lib.zr_scene_set_all(s, C.byref(ds.desc)) == 0 and lib.zr_scene_commit(s) == 0, lib.zr_last_error()
    lib.zr_scene_destroy(s)


# ---- what the render entry points validate, pinned ------------------------------------------------------------------------------
# (return code, zr_last_error text) of every entry point for every bad input below, recorded from the library of commit 09e3243 (this test run against it through ZR_LIB), before the host
# drivers were regrouped (zr_render.cpp: prepare_frame, check_env, scene_ready): the table states what the library did, not what it ought to do, and a
# change to it is a behaviour change.  zr_trace and zr_trace_paths accept a scene of another context; every other entry refuses it.
_ENTRIES = ["zr_render", "zr_render_device", "zr_render_aov", "zr_render_passes", "zr_render_bvh_debug", "zr_trace", "zr_trace_paths", "zr_kat_background"]
_NULL = "null argument"
_REGION = "region outside the 96x64 frame or bad tile parameters"
_ENVMODE = "unknown environment mode 99"
_HDR = "environment texture id out of range"
_OTHER = "scene belongs to another context"
_UNCOMMITTED = {e: (-3, "zr_scene_commit must precede " + ("zr_render" if e == "zr_render_device" else e)) for e in _ENTRIES}
_FRAME_ENTRIES = _ENTRIES[:5]      # take a region
_ENV_ENTRIES = ["zr_render", "zr_render_device", "zr_render_passes", "zr_render_bvh_debug", "zr_kat_background"]
_VALIDATION = {
    "valid": {e: (0, "") for e in _ENTRIES},
    "uncommitted": _UNCOMMITTED,
    "other_context": {e: ((0, "") if e in ("zr_trace", "zr_trace_paths") else (-1, _OTHER)) for e in _ENTRIES},
    "region_outside": {e: ((-1, _REGION) if e in _FRAME_ENTRIES else (0, "")) for e in _ENTRIES},
    "tile_rem": {e: ((-1, _REGION) if e in _FRAME_ENTRIES else (0, "")) for e in _ENTRIES},
    "tile_size": {e: ((-1, _REGION) if e in _FRAME_ENTRIES else (0, "")) for e in _ENTRIES},
    "env_mode": {e: ((-1, _ENVMODE) if e in _ENV_ENTRIES else (0, "")) for e in _ENTRIES},
    "hdr_texture": {e: ((-1, _HDR) if e in _ENV_ENTRIES else (0, "")) for e in _ENTRIES},
    # no output at all: fine for the AOV and split passes and for an empty batch of rays / requests / directions, an error for a frame
    "null_outputs": {e: ((-1, _NULL) if e in ("zr_render", "zr_render_device", "zr_render_bvh_debug") else (0, "")) for e in _ENTRIES},
    # ... but only after the state checks
    "uncommitted_null_outputs": {e: ((-1, _NULL) if e in ("zr_render", "zr_render_device", "zr_render_bvh_debug") else _UNCOMMITTED[e]) for e in _ENTRIES},
    "other_context_null_outputs": {e: ((-1, _NULL) if e in ("zr_render", "zr_render_device", "zr_render_bvh_debug") else
                                       (0, "") if e in ("zr_trace", "zr_trace_paths") else (-1, _OTHER)) for e in _ENTRIES},
    # a bad region and a bad environment together: the region is looked at first
    "region_and_env_mode": {e: ((-1, _REGION) if e in _FRAME_ENTRIES else (-1, _ENVMODE) if e in _ENV_ENTRIES else (0, "")) for e in _ENTRIES},
}


def observed_validation(ctx):
    """{case: {entry point: (return code, error text or "")}} for the cases of _VALIDATION, on a 96 x 64 frame of mix0"""
    import ctypes as C
    import torch
    from raytracer_project_amd import capi
    lib = ctx.lib
    ds = demo_scene("mix0")
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel = 96, 64, 2
    good = gpu_scene(ctx, "mix0")._s
    other_ctx = capi.Context(0)
    other = capi.Scene(other_ctx, ds.desc)
    raw = lib.zr_scene_create(ctx._c)
    h, w = cam.image_height, cam.image_width
    frames = [np.zeros((h, w, 3)) for _ in range(3)]
    d_frame = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    rays = np.array([[0.0, 1.0, 5.0, 0.0, 0.0, -1.0]] * 4)
    hits = np.zeros(4, dtype=capi.HIT_DTYPE)
    req = np.array([[3, 4, 0], [50, 20, 1]], dtype=np.int32)
    paths = np.zeros((2, 3, 17))
    dirs = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    bg = np.zeros((2, 3))
    ap = capi.AovParams(100.0)
    dp = capi.BvhDebugParams.defaults()
    bad_mode = capi.Env.from_buffer_copy(bytes(ds.env)); bad_mode.mode = 99
    bad_hdr = capi.Env.from_buffer_copy(bytes(ds.env)); bad_hdr.mode, bad_hdr.hdr_texture = 1, 1000000   # ZR_ENV_HDR_MAP
    outside = capi.Region(w - 8, 0, 16, 8, 0, 0, 0, 0)

    def call(entry, s, reg, env, outputs):
        rp = C.byref(reg) if reg is not None else None
        o = [f.ctypes.data if outputs else None for f in frames]
        seed = C.c_uint64(ds.seed)
        if entry == "zr_render":
            return lib.zr_render(ctx._c, s, C.byref(cam), C.byref(env), seed, rp, 0, o[0], None, None)
        if entry == "zr_render_device":
            rc = lib.zr_render_device(ctx._c, s, C.byref(cam), C.byref(env), seed, rp, 0, C.c_void_p(d_frame.data_ptr()) if outputs else None, None)
            torch.cuda.synchronize()
            return rc
        if entry == "zr_render_aov":
            return lib.zr_render_aov(ctx._c, s, C.byref(cam), seed, rp, C.byref(ap), o[0], o[1], o[2])
        if entry == "zr_render_passes":
            return lib.zr_render_passes(ctx._c, s, C.byref(cam), C.byref(env), seed, rp, o[0], o[1], o[2])
        if entry == "zr_render_bvh_debug":
            return lib.zr_render_bvh_debug(ctx._c, s, C.byref(cam), C.byref(env), seed, rp, C.byref(dp), o[0], None, None)
        if entry == "zr_trace":
            return lib.zr_trace(ctx._c, s, rays.ctypes.data if outputs else None, 4 if outputs else 0, 0.001, float("inf"), C.c_uint64(1), C.c_uint64(7), 0,
                                hits.ctypes.data if outputs else None)
        if entry == "zr_trace_paths":
            return lib.zr_trace_paths(ctx._c, s, C.byref(cam), seed, req.ctypes.data if outputs else None, 2 if outputs else 0, 3, paths.ctypes.data if outputs else None)
        if entry == "zr_kat_background":
            return lib.zr_kat_background(ctx._c, s, C.byref(env), dirs.ctypes.data if outputs else None, 2 if outputs else 0, bg.ctypes.data if outputs else None)
        raise KeyError(entry)

    cases = {
        "valid": (good, None, ds.env, True),
        "uncommitted": (raw, None, ds.env, True),
        "other_context": (other._s, None, ds.env, True),
        "region_outside": (good, outside, ds.env, True),
        "tile_rem": (good, capi.Region(0, 0, 0, 0, 16, 2, 2, 0), ds.env, True),
        "tile_size": (good, capi.Region(0, 0, 0, 0, 2048, 0, 0, 0), ds.env, True),
        "env_mode": (good, None, bad_mode, True),
        "hdr_texture": (good, None, bad_hdr, True),
        "null_outputs": (good, None, ds.env, False),
        "uncommitted_null_outputs": (raw, None, ds.env, False),
        "other_context_null_outputs": (other._s, None, ds.env, False),
        "region_and_env_mode": (good, outside, bad_mode, True),
    }
    seen = {}
    try:
        for case, args in cases.items():
            seen[case] = {}
            for entry in _ENTRIES:
                rc = call(entry, *args)
                seen[case][entry] = (rc, lib.zr_last_error().decode() if rc != 0 else "")
    finally:
        lib.zr_scene_destroy(raw)
        other.close(); other_ctx.close()
    return seen


def test_entry_point_validation_is_pinned(ctx):
    """Every render entry point against every bad input of _VALIDATION: the return code and the error text."""
    seen = observed_validation(ctx)
    assert set(seen) == set(_VALIDATION)
    wrong = [(case, e, seen[case][e], _VALIDATION[case][e]) for case in _VALIDATION for e in _ENTRIES if tuple(seen[case][e]) != tuple(_VALIDATION[case][e])]
    for row in wrong:
        print("%s / %s: got %r, recorded %r" % row)
    assert not wrong, wrong


@pytest.mark.parametrize("region", [(16, 8, 40, 24, 16, 0, 0, 0), (0, 0, 0, 0, 16, 3, 1, 0), (10, 5, 70, 50, 32, 2, 1, 1)], ids=["rectangle", "sharded", "skewed"])
def test_region_renders_touch_only_their_pixels(region, ctx):
    """zr_render, the AOV passes, the split passes and the BVH debug view write the pixels of their region's tiles and no others: the caller's
    buffers are pre-filled with a sentinel."""
    from raytracer_project_amd import capi
    ds = demo_scene("mix0")
    sc = gpu_scene(ctx, "mix0")
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel = 96, 64, 2
    h, w = cam.image_height, cam.image_width
    reg = capi.Region(*region)
    ts, mod, rem, skew = reg.tile_size, max(reg.tile_mod, 1), reg.tile_rem, reg.tile_skew
    x0, y0, x1, y1 = (reg.x0, reg.y0, reg.x0 + reg.w, reg.y0 + reg.h) if reg.w > 0 else (0, 0, w, h)
    tiles_x = (w + ts - 1) // ts
    yy, xx = np.mgrid[0:h, 0:w]
    part = (xx // ts + skew * (yy // ts)) % mod if skew > 0 else ((yy // ts) * tiles_x + xx // ts) % mod
    inside = (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1) & (part == rem)
    assert inside.any() and not inside.all()
    SENTINEL = -7.25
    lib = ctx.lib
    import ctypes as C
    bufs = {k: np.full((h, w, 3), SENTINEL) for k in ("render", "albedo", "normal", "zdepth", "beauty", "reflection", "refraction", "debug")}
    seed, rp = C.c_uint64(ds.seed), C.byref(reg)
    ap, dp = capi.AovParams(100.0), capi.BvhDebugParams.defaults()
    p = lambda k: bufs[k].ctypes.data
    assert lib.zr_render(ctx._c, sc._s, C.byref(cam), C.byref(ds.env), seed, rp, 0, p("render"), None, None) == 0, lib.zr_last_error()
    assert lib.zr_render_aov(ctx._c, sc._s, C.byref(cam), seed, rp, C.byref(ap), p("albedo"), p("normal"), p("zdepth")) == 0, lib.zr_last_error()
    assert lib.zr_render_passes(ctx._c, sc._s, C.byref(cam), C.byref(ds.env), seed, rp, p("beauty"), p("reflection"), p("refraction")) == 0, lib.zr_last_error()
    assert lib.zr_render_bvh_debug(ctx._c, sc._s, C.byref(cam), C.byref(ds.env), seed, rp, C.byref(dp), p("debug"), None, None) == 0, lib.zr_last_error()
    for k, b in bufs.items():
        assert (b[~inside] == SENTINEL).all(), f"{k}: pixels outside the region were written"
        assert (b[inside] != SENTINEL).all(), f"{k}: pixels of the region were left out"
    # and the region's pixels are the whole frame's
    whole = sc.render(cam, ds.env, ds.seed)
    assert np.array_equal(bufs["render"][inside], whole[inside])


# rows_done after B batches of 12 tiles of a 128 x 128 frame in 16-pixel tiles (8 tiles per row): the last tile of batch B lies in tile row
# (12 B - 1) // 8 = 1, 2, 4, 5, 7.  The pixel-group path of zr_render reports the rows ABOVE that tile row, the BVH debug view the rows down to its
# lower edge: two rules, recorded as they are.
_ROWS_AFTER_BATCH = {"pixel_group": {1: 16, 2: 32, 3: 64, 4: 80, 5: 112}, "bvh_debug": {1: 32, 2: 48, 3: 80, 4: 96, 5: 128}}


@pytest.mark.parametrize("which", ["pixel_group", "bvh_debug"])
def test_rows_done_after_a_batch(which, built, monkeypatch):
    """The two tile-batch loops (zr_render through the pixel-group kernel, ZR_KERNEL=0, and zr_render_bvh_debug) advance rows_done after every batch.
    The render is cancelled as soon as rows_done moves; the error text says after how many batches, and rows_done must hold that batch's value."""
    import ctypes as C
    import re
    import threading
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_KERNEL", "0" if which == "pixel_group" else "2")
    monkeypatch.setenv("ZR_BATCH_TILES", "12")
    c = capi.Context(0)
    try:
        ds = demo_scene("mix0")
        sc = capi.Scene(c, ds.desc)
        cam = ds.camera.copy()
        cam.image_width, cam.image_height, cam.samples_per_pixel = 128, 128, 256 if which == "pixel_group" else 1024   # batches of milliseconds: the watcher is in time
        reg = capi.Region(0, 0, 0, 0, 16, 0, 0, 0)
        out = np.zeros((128, 128, 3))
        flag, rows = C.c_uint8(1), C.c_int(-5)
        done = threading.Event()

        def watch():
            while not done.is_set():
                if rows.value > 0:
                    flag.value = 0
                    return
        t = threading.Thread(target=watch); t.start()
        try:
            if which == "pixel_group":
                rc = c.lib.zr_render(c._c, sc._s, C.byref(cam), C.byref(ds.env), C.c_uint64(ds.seed), C.byref(reg), 0, out.ctypes.data, C.byref(flag), C.byref(rows))
            else:
                dp = capi.BvhDebugParams.defaults()
                rc = c.lib.zr_render_bvh_debug(c._c, sc._s, C.byref(cam), C.byref(ds.env), C.c_uint64(ds.seed), C.byref(reg), C.byref(dp), out.ctypes.data,
                                               C.byref(flag), C.byref(rows))
        finally:
            done.set(); t.join()
        msg = c.lib.zr_last_error().decode()
        print(f"{which}: rc {rc}, rows_done {rows.value}, {msg!r}")
        assert rc == capi.ZR_E_CANCELLED, (rc, msg)
        m = re.fullmatch(r"render cancelled after (\d+) of 6 batches", msg)
        assert m, msg
        b = int(m.group(1))
        assert 1 <= b <= 5
        assert rows.value == _ROWS_AFTER_BATCH[which][b], (b, rows.value)
        sc.close()
    finally:
        c.close()


@pytest.mark.parametrize("name", ["mix0", "mix1", "inst0", "inst2"])
def test_builders_agree_on_what_does_not_depend_on_the_tree(name, ctx):
    """Both builders commit the same world (each with ZR_BUILD_CHECK=1): the same objects, the same kernel builds, the same leaf primitives — per leaf
    kind, the caller's indices the leaves of the world's tree name, each once and as many as the world list has entries — and the same material behind 2000
    fixed camera rays."""
    ds = demo_scene(name)
    host, dev = gpu_scene(ctx, name, (), "host"), gpu_scene(ctx, name, (), "device")
    assert host.stats()["objects"] == dev.stats()["objects"]
    assert host.kernels() == dev.kernels()

    def leaf_src(sc):
        b = sc.tree_boxes()
        leaves = b[(b["leaf"] == 1) & (b["tree"] == 0)]   # the world's tree (a placed run's own tree lists its triangles once per group, not per entry)
        assert (leaves["count"] <= 4).all()
        return {int(k): np.sort(np.concatenate([l["src"][:l["count"]] for l in leaves[leaves["kind"] == k]])) for k in np.unique(leaves["kind"])}
    hs, dv = leaf_src(host), leaf_src(dev)
    assert hs.keys() == dv.keys()
    for k in hs:
        assert np.array_equal(hs[k], dv[k]), (name, k)
        if k in (4, 6):   # wrapped objects and placed runs are named by their world-list entry: each exactly once
            assert len(np.unique(hs[k])) == len(hs[k]), (name, k)
    assert sum(len(v) for v in hs.values()) == host.stats()["objects"]
    cam = ds.camera.copy()
    rng = np.random.default_rng(2000)
    px = np.stack([rng.integers(0, cam.image_width, 2000), rng.integers(0, cam.image_height, 2000), np.zeros(2000, np.int64)], axis=1).astype(np.int32)
    rays = np.ascontiguousarray(ctx.kat_camera_rays(cam, ds.seed, px)[:, :6])
    assert np.array_equal(host.trace(rays)["mat"], dev.trace(rays)["mat"])
