"""Progressive accumulation (zr_accum): a frame rendered in batches of samples.

The contract: sample s of a pixel belongs to lane s % 64, a lane adds its samples in increasing s, and the lanes are combined by the xor
butterfly of the kernel that rendered them.  So any split of [0, N) into consecutive batches gives the one-shot frame bit for bit, and every
prefix [0, k) is the k-spp image.  tests/accum_model.py restates the order in NumPy.

CPU: the exports and the refusals that need no device, the model's split invariance, and the model against the oracle's per-sample radiance.
GPU (-m gpu): split invariance on every route, prefixes, a sample range against the reference, the order itself, the state rules, zr_render's
forced batching and the drop-in's camera::samples_per_pass."""
import ctypes as C

import numpy as np
import pytest

import accum_model as am
from conftest import demo_scene, rel_err

REL_TOL = 1e-4      # the suite's bar (tests/test_gpu_parity.py): "within 1e-4 relative per-channel"
ABS_FLOOR = 1e-7

ACCUM_SYMBOLS = ["zr_accum_create", "zr_accum_destroy", "zr_accum_reset", "zr_render_accumulate", "zr_accum_resolve", "zr_accum_resolve_device",
                 "zr_accum_state"]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------

def test_accumulator_entry_points_are_exported(built):
    from raytracer_project_amd import capi
    lib = capi.load()
    for name in ACCUM_SYMBOLS:
        assert hasattr(lib, name) and name in capi.CAPI_SYMBOLS, name
    assert hasattr(capi.load_scenes(), "zrs_render_dropin_progressive")
    assert hasattr(capi, "Accumulator")
    assert lib.zr_abi_version() == 3


def test_null_arguments_are_refused_without_a_device(built):
    """Every entry looks at its pointers before it touches a device: ZR_E_INVALID (NULL from create) and a message."""
    from raytracer_project_amd import capi
    lib = capi.load()
    cam, env = capi.Camera(), capi.Env()
    out = np.zeros(3)
    st = (C.c_int64 * 4)()
    assert lib.zr_accum_create(None, 64, 64, None) is None
    assert b"null" in lib.zr_last_error()
    calls = [lambda: lib.zr_accum_reset(None, 0),
             lambda: lib.zr_render_accumulate(None, None, C.byref(cam), C.byref(env), C.c_uint64(1), None, 4, 0, None),
             lambda: lib.zr_accum_resolve(None, out.ctypes.data),
             lambda: lib.zr_accum_resolve_device(None, None, None),
             lambda: lib.zr_accum_state(None, C.byref(st))]
    for call in calls:
        assert call() == capi.ZR_E_INVALID
        assert b"null" in lib.zr_last_error()
    lib.zr_accum_destroy(None)   # like free(NULL)


@pytest.mark.parametrize("asc_lanes", [1, 64])
def test_model_is_split_invariant(asc_lanes):
    """Lane sums carried from batch to batch do not know where the batches were cut — a sum of batch means does."""
    rng = np.random.default_rng(7)
    s = rng.random((5, 7, 100, 3)) * np.exp(rng.normal(0, 3, (5, 7, 100, 1)))
    whole = am.frame(s, asc_lanes=asc_lanes)
    for splits in ([1] * 100, [63, 37], [64, 36], [65, 35], [37, 27, 36], [1, 99]):
        assert np.array_equal(am.frame(s, splits=splits, asc_lanes=asc_lanes), whole), splits
    means = (s[..., :37, :].mean(axis=-2) * 37 + s[..., 37:64, :].mean(axis=-2) * 27 + s[..., 64:, :].mean(axis=-2) * 36) / 100
    assert not np.array_equal(means, whole) and np.allclose(means, whole, rtol=1e-13)
    # fewer samples than lanes: the pixel-group kernel's lanes_for(n) lanes, two samples in some of them
    for n in (1, 16, 37, 63):
        L = am.lanes_for(n)
        direct = np.zeros(s.shape[:2] + (L, 3))
        for k in range(n):
            direct[..., k % L, :] += s[..., k, :]
        m = 1
        while m < L:
            direct = direct + direct[..., np.arange(L) ^ m, :]
            m <<= 1
        assert np.array_equal(am.frame(s[..., :n, :], asc_lanes=L), direct[..., 0, :] * (1.0 / n)), n


PREFIX_TILES = [("cfg2", (), (600, 300, 40, 24)), ("cfg3", (200, 20, 256, 128), (900, 500, 40, 24)), ("cfg5", (), (250, 300, 40, 24)), ("mix0", (), None)]


@pytest.mark.parametrize("name,args,rect", PREFIX_TILES, ids=[t[0] for t in PREFIX_TILES])
def test_model_matches_the_oracle_on_every_prefix(name, args, rect, built):
    """The reference restatement keys a sample by (seed, pixel, sample) only: its per-sample radiance at spp = 37 is the first 37 samples at
    spp = 100, exactly.  And the model over samples[:k] is the oracle's spp = k frame up to the rounding of a reordered FP64 sum of k terms,
    k * 2^-52 relative: 8.2e-15 at k = 37, 2.2e-14 at k = 100 (observed maxima: 1.6e-15 at k = 37, 2.7e-15 at k = 100, on mix0)."""
    from oracle import zr_oracle_py as zo
    from raytracer_project_amd import capi
    ds = demo_scene(name, args)
    osc = zo.OracleScene(ds.desc)
    reg = capi.Region(*rect, 0, 0, 0, 0) if rect else None
    cam = ds.camera.copy()
    cam.samples_per_pixel = 100
    _, _, s100, _ = osc.render(cam, ds.env, ds.seed, reg, per_sample=True)
    for k in (37, 100):
        cam.samples_per_pixel = k
        frame, _, sk, _ = osc.render(cam, ds.env, ds.seed, reg, per_sample=True)
        if rect:
            frame = frame[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]
        assert np.array_equal(sk, s100[:, :, :k])
        got = am.frame(s100[:, :, :k])
        err = np.abs(got - frame)
        print(f"{name} k={k}: max rel diff {float((err / np.maximum(np.abs(frame), 1e-300)).max()):.3e}")
        assert (err <= k * 2.0 ** -52 * np.abs(frame)).all()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(built):
    from raytracer_project_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


_scenes = {}


def _scene(ctx, name, args=()):
    from raytracer_project_amd import capi
    key = (id(ctx), name, tuple(args))
    if key not in _scenes:
        _scenes[key] = capi.Scene(ctx, demo_scene(name, args).desc)
    return _scenes[key]


def _region(rect):
    from raytracer_project_amd import capi
    return capi.Region(*rect, 0, 0, 0, 0) if rect else None


def _ctr(k):
    return (int(k.primary_samples), int(k.segments), int(k.rng_draws), int(k.hits))


def _split_case(c, name, rect, max_depth, want_path, N, splits_list):
    """one scene and region: every split of [0, N) resolves to Scene.render at spp = N, and the batches' counters add up to its counters"""
    from raytracer_project_amd import capi
    ds = demo_scene(name)
    sc = _scene(c, name)
    cam = ds.camera.copy()
    if max_depth:
        cam.max_depth = max_depth
    reg = _region(rect)
    cam.samples_per_pixel = N
    want = sc.render(cam, ds.env, ds.seed, reg, count=True)
    k = c.counters()
    assert int(k.path) == want_path, (name, int(k.path))
    want_ctr = _ctr(k)
    acc = capi.Accumulator(c, cam.image_width, cam.image_height, reg)
    try:
        cam.samples_per_pixel = 3   # ignored by accumulate
        for splits in splits_list:
            assert sum(splits) == N
            acc.reset(0)
            tot = np.zeros(4, dtype=np.int64)
            for n in splits:
                assert acc.accumulate(sc, cam, ds.env, ds.seed, n, count=True) == 0
                kb = c.counters()
                assert int(kb.path) == want_path
                tot += np.array(_ctr(kb), dtype=np.int64)
            st = acc.state()
            assert (st["first"], st["done"]) == (0, N)
            got = acc.resolve()
            assert np.array_equal(got, want), (name, N, splits, float(np.abs(got - want).max()))
            assert tuple(int(x) for x in tot) == want_ctr, (name, N, splits)
    finally:
        acc.close()


SPLITS = {100: [(100,), (37, 27, 36), (64, 36)], 16: [(16,), (1,) * 16]}
ROUTES = [("cfg2", (600, 300, 40, 24), 0, 2), ("mix0", None, 0, 2), ("cfg5", (250, 300, 40, 24), 0, 3), ("mix2", None, 300, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("N", [100, 16])
@pytest.mark.parametrize("name,rect,max_depth,path", ROUTES, ids=["lean_pipeline", "general_pipeline", "fused", "pixel_group_depth300"])
def test_split_invariance_bit_for_bit(name, rect, max_depth, path, N, ctx):
    _split_case(ctx, name, rect, max_depth, path, N, SPLITS[N])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [100, 16])
def test_split_invariance_with_the_pixel_group_kernel(N, built, monkeypatch):
    """ZR_KERNEL=0 (read when the context is created): every batch through the pixel-group route"""
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_KERNEL", "0")
    c = capi.Context(0)
    try:
        _split_case(c, "cfg2", (600, 300, 40, 24), 0, 0, N, SPLITS[N])
    finally:
        for key in [k for k in _scenes if k[0] == id(c)]:
            _scenes.pop(key).close()
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,rect", [("cfg2", (600, 300, 40, 24)), ("cfg5", (250, 300, 40, 24)), ("mix0", None)])
def test_every_prefix_is_an_image(name, rect, ctx):
    """after batches covering [0, k) the accumulator resolves to the k-spp frame exactly, for k = 1, 37, 64"""
    from raytracer_project_amd import capi
    ds = demo_scene(name)
    sc = _scene(ctx, name)
    cam = ds.camera.copy()
    reg = _region(rect)
    acc = capi.Accumulator(ctx, cam.image_width, cam.image_height, reg)
    try:
        done = 0
        for k in (1, 37, 64):
            acc.accumulate(sc, cam, ds.env, ds.seed, k - done)
            done = k
            got = acc.resolve()
            cam_k = cam.copy()
            cam_k.samples_per_pixel = k
            assert np.array_equal(got, sc.render(cam_k, ds.env, ds.seed, reg)), (name, k)
    finally:
        acc.close()


RANGE_TILES = [("cfg2", (), (600, 300, 16, 16)), ("cfg3", (200, 20, 256, 128), (900, 500, 24, 24)), ("mix0", (), (30, 20, 16, 16))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,args,rect", RANGE_TILES, ids=["cfg2", "cfg3_small", "mix0"])
def test_a_sample_range_matches_the_reference(name, args, rect, ctx):
    """reset(37), 27 samples: the mean of the oracle's samples 37 .. 63, at the suite's bar with no channel excluded"""
    from oracle import zr_oracle_py as zo
    from raytracer_project_amd import capi
    ds = demo_scene(name, args)
    sc = _scene(ctx, name, args)
    cam = ds.camera.copy()
    reg = _region(rect)
    acc = capi.Accumulator(ctx, cam.image_width, cam.image_height, reg)
    try:
        acc.reset(37)
        acc.accumulate(sc, cam, ds.env, ds.seed, 27)
        st = acc.state()
        assert (st["first"], st["done"], st["pixels"]) == (37, 27, rect[2] * rect[3])
        got = acc.resolve()[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]
    finally:
        acc.close()
    cam.samples_per_pixel = 64
    _, _, samples, _ = zo.OracleScene(ds.desc).render(cam, ds.env, ds.seed, reg, per_sample=True)
    want = samples[:, :, 37:64].mean(axis=2)
    err = rel_err(got, want, ABS_FLOOR)
    print(f"{name}: samples 37..63, max rel err {float(err.max()):.3e}")
    assert not (err > REL_TOL).any(), f"{name}: {int((err > REL_TOL).sum())} of {err.size} channels exceed {REL_TOL} (max {float(err.max()):.3e})"


@pytest.mark.gpu
def test_the_order_is_the_documented_one(ctx):
    """Single samples read back through reset(k); accumulate(1); resolve() — a lone sample resolves to itself — and summed by the model in
    the documented order reproduce the device's one-shot frame bit for bit."""
    from raytracer_project_amd import capi
    ds = demo_scene("cfg2")
    sc = _scene(ctx, "cfg2")
    cam = ds.camera.copy()
    rect, N = (604, 304, 8, 8), 70
    reg = _region(rect)
    cam.samples_per_pixel = N
    want = sc.render(cam, ds.env, ds.seed, reg)[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]
    acc = capi.Accumulator(ctx, cam.image_width, cam.image_height, reg)
    samples = np.zeros((rect[3], rect[2], N, 3))
    try:
        for k in range(N):
            acc.reset(k)
            acc.accumulate(sc, cam, ds.env, ds.seed, 1)
            samples[:, :, k] = acc.resolve()[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]
    finally:
        acc.close()
    assert np.array_equal(am.frame(samples), want)
    assert np.array_equal(am.frame(samples, splits=(37, 27, 6)), want)


@pytest.mark.gpu
def test_state_rules(ctx):
    from raytracer_project_amd import capi
    lib = ctx.lib
    ds = demo_scene("mix0")
    sc = _scene(ctx, "mix0")
    other = _scene(ctx, "mix2")
    cam = ds.camera.copy()
    h, w = cam.image_height, cam.image_width
    rect = (30, 20, 16, 16)
    reg = _region(rect)
    assert lib.zr_accum_create(ctx._c, 0, h, None) is None and lib.zr_last_error()
    bad = capi.Region(90, 60, 16, 16, 0, 0, 0, 0)
    assert lib.zr_accum_create(ctx._c, w, h, C.byref(bad)) is None and b"region" in lib.zr_last_error()
    acc = capi.Accumulator(ctx, w, h, reg)
    try:
        st = acc.state()
        assert (st["first"], st["done"], st["pixels"]) == (0, 0, 256) and st["device_bytes"] >= 256 * 1536
        out = np.zeros((h, w, 3))
        assert lib.zr_accum_resolve(acc._a, out.ctypes.data) == capi.ZR_E_STATE       # nothing accumulated yet
        assert lib.zr_accum_reset(acc._a, -1) == capi.ZR_E_INVALID

        def batch(scene, camera, seed, n, keep_going=None):
            kg = C.cast(C.byref(keep_going), C.c_void_p) if keep_going is not None else None
            return lib.zr_render_accumulate(ctx._c, scene._s, C.byref(camera), C.byref(ds.env), C.c_uint64(seed), acc._a, n, 0, kg)

        small = cam.copy()
        small.image_width = w // 2
        assert batch(sc, small, ds.seed, 4) == capi.ZR_E_INVALID      # another size
        assert batch(sc, cam, ds.seed, 0) == capi.ZR_E_INVALID        # no samples
        assert acc.state()["done"] == 0
        assert batch(sc, cam, ds.seed, 5) == 0
        moved = cam.copy()
        moved.vfov = cam.vfov + 1.0
        assert batch(sc, moved, ds.seed, 4) == capi.ZR_E_INVALID      # another camera
        assert batch(sc, cam, ds.seed + 1, 4) == capi.ZR_E_INVALID    # another seed
        assert batch(other, cam, ds.seed, 4) == capi.ZR_E_INVALID     # another scene
        spp_only = cam.copy()
        spp_only.samples_per_pixel = 999
        assert batch(sc, spp_only, ds.seed, 3) == 0                   # samples_per_pixel is ignored
        before, frame = acc.state(), acc.resolve()
        assert before["done"] == 8
        # a batch cancelled from the start is discarded whole
        stop = C.c_uint8(0)
        assert batch(sc, cam, ds.seed, 16, stop) == capi.ZR_E_CANCELLED
        assert acc.state() == before and np.array_equal(acc.resolve(), frame)
        # only the region's pixels are written
        canvas = np.full((h, w, 3), -1.0)
        acc.resolve(canvas)
        inside = np.zeros((h, w), bool)
        inside[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = True
        assert (canvas[~inside] == -1.0).all() and np.array_equal(canvas[inside], frame[inside])
        cam8 = cam.copy()
        cam8.samples_per_pixel = 8
        assert np.array_equal(frame, sc.render(cam8, ds.env, ds.seed, reg))
        # reset starts a new frame: another seed is welcome again
        acc.reset(0)
        assert batch(sc, cam, ds.seed + 1, 2) == 0
    finally:
        acc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,rect,path", [("cfg2", (600, 300, 40, 24), 2), ("cfg5", (250, 300, 40, 24), 3)], ids=["pipeline", "fused"])
def test_zr_render_in_forced_batches(name, rect, path, ctx, monkeypatch):
    """ZR_STREAM_BATCH_UNITS below the frame's work units: zr_render renders the frame in sample batches through the same route — same image
    bit for bit, the frame's counters, and (the pipeline) more rounds than one run takes, since every batch drains on its own."""
    ds = demo_scene(name)
    sc = _scene(ctx, name)
    cam = ds.camera.copy()
    cam.samples_per_pixel = 100
    reg = _region(rect)
    want = sc.render(cam, ds.env, ds.seed, reg, count=True)
    k0 = ctx.counters()
    assert int(k0.path) == path
    monkeypatch.setenv("ZR_STREAM_BATCH_UNITS", str(rect[2] * rect[3] * 40))   # 40 samples per pixel per run: 100 spp in 3 batches
    got = sc.render(cam, ds.env, ds.seed, reg, count=True)
    k1 = ctx.counters()
    assert np.array_equal(got, want)
    assert _ctr(k1) == _ctr(k0) and int(k1.path) == path
    assert int(k1.rounds) >= 3 and int(k1.rounds) > int(k0.rounds)
    # a polled render in batches: finishes, reports every row, same image
    out = np.full(want.shape, -1.0)
    flag = C.c_uint8(1); rows = C.c_int(-5)
    rc = ctx.lib.zr_render(ctx._c, sc._s, C.byref(cam), C.byref(ds.env), C.c_uint64(ds.seed), C.byref(reg), 0, out.ctypes.data,
                           C.cast(C.byref(flag), C.c_void_p), C.cast(C.byref(rows), C.c_void_p))
    assert rc == 0 and rows.value == cam.image_height
    inside = np.zeros(want.shape[:2], bool)
    inside[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = True
    assert np.array_equal(out[inside], want[inside]) and (out[~inside] == -1.0).all()
    monkeypatch.delenv("ZR_STREAM_BATCH_UNITS")
    assert np.array_equal(sc.render(cam, ds.env, ds.seed, reg), want)


@pytest.mark.gpu
def test_dropin_samples_per_pass(ctx):
    """camera::samples_per_pass = 8 at 20 spp: passes of 8, 8 and 4 samples, the one-shot frame bit for bit, current_samples_count = 20;
    samples_per_pass = 0 is the one-shot render and leaves current_samples_count alone (-7: what the helper put there)."""
    ds = demo_scene("mix0")
    one_shot, _ = ds.render_dropin(spp=20)
    frame, count, updates = ds.render_dropin_progressive(8, spp=20)
    assert np.array_equal(frame, one_shot)
    assert (count, updates) == (20, 3)
    frame0, count0, updates0 = ds.render_dropin_progressive(0, spp=20)
    assert np.array_equal(frame0, one_shot)
    assert (count0, updates0) == (-7, 0)


@pytest.mark.gpu
def test_dropin_cancelled_before_the_first_pass(ctx):
    """render_flag clear going in: zr_render_accumulate refuses the first batch before it begins, so the frame stays zero, the route has reset
    current_samples_count from -7 to 0 and no pass reached render_accumulator.  The leased context stays usable: the same render with the flag set
    gives afterwards, byte for byte, what it gave before."""
    ds = demo_scene("mix0")
    size = dict(width=96, height=64, spp=20)
    before = ds.render_dropin_progressive(8, **size)
    assert before[1:] == (20, 3)
    frame, count, updates = ds.render_dropin_progressive(8, flag=False, **size)
    assert frame.shape == (64, 96, 3) and not frame.any()
    assert (count, updates) == (0, 0)
    after = ds.render_dropin_progressive(8, flag=True, **size)
    assert after[0].tobytes() == before[0].tobytes() and after[1:] == before[1:]
