"""The pipeline's round loop with lagged polls (zr_stream.hip stream_render, zr_round_polls.h): a frame nobody polls keeps ZR_STREAM_POLL_LAG + 1 rounds in flight
and waits for the oldest round's poll only; ZR_STREAM_POLL_LAG=0 is the loop that drains every stream at each poll, which polled frames (keep_going, rows_done)
keep whatever the lag.  How the host learns what the device did may not change what the device does: for LAG 1 and 2 the timed frame is the LAG 0 frame bit for
bit, the counting render's books and its round count are equal, and the launch log holds the launches of the rounds up to the one that emptied the pools, by one
rule in every mode (Context.round_loop() says when the survivors moved to the drain pool and on how many sub-pools the frame began)."""
import ctypes as C
import re
import threading

import numpy as np
import pytest

import frame_edge_worlds as fw
from conftest import demo_scene

pytestmark = pytest.mark.gpu

LAGS = (0, 1, 2)
BOOKS = ("primary_samples", "segments", "hits", "rng_draws", "escaped", "shade_lanes", "rounds")   # samples, segments, hits, draws, escaped, shade_lanes, rounds


def _expected_launches(rounds, drain_round, pools):
    """EXTEND launches of a frame of `rounds` rounds: the start-up launches one round on all sub-pools but the last (that is round 1 when there are several),
    every loop round one launch per sub-pool, and one only after the survivors moved to the drain pool (behind loop round `drain_round`; 0: never)"""
    start = 1 if pools > 1 else 0
    loop_rounds = rounds - start
    n = pools - 1
    for r in range(1, loop_rounds + 1):
        n += pools if (drain_round == 0 or r <= drain_round) else 1
    return n


def _one_mode(ctx, sc, cam, env, seed, lag, monkeypatch):
    """timed frame, its (rounds, drain_round, sub_pools, launches logged), the counting render's books and its round-loop figures, with ZR_STREAM_POLL_LAG=lag"""
    monkeypatch.setenv("ZR_STREAM_POLL_LAG", str(lag))
    try:
        ctx.kernel_times_ms(1 << 16)   # (drains the launch log)
        frame = sc.render(cam, env, seed, None)
        k = ctx.counters()
        assert k.path == 2
        drain_round, pools = ctx.round_loop()
        timed = (int(k.rounds), drain_round, pools, len(ctx.kernel_times_ms(1 << 16)))
        counted = sc.render(cam, env, seed, None, count=True)
        k = ctx.counters()
        books = tuple(int(getattr(k, f)) for f in BOOKS)
        cdrain, cpools = ctx.round_loop()
        clog = len(ctx.kernel_times_ms(1 << 16))
        return frame, timed, counted, books, (int(k.rounds), cdrain, cpools, clog)
    finally:
        monkeypatch.delenv("ZR_STREAM_POLL_LAG")


def _all_modes(ctx, sc, cam, env, seed, monkeypatch, what):
    got = {lag: _one_mode(ctx, sc, cam, env, seed, lag, monkeypatch) for lag in LAGS}
    base = got[0]
    for lag in LAGS:
        frame, timed, counted, books, cfig = got[lag]
        print(f"{what}, lag {lag}: timed (rounds, drain round, sub-pools, launches) {timed}, counting {cfig}, books {dict(zip(BOOKS, books))}")
        assert np.array_equal(frame, base[0]), f"{what}: the timed frame with lag {lag} differs from lag 0"
        assert np.array_equal(counted, base[2]), f"{what}: the counting frame with lag {lag} differs from lag 0"
        assert books == base[3], f"{what}, lag {lag}: {dict(zip(BOOKS, books))} against {dict(zip(BOOKS, base[3]))}"
        assert timed[0] == base[1][0], f"{what}: {timed[0]} rounds with lag {lag}, {base[1][0]} with lag 0"
        for rounds, drain_round, pools, launches in (timed, cfig):
            if rounds == 0:
                assert launches == 0, f"{what}, lag {lag}: {launches} launches logged for a frame without a round"
            else:
                assert launches == _expected_launches(rounds, drain_round, pools), (what, lag, rounds, drain_round, pools, launches)
    return got


# ---- cfg3 with the reduced mesh: two lean sub-pools ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cfg3_ds(built):
    return demo_scene("cfg3", (200, 20, 256, 128))


def _cfg3_camera(ds, spp=16):
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel = 480, 270, spp
    return cam


@pytest.mark.parametrize("pools,prepass", [(None, True), (1, True), (3, True), (None, False)], ids=["auto", "pools1", "pools3", "no-prepass"])
def test_cfg3_lagged_is_the_draining_loop(pools, prepass, cfg3_ds, monkeypatch):
    """480 x 270 at 16 spp: 259 200 slots for the counting render, two lean sub-pools of at least 64 Ki by default; again on one and on three sub-pools
    (ZR_STREAM_POOLS is read when the context is made) and without the sky pre-pass"""
    from raytracer_project_amd import capi
    ds = cfg3_ds
    if pools is not None:
        monkeypatch.setenv("ZR_STREAM_POOLS", str(pools))
    if not prepass:
        monkeypatch.setenv("ZR_SKY_PREPASS", "0")
    ctx = capi.Context(0)
    sc = capi.Scene(ctx, ds.desc)
    try:
        assert sc.kernels()["shade_lean"] == 1
        got = _all_modes(ctx, sc, _cfg3_camera(ds), ds.env, ds.seed, monkeypatch, f"cfg3 pools {pools} prepass {prepass}")
    finally:
        sc.close(); ctx.close()
    for lag in LAGS:
        assert got[lag][4][2] == (2 if pools is None else pools), f"the counting render began on {got[lag][4][2]} sub-pools"
        assert float(got[lag][0].sum()) > 0


# ---- frames smaller than a block of slots, and a frame without a round ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", [pytest.param(c, id=c.name) for c in (fw.shape_cell(1, 1), fw.shape_cell(7, 1), fw.all_sky_cell())])
def test_tiny_frames(cell, built, monkeypatch):
    """1 x 1 and 7 x 1 at 3 spp (3 and 21 work units: less than one block of 256 slots) through the pipeline, and the all-sky 1 x 7 cell, whose timed frame
    has nothing to walk (no round at all) while its counting render ends in its first rounds"""
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_FUSED", "0")
    ctx = capi.Context(0)
    sc = capi.Scene(ctx, cell.world.scene_desc)
    try:
        got = _all_modes(ctx, sc, cell.cam, fw.solid_env(), cell.seed, monkeypatch, cell.name)
        if cell.name.endswith("_sky"):
            for lag in LAGS:
                assert got[lag][1][0] == 0 and got[lag][4][0] >= 1, "the all-sky cell's timed frame must not reach the round loop, its counting render must"
    finally:
        sc.close(); ctx.close()


# ---- deep paths: the drain pool ----------------------------------------------------------------------------------------------------------------------------

def test_deep_paths_reach_the_drain_pool(built, monkeypatch):
    """cfg5 through the pipeline at 64 x 64, 16 spp, depth 50: the frame lives on its longest paths, and in every mode the survivors are moved to the drain pool
    and rounds are run on it"""
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_FUSED", "0")
    ds = demo_scene("cfg5")
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth = 64, 64, 16, 50
    ctx = capi.Context(0)
    sc = capi.Scene(ctx, ds.desc)
    try:
        got = _all_modes(ctx, sc, cam, ds.env, ds.seed, monkeypatch, "cfg5 depth 50")
    finally:
        sc.close(); ctx.close()
    for lag in LAGS:
        for rounds, drain_round, pools, _ in (got[lag][1], got[lag][4]):
            start = 1 if pools > 1 else 0
            assert 0 < drain_round < rounds - start, f"lag {lag}: {rounds} rounds, survivors moved after loop round {drain_round}: no round ran on the drain pool"


# ---- polled frames keep the draining loop --------------------------------------------------------------------------------------------------------------------

def _polled(ctx, sc, cam, ds, flag, rows, out):
    return ctx.lib.zr_render(ctx._c, sc._s, C.byref(cam), C.byref(ds.env), C.c_uint64(ds.seed), None, 0, out.ctypes.data, C.cast(C.byref(flag), C.c_void_p),
                             C.cast(C.byref(rows), C.c_void_p) if rows is not None else None)


def test_polled_frame_reaches_the_drain_pool(built, monkeypatch):
    """the world of test_deep_paths_reach_the_drain_pool with rows_done set and keep_going left at 1: the cadenced loop under a progress sink (runs of two rounds)
    decides the drain switch from its polls, the frame is the plain one bit for bit and counts the rounds of the plain frame with ZR_STREAM_POLL_LAG=0"""
    from raytracer_project_amd import capi
    monkeypatch.setenv("ZR_FUSED", "0")
    ds = demo_scene("cfg5")
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth = 64, 64, 16, 50
    h, w = cam.image_height, cam.image_width
    ctx = capi.Context(0)
    sc = capi.Scene(ctx, ds.desc)
    try:
        monkeypatch.setenv("ZR_STREAM_POLL_LAG", "0")
        plain = sc.render(cam, ds.env, ds.seed, None)
        plain_rounds = int(ctx.counters().rounds)
        monkeypatch.delenv("ZR_STREAM_POLL_LAG")
        out = np.zeros((h, w, 3)); flag = C.c_uint8(1); rows = C.c_int(0)
        assert _polled(ctx, sc, cam, ds, flag, rows, out) == 0 and rows.value == h
        rounds = int(ctx.counters().rounds)
        drain_round, pools = ctx.round_loop()
        print(f"polled cfg5 depth 50: {rounds} rounds on {pools} sub-pool(s), survivors moved after loop round {drain_round}; the plain frame takes {plain_rounds}")
        assert np.array_equal(out, plain)
        assert 0 < drain_round < rounds - (1 if pools > 1 else 0), "no round of the polled frame ran on the drain pool"
        assert rounds == plain_rounds
    finally:
        sc.close(); ctx.close()


@pytest.mark.parametrize("lag", [1, 2])
def test_polled_frames(lag, cfg3_ds, monkeypatch):
    """a frame with rows_done (every row reported, the frame unchanged) and one whose keep_going another thread clears as soon as rows_done moves (cancelled,
    short of the whole frame's rounds, only finished work in the image), whatever the lag says: polled frames do not take the lagged loop"""
    from raytracer_project_amd import capi
    ds = cfg3_ds
    cam = _cfg3_camera(ds, 64)
    h, w = cam.image_height, cam.image_width
    monkeypatch.setenv("ZR_STREAM_POLL_LAG", str(lag))
    ctx = capi.Context(0)
    sc = capi.Scene(ctx, ds.desc)
    try:
        plain = sc.render(cam, ds.env, ds.seed, None)
        full_rounds = int(ctx.counters().rounds)
        out = np.zeros((h, w, 3)); flag = C.c_uint8(1); rows = C.c_int(0)
        assert _polled(ctx, sc, cam, ds, flag, rows, out) == 0 and rows.value == h
        assert np.array_equal(out, plain)
        assert int(ctx.counters().rounds) == full_rounds, "a polled frame and a plain one count the same rounds"
        out = np.zeros((h, w, 3)); flag = C.c_uint8(1); rows = C.c_int(0)
        done = threading.Event()

        def watch():
            while not done.is_set():
                if rows.value > 0:
                    flag.value = 0
                    return
        t = threading.Thread(target=watch); t.start()
        try:
            rc = _polled(ctx, sc, cam, ds, flag, rows, out)
        finally:
            done.set(); t.join()
        msg = ctx.lib.zr_last_error().decode()
        print(f"lag {lag}: rc {rc}, rows_done {rows.value} of {h}, {msg!r}; the whole frame takes {full_rounds} rounds")
        assert rc == -4 and "cancel" in msg.lower()
        cancelled_after = int(re.search(r"after (\d+) rounds", msg).group(1))
        assert 0 < cancelled_after < full_rounds and 0 < rows.value < h
        assert np.isfinite(out).all() and (out >= 0).all() and out.sum() < plain.sum(), "a cancelled frame holds finished work only"
        assert np.array_equal(sc.render(cam, ds.env, ds.seed, None), plain), "the context is usable after a cancelled frame"
    finally:
        sc.close(); ctx.close()
