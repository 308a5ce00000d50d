"""The measurements behind DESIGN §20 (direct light sampling) and profiles/direct_light.txt.

  python scripts/dev/direct_sweep.py [--out FILE] [--part direct|env|all]

cfg5 at 300 x 300 and mix0 at 384 x 256 (the denoiser and robust sweeps' scenes and sizes); truth is the 4096-spp frame of zr_render — the plain
integrator, from code that is not under test.  Per scene:

  MSE       at 64 / 128 / 256 spp of a direct accumulator and of a plain one (one seed, not the truth's), and F = MSE(plain) / MSE(direct)
  time      wall time per sample of a 256-spp batch (zr_render_accumulate returns when the batch is done; best of three): the direct kernel, the plain pixel-group route
            (ZR_KERNEL=0) and the route zr_render takes (fused kernel or pipeline)
  E         equal-time efficiency = F x time(plain route) / time(direct), against either route
  robust    the Gini-trimmed resolve at the default strength on the direct and on the plain accumulator at 64 spp: F against that accumulator's own plain resolve,
            and the energy kept
  filters   zr_denoise_guided and zr_denoise_nlm at their defaults at 64 spp on both accumulators: F against the plain accumulator's plain resolve

--part env: the measurements behind DESIGN §21 (environment-map sampling) and profiles/env_light.txt, on two map-lit worlds: cfg3 at 240 x 135 under its own
4096 x 2048 map, and mix0 at 384 x 256 with its sun swapped for the 64 x 32 map of tests/golden.  Per world: how peaked the map is, the table's build time, MSE
against zr_render at 4096 spp of a plain, a direct and a direct + environment accumulator at 64 / 128 / 256 spp, and the time per sample of a 256-spp batch
with the environment off and on.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from raytracer_project_amd import capi  # noqa: E402

SCENES = {"cfg5": (300, 300), "mix0": (384, 256)}
COUNTS = (64, 128, 256)


def mse(f, t):
    return float(((f - t) ** 2).mean())


def timed_batch(ctx, sc, cam, env, seed, n, direct, environment=False):
    """wall time of one n-sample batch on a fresh accumulator, after a warm-up batch (the batch is synchronous: zr_render_accumulate returns when it is done)"""
    acc = capi.Accumulator(ctx, cam.image_width, cam.image_height)
    if direct:
        acc.set_direct()
    if environment:
        acc.set_direct_env()
    acc.accumulate(sc, cam, env, seed, 64)
    best = 1e30
    for _ in range(3):
        acc.reset()
        t0 = time.perf_counter()
        acc.accumulate(sc, cam, env, seed, n)
        best = min(best, time.perf_counter() - t0)
    acc.close()
    return best


def with_map(desc, texels):
    """a copy of a scene description with one more F32 image texture -> (description, texture id, what must stay alive)"""
    import ctypes as C
    d = type(desc).from_buffer_copy(desc)
    old = bytes((C.c_ubyte * desc.texel_bytes).from_address(desc.texels)) if desc.texel_bytes else b""
    blob = old + b"\0" * (-len(old) % 4)
    offset = len(blob)
    blob += np.ascontiguousarray(texels, dtype=np.float32).tobytes()
    texs = (capi.Texture * (desc.n_textures + 1))()
    if desc.n_textures:
        C.memmove(texs, desc.textures, desc.n_textures * C.sizeof(capi.Texture))
    texs[desc.n_textures] = capi.Texture(3, 0, 0, texels.shape[1], texels.shape[0], 0, offset, 0.0, (C.c_double * 3)(0, 0, 0))
    buf = (C.c_ubyte * len(blob)).from_buffer_copy(blob)
    d.textures, d.n_textures = C.cast(texs, C.c_void_p), desc.n_textures + 1
    d.texels, d.texel_bytes = C.cast(buf, C.c_void_p), len(blob)
    return d, desc.n_textures, (texs, buf)


def env_part(ctx, say):
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    golden = np.load(os.path.join(root, "tests", "golden", "texels_hdr_64x32.npz"))["texels"].reshape(32, 64, 3)
    for name, (w, h) in (("cfg3", (240, 135)), ("mix0", (384, 256))):
        ds = capi.DemoScene(name)
        cam = ds.camera.copy()
        cam.image_width, cam.image_height = w, h
        desc, env, keep = ds.desc, ds.env, None
        if name == "mix0":
            desc, tex, keep = with_map(ds.desc, golden)
            env = capi.Env()
            env.mode, env.hdr_texture, env.intensity = 1, tex, 1.0
            env.hdri_rotation, env.hdri_tilt, env.hdri_roll = 0.7, -0.3, 1.9
        sc = capi.Scene(ctx, desc)
        tab = sc.env_light(env)
        wt = np.diff(np.concatenate([np.zeros((tab["height"], 1)), tab["cdf"]], axis=1), axis=1).ravel()
        wt = np.sort(wt)[::-1] / tab["total"]
        top = {f: float(wt[:max(1, int(len(wt) * f))].sum()) for f in (0.001, 0.01, 0.1)}
        say(f"== {name} {w} x {h}: map {tab['width']} x {tab['height']}, {tab['weighted']} texels with weight, T = {tab['total']:.6g}, table built in "
            f"{tab['build_ms']:.3f} ms (device), {len(sc.lights())} emitter slots")
        say(f"{name} peakedness | share of T in the heaviest 0.1 % / 1 % / 10 % of the texels: {top[0.001]:.4f} / {top[0.01]:.4f} / {top[0.1]:.4f} "
            f"(a flat map: 0.001 / 0.01 / 0.1 by solid angle)")
        tc = cam.copy(); tc.samples_per_pixel = 4096
        truth = sc.render(tc, env, ds.seed, None)
        accs = {}
        for label in ("plain", "direct", "direct+env"):
            acc = capi.Accumulator(ctx, w, h)
            if label != "plain":
                acc.set_direct()
            if label == "direct+env":
                acc.set_direct_env()
            accs[label] = acc
        for k in COUNTS:
            res = {}
            for label, acc in accs.items():
                acc.accumulate(sc, cam, env, ds.seed + 1, k - acc.state()["done"])
                res[label] = mse(acc.resolve(), truth)
            say(f"{name} {k:4d} spp | MSE plain {res['plain']:.5e}  direct {res['direct']:.5e}  direct+env {res['direct+env']:.5e}  "
                f"F(direct) = {res['plain'] / res['direct']:.3f}  F(direct+env) = {res['plain'] / res['direct+env']:.3f}")
        t_off = timed_batch(ctx, sc, cam, env, ds.seed, 256, True)
        t_on = timed_batch(ctx, sc, cam, env, ds.seed, 256, True, True)
        t_route = timed_batch(ctx, sc, cam, env, ds.seed, 256, False)
        per = 1e9 / (w * h * 256)
        say(f"{name}  256-spp batch, wall | direct {t_off * 1e3:.1f} ms ({t_off * per:.2f} ns/sample)  direct+env {t_on * 1e3:.1f} ms ({t_on * per:.2f})  "
            f"zr_render's route {t_route * 1e3:.1f} ms ({t_route * per:.2f})")
        say()
        for acc in accs.values():
            acc.close()
        sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", default="all", choices=("direct", "env", "all"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    ctx = capi.Context(0)
    if args.part in ("env", "all"):
        env_part(ctx, say)
    for name, (w, h) in (SCENES.items() if args.part in ("direct", "all") else ()):
        ds = capi.DemoScene(name)
        cam = ds.camera.copy()
        cam.image_width, cam.image_height = w, h
        sc = capi.Scene(ctx, ds.desc)
        tc = cam.copy(); tc.samples_per_pixel = 4096
        truth = sc.render(tc, ds.env, ds.seed, None)
        tab = sc.lights()
        say(f"== {name} {w} x {h}: {len(tab)} light slots on {len(set(zip(tab['kind'], tab['index'])))} objects, environment mode {ds.env.mode}")
        a, n, _ = sc.render_aov(cam, ds.seed, 1.0)
        accs = {}
        for label, direct in (("plain", False), ("direct", True)):
            acc = capi.Accumulator(ctx, w, h)
            if direct:
                acc.set_direct()
            accs[label] = acc
        res = {}
        for k in COUNTS:
            for label, acc in accs.items():
                acc.accumulate(sc, cam, ds.env, ds.seed + 1, k - acc.state()["done"])
                res[label, k] = mse(acc.resolve(), truth)
            say(f"{name} {k:4d} spp | MSE plain {res['plain', k]:.5e}  direct {res['direct', k]:.5e}  F = {res['plain', k] / res['direct', k]:.3f}")
            if k == 64:
                base = res["plain", 64]
                for label, acc in accs.items():
                    plain = acc.resolve()
                    col, var, trim = acc.resolve_robust(capi.RobustParams.defaults())
                    say(f"{name}   64 spp | {label:6s} accumulator, robust resolve (default): F = {mse(plain, truth) / mse(col, truth):.3f} against its own plain resolve, "
                        f"energy kept {col.sum() / plain.sum():.3f}, mean trim {trim.mean():.2f}")
                    ha, hb = acc.halves()
                    pv = acc.variance()
                    g = ctx.denoise_guided(capi.DenoiseGuidedParams.defaults(), plain, pv, a, n)[0]
                    m = ctx.denoise_nlm(capi.DenoiseNlmParams.defaults(), ha, hb, pv, a, n)[0]
                    say(f"{name}   64 spp | {label:6s} accumulator, filters against the plain accumulator's resolve: guided F = {base / mse(g, truth):.3f}, "
                        f"nlm F = {base / mse(m, truth):.3f}")
        t_direct = timed_batch(ctx, sc, cam, ds.env, ds.seed, 256, True)
        t_route = timed_batch(ctx, sc, cam, ds.env, ds.seed, 256, False)
        os.environ["ZR_KERNEL"] = "0"   # the plain pixel-group route: a context reads the variable when it is made
        ctx0 = capi.Context(0)
        del os.environ["ZR_KERNEL"]
        sc0 = capi.Scene(ctx0, ds.desc)
        t_group = timed_batch(ctx0, sc0, cam, ds.env, ds.seed, 256, False)
        path0 = ctx0.counters().path
        sc0.close(); ctx0.close()
        per = 1e9 / (w * h * 256)
        f256 = res["plain", 256] / res["direct", 256]
        say(f"{name}  256-spp batch, wall | direct {t_direct * 1e3:.1f} ms ({t_direct * per:.2f} ns/sample)  pixel-group route (path {path0}) {t_group * 1e3:.1f} ms "
            f"({t_group * per:.2f})  zr_render's route {t_route * 1e3:.1f} ms ({t_route * per:.2f})")
        say(f"{name}  equal-time efficiency at 256 spp | against the pixel-group route {f256 * t_group / t_direct:.3f}, against zr_render's route {f256 * t_route / t_direct:.3f}")
        say()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
