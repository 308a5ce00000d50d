"""The measurements behind zr_denoise_guided's defaults and DESIGN §13.

  python scripts/dev/denoise_guided_sweep.py [--out FILE]                 the quality sweep
  python scripts/dev/denoise_guided_sweep.py --timing 1920x1080 [--out FILE]   wall clock of the two routes (run it under rocprofv3 --kernel-trace --stats
                                                                               for the per-kernel times)

The sweep: cfg5 at 300 x 300 and mix0 at 384 x 256 (tests/test_denoise.py's quality scenes and sizes), each rendered at 64 spp into an accumulator;
truth is 4096 spp from zr_render (its own variance is 1/64 of the input's).  For sigma_variance in {1, 1.5, 2, 3, 4} x iterations in {4, 5}, epsilon 1e-8,
demodulation off and on: F = MSE(noisy) / MSE(filtered), and F of zr_denoise with its defaults on the same inputs.  The same once on an adaptive cfg5
frame (min 64, step 64, max 256, threshold = the median of the 64-spp error map).  The defaults are the setting with the best worse-of-two-scenes F.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from raytracer_project_amd import capi  # noqa: E402

SCENES = {"cfg5": (300, 300), "mix0": (384, 256)}
SIGMAS, ITERATIONS = (1.0, 1.5, 2.0, 3.0, 4.0), (4, 5)


def inputs(ctx, name):
    """{case: (noisy, variance, albedo, normal, truth)} for the scene's 64-spp frame and, on cfg5, its adaptive frame"""
    ds = capi.DemoScene(name)
    cam = ds.camera.copy()
    cam.image_width, cam.image_height = SCENES[name]
    cam.samples_per_pixel = 64
    sc = capi.Scene(ctx, ds.desc)
    acc = capi.Accumulator(ctx, cam.image_width, cam.image_height)
    acc.accumulate(sc, cam, ds.env, ds.seed, 64)
    a, n, _ = sc.render_aov(cam, ds.seed, 1.0)
    tc = cam.copy(); tc.samples_per_pixel = 4096
    truth = sc.render(tc, ds.env, ds.seed, None)
    cases = {name: (acc.resolve(), acc.variance(), a, n, truth)}
    if name == "cfg5":
        thr = float(np.median(acc.error()))
        ad = capi.Accumulator(ctx, cam.image_width, cam.image_height)
        _, st = ad.render_adaptive(sc, cam, ds.env, ds.seed, capi.AdaptiveParams.defaults(min_samples=64, max_samples=256, step_samples=64, threshold=thr))
        cases["cfg5-adaptive"] = (ad.resolve(), ad.variance(), a, n, truth)
        print(f"# cfg5-adaptive: threshold {thr:.5f}, {st.as_dict()}, mean count {ad.sample_counts().mean():.1f}")
        ad.close()
    acc.close(); sc.close()
    return cases


def sweep(out):
    ctx = capi.Context(0)
    cases = {}
    for name in SCENES:
        cases.update(inputs(ctx, name))
    names = list(cases)
    mse = lambda f, t: float(((f - t) ** 2).mean())
    lines = ["denoise_guided_sweep.py: F = MSE(noisy) / MSE(filtered) against 4096 spp; inputs: 64-spp accumulators (cfg5 300x300, mix0 384x256), "
             "cfg5-adaptive: min 64, step 64, max 256, threshold = median of the 64-spp error map; epsilon 1e-8",
             "setting | " + " | ".join(names) + " | worse of cfg5, mix0"]
    base = {k: mse(v[0], v[4]) for k, v in cases.items()}
    lines.append("MSE(noisy) | " + " | ".join(f"{base[k]:.4e}" for k in names) + " |")
    row = {k: base[k] / mse(ctx.denoise(capi.DenoiseParams.defaults(), v[0], v[2], v[3]), v[4]) for k, v in cases.items()}
    lines.append("zr_denoise defaults | " + " | ".join(f"{row[k]:.3f}" for k in names) + f" | {min(row['cfg5'], row['mix0']):.3f}")
    best = None
    for demod in (0, 1):
        for it in ITERATIONS:
            for sv in SIGMAS:
                p = capi.DenoiseGuidedParams.defaults(iterations=it, demodulate_albedo=demod, sigma_variance=sv, epsilon=1e-8)
                row = {k: base[k] / mse(ctx.denoise_guided(p, v[0], v[1], v[2], v[3])[0], v[4]) for k, v in cases.items()}
                worse = min(row["cfg5"], row["mix0"])
                lines.append(f"guided sigma_v {sv} iterations {it} demodulate {demod} | " + " | ".join(f"{row[k]:.3f}" for k in names) + f" | {worse:.3f}")
                if best is None or worse > best[0]:
                    best = (worse, lines[-1])
    lines.append("best worse-of-two: " + best[1])
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        open(out, "w").write(text)


def timing(size, out, repeats=7):
    """wall clock, median of `repeats` after a warm-up: zr_accum_denoise against resolve + variance + zr_denoise_guided with host pointers, and zr_denoise"""
    w, h = (int(x) for x in size.split("x"))
    ctx = capi.Context(0)
    ds = capi.DemoScene("cfg5")
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel = w, h, 64
    sc = capi.Scene(ctx, ds.desc)
    acc = capi.Accumulator(ctx, w, h)
    acc.accumulate(sc, cam, ds.env, ds.seed, 64)
    a, n, _ = sc.render_aov(cam, ds.seed, 1.0)
    p = capi.DenoiseGuidedParams.defaults()
    frame = np.zeros((h, w, 3)); var = np.zeros((h, w, 3)); o = np.zeros((h, w, 3)); ov = np.zeros((h, w, 3))

    def host_route():
        acc.resolve(frame); acc.variance(var)
        ctx.denoise_guided(p, frame, var, a, n, out=o, out_variance=ov)

    def med(f):
        f()
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
        return f"{statistics.median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f})"

    lines = [f"denoise_guided_sweep.py --timing {size}: cfg5, 64-spp accumulator, defaults, wall clock, median of {repeats} after a warm-up",
             "zr_accum_denoise | " + med(lambda: acc.denoise(p, a, n)),
             "zr_accum_resolve + zr_accum_variance + zr_denoise_guided (host pointers) | " + med(host_route),
             "zr_denoise_guided alone (host pointers) | " + med(lambda: ctx.denoise_guided(p, frame, var, a, n, out=o, out_variance=ov)),
             "zr_denoise (host pointers) | " + med(lambda: ctx.denoise(capi.DenoiseParams.defaults(), frame, a, n, out=o))]
    acc.close(); sc.close(); ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        open(out, "w").write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--timing", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.timing:
        timing(args.timing, args.out)
    else:
        sweep(args.out)
