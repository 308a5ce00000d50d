"""The measurements behind ZR_ROBUST_DEFAULT_STRENGTH and DESIGN §19.

  python scripts/dev/robust_sweep.py [--out FILE]                     the quality sweep
  python scripts/dev/robust_sweep.py --timing 1920x1080 [--out FILE]  accum_resolve_robust against accum_variance on one accumulator (zr_get_kernel_times)

cfg5 at 300 x 300 and mix0 at 384 x 256 (the denoiser sweeps' scenes and sizes), each rendered into one accumulator that is read at 64, 128 and 256 spp;
truth is the 4096-spp frame of zr_render — the plain mean, from code that is not under test.  Per scene and sample count, for ZR_ROBUST_GINI at strength
0.25 ... 4 and ZR_ROBUST_FIXED at t = 4, 8, 16, 31:

  F    = MSE(plain resolve) / MSE(robust resolve)                                   above 1: the robust frame is closer to the truth
  Frel = the same ratio of relative MSE, mean of (f - t)^2 / (t^2 + 1e-4), with the brightest 0.1 % of the truth's pixels (by channel sum) left out
  E    = sum(robust frame) / sum(plain frame)                                       the energy a trimmed mean loses on skewed pixels

The default is the Gini strength with the best worst F over the six cells (two scenes x three counts); if no strength has that F above 1 it stays 1.0.
Then, at 64 spp, zr_denoise_guided and zr_denoise_nlm with their defaults, fed the plain colour and variance and fed the robust ones (the non-local-means
filter reads the accumulator's two half images either way: only its variance changes): F against MSE(plain resolve).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from raytracer_project_amd import capi  # noqa: E402

SCENES = {"cfg5": (300, 300), "mix0": (384, 256)}
COUNTS = (64, 128, 256)
STRENGTHS = (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0)
TRIMS = (4, 8, 16, 31)


def mse(f, t):
    return float(((f - t) ** 2).mean())


def rel_mse(f, t, keep):
    return float((((f - t) ** 2) / (t * t + 1e-4))[keep].mean())


def sweep(out):
    ctx = capi.Context(0)
    settings = [("plain (strength 0)", capi.RobustParams.defaults(strength=0.0))]
    settings += [(f"GINI strength {s:g}", capi.RobustParams.defaults(strength=s)) for s in STRENGTHS]
    settings += [(f"FIXED t {t}", capi.RobustParams.defaults(mode=capi.ROBUST_FIXED, trim=t)) for t in TRIMS]
    cells = [(name, k) for name in SCENES for k in COUNTS]
    table = {label: {} for label, _ in settings}
    base, mean_trim, denoise_rows = {}, {}, []
    for name, (w, h) in SCENES.items():
        ds = capi.DemoScene(name)
        cam = ds.camera.copy()
        cam.image_width, cam.image_height = w, h
        sc = capi.Scene(ctx, ds.desc)
        tc = cam.copy(); tc.samples_per_pixel = 4096
        truth = sc.render(tc, ds.env, ds.seed, None)
        lum = truth.sum(axis=2)
        keep = lum <= np.quantile(lum, 0.999)
        a, n, _ = sc.render_aov(cam, ds.seed, 1.0)
        acc = capi.Accumulator(ctx, w, h)
        for k in COUNTS:
            acc.accumulate(sc, cam, ds.env, ds.seed, k - acc.state()["done"])
            plain = acc.resolve()
            assert plain.tobytes() == acc.resolve_robust(capi.RobustParams.defaults(mode=capi.ROBUST_FIXED, trim=0))[0].tobytes()
            base[name, k] = (mse(plain, truth), rel_mse(plain, truth, keep))
            for label, p in settings:
                col, var, t = acc.resolve_robust(p)
                table[label][name, k] = (base[name, k][0] / mse(col, truth), base[name, k][1] / rel_mse(col, truth, keep), col.sum() / plain.sum())
                mean_trim[label, name, k] = float(t.mean())
            if k == 64:   # the denoisers on the plain and on the robust inputs
                ha, hb = acc.halves()
                pv = acc.variance()
                for label, p in [s for s in settings if s[0] in ("GINI strength 0.5", "GINI strength 1", "GINI strength 2")]:
                    rc, rv, _ = acc.resolve_robust(p)
                    g_plain = ctx.denoise_guided(capi.DenoiseGuidedParams.defaults(), plain, pv, a, n)[0]
                    g_rob = ctx.denoise_guided(capi.DenoiseGuidedParams.defaults(), rc, rv, a, n)[0]
                    n_plain = ctx.denoise_nlm(capi.DenoiseNlmParams.defaults(), ha, hb, pv, a, n)[0]
                    n_rob = ctx.denoise_nlm(capi.DenoiseNlmParams.defaults(), ha, hb, rv, a, n)[0]
                    b = base[name, 64][0]
                    denoise_rows.append(f"{name} 64 spp, {label} | guided: plain inputs {b / mse(g_plain, truth):.3f}, robust inputs {b / mse(g_rob, truth):.3f} | "
                                        f"nlm: plain variance {b / mse(n_plain, truth):.3f}, robust variance {b / mse(n_rob, truth):.3f}")
        acc.close(); sc.close()
    lines = ["robust_sweep.py: F = MSE(plain) / MSE(robust) | Frel (relative MSE, brightest 0.1 % of the truth left out) | E = energy kept | mean t; truth: 4096 spp "
             "from zr_render; accumulators of cfg5 300x300 and mix0 384x256 read at 64, 128, 256 spp",
             "setting | " + " | ".join(f"{n} {k}" for n, k in cells) + " | worst F | worst Frel",
             "MSE(plain), relMSE(plain) | " + " | ".join(f"{base[c][0]:.4e} {base[c][1]:.4e}" for c in cells) + " | |"]
    best = None
    for label, p in settings:
        row = table[label]
        worst, worst_rel = min(row[c][0] for c in cells), min(row[c][1] for c in cells)
        lines.append(f"{label} | " + " | ".join(f"{row[c][0]:.3f} {row[c][1]:.3f} {row[c][2]:.4f} {mean_trim[(label,) + c]:.1f}" for c in cells) + f" | {worst:.3f} | {worst_rel:.3f}")
        if p.mode == capi.ROBUST_GINI and p.strength > 0 and (best is None or worst > best[0]):
            best = (worst, p.strength, lines[-1])
    lines.append(f"best worst-of-six F among the Gini strengths: {best[0]:.3f} at strength {best[1]:g}" +
                 (": above 1, the default" if best[0] > 1 else ": no strength beats the plain resolve on both scenes, the default stays 1.0"))
    lines.append("denoisers at 64 spp with their defaults, F = MSE(plain resolve) / MSE(filtered):")
    lines += denoise_rows
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        open(out, "w").write(text)


def timing(size, out, reps=15):
    """HIP-event times of the two kernels' launches in one process on one cfg5 accumulator at 64 spp, `reps` launches each after 3 warm-up launches"""
    os.environ["ZR_TIMELOG_KIND"] = "4"   # read when the context is created: zr_get_kernel_times then reports the accumulator's query kernels
    w, h = (int(x) for x in size.split("x"))
    ctx = capi.Context(0)
    ds = capi.DemoScene("cfg5")
    cam = ds.camera.copy()
    cam.image_width, cam.image_height = w, h
    sc = capi.Scene(ctx, ds.desc)
    acc = capi.Accumulator(ctx, w, h)
    acc.accumulate(sc, cam, ds.env, ds.seed, 64)
    col, var, trim = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w), dtype=np.int32)

    def timed(call):
        for _ in range(3):
            call()
        ctx.kernel_times_ms(4096)
        for _ in range(reps):
            call()
        t = np.array(ctx.kernel_times_ms(4096))
        assert len(t) == reps, len(t)
        return f"median {np.median(t):.3f} ms  min {t.min():.3f}  max {t.max():.3f}   {w * h * 1536 / 1e6 / np.median(t):.0f} GB/s of lane sums"

    import ctypes as C
    gini, fixed0 = capi.RobustParams.defaults(), capi.RobustParams.defaults(mode=capi.ROBUST_FIXED, trim=0)
    lines = [f"robust_sweep.py --timing {size}: cfg5, 64-spp accumulator, {reps} launches each after 3 warm-up, {w * h * 1536 / 1e9:.3f} GB of lane sums read per launch",
             "accum_variance | " + timed(lambda: acc.variance(var)),
             "accum_resolve_robust GINI, colour + variance + trim | " + timed(lambda: acc.resolve_robust(gini, col, var, trim)),
             "accum_resolve_robust GINI, colour only | " + timed(lambda: ctx.lib.zr_accum_resolve_robust(acc._a, C.byref(gini), col.ctypes.data, None, None)),
             "accum_resolve_robust FIXED t = 0, all outputs | " + timed(lambda: acc.resolve_robust(fixed0, col, var, trim)),
             "accum_variance (again) | " + timed(lambda: acc.variance(var))]
    t = acc.resolve_robust(gini)[2]
    lines.append(f"trim map at the default strength: mean t {t.mean():.2f}, t = 0 in {(t == 0).mean() * 100:.1f} % of the pixels, t = 31 in {(t == 31).mean() * 100:.1f} %")
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
