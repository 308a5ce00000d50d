"""The measurements behind zr_temporal_params' defaults and DESIGN §15.

  python scripts/dev/temporal_sweep.py [--out FILE]                    the quality sweep
  python scripts/dev/temporal_sweep.py --timing 1920x1080 [--out FILE]    wall clock of one frame's temporal stage (run it under rocprofv3 --kernel-trace
                                                                          --stats for the per-kernel times)

The sweep: cfg5 at 300 x 300 and mix0 at 384 x 256 (tests/test_temporal.py's quality scenes and sizes) along its 8-frame camera path (about 3 px per frame
along the camera's u at the reference depth plus 1 mrad of yaw per frame), 64 spp per frame with seed + k; truth is the last camera at 4096 spp.  For alpha in
{0.1, 0.2, 0.4} x plane_tolerance in {0.003, 0.01, 0.03} (max_history 32, normal_cos 0.9), with F = MSE(last noisy frame) / MSE(x):
  F_t       the temporal colour over the pixels whose final history length is >= 4 (and their share of the frame)
  F_g       the guided filter (defaults) on the temporal colour and variance, whole frame; "alone" is the same filter on the last frame by itself
  F_g opaque  the same two over the pixels whose first hit is neither a dielectric nor a medium
The defaults are the setting with the best worse-of-two-scenes F_g.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from raytracer_project_amd import capi  # noqa: E402
import temporal_model as tm  # noqa: E402   (camera_path)

SCENES = {"cfg5": (300, 300, 1355.0), "mix0": (384, 256, None)}
ALPHAS, TOLERANCES = (0.1, 0.2, 0.4), (0.003, 0.01, 0.03)
FRAMES = 8


def opaque_mask(ds, mat):
    """pixels whose first hit is neither a dielectric nor a medium (misses count as opaque)"""
    n = int(ds.desc.n_materials)
    kinds = np.array([m.kind for m in C.cast(ds.desc.materials, C.POINTER(capi.Material * n)).contents], dtype=np.int64)
    hit = mat != 0xFFFFFFFF
    k = np.where(hit, kinds[np.where(hit, mat, 0)], -1)
    return (k != 2) & (k != 4)


def scene_inputs(ctx, name):
    w, h, depth = SCENES[name]
    ds = capi.DemoScene(name)
    cam = ds.camera.copy()
    cam.image_width, cam.image_height = w, h
    depth = depth or float(np.linalg.norm(np.array(list(cam.lookat)) - np.array(list(cam.lookfrom))))
    path = tm.camera_path(cam, FRAMES, depth, 3.0, 0.001)
    sc = capi.Scene(ctx, ds.desc)
    acc = capi.Accumulator(ctx, w, h)
    frames = []
    for k, c in enumerate(path):
        acc.reset(0)
        acc.accumulate(sc, c, ds.env, ds.seed + k, 64)
        frames.append((acc.resolve(), acc.variance()))
    acc.close()
    last = path[-1]
    a, n, _ = sc.render_aov(last, ds.seed, 1.0)
    tc = last.copy(); tc.samples_per_pixel = 4096
    truth = sc.render(tc, ds.env, ds.seed, None)
    return dict(ds=ds, scene=sc, path=path, frames=frames, albedo=a, normal=n, truth=truth, opaque=opaque_mask(ds, sc.render_gbuffer(last, ds.seed)["mat"]), w=w, h=h)


def sweep(out):
    ctx = capi.Context(0)
    sets = {name: scene_inputs(ctx, name) for name in SCENES}
    gp = capi.DenoiseGuidedParams.defaults()
    mse = lambda f, t, m=None: float(((f - t) ** 2).mean()) if m is None else float(((f - t) ** 2)[m].mean())
    lines = [f"temporal_sweep.py: F = MSE(last noisy frame) / MSE(x) against 4096 spp; {FRAMES} frames of 64 spp along the test path (cfg5 300x300, mix0 384x256); "
             "max_history 32, normal_cos 0.9; per scene: F_t (share of the frame with history >= 4) | F_g whole | F_g opaque",
             "setting | " + " | ".join(SCENES) + " | worse F_g of cfg5, mix0"]
    alone = {}
    for name, s in sets.items():
        noisy, var = s["frames"][-1]
        g, _ = ctx.denoise_guided(gp, noisy, var, s["albedo"], s["normal"])
        alone[name] = (mse(noisy, s["truth"]) / mse(g, s["truth"]), mse(noisy, s["truth"], s["opaque"]) / mse(g, s["truth"], s["opaque"]))
    lines.append("MSE(noisy), opaque share | " + " | ".join(f"{mse(s['frames'][-1][0], s['truth']):.4e}, {s['opaque'].mean():.3f}" for s in sets.values()) + " |")
    lines.append("guided filter alone | " + " | ".join(f"- | {alone[k][0]:.3f} | {alone[k][1]:.3f}" for k in sets) + f" | {min(v[0] for v in alone.values()):.3f}")
    best = None
    for alpha in ALPHAS:
        for tol in TOLERANCES:
            p = capi.TemporalParams.defaults(alpha=alpha, plane_tolerance=tol)
            cells, fg = [], {}
            for name, s in sets.items():
                hist = capi.Temporal(ctx, s["w"], s["h"])
                for k, (c, (col, var)) in enumerate(zip(s["path"], s["frames"])):
                    t, tv, n = hist.accumulate(s["scene"], c, s["ds"].seed, col, var, p)
                hist.close()
                noisy, truth, old = s["frames"][-1][0], s["truth"], n >= 4
                g, _ = ctx.denoise_guided(gp, t, tv, s["albedo"], s["normal"])
                fg[name] = mse(noisy, truth) / mse(g, truth)
                cells.append(f"{mse(noisy, truth, old) / mse(t, truth, old):.3f} ({old.mean():.3f}) | {fg[name]:.3f} | "
                             f"{mse(noisy, truth, s['opaque']) / mse(g, truth, s['opaque']):.3f}")
            worse = min(fg.values())
            lines.append(f"alpha {alpha} plane_tolerance {tol} | " + " | ".join(cells) + f" | {worse:.3f}")
            if best is None or worse > best[0]:
                best = (worse, lines[-1])
    lines.append("best worse-of-two: " + best[1])
    for s in sets.values():
        s["scene"].close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        open(out, "w").write(text)


def timing(size, out, repeats=7):
    """wall clock, median of `repeats` after a warm-up, of zr_accum_temporal on a 64-spp cfg5 accumulator along the path, against the host route"""
    w, h = (int(x) for x in size.split("x"))
    ctx = capi.Context(0)
    ds = capi.DemoScene("cfg5")
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel = w, h, 64
    path = tm.camera_path(cam, repeats + 1, 1355.0, 3.0, 0.001)
    sc = capi.Scene(ctx, ds.desc)
    acc = capi.Accumulator(ctx, w, h)
    acc.accumulate(sc, cam, ds.env, ds.seed, 64)
    col, var = acc.resolve(), acc.variance()

    def med(f):
        f(path[0])
        ts = []
        for c in path[1:]:
            t0 = time.perf_counter(); f(c); ts.append((time.perf_counter() - t0) * 1e3)
        return f"{statistics.median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f})"

    hist = capi.Temporal(ctx, w, h)
    lines = [f"temporal_sweep.py --timing {size}: cfg5, one 64-spp accumulator taken into the history along the path, defaults, wall clock, median of {repeats} after a warm-up",
             "zr_accum_temporal (three frames down) | " + med(lambda c: acc.temporal(hist, sc, c, ds.seed))]
    hist.reset()
    lines.append("zr_temporal_accumulate (two frames up, three down) | " + med(lambda c: hist.accumulate(sc, c, ds.seed, col, var)))
    lines.append("zr_render_gbuffer (four planes down) | " + med(lambda c: sc.render_gbuffer(c, ds.seed)))
    hist.close(); acc.close(); sc.close(); ctx.close()
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
