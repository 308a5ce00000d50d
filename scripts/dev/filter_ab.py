"""development aid (MI355X): a SHA-256 of every output of the image filters on fixed inputs, to compare two builds of the library bit for bit.

    python scripts/dev/filter_ab.py > change.txt;  ZR_LIB=<another libzr_hip.so> python scripts/dev/filter_ab.py > other.txt;  diff change.txt other.txt

zr_denoise, zr_denoise_guided, zr_denoise_nlm and zr_sharpen_frame on seeded synthetic frames (1 x 1, 7 x 5, 17 x 18, 333 x 77; demodulation and the depth
guide on and off; 0, 1 and 5 levels; five non-local-means windows), then zr_accum_denoise, zr_accum_denoise_nlm and zr_accum_temporal (two frames) on a
64-spp accumulator of cfg5 at 96 x 64."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from raytracer_project_amd import capi  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def frames(w, h):
    rng = np.random.default_rng(5000 + 31 * w + h)
    f = {"albedo": rng.uniform(0.0, 0.9, (h, w, 3)), "normal": rng.uniform(0.0, 1.0, (h, w, 3)), "zdepth": np.repeat(rng.uniform(0.2, 0.9, (h, w, 1)), 3, axis=2),
         "variance": rng.exponential(0.01, (h, w, 3))}
    f["color"] = f["albedo"] * rng.exponential(1.0, (h, w, 1))
    noise = rng.normal(0.0, 0.05, (h, w, 3))
    f["half_a"], f["half_b"] = f["color"] + noise, f["color"] - noise
    f["albedo"][rng.random((h, w)) < 0.05] = 0.0
    f["normal"][rng.random((h, w)) < 0.05] = 0.5
    for name, values in (("albedo", (np.nan, np.inf)), ("normal", (np.nan, -np.inf)), ("color", (np.nan, np.inf)), ("zdepth", (np.nan, np.inf)),
                         ("variance", (np.nan, -1.0)), ("half_a", (np.nan, -np.inf)), ("half_b", (np.inf, np.nan))):
        m = rng.random(f[name].shape) < 0.01
        f[name][m] = rng.choice(values, size=int(m.sum()))
    return f


def main():
    ctx = capi.Context(0)
    for w, h in ((1, 1), (7, 5), (17, 18), (333, 77)):
        f = frames(w, h)
        for demod in (0, 1):
            for depth in (False, True):
                z = f["zdepth"] if depth else None
                for it in (0, 1, 5):
                    tag = f"{w}x{h} demod={demod} depth={int(depth)} iterations={it}"
                    p = capi.DenoiseParams.defaults(iterations=it, demodulate_albedo=demod, sigma_depth=0.05 if depth else 0.0)
                    print("zr_denoise", tag, sha(ctx.denoise(p, f["color"], f["albedo"], f["normal"], z)))
                    g = capi.DenoiseGuidedParams.defaults(iterations=it, demodulate_albedo=demod, sigma_depth=0.05 if depth else 0.0)
                    out, var = ctx.denoise_guided(g, f["color"], f["variance"], f["albedo"], f["normal"], z)
                    print("zr_denoise_guided", tag, sha(out), sha(var))
            for r, pf in ((0, 0), (1, 0), (3, 1), (7, 1), (10, 3)):
                n = capi.DenoiseNlmParams.defaults(search_radius=r, patch_radius=pf, demodulate_albedo=demod)
                out, err = ctx.denoise_nlm(n, f["half_a"], f["half_b"], f["variance"], f["albedo"], f["normal"])
                print("zr_denoise_nlm", f"{w}x{h} demod={demod} r={r} f={pf}", sha(out), sha(err))
        clean = np.nan_to_num(f["color"], nan=0.0, posinf=0.0, neginf=0.0)
        for amount in (0.2, 0.75):
            print("zr_sharpen_frame", f"{w}x{h} amount={amount}", sha(ctx.sharpen(clean, amount)))

    W, H = 96, 64
    ds = capi.DemoScene("cfg5")
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel = W, H, 64
    sc = capi.Scene(ctx, ds.desc)
    acc = capi.Accumulator(ctx, W, H)
    acc.accumulate(sc, cam, ds.env, ds.seed, 64)
    albedo, normal, zdepth = sc.render_aov(cam, ds.seed, 1.0)
    print("accumulator", f"cfg5 {W}x{H} 64 spp", sha(acc.resolve()), sha(acc.variance()))
    for depth in (False, True):
        g = capi.DenoiseGuidedParams.defaults(sigma_depth=0.05 if depth else 0.0)
        print("zr_accum_denoise", f"depth={int(depth)}", *[sha(o) for o in acc.denoise(g, albedo, normal, zdepth if depth else None)])
    for demod in (0, 1):
        print("zr_accum_denoise_nlm", f"demod={demod}", *[sha(o) for o in acc.denoise_nlm(capi.DenoiseNlmParams.defaults(demodulate_albedo=demod), albedo, normal)])
    hist = capi.Temporal(ctx, W, H)
    print("zr_accum_temporal", "frame 0", *[sha(o) for o in acc.temporal(hist, sc, cam, ds.seed)])
    moved = cam.copy()
    moved.lookfrom[0] += 0.5
    acc.reset(0)
    acc.accumulate(sc, moved, ds.env, ds.seed + 1, 64)
    print("zr_accum_temporal", "frame 1", *[sha(o) for o in acc.temporal(hist, sc, moved, ds.seed + 1)])
    hist.close(); acc.close(); sc.close(); ctx.close()


if __name__ == "__main__":
    main()
