"""What rendering a frame in sample batches costs, and what it gains on a frame beyond one run of the pipeline.

  python scripts/dev/progressive_time.py batches [scene] [spp] [repeats]   one-shot zr_render against 2, 4 and 8 equal batches of zr_render_accumulate
  python scripts/dev/progressive_time.py big [scene] [spp]                one zr_render of a frame of more than 2^32 work units (default cfg2, 2112 spp)
  python scripts/dev/progressive_time.py bytes                            zr_accum_state's device bytes at 1080p and 4K

Wall-clock per frame around the blocking calls (resolve included), median of `repeats` after one warm-up.  Prints one JSON line per row.
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from raytracer_project_amd import capi   # noqa: E402


def timed(f, repeats):
    f()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def batches(name="cfg3", spp=512, repeats=3):
    import numpy as np
    ds = capi.DemoScene(name)
    ctx = capi.Context(0)
    sc = capi.Scene(ctx, ds.desc)
    cam = ds.camera.copy()
    cam.samples_per_pixel = spp
    out = np.zeros((cam.image_height, cam.image_width, 3))
    ref = sc.render(cam, ds.env, ds.seed).copy()
    med, lo, hi = timed(lambda: sc.render(cam, ds.env, ds.seed, out=out), repeats)
    print(json.dumps({"scene": name, "spp": spp, "batches": 1, "what": "zr_render", "ms": round(med, 2), "min": round(lo, 2), "max": round(hi, 2)}), flush=True)
    acc = capi.Accumulator(ctx, cam.image_width, cam.image_height)
    print(json.dumps({"accumulator_bytes": acc.state()["device_bytes"], "pixels": acc.state()["pixels"]}), flush=True)
    for nb in (1, 2, 4, 8):
        def run():
            acc.reset(0)
            for _ in range(nb):
                acc.accumulate(sc, cam, ds.env, ds.seed, spp // nb)
            acc.resolve(out)
        med, lo, hi = timed(run, repeats)
        print(json.dumps({"scene": name, "spp": spp, "batches": nb, "what": "zr_render_accumulate + resolve", "ms": round(med, 2), "min": round(lo, 2),
                          "max": round(hi, 2), "equal_to_one_shot": bool(np.array_equal(out, ref))}), flush=True)


def big(name="cfg2", spp=2112):
    import numpy as np
    ds = capi.DemoScene(name)
    ctx = capi.Context(0)
    sc = capi.Scene(ctx, ds.desc)
    cam = ds.camera.copy()
    cam.image_width, cam.image_height, cam.samples_per_pixel = 1920, 1080, spp
    out = np.zeros((cam.image_height, cam.image_width, 3))
    t0 = time.perf_counter()
    sc.render(cam, ds.env, ds.seed, out=out)
    ms = (time.perf_counter() - t0) * 1e3
    k = ctx.counters()
    print(json.dumps({"scene": name, "frame": "1920x1080", "spp": spp, "units": 1920 * 1080 * spp, "ms": round(ms, 1), "path": int(k.path), "rounds": int(k.rounds),
                      "kernel_ms": round(k.kernel_ms, 1), "checksum": float(out.sum())}), flush=True)


def accumulator_bytes():
    ctx = capi.Context(0)
    for w, h in ((1920, 1080), (3840, 2160)):
        acc = capi.Accumulator(ctx, w, h)
        print(json.dumps({"frame": f"{w}x{h}", **acc.state()}), flush=True)
        acc.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    if not a or a[0] == "batches":
        batches(a[1] if len(a) > 1 else "cfg3", int(a[2]) if len(a) > 2 else 512, int(a[3]) if len(a) > 3 else 3)
    elif a[0] == "big":
        big(a[1] if len(a) > 1 else "cfg2", int(a[2]) if len(a) > 2 else 2112)
    elif a[0] == "bytes":
        accumulator_bytes()
    else:
        sys.exit(__doc__)
