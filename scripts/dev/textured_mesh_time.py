"""development aid (GPU): what a texture on the headline mesh costs.  The cfg3 world from the package's own scene generator, its mesh given a
spherical UV projection about the mesh's centre, rendered three ways on the general SHADE build:
  solid     the world as it is, committed with ZR_SHADE_LEAN=0 (solid colours, no coordinates): the like-for-like baseline
  image     a seeded 1024 x 1024 8-bit image on the mesh's material, coordinates attached
  image+bump  a second seeded 1024 x 1024 image as that material's bump map on top
(the lean default, which is what bench.py times, is printed too).  Prints ms per frame (median of --steps after a warm-up) and device bytes per variant.
  python scripts/dev/textured_mesh_time.py [--steps 3] [--spp N] [--width W --height H]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from raytracer_project_amd import capi   # noqa: E402


def spherical_uv(tri_v):
    """(n, 3, 2): u = (atan2(-z, x) + pi) / 2 pi, v = acos(-y) / pi of every vertex's direction from the mesh's centre (sphere.hpp:70-79's map)"""
    v = tri_v.reshape(-1, 3)
    d = v - 0.5 * (v.min(0) + v.max(0))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    u = (np.arctan2(-d[:, 2], d[:, 0]) + np.pi) / (2 * np.pi)
    w = np.arccos(np.clip(-d[:, 1], -1, 1)) / np.pi
    return np.stack([u, w], 1).reshape(-1, 3, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    a = ap.parse_args()
    ds = capi.DemoScene("cfg3")
    cam = ds.camera.copy()
    if a.spp: cam.samples_per_pixel = a.spp
    if a.width: cam.image_width = a.width
    if a.height: cam.image_height = a.height
    d0 = ds.desc
    n = int(d0.n_tris)
    tri_v = np.ctypeslib.as_array(C.cast(d0.tri_v, C.POINTER(C.c_double)), (n * 9,)).copy()
    tri_mat = np.ctypeslib.as_array(C.cast(d0.tri_mat, C.POINTER(C.c_uint32)), (n,))
    mesh_mat = int(np.bincount(tri_mat).argmax())
    uv = spherical_uv(tri_v)
    mats = list(C.cast(d0.materials, C.POINTER(capi.Material * int(d0.n_materials))).contents)
    texs = list(C.cast(d0.textures, C.POINTER(capi.Texture * int(d0.n_textures))).contents)
    rng = np.random.default_rng(2024)
    blob = bytes(C.cast(d0.texels, C.POINTER(C.c_ubyte * int(d0.texel_bytes))).contents) if d0.texel_bytes else b""
    blob += bytes(-len(blob) % 16)
    image_at = len(blob); blob += rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8).tobytes()
    bump_at = len(blob); blob += rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8).tobytes()
    zero3 = (C.c_double * 3)(0, 0, 0)
    image_tex, bump_tex = len(texs), len(texs) + 1
    texs += [capi.Texture(2, 0, 0, 1024, 1024, 0, image_at, 0.0, zero3), capi.Texture(2, 0, 0, 1024, 1024, 0, bump_at, 0.0, zero3)]
    keep = []

    def desc(image, bump):
        d = capi.SceneDesc()
        C.memmove(C.byref(d), C.byref(d0), C.sizeof(capi.SceneDesc))
        mm = (capi.Material * len(mats))(*mats)
        if image: mm[mesh_mat].tex = image_tex
        if bump: mm[mesh_mat].bump_tex = bump_tex; mm[mesh_mat].bump_strength = 1.0
        tt = (capi.Texture * len(texs))(*texs)
        bb = (C.c_ubyte * len(blob)).from_buffer_copy(blob)
        keep.extend([mm, tt, bb])
        d.materials = C.cast(mm, C.c_void_p); d.n_materials = len(mats)
        d.textures = C.cast(tt, C.c_void_p); d.n_textures = len(texs)
        d.texels = C.cast(bb, C.c_void_p); d.texel_bytes = len(blob)
        return d

    ctx = capi.Context(0)
    print(f"cfg3: {n} triangles, mesh material {mesh_mat}, {cam.image_width} x {cam.image_height} at {cam.samples_per_pixel} spp, {a.steps} steps")
    for name, lean, image, bump in (("lean default (bench.py)", "1", False, False), ("solid, ZR_SHADE_LEAN=0", "0", False, False), ("image", "0", True, False),
                                    ("image + bump", "0", True, True)):
        os.environ["ZR_SHADE_LEAN"] = lean   # read at commit
        sc = capi.Scene(ctx, desc(image, bump), tri_uv=uv if image else None)
        out = np.zeros((cam.image_height, cam.image_width, 3))
        sc.render(cam, ds.env, ds.seed, out=out)
        ms = []
        for _ in range(a.steps):
            t0 = time.perf_counter(); sc.render(cam, ds.env, ds.seed, out=out); ms.append((time.perf_counter() - t0) * 1e3)
        st, k = sc.stats(), sc.kernels()
        print(f"{name:26s} {statistics.median(ms):9.2f} ms per frame (min {min(ms):.2f}, max {max(ms):.2f})   device bytes {st['device_bytes']:>11d}   "
              f"shade_lean {k['shade_lean']}   checksum {float(out.sum()):.6f}", flush=True)
        sc.close()
    ctx.close()


if __name__ == "__main__":
    main()
