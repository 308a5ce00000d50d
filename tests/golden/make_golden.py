#!/usr/bin/env python3
"""Generates tests/golden/*.npz from the GENUINE reference arithmetic.

Runs only in the build container: it executes oracle/_ref/zenith_ref, which oracle/Makefile compiles from
the headers under /root/reference (never copied into this repo) plus oracle/ref_harness.cpp.  The fixtures
are data only — inputs (scene name, region, seed, rays) and expected outputs (radiance, hit records,
segment / RNG-draw counts).  Commit the .npz files together with this script.

    python tests/golden/make_golden.py            # everything (cfg3_full takes ~1 min: 1M-triangle BVH)
    python tests/golden/make_golden.py cfg1 mix0  # selected fixtures
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))   # tests/post_model.py: the edge inputs of the post stack
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "zenith_ref")

# name -> (scene, x0, y0, w, h, spp (0 = the config's own), per_sample, extra scene args)
TILES = {
    "cfg1_full": ("cfg1", 0, 0, 400, 225, 0, False, []),             # the whole plumbing config
    "cfg1_tile": ("cfg1", 180, 100, 16, 16, 0, True, []),
    "cfg2_tile": ("cfg2", 600, 300, 16, 16, 0, False, []),            # full 256 spp
    "cfg2_tile_b": ("cfg2", 300, 420, 12, 12, 0, False, []),
    "cfg3_small": ("cfg3", 900, 500, 24, 24, 64, False, [200, 20, 256, 128]),   # 8 000 triangles, 256x128 HDRI
    "cfg3_full": ("cfg3", 944, 528, 16, 16, 0, False, []),            # 1 000 000 triangles, 4096x2048 HDRI, 512 spp
    "cfg5_tile": ("cfg5", 250, 300, 8, 8, 0, False, []),              # 1024 spp, depth 50
    "cfg5_tile_b": ("cfg5", 150, 450, 8, 8, 256, True, []),            # glass sphere region
    "mix0_full": ("mix0", 0, 0, 96, 64, 0, False, []),
    "mix1_full": ("mix1", 0, 0, 96, 64, 0, False, []),
    "mix2_full": ("mix2", 0, 0, 96, 64, 0, False, []),
    "mix0_tile": ("mix0", 30, 20, 16, 16, 0, True, []),
    "mesh0_full": ("mesh0", 0, 0, 96, 64, 0, False, []),            # OBJ ingest through `model`
    "inst1_full": ("inst1", 0, 0, 112, 72, 0, False, []),           # grouping corner cases: mixed shared child, nested wrappers, bare + placed, single placement
    "inst2_full": ("inst2", 0, 0, 128, 80, 0, False, []),           # a composite prefab x 6 (mesh inside the prefab: a group inside a group, sphere, placed cube, pedestal) + the mesh by itself
    "inst0_full": ("inst0", 0, 0, 128, 80, 0, False, []),           # one mesh placed 36 times + one placed 8 times (two-level BVH on the device)
    # the reference's own demo workload (scene_management.hpp:103-236): 900 instanced prefabs, a wrapped mesh, fog
    "demo_tile": ("demo", 560, 300, 48, 32, 32, False, []),          # mesh + mirror sphere + glass cube
    "demo_tile_b": ("demo", 200, 420, 40, 24, 32, True, []),         # the instance grid through the fog
    "cfg3w_small": ("cfg3w", 900, 500, 24, 24, 64, False, [200, 20, 256, 128]),
}
TRACES = {
    # name -> (scene, rays, seed, probe-box clamp lo, hi, extra scene args)
    "trace_mix0": ("mix0", 4096, 11, -6, 6, []),
    "trace_cfg2": ("cfg2", 2048, 12, -12, 12, []),
    "trace_cfg5": ("cfg5", 2048, 13, -30, 600, []),
    "trace_cfg3_small": ("cfg3", 2048, 14, -4, 4, [200, 20, 256, 128]),
    "trace_mesh0": ("mesh0", 4096, 15, -3, 4, []),
    "trace_inst0": ("inst0", 4096, 18, -7, 7, []),
    "trace_inst1": ("inst1", 4096, 19, -5, 5, []),
    "trace_inst2": ("inst2", 4096, 24, -6, 6, []),
    "trace_demo": ("demo", 4096, 16, -16, 16, []),
    "trace_cfg3w_small": ("cfg3w", 4096, 17, -4, 4, [200, 20, 256, 128]),   # a placed (wrapped) mesh: baked to world space on the device
    # adversarial rays (ZR_TRACE_ADVERSARIAL: zero direction components, tiny/large scales, round and far origins)
    "trace_adv_mix0": ("mix0", 4096, 21, -6, 6, [], True),
    "trace_adv_cfg2": ("cfg2", 4096, 22, -12, 12, [], True),
    "trace_adv_cfg3_small": ("cfg3", 4096, 23, -4, 4, [200, 20, 256, 128], True),
}


# first-hit AOV tiles: name -> (scene, x0, y0, w, h, z_depth_max_dist, extra scene args)
AOVS = {
    "aov_mix0": ("mix0", 0, 0, 96, 64, 20.0, []),
    "aov_mix1": ("mix1", 8, 8, 64, 40, 12.0, []),
    "aov_cfg2": ("cfg2", 560, 280, 48, 32, 20.0, []),
    "aov_mesh0": ("mesh0", 0, 0, 96, 64, 9.0, []),
    "aov_inst0": ("inst0", 0, 0, 128, 80, 25.0, []),
    "aov_inst2": ("inst2", 0, 0, 128, 80, 25.0, []),
}

# beauty / reflection / refraction with the split flags on (camera.hpp:490-517): (scene, x0, y0, w, h, spp, scene args)
PASSES = {
    "passes_mix0": ("mix0", 0, 0, 96, 64, 16, []),
    "passes_mix2": ("mix2", 0, 0, 64, 48, 16, []),
    "passes_cfg2": ("cfg2", 560, 280, 48, 32, 32, []),
    "passes_cfg5": ("cfg5", 150, 350, 32, 24, 32, []),
    "passes_inst0": ("inst0", 16, 8, 96, 64, 16, []),
}

# the post stack (bloom, sharpen, process, 8-bit; analyze_framebuffer) through the genuine post_processor / bloom_filter:
# (scene, spp of the input frame, presets of `zenith_ref post`)
POSTS = {
    "post_cfg1": ("cfg1", 4, [0, 1, 2, 3, 4, 5, 6, 7]),
    "post_mix0": ("mix0", 8, [1, 3]),
}
# the post stack at its edges is a family of its own, "post_edges": make_post_edges() below, inputs from tests/post_model.py


def make_post_edges(tmp):
    """post_edges.npz: the post stack at its edges.  tests/post_model.py describes frames, parameter sets and cases; `zenith_ref post_raw` runs the genuine
    post_processor / bloom_filter on each.  Hundreds of tiny arrays would cost more in archive headers than in data, so they are packed: `frames` holds
    every input frame end to end, `rgb8` the 8-bit image of every case, `hist` one histogram row per frame; meta lists per frame its shape, offset, row,
    average / maximum luminance and both auto-exposure values, and per case its frame, parameters and offset."""
    import post_model as pm
    meta = {"cases": [], "frames": {}}
    frames = dict(pm.post_frames())
    packed_frames, packed_rgb8, hists, at = [], [], [], 0
    for name, frame in list(frames.items()) + list(pm.stat_frames().items()):
        pre = os.path.join(tmp, "pe_" + name)
        np.ascontiguousarray(frame, dtype="<f8").tofile(pre + ".bin")
        m = run("post_raw", pre + ".bin", frame.shape[1], frame.shape[0], pre)
        meta["frames"][name] = dict({k: m[k] for k in ("average_luminance", "max_luminance", "auto_exposure_on", "auto_exposure_off", "exposure")},
                                    shape=list(frame.shape), offset=at, row=len(hists))
        packed_frames.append(frame.ravel()); at += frame.size
        hists.append(np.load(pre + "_hist.npy"))
    at = 0
    for name, fname, p, data, gamma in pm.cases():
        frame = frames[fname]
        pre = os.path.join(tmp, "pe_case_" + name)
        m = run("post_raw", os.path.join(tmp, "pe_" + fname + ".bin"), frame.shape[1], frame.shape[0], pre, *pm.ref_arguments(p, data, gamma))
        for k in pm.FLOAT_FIELDS:   # the harness parsed what was meant
            assert np.float32(m[k]) == np.float32(p[k]), (name, k, m[k], p[k])
        assert m["bloom_radius"] == p["bloom_radius"] and m["debug"] == p["debug"] and m["is_data_pass"] == int(data) and m["apply_gamma"] == int(gamma)
        assert m["color_balance"] == p["color_balance"] and m["sharpen_amount"] == p["sharpen_amount"]
        rgb8 = np.load(pre + "_rgb8.npy")
        assert rgb8.shape == frame.shape
        meta["cases"].append({"name": name, "frame": fname, "params": p, "is_data_pass": data, "apply_gamma": gamma, "offset": at})
        packed_rgb8.append(rgb8.ravel()); at += rgb8.size
    out = os.path.join(HERE, "post_edges.npz")
    np.savez_compressed(out, meta=np.array(json.dumps(meta)), frames=np.concatenate(packed_frames), rgb8=np.concatenate(packed_rgb8), hist=np.stack(hists))
    print("post_edges", len(meta["cases"]), "cases,", len(meta["frames"]), "frames,", os.path.getsize(out), "bytes")


def kat_inputs():
    """Hand-placed inputs of the per-function known-answer fixture (scene "kat0", scenes/zr_scenes_mix.inc).
    rays: (o, d, tmin, tmax); the comment names the reference behaviour each one pins."""
    INF = float("inf")
    R = []

    def ray(o, d, tmin=0.001, tmax=INF):
        R.append(list(o) + list(d) + [tmin, tmax])
    # sphere::hit (sphere.hpp:18-79): centre (0, 4, 0), r = 1, image-textured
    ray((0, 4, 5), (0, 0, -1))                       # near root, front face
    ray((0, 4, 0), (0, 0, -1))                       # origin inside: near root negative, far root taken, back face
    ray((0, 9, 0), (0, -1, 0))                       # north pole: up x n vanishes -> tangent fallback z x n (sphere.hpp:50-59), v = 1
    ray((0, 1, 0), (0, 1, 0))                        # south pole, v = 0
    ray((1e-9, 9, 0), (0, -1, 0))                    # a hair off the pole: the fallback threshold
    ray((1, 4, 5), (0, 0, -1))                       # tangent ray: discriminant exactly 0
    ray((0, 4, 5), (0, 0, -1), 0.001, 4.0)           # t == ray_t.max: surrounds() is strict -> miss
    ray((0, 4, 5), (0, 0, -1), 0.001, 4.000001)
    ray((0, 4, 5), (0, 0, -1), 4.0, INF)             # t == ray_t.min: strict -> the far root (t = 6)
    for k in range(8):                               # around the equator: u = (atan2(-z, x) + pi) / 2 pi incl. the seam
        c, sn = np.cos(k * np.pi / 4), np.sin(k * np.pi / 4)
        ray((5 * c, 4, 5 * sn), (-5 * c, 0, -5 * sn))          # un-normalised direction: t = 0.8
    ray((0, 4, 5), (0, 0, -1e-3))                    # short direction vector: t = 4000
    # cube::hit (cube.hpp:44-142): bare, origin-centred, half extents (1, 0.5, 0.75)
    ray((3, .1, .2), (-1, 0, 0)); ray((-3, .1, .2), (1, 0, 0)); ray((.3, 3, .2), (0, -1, 0))
    ray((.3, -2, .2), (0, 1, 0)); ray((.3, .1, 3), (0, 0, -1)); ray((.3, .1, -1.5), (0, 0, 1))
    ray((0.2, 0.1, -0.1), (1, 0.3, 0.2))             # origin inside: rec.t = ray_t.min, no face matches -> the +z fallthrough
    ray((3, 0.5, 0), (-1, 0, 0))                     # along the top face plane: 0 * inf = NaN in the y slab, fmax / fmin ignore it
    ray((3, 3, 3), (-1, -1, -1))
    ray((3, 0.5000001, 0), (-1, 0, 0))               # just above the face (inside the padded box): miss
    # dielectric sphere (6, 0, 0)
    ray((6, 0, 5), (0, 0, -1))
    ray((6, 0, 0), (0, 0.6, 0.8))                    # from inside, normal incidence: exit IOR
    ray((6, 0.9, 0), (1, 0, 0))                      # from inside at 64 degrees: total internal reflection, no draw
    ray((6.95, 0, 5), (0, 0, -1))                    # grazing from outside: Schlick close to 1
    # metal
    ray((0, -4, 5), (0, 0, -1))                      # fuzz 0 still draws a unit vector (material.hpp:141)
    ray((2, -4, 5), (-0.3, 0, -1))
    ray((6.99, 4, 5), (0, 0, -1))                    # fuzz 0.4 at grazing incidence: scatter may return false
    ray((6, 4, 5), (0, 0, -1))                       # bump map + nested checker
    ray((-6, 0, 5), (0, 0, -1))                      # diffuse_light: emitted = texture, scatter false
    ray((-6, 3, 5), (0, 0, -1))                      # failed image load: cyan
    ray((-6.1, -3, 5), (0, 0, -1))                   # sphere built with r = -0.75: box from |r|, hit radius max(0, r) = 0 -> miss
    ray((6, -4, 5), (0, 0, -1)); ray((6.5, -4.3, 5), (0, 0, -1))      # bumped lambertian
    # triangle::hit (triangle.hpp:17-82): A (3,0,-2) B (5,0,-2) C (3,2,-2), plane z = -2
    ray((3.5, 0.5, 3), (0, 0, -1))
    ray((4, 0, 3), (0, 0, -1))                       # on edge AB: the edge test is >= 0
    ray((3, 0, 3), (0, 0, -1))                       # on vertex A
    ray((4, 1, 3), (0, 0, -1))                       # on edge BC
    ray((4, -1e-12, 3), (0, 0, -1))                  # a hair outside
    ray((3.5, 0.5, 3), (0, 0, -1), 0.001, 5.0)       # t == ray_t.max: contains() is inclusive -> hit
    ray((3.5, 0.5, 3), (0, 0, -1), 0.001, 4.999999999)
    ray((3.5, 0.5, 3), (0, 0, -1), 5.0, INF)         # t == ray_t.min: inclusive -> hit
    ray((3.5, 0.5, -2), (1, 0, 0))                   # in the plane: |N.d| < 1e-8 -> miss
    ray((3.5, 0.5, -5), (0, 0, 1))                   # back face
    ray((3.0, 0.5, -1.9999999999), (1, 0, -1e-9))    # geometrically a hit, rejected by the parallel threshold
    ray((3.5, 0.5, 3), (0, 0, -1e6))                 # t = 5e-6 < ray_t.min
    ray((1.5, 9, 0), (0, -1, 0))                     # through the degenerate triangle at y = 8: never hit
    ray((-4, 0.8333, 3), (0, 0, -1)); ray((-4, 0.8333, -6), (0, 0, 1))   # tilted triangle with smooth normals, both sides
    # cube under translate: front_face forced true (translate.hpp:29)
    ray((0.1, 0.2, 9), (0, 0, -1)); ray((0, 0, 6), (0, 0, 1))
    # constant_medium in a sphere (0, 0, -8) r = 2
    ray((0, 0, -3), (0, 0, -1)); ray((0, 0, -8), (1, 0, 0)); ray((3, 0, -3), (0, 0, -1)); ray((0, 0, -3), (0, 0, -1), 0.001, 4.0)
    # closest of several, signed zeros, far origin
    ray((-10, 0, 0), (1, 0, 0)); ray((10, 0, 0), (-1, 0, 0)); ray((0, 4, 5), (-0.0, 0.0, -1)); ray((0, 4, 1e6), (0, 0, -1))
    rays = np.array(R, dtype=np.float64)

    # texture::value: every kat texture at and beyond the edges of the unit square
    edge = [0.0, 1.0, -0.25, 1.25, 0.5, 0.999999, 1e-9, 2.5, -3.75, 0.0625, 0.9375]
    pts = [(0, 0, 0), (0.5, 0, 0), (-0.5, 0.25, 1.5), (1.4999999, -1.5, 0.7), (-1e-12, 3.0, -0.75)]
    T = [[t, u, v, *pts[(iu + 3 * iv + t) % len(pts)]] for t in range(6) for iu, u in enumerate(edge) for iv, v in enumerate(edge)]
    tex = np.array(T, dtype=np.float64)

    # get_background_color: mode, bg rgb, intensity, yaw, tilt, roll, sun dir, sun colour, sun intensity, sun size | direction
    s0 = np.array([1.0, 0.5, -0.5]) / np.linalg.norm([1.0, 0.5, -0.5])
    envs = [
        [0, 0, 0, 0, 1.0, 0, 0, 0, *s0, 1, 1, 1, 1.0, 1.0],                       # the default PHYSICAL_SUN
        [0, 0, 0, 0, 0.8, 0, 0, 0, 1.0, 0.06, -0.45, 1, 0.9, 0.8, 3.0, 8.0],      # low sun: sunset branch, not normalised
        [0, 0, 0, 0, 1.3, 0, 0, 0, 1.0, -0.02, -0.3, 1, 1, 1, 2.0, 4.0],          # sun just below the horizon
        [0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, -0.5, 0.0, 1, 1, 1, 1.0, 1.0],            # night: no disc
        [2, 0.25, 0.3, 0.35, 1.2, 0, 0, 0, *s0, 1, 1, 1, 1.0, 1.0],               # SOLID_COLOR
        [1, 0, 0, 0, 0.75, 1.1, 0.35, -0.4, *s0, 1, 1, 1, 1.0, 1.0],              # HDR_MAP, yaw / tilt / roll
        [1, 0, 0, 0, 1.0, 0, 0, 0, *s0, 1, 1, 1, 1.0, 1.0],                       # HDR_MAP, no rotation: poles and the seam
    ]
    rng = np.random.default_rng(20261004)
    dirs = [(0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), (1, 1e-12, 0), (1, -1e-12, 0), (-1, 0, 1e-12), (-1, 0, -1e-12),
            (3, 4, 0), (0.001, 0.002, 0.002)]
    dirs += [tuple(v) for v in rng.normal(size=(20, 3))]
    B = []
    for e in envs:
        sun = np.array(e[8:11]) / np.linalg.norm(e[8:11])
        mine = list(dirs)
        if e[0] == 0:   # at, inside and across the edge of the sun disc (threshold 1 - sun_size / 1000, smoothstep 2e-4 wide)
            thr = 1.0 - e[15] * 0.001
            ortho = np.cross(sun, [0.3, 0.1, 0.9]); ortho /= np.linalg.norm(ortho)
            for cosang in (1.0, thr + 0.0003, thr + 0.0001, thr + 0.00005, thr - 0.00001):
                mine.append(tuple(cosang * sun + np.sqrt(max(0.0, 1 - cosang * cosang)) * ortho))
        B += [e + list(d) for d in mine]
    bg = np.array(B, dtype=np.float64)
    cam = {"kat0": np.array([[i, j, s] for (i, j) in [(0, 0), (63, 0), (0, 47), (63, 47), (31, 23)] for s in range(4)], dtype=np.float64),
           "cfg1": np.array([[i, j, s] for (i, j) in [(0, 0), (399, 0), (0, 224), (399, 224), (200, 112)] for s in range(2)], dtype=np.float64)}
    return rays, tex, bg, cam


def make_kat(tmp):
    rays, tex, bg, cam = kat_inputs()
    arrays, metas = {"rays": rays, "tex_in": tex, "bg_in": bg}, {}
    for what, arr, outs in (("hits", rays, ("recs", "scat")), ("tex", tex, ("rgb",)), ("bg", bg, ("rgb",))):
        f = os.path.join(tmp, f"kat_{what}.bin"); pre = os.path.join(tmp, f"kat_{what}")
        arr.tofile(f)
        metas[what] = run("kat", "kat0", what, f, len(arr), pre)
        for o in outs:
            arrays[f"{what}_{o}" if what != "hits" else o] = np.load(f"{pre}_{o}.npy")
    for scene, req in cam.items():
        f = os.path.join(tmp, f"kat_cam_{scene}.bin"); pre = os.path.join(tmp, f"kat_cam_{scene}")
        req.tofile(f)
        metas[f"cam_{scene}"] = run("kat", scene, "cam", f, len(req), pre)
        arrays[f"cam_req_{scene}"] = req.astype(np.int32)
        arrays[f"cam_rays_{scene}"] = np.load(pre + "_rays.npy")
    np.savez_compressed(os.path.join(HERE, "kat_kat0.npz"), meta=np.array(json.dumps(metas)), **arrays)
    print("kat_kat0", {k: v.shape for k, v in arrays.items()})


def kat1_inputs():
    """Hand-placed rays of the wrapper-chain fixture (scene "kat1", scenes/zr_scenes_mix.inc, whose cell layout this mirrors): rows of (o, d, tmin, tmax).
    Object k sits in cell k, centred at (8 (k % 10) - 36, 8 (k // 10) - 28, 8 ((k % 10 + k // 10) % 11) - 40): an axis-parallel ray through one cell
    meets no other, so no record carries another object's u, v or tangent (triangle::hit and constant_medium::hit leave them as they find them).  Every
    comment names the behaviour its rays pin.  Returns the rays and the rows of the exact face-normal ties."""
    INF = float("inf")
    R, ties = [], []

    def ray(o, d, tmin=0.001, tmax=INF):
        R.append([float(x) for x in o] + [float(x) for x in d] + [tmin, tmax])

    def tie(o, d):
        ties.append(len(R)); ray(o, d)

    def at(k):
        return np.array([8.0 * (k % 10) - 36.0, 8.0 * (k // 10) - 28.0, 8.0 * ((k % 10 + k // 10) % 11) - 40.0])

    def step(x, way, meets=None):
        """x one representable step up (+1) or down (-1).  The step is one unit in the last place of x or, where the ray meets the object at a coordinate
        `meets` of larger magnitude, of that: a smaller one is lost as soon as the hit point is written down in world coordinates, and the neighbour is
        the tie again for every form that is stored there"""
        return float(x + way * np.spacing(max(abs(x), abs(x if meets is None else meets))))

    def linear(ops):
        """the 3x3 matrix of a wrapper chain's object -> world map (innermost wrapper first) for quarter turns, scales and translates"""
        m = np.eye(3)
        for kind, a in ops:
            c, s = {0: (1, 0), 1: (0, 1), -1: (0, -1), 2: (-1, 0), 4: (1, 0)}[a] if kind in ("rx", "ry", "rz") else (0, 0)
            if kind == "rx":
                m = np.array([[1, 0, 0], [0, c, -s], [0, s, c]], float) @ m      # rotate_x.hpp:59-60
            elif kind == "ry":
                m = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]], float) @ m      # rotate_y.hpp:63-64
            elif kind == "rz":
                m = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], float) @ m      # rotate_z.hpp:56-57
            elif kind == "s":
                m = np.diag(a) @ m
        return m

    def place(ops, p):
        p = np.array(p, float)
        for k, (kind, a) in enumerate(ops):
            p = p + np.array(a, float) if kind == "t" else linear(ops[k:k + 1]) @ p
        return p

    def probe(a, axes=(0, 1, 2), dist=3.0):
        """axis-parallel rays from both sides towards the world point a"""
        for k in axes:
            e = np.zeros(3); e[k] = 1.0
            ray(a + dist * e, -e); ray(a - dist * e, e)

    # ---- face-normal ties on spheres (cells 0-9): the tangent ray x = centre + r, straight down -z, has discriminant exactly 0 and an outward normal
    # exactly perpendicular to it; a wrapper that calls set_face_normal again (translate, rotate_y) then ends with front_face = false and the OUTWARD normal
    for k, r in ((0, 1), (1, 1), (2, 2), (3, 1), (6, 1), (7, 1), (8, 1), (9, 1), (4, 1), (5, 1)):
        c = at(k)
        tie(c + (r, 0, 5), (0, 0, -1))                                          # the tie
        if k not in (4, 5):   # (|x| >= 8 there: one step of x moves the discriminant by whole units of its last place, whatever the contraction)
            ray((step(c[0] + r, -1), c[1], c[2] + 5), (0, 0, -1))               # one step inside: a grazing hit
            ray((step(c[0] + r, +1), c[1], c[2] + 5), (0, 0, -1))               # one step outside: a miss
        tie(c + (0, r, 5), (0, 0, -2))                                       # the same tie at the top, direction not unit
        probe(c, (2,))
    c = at(2)   # radius 2 under scale(2): t is the world ray's although the local direction is half as long — kat0's interval ends again (strict for a sphere)
    ray(c + (0, 0, 5), (0, 0, -1), 0.001, 3.0); ray(c + (0, 0, 5), (0, 0, -1), 0.001, 3.000001); ray(c + (0, 0, 5), (0, 0, -1), 3.0, INF)
    # ---- ... and on triangles with bent vertex normals (cells 10-16): at (0, -1/2, 0) vertex B weighs 1/2, the interpolated normal is (1, 0, 1) / sqrt 2 and
    # the direction (1, 0, -1) is exactly perpendicular to it while N.d = -1 for the geometric normal; from behind, (-1, 0, 1) ties the same way
    for k, f in ((10, 1), (11, 1), (12, 1), (13, 1), (14, 2), (15, 1), (16, 1)):
        c = at(k)
        h = c + f * np.array([0, -0.5, 0])
        tie(h + (-4, 0, 4), (1, 0, -1))                                     # the tie, front
        ray((step(h[0] - 4, -1, h[0]), h[1], h[2] + 4), (1, 0, -1)); ray((step(h[0] - 4, +1, h[0]), h[1], h[2] + 4), (1, 0, -1))   # one step to either side
        tie(h + (4, 0, -4), (-1, 0, 1))                                     # the tie, from behind
        ray((step(h[0] + 4, -1, h[0]), h[1], h[2] - 4), (-1, 0, 1)); ray((step(h[0] + 4, +1, h[0]), h[1], h[2] - 4), (-1, 0, 1))
        probe(h, (2,))
    c = at(14) + (-0.5, -1, 0)   # under scale(2), t = 3 exactly: contains() is inclusive for a triangle
    ray(c + (0, 0, 3), (0, 0, -1), 0.001, 3.0); ray(c + (0, 0, 3), (0, 0, -1), 0.001, 2.999999999); ray(c + (0, 0, 3), (0, 0, -1), 3.0, INF)
    # ---- exact angles (cells 20-64): rotate_x / rotate_y / rotate_z by 0, 90, -90, 180, 360 around a sphere, a cube and a triangle; the probes aim at the
    # round point where the turned centre lands (rotate_y's children sit on the axis)
    for axis, name in enumerate(("rx", "ry", "rz")):
        for j, quarter in enumerate((0, 1, -1, 2, 4)):
            for shape in range(3):
                off = (0, 0, 0) if axis == 1 else (1, 1, 0)
                inner = (0, -0.5, 0) if shape == 2 else (0, 0, 0)   # a point inside the triangle
                ops = [("t", off), (name, quarter), ("t", at(20 + (axis * 5 + j) * 3 + shape))]
                a = place(ops, inner)
                probe(a)
                if shape == 2:   # the triangle's plane after the turn: both faces along its normal
                    n = linear(ops) @ np.array([0, 0, 1.0])
                    ray(a + 2.5 * n + (0.125, 0.125, 0.125), -n); ray(a - 2.5 * n + (0.125, 0.125, 0.125), n)
    # ---- mirrors and extreme scales (cells 65-82) around an off-centre sphere, a triangle (both faces) and a cube (the placed-cube pattern)
    tiny, huge = 2.0 ** -20, 2.0 ** 20
    for i, f in enumerate(((-1, 1, 1), (1, -2, 1), (-1, -1, -1), (tiny,) * 3, (huge,) * 3, (1024.0, 1.0 / 1024.0, 1.0))):
        inv = 1.0 / np.abs(np.array(f)); r = inv.min()
        for shape in range(3):
            ops = [("s", f), ("t", at(65 + 3 * i + shape))]
            a = place(ops, (0.5 * r, 0.25 * r, 0) if shape == 0 else (0, -0.25 * inv[1], 0) if shape == 1 else (0, 0, 0))
            probe(a)
            ray(a + (0.0625, 0.03125, 3), (0, 0, -4)); ray(a + (0.0625, 0.03125, -3), (0, 0, 0.25))   # off the centre, directions of length 4 and 1/4
    c = at(68) + (0.25, -0.25, 0)   # sphere r = 1/2 under scale(1, -2, 1): the local direction is not unit, t = 4.5 at the pole z = 1/2; strict ends
    ray(c + (0, 0, 5), (0, 0, -1), 0.001, 4.5); ray(c + (0, 0, 5), (0, 0, -1), 0.001, 4.500001); ray(c + (0, 0, 5), (0, 0, -1), 4.5, INF)
    c = at(70) + (0.25, 0.125, 0)   # the cube beside it (half extents (1, 1/4, 3/4) x (1, -2, 1)): t = 4.25 on the face z = 3/4; tmax < tmin is what misses
    ray(c + (0, 0, 5), (0, 0, -1), 0.001, 4.25); ray(c + (0, 0, 5), (0, 0, -1), 0.001, 4.249999); ray(c + (0, 0, 5), (0, 0, -1), 4.25, INF)
    for k in (83, 84):              # translate -> rotate_y -> scale with negative factors, at angles that are nothing special
        probe(at(k)); ray(at(k) + (0.25, 0.125, 4), (0, 0, -1)); ray(at(k) + (3, 0.25, 3), (-1, 0, -1)); ray(at(k) + (-3, -0.125, 3), (1, 0, -1))
    # ---- order and depth (cells 85-92 and the origin)
    for k in (85, 86, 87, 88):      # translate(rotate_x(cube)) against rotate_x(translate(cube)); scale inside / outside rotate_z
        probe(at(k)); ray(at(k) + (0.25, 0.125, 4), (0, 0, -1)); ray(at(k) + (4, 0.375, 0.25), (-1, 0, 0)); ray(at(k) + (0.5, 4, 0.125), (0, -1, 0))
    a = at(89) + (0, 1, 0)          # eight wrappers (ZR_MAX_CHAIN): the sphere ends with radius 1 around cell + (0, 1, 0)
    probe(a); ray(a + (1, 0, 5), (0, 0, -1)); ray(a + (0.5, 0.25, 5), (0, 0, -1))
    for k in (90, 91, 92):          # nested material_instance, inside and outside a translate: the outer one wins
        probe(at(k), (2,)); ray(at(k) + (0.5, 0.25, 5), (0, 0, -1)); ray(at(k) + (1, 0, 5), (0, 0, -1))
    probe(np.zeros(3)); ray((0.25, 0.125, 5), (0, 0, -1))   # (the axes through the origin pass between the cells)
    # ---- media under wrappers (cells 93-99): from outside, from inside with d.x > 0 and d.x < 0 (translate re-faces the arbitrary (1, 0, 0) normal), with
    # ray_t.max inside the boundary, with a direction that is not unit, and along +-x from outside
    for k in range(93, 100):
        a = at(k) + ((-1, 1, 0) if k == 97 else (0, 0, 0))
        for rep in range(2):
            ray(a + (0, 0, 5), (0, 0, -1)); ray(a, (1, 0, 0)); ray(a, (-1, 0, 0)); ray(a + (0.125, 0, 0.25), (0.5, 0.25, -0.125))
            ray(a + (0, 0, 5), (0, 0, -1), 0.001, 5.0); ray(a + (0, 0, 5), (0, 0, -2)); ray(a + (-5, 0, 0.25), (1, 0, 0)); ray(a + (5, 0.125, 0.25), (-1, 0, 0))
            ray(a + (0, 5, 0.125), (0, -1, 0)); ray(a + (0, 0, 5), (0, 0, -1), 4.5, INF)
    # ---- a shared mesh under three chains (cells 100-102): a fan of four triangles around the origin in the plane y = 0 and a fin of two in the plane x = 0
    faces = [(0, 0, -0.5), (0.5, 0, 0), (0, 0, 0.5), (-0.5, 0, 0)]
    for k, ops in ((100, [("s", (-1, 1, 1))]), (101, [("rx", 1)]), (102, [("s", (2, 2, 2)), ("ry", 2)])):
        ops = ops + [("t", at(k))]
        m = linear(ops)
        down = m @ np.array([0, -1.0, 0]); side = m @ np.array([1.0, 0, 0])
        for q in faces:             # each fan face from below (its front is up) and, beside the fin, from above
            ray(place(ops, (q[0], -2, q[2])), -down)
            ray(place(ops, (q[0] + 0.25, 2, q[2] + 0.125)), down)
        for q in ((0, 0.75, -0.5), (0, 0.5, 0.5)):   # each fin face from both sides
            ray(place(ops, (2, q[1], q[2])), -side); ray(place(ops, (-2, q[1], q[2])), side)
        if k == 100:                # exact under the mirror: the shared vertex of all four fan faces, and the edge origin-c, from below
            ray(place(ops, (0, -2, 0)), -down); ray(place(ops, (0.5, -2, 0.5)), -down); ray(place(ops, (1, -2, 1)), -down); ray(place(ops, (1.0000001, -2, 1)), -down)
    # ---- between the cells: nothing there
    for k in range(0, 103, 3):
        ray(at(k) + (4, 4, 5), (0, 0, -1)); ray(at(k) + (4, 3.5, -5), (0.0078125, 0, 1))
    return np.array(R, dtype=np.float64), np.array(ties)


def make_kat1(tmp):
    rays, _ = kat1_inputs()
    f = os.path.join(tmp, "kat1_hits.bin"); pre = os.path.join(tmp, "kat1_hits")
    rays.tofile(f)
    meta = run("kat", "kat1", "hits", f, len(rays), pre)
    recs = np.load(pre + "_recs.npy")
    meta["rays_hit"] = int((recs[:, 0] > 0).sum())
    np.savez_compressed(os.path.join(HERE, "kat_kat1.npz"), meta=np.array(json.dumps({"hits": meta})), rays=rays, recs=recs, scat=np.load(pre + "_scat.npy"))
    print("kat_kat1", len(rays), "rays,", meta["rays_hit"], "hit,", os.path.getsize(os.path.join(HERE, "kat_kat1.npz")), "bytes")


def kat2_inputs():
    """Hand-placed rays of the lean known-answer fixture (scene "kat2", scenes/zr_scenes_mix.inc; layout and models: tests/shade_edge_worlds.py): rows of
    (o, d, 0.001, inf), ray k drawing from the stream (0x5EED3001, 0x7ACE, k).  Returns the rays, the rows of every class by name, and for the rows of the
    dielectric threshold the offset they were constructed at.  Every comment names what its rays pin."""
    import shade_edge_worlds as sw
    INF = float("inf")
    R, cls, delta = [], {}, {}
    at, tris, sphs = sw.at, sw.triangles(), sw.spheres()
    V = lambda *x: np.array(x, float)   # noqa: E731

    def ray(o, d, *tags):
        row = len(R)
        R.append([float(x) for x in o] + [float(x) for x in d] + [0.001, INF])
        for t in tags:
            cls.setdefault(t, []).append(row)
        return row

    def place(cell, q):
        """the world point of the local point q of a triangle cell (only form 6 turns: rotate_y.hpp:63-64 by 0.5, then the translate)"""
        if tris[cell][1] == 6:
            c, s = np.cos(0.5), np.sin(0.5)
            return np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]]) @ np.array(q, float) + at(cell)
        return at(cell) + np.array(q, float)

    # ---- face-normal ties on triangles, class (a): on the line x = 0 of a "bent" triangle vertex B weighs exactly 1/2, the interpolated normal is (s, 0, s) and
    # dot((a, y, -a), n) = a s - a s with both products exact for a = 1, 2; every form (0, 1 and 2 wrappers) x lambertian / metal / dielectric, both faces
    for cell in range(18):
        kind = tris[cell][2]
        for y in (-0.875, -0.75, -0.5, -0.25, -0.125):
            h = at(cell) + (0, y, 0)
            for a in (1.0, 2.0):
                ray(h + (-4, 0, 4), (a, 0, -a), "tie", "tie_a", "tie_a_" + kind); ray(h + (4, 0, -4), (-a, 0, a), "tie", "tie_a", "tie_a_" + kind)
    # ---- ... class (b): the same ties with a = k / 8 drawn by a seeded search, kept where a s rounds (the two rounded products still cancel exactly in the
    # reference's order; a fused multiply-add leaves the rounding error of one product, of either sign) and the model of triangle::hit confirms the tie
    rng = np.random.default_rng(20261019)
    for cell in range(18):
        kind = tris[cell][2]
        verts, normals = sw.tri_local(sw.BENT)
        verts = [v + at(cell) for v in verts]
        kept = 0
        while kept < 8:
            a = float(2 * rng.integers(1, 64) + 1) / 8.0
            y = float(rng.integers(1, 16)) / 16.0 - 1.0
            back = bool(rng.integers(0, 2))
            dy = float(rng.integers(-3, 4)) / 4.0   # the normal's y is exactly 0: any y of the direction leaves the tie
            h = at(cell) + (0, y, 0)
            d = V(-a, dy, a) if back else V(a, dy, -a)
            o = h - 4.0 * d
            m = sw.triangle_face(verts, normals, o, d)
            if m is None or m[3] != 0.0 or not sw.inexact_products(d, m[2]):
                continue
            ray(o, d, "tie", "tie_b", "tie_b_" + kind); kept += 1
    # ---- ... and on spheres.  Class (a): the tangent ray x = centre + r straight down -z (discriminant exactly 0, outward normal (1, 0, 0)), and at the top
    for cell, (kind, wrapped) in sphs.items():
        c = at(cell)
        ray(c + (1, 0, 5), (0, 0, -1), "tie", "tie_a", "tie_a_sphere"); ray(c + (0, 1, 5), (0, 0, -2), "tie", "tie_a", "tie_a_sphere")
    # Class (b): tangent rays along (a, 0, -a) at the point centre + (s, 0, s), s = sqrt(1/2) to within a few units in the last place, searched with the model
    # of sphere::hit, 20 000 candidates per sphere at the most (a fraction of a second): kept where the discriminant does not go negative, the products a n.x and a n.z round and still cancel
    found = 0
    rng = np.random.default_rng(20261020)
    s0 = float(np.sqrt(0.5))
    for cell in (40, 42, 48, 41, 43, 49):
        kept, tries = 0, 0
        while kept < 8 and tries < 20000:
            tries += 1
            a = float(2 * rng.integers(1, 1 << 25) + 1) / float(1 << 23)   # (26 bits: around |centre| ~ 40 the normal's components keep ~47, so a short a multiplies exactly)
            sx, sz = s0 + float(rng.integers(-3, 4)) * np.spacing(s0), s0 + float(rng.integers(-3, 4)) * np.spacing(s0)
            o = at(cell) + V(sx - 4 * a, 0, sz + 4 * a)
            d = V(a, 0, -a)
            # the reference meets a sphere under a translate in the translate's frame (translate.hpp: origin - offset), a bare one where it stands
            m = sw.sphere_face(np.zeros(3), 1.0, o - at(cell), d) if sphs[cell][1] else sw.sphere_face(at(cell), 1.0, o, d)
            if m is None or m[3] != 0.0 or not sw.inexact_products(d, m[2]):
                continue
            ray(o, d, "tie", "tie_b", "tie_b_sphere"); kept += 1; found += 1
    # ---- the dielectric threshold ri sin(theta) = 1 on the flat glass triangles (cells 18-25, bare and under a translate), for every index and face that has
    # one (ri > 1: index 1.5 and 2.4 from behind the bare triangle, index 1 / 1.5 from the front and, under the translate, from behind too; with index 1.0 ri sin(theta) never exceeds 1): sin(theta) = (1 / ri) stepped by
    # whole units in the last place, or (1 / ri)(1 + delta); six keys each, so that below the threshold both the reflect and the refract draw occur
    steps = [("0", 0, 0.0)] + [(f"{sg}{n}ulp", (1 if sg == "+" else -1) * n, 0.0) for n in (1, 2, 4) for sg in "+-"] + \
            [(f"{sg}{e:g}", 0, (1 if sg == "+" else -1) * e) for e in (1e-12, 1e-9, 1e-6) for sg in "+-"]
    for g, index in enumerate(sw.GLASS_INDEX):
        for cell in (18 + 2 * g, 19 + 2 * g):
            for front in (True, False):
                # (under the translate set_face_normal runs again on the turned normal and answers front_face = true from either side: translate.hpp:29)
                ri = (1.0 / index) if front or cell % 2 else index
                if not ri > 1.0:
                    continue
                hit = at(cell) + (0.125, -0.25, 0)
                for label, ulps, dl in steps:
                    s = 1.0 / ri
                    s = s + ulps * np.spacing(s) if ulps else s * (1.0 + dl)
                    d = V(s, 0, -np.sqrt(1.0 - s * s)) if front else V(s, 0, np.sqrt(1.0 - s * s))
                    for rep in range(6):
                        delta[ray(hit - 4.0 * d, d, "threshold")] = label
    # ---- exact normal incidence (ct == 1) on every flat glass triangle from both faces, with directions of length 1e-3, 1 and 1e3; the same lengths at an
    # oblique angle; and grazing incidence, ct = 1e-10 (the direction is long, because triangle::hit rejects |N.d| < 1e-8 before normalising)
    for cell in range(18, 26):
        hit = at(cell) + (0.125, -0.25, 0)
        for sgn in (1.0, -1.0):
            for ln in (1e-3, 1.0, 1e3):
                ray(hit + (0, 0, 4 * sgn), (0, 0, -sgn * ln), "normal_incidence", "unnormalised")
                ray(hit + V(-1.2, -0.4, 4 * sgn), ln * V(0.3, 0.1, -sgn), "unnormalised")
            ray(hit + V(-4, 0, 4e-10 * sgn), 1e3 * V(1, 0, -1e-10 * sgn), "grazing")
    # ---- ct clamped by fmin: rays through the centre of every glass sphere along seeded directions that are nothing special: dot(-unit(d), n) comes out a
    # unit in the last place above 1 on some of them
    rng = np.random.default_rng(20261021)
    for cell in range(48, 56):
        for k in range(24):
            w = rng.normal(size=3); w /= np.linalg.norm(w)
            ray(at(cell) + 5.0 * w, -w * (1.0, 0.125, 7.0)[k % 3], "central")
    # ---- metal: fuzz 0 at normal, 45 degree and grazing incidence on the flat mirror and the mirror spheres ...
    hit = at(26) + (0.125, -0.25, 0)
    for d in (V(0, 0, -1), V(1, 0, -1), V(1, 0, -1e-6), V(0, 0, 1), V(1, 0, 1)):
        ray(hit - 4.0 * d, d, "mirror")
    for cell in (42, 43):
        for o, d in (((0, 0, 5), (0, 0, -1)), ((np.sqrt(0.5), 0, 5), (0, 0, -1)), ((0.999999, 0, 5), (0, 0, -1))):
            ray(at(cell) + o, d, "mirror")
    # ... and fuzz 0.4 and 1 at grazing incidence on a hundred keys per sphere: the fuzzed reflection dips below the surface on some, scatter answers both ways
    for cell in (44, 45, 46, 47):
        for k in range(100):
            ray(at(cell) + (0.99, 0, 5), (0, 0, -1), "fuzzy_grazing")
    n27 = place(27, (0, 0, 1)) - at(27)   # the fuzzy triangle turned by 0.5 about y: along its normal from both sides, then low over its face on forty keys
    t27 = place(27, (1, 0, 0)) - at(27)
    a27 = place(27, (0.125, -0.25, 0))
    ray(a27 + 3.0 * n27, -n27, "turned"); ray(a27 - 3.0 * n27, n27, "turned")
    for k in range(40):
        ray(a27 + 1.0 * n27 - 3.0 * t27, 3.0 * t27 - 1.0 * n27, "turned", "fuzzy_grazing")
    # ---- vertex normals that oppose the face (cells 30-34; the interpolated normal's z changes sign at u = 5/9, x = 1/9): straight down, straight up and
    # obliquely on both sides of that line — a reflection about such a normal goes below the geometric face; four keys each for the fuzzed metals
    for cell in range(30, 35):
        for x in (-0.75, -0.5, -0.25, 0.0, 0.125, 0.25, 0.375):
            hit = at(cell) + (x, -0.5, 0)
            for d in (V(0, 0, -1), V(0, 0, 1), V(0.5, 0, -1), V(-0.5, 0.25, 1)):
                for rep in range(4 if cell in (31, 32) else 1):
                    ray(hit - 3.0 * d, d, "opposed")
    # ---- vertex normals that cancel (cells 35-37): on x = 0 the interpolated normal is 0, unit_vector answers (0, 0, 0) (its `< 1e-8` branch) and front_face is
    # false with a normal of zeros; a step of 2^-30 to either side it is (0, 0, +-1) again
    for cell in (35, 36, 37):
        for x in (0.0, 2.0 ** -30, -2.0 ** -30):
            for y in (-0.5, -0.25):
                ray(at(cell) + (x, y, 3), (0, 0, -1), "cancel"); ray(at(cell) + (x, y, -3), (0, 0, 1), "cancel"); ray(at(cell) + (x - 1.5, y, 3), (0.5, 0, -1), "cancel")
    # ---- lambertian's degenerate direction, reached on purpose: the unit vector ray k draws depends on k alone, so ray k goes straight at the point of a
    # lambertian sphere (bare, and under a translate) whose outward normal is -ruv(k): normal + ruv is ~1e-16 in every component and the direction falls
    # back to the normal; its neighbour arrives 1e-7 to the side, where the sum is ~1e-7 and must stand
    for k in range(16):
        for near in (False, True):
            row = len(R)
            ruv, _ = sw.random_unit_vector(sw.kat_key(row))
            if near:
                side = np.cross(ruv, V(0, 0, 1) if abs(ruv[2]) < 0.9 else V(1, 0, 0)); side /= np.linalg.norm(side)
                w = ruv + 1e-7 * side; w /= np.linalg.norm(w)
            else:
                w = ruv
            ray(at(40 + k % 2) - 5.0 * w, w, "lambert_near" if near else "lambert_fallback")
    # ---- triangle hit positions: the vertices, the edge midpoints and the centroid of every triangle from both faces (the turned one: its centroid and a
    # point beside it only — its baked vertices are rounded, and which side of an edge such a ray passes is the reference's local arithmetic)
    for cell, (shape, form, kind) in sorted(tris.items()):
        verts, _ = sw.tri_local(shape)
        a, b, c = verts
        pts = [(a + b + c) / 3.0, (a + b + c) / 3.0 + (0.0625, 0.03125, 0)] if form == 6 else [a, b, c, (a + b) / 2, (b + c) / 2, (c + a) / 2, (a + b + c) / 3.0]
        nrm = place(cell, (0, 0, 1)) - at(cell)
        for q in pts:
            ray(place(cell, q) + 3.0 * nrm, -nrm, "tri_positions"); ray(place(cell, q) - 3.0 * nrm, nrm, "tri_positions")
    # ---- sphere hit positions: the poles, the equator, from outside and from inside, on every sphere (the light, the one without a material and the one with
    # a negative radius, which nothing hits, among them)
    for cell in list(sphs) + [58]:
        c = at(cell) + ((0.125, 0.0625, 0.25) if cell == 58 else (0, 0, 0))   # (beside the centre there: a ray through the centre of a sphere of radius 0 "hits" it with a normal of NaNs)
        for e in (V(1, 0, 0), V(0, 1, 0), V(0, 0, 1)):
            ray(c + 5.0 * e, -e, "sphere_positions"); ray(c - 5.0 * e, e, "sphere_positions")
            ray(c, e, "sphere_positions", "sphere_inside"); ray(c + (0.25, 0.125, -0.5), -0.5 * e, "sphere_positions", "sphere_inside")
        ray(c + (0.5, 0.25, 5), (0, 0, -1), "sphere_positions")
    # ---- between the cells: nothing there
    for k in range(0, 60, 4):
        ray(at(k) + (4, 4, 5), (0, 0, -1), "between")
    return np.array(R, dtype=np.float64), {k: np.array(v) for k, v in cls.items()}, delta, found


def make_kat2(tmp):
    rays, cls, delta, found = kat2_inputs()
    f = os.path.join(tmp, "kat2_hits.bin"); pre = os.path.join(tmp, "kat2_hits")
    rays.tofile(f)
    meta = run("kat", "kat2", "hits", f, len(rays), pre)
    recs = np.load(pre + "_recs.npy")
    meta["rays_hit"] = int((recs[:, 0] > 0).sum())
    meta["sphere_ties_b"] = found   # class (b) ties on spheres the search found (0: none among its candidates)
    meta["absent"] = ("bent normals with dot(-unit(d), n) < 0 (1 - ct > 1): set_face_normal (hittable.hpp:22-25) always leaves the normal against the ray, and a "
                      "lean world has no bump map to replace it, so no record of this world has it; it occurs by rounding on the ties only, which are here")
    out = os.path.join(HERE, "kat_kat2.npz")
    np.savez_compressed(out, meta=np.array(json.dumps({"hits": meta})), rays=rays, recs=recs, scat=np.load(pre + "_scat.npy"))
    print("kat_kat2", len(rays), "rays,", meta["rays_hit"], "hit,", {k: len(v) for k, v in cls.items()}, os.path.getsize(out), "bytes")


def make_refdemo(tmp):
    """The reference's OWN demo world (load_materials + sceneAssetsLoader + build_geometry, scene_management.hpp:28-236) for the GPU: the scene reads the
    reference's assets/ at run time, which never travel — so the world travels FLATTENED.  oracle/_ref/refscene_dropin (the reference's scene code compiled
    unchanged against the drop-in) dumps every array of the zr_scene_desc it flattens to (decoded texels included), oracle/_ref/zenith_ref (the same scene
    code against the reference's own headers) renders the full frame at 8 spp and two tiles at the scene's 16 spp.  tests/test_refdemo_gpu.py commits the
    arrays through the C ABI and compares."""
    from refdemo_assets import REF as REF_TREE, asset_dir
    dropin = os.path.join(ROOT, "oracle", "_ref", "refscene_dropin")
    os.makedirs(os.path.join(tmp, "refdemo_cwd"))
    cwd = asset_dir(os.path.join(tmp, "refdemo_cwd"), ref=REF_TREE)
    pre = os.path.join(tmp, "refdemo_d")
    p = subprocess.run([dropin, "dump", pre], cwd=cwd, capture_output=True, text=True, check=True)
    meta = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    names = ["spheres", "sphere_mat", "tri_v", "tri_n", "tri_mat", "cubes", "cube_mat", "media", "ops", "objects", "groups", "materials", "textures", "texels", "camera", "env"]
    arrays = {n: np.load(f"{pre}_{n}.npy") for n in names}
    np.savez_compressed(os.path.join(HERE, "refdemo_scene.npz"), meta=np.array(json.dumps(meta)), **arrays)
    print("refdemo_scene", meta)
    frames = {}
    for name, (x0, y0, w, h, spp) in {"full8": (0, 0, 640, 360, 8), "tile_a": (40, 250, 24, 16, 16), "tile_b": (300, 150, 32, 24, 16)}.items():
        out = os.path.join(tmp, "refdemo_" + name)
        r = subprocess.run([REF, "tile", "refdemo", str(x0), str(y0), str(w), str(h), str(spp), str(os.cpu_count() or 1), out, "0"], cwd=cwd, capture_output=True, text=True, check=True)
        m = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        frames[name] = np.load(out + "_mean.npy"); frames[name + "_meta"] = np.array(json.dumps(m))
        print("refdemo", name, m)
    np.savez_compressed(os.path.join(HERE, "refdemo_frames.npz"), **frames)


def run(*args):
    p = subprocess.run([REF] + [str(a) for a in args], capture_output=True, text=True, check=True)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/zenith_ref missing: run `make -C oracle ref` (needs /root/reference)")
    want = set(sys.argv[1:])
    with tempfile.TemporaryDirectory() as tmp:
        for name, (scene, x0, y0, w, h, spp, ps, extra) in TILES.items():
            if want and name not in want and scene not in want:
                continue
            pre = os.path.join(tmp, name)
            meta = run("tile", scene, x0, y0, w, h, spp, os.cpu_count() or 1, pre, 1 if ps else 0, *extra)
            meta["scene_args"] = extra
            arrays = {"mean": np.load(pre + "_mean.npy"), "meta": np.array(json.dumps(meta))}
            if ps:
                arrays["samples"] = np.load(pre + "_samples.npy")
                arrays["counts"] = np.load(pre + "_counts.npy")
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)
            print(name, meta)
        for name, spec in TRACES.items():
            scene, n, seed, clo, chi, extra = spec[:6]
            adv = len(spec) > 6 and spec[6]
            if want and name not in want and scene not in want:
                continue
            pre = os.path.join(tmp, name)
            if adv:
                os.environ["ZR_TRACE_ADVERSARIAL"] = "1"
            else:
                os.environ.pop("ZR_TRACE_ADVERSARIAL", None)
            meta = run("trace", scene, n, seed, pre, clo, chi, *extra)
            os.environ.pop("ZR_TRACE_ADVERSARIAL", None)
            meta["scene_args"] = extra
            meta["adversarial"] = bool(adv)
            np.savez_compressed(os.path.join(HERE, name + ".npz"), rays=np.load(pre + "_rays.npy"),
                                recs=np.load(pre + "_recs.npy"), meta=np.array(json.dumps(meta)))
            print(name, meta)
        for name, (scene, x0, y0, w, h, zmax, extra) in AOVS.items():
            if want and name not in want and scene not in want:
                continue
            pre = os.path.join(tmp, name)
            meta = run("aov", scene, x0, y0, w, h, zmax, pre, "-", *extra)
            meta["scene_args"] = extra
            np.savez_compressed(os.path.join(HERE, name + ".npz"), albedo=np.load(pre + "_albedo.npy"), normal=np.load(pre + "_normal.npy"),
                                zdepth=np.load(pre + "_zdepth.npy"), meta=np.array(json.dumps(meta)))
            print(name, meta)
        for name, (scene, x0, y0, w, h, spp, extra) in PASSES.items():
            if want and name not in want and scene not in want:
                continue
            pre = os.path.join(tmp, name)
            meta = run("passes", scene, x0, y0, w, h, spp, pre, *extra)
            meta["scene_args"] = extra
            np.savez_compressed(os.path.join(HERE, name + ".npz"), beauty=np.load(pre + "_beauty.npy"), reflection=np.load(pre + "_reflection.npy"),
                                refraction=np.load(pre + "_refraction.npy"), meta=np.array(json.dumps(meta)))
            print(name, meta)
        for name, (scene, spp, presets) in POSTS.items():
            if want and name not in want and scene not in want:
                continue
            arrays, metas = {}, []
            for k in presets:
                pre = os.path.join(tmp, f"{name}_{k}")
                meta = run("post", scene, k, pre, spp)
                metas.append(meta)
                arrays["frame"] = np.load(pre + "_frame.npy")      # the same input frame for every preset
                arrays[f"rgb8_{k}"] = np.load(pre + "_rgb8.npy")
                arrays["hist"] = np.load(pre + "_hist.npy")
            np.savez_compressed(os.path.join(HERE, name + ".npz"), meta=np.array(json.dumps(metas)), **arrays)
            print(name, [m["preset"] for m in metas])
        if not want or "post_edges" in want:
            make_post_edges(tmp)
        if not want or "refdemo" in want:
            from refdemo_assets import store
            store()   # tests/golden/refdemo_assets.npz: the images tests/test_refdemo.py gives the scene code
            make_refdemo(tmp)
        if not want or "kat" in want or "kat0" in want:
            make_kat(tmp)
        if not want or "kat" in want or "kat1" in want:
            make_kat1(tmp)
        if not want or "kat" in want or "kat2" in want:
            make_kat2(tmp)
        if not want or "texels" in want:
            out = os.path.join(tmp, "texels.npy")
            subprocess.run([REF, "texels", "64", "32", out], check=True)
            np.savez_compressed(os.path.join(HERE, "texels_hdr_64x32.npz"), texels=np.load(out))
            print("texels 64x32")


if __name__ == "__main__":
    main()
