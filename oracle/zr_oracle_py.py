"""zr_oracle_py — TEST INFRASTRUCTURE.  ctypes view of the CPU restatement (oracle/libzr_oracle.so) and of the
genuine-reference harness binary (oracle/_ref/zenith_ref).

May only be imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg, and only as the
checker / reported baseline — never by the product path (raytracer_project_amd/).
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np

from raytracer_project_amd import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_LIB = os.path.join(_HERE, "libzr_oracle.so")
REF_BIN = os.path.join(_HERE, "_ref", "zenith_ref")

_lib = None


def build():
    subprocess.run(["make", "-s", "-C", _HERE, "all"], check=True)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(ORACLE_LIB):
        build()
    lib = C.CDLL(ORACLE_LIB)
    vp = C.c_void_p
    lib.zro_scene_create.restype = vp
    lib.zro_scene_create.argtypes = [C.POINTER(capi.SceneDesc)]
    lib.zro_scene_destroy.argtypes = [vp]
    lib.zro_render.argtypes = [vp, C.POINTER(capi.Camera), C.POINTER(capi.Env), C.c_uint64, C.POINTER(capi.Region),
                               C.c_int, vp, vp, vp, C.POINTER(capi.Counters)]
    lib.zro_render_aov.argtypes = [vp, C.POINTER(capi.Camera), C.c_uint64, C.POINTER(capi.Region), C.c_double, vp, vp, vp]
    lib.zro_render_passes.argtypes = [vp, C.POINTER(capi.Camera), C.POINTER(capi.Env), C.c_uint64, C.POINTER(capi.Region), vp, vp, vp,
                                      C.POINTER(capi.Counters)]
    lib.zro_trace_paths.argtypes = [vp, C.POINTER(capi.Camera), C.c_uint64, vp, C.c_int, C.c_int, vp]
    lib.zro_post_process.argtypes = [C.POINTER(capi.PostParams), vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.zro_analyze_frame.argtypes = [vp, C.c_size_t, C.POINTER(capi.ImageStats)]
    lib.zro_auto_exposure.restype = C.c_double
    lib.zro_auto_exposure.argtypes = [C.c_float, C.c_float, C.c_int, C.c_float, C.c_float]
    lib.zro_trace.argtypes = [vp, vp, C.c_size_t, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_uint32, vp]
    lib.zro_scatter.argtypes = [vp, vp, vp, C.c_uint64, vp, vp]
    lib.zro_kat_scatter.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.zro_kat_texture.argtypes = [vp, C.c_uint32, vp, C.c_size_t, vp]
    lib.zro_kat_background.argtypes = [vp, C.POINTER(capi.Env), vp, C.c_size_t, vp]
    lib.zro_kat_camera_rays.argtypes = [C.POINTER(capi.Camera), C.c_uint64, vp, C.c_size_t, vp]
    _lib = lib
    return lib


class OracleScene:
    """The CPU restatement over a flattened scene (the arrays must outlive this object)."""

    def __init__(self, desc):
        self.lib = load()
        self._keep = desc
        self._s = self.lib.zro_scene_create(C.byref(desc))
        if not self._s:
            raise ValueError("the oracle refuses this scene: a texture tree with a cycle or more than 15 checkers above a leaf")

    def render(self, camera, env, seed, region=None, threads=None, per_sample=False):
        """Returns (frame[H,W,3], counters, samples[h,w,spp,3] | None, counts[h,w,spp,2] | None)."""
        h, w, spp = camera.image_height, camera.image_width, camera.samples_per_pixel
        out = np.zeros((h, w, 3), dtype=np.float64)
        rw, rh = (region.w, region.h) if region is not None and region.w > 0 else (w, h)
        samples = np.zeros((rh, rw, spp, 3), dtype=np.float64) if per_sample else None
        counts = np.zeros((rh, rw, spp, 2), dtype=np.uint32) if per_sample else None
        ctr = capi.Counters()
        threads = threads or min(16, os.cpu_count() or 1)
        rc = self.lib.zro_render(self._s, C.byref(camera), C.byref(env), C.c_uint64(seed),
                                 C.byref(region) if region is not None else None, threads, out.ctypes.data,
                                 samples.ctypes.data if per_sample else None, counts.ctypes.data if per_sample else None,
                                 C.byref(ctr))
        if rc != 0:
            raise RuntimeError(f"oracle render failed: {rc}")
        return out, ctr, samples, counts

    def render_aov(self, camera, seed, region, zmax):
        outs = [np.zeros((region.h, region.w, 3), dtype=np.float64) for _ in range(3)]
        self.lib.zro_render_aov(self._s, C.byref(camera), C.c_uint64(seed), C.byref(region), float(zmax), outs[0].ctypes.data,
                                outs[1].ctypes.data, outs[2].ctypes.data)
        return outs

    def trace_paths(self, camera, seed, requests, max_segments):
        req = np.ascontiguousarray(requests, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((req.shape[0], max_segments, 17), dtype=np.float64)
        self.lib.zro_trace_paths(self._s, C.byref(camera), C.c_uint64(seed), req.ctypes.data, req.shape[0], max_segments, out.ctypes.data)
        return out

    def render_passes(self, camera, env, seed, region):
        """beauty / reflection / refraction tiles (region-sized) + counters"""
        outs = [np.zeros((region.h, region.w, 3), dtype=np.float64) for _ in range(3)]
        ctr = capi.Counters()
        self.lib.zro_render_passes(self._s, C.byref(camera), C.byref(env), C.c_uint64(seed), C.byref(region), outs[0].ctypes.data,
                                   outs[1].ctypes.data, outs[2].ctypes.data, C.byref(ctr))
        return outs, ctr

    def trace(self, rays, tmin=0.001, tmax=float("inf"), seed=1, pixel=0x7ACE, bounce=0):
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        out = np.zeros(rays.shape[0], dtype=capi.HIT_DTYPE)
        self.lib.zro_trace(self._s, rays.ctypes.data, rays.shape[0], tmin, tmax, C.c_uint64(seed), C.c_uint64(pixel), bounce,
                           out.ctypes.data)
        return out

    def scatter(self, ray, hit, key):
        att = np.zeros(3); out = np.zeros(6)
        ray = np.ascontiguousarray(ray, dtype=np.float64)
        h = np.ascontiguousarray(hit)
        ok = self.lib.zro_scatter(self._s, ray.ctypes.data, h.ctypes.data, C.c_uint64(key), att.ctypes.data, out.ctypes.data)
        return bool(ok), att, out

    # ---- per-function known answers (the CPU side of capi.Scene.kat_*) ----
    def kat_scatter(self, rays, hits, keys, first_draw=None):
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        hits = np.ascontiguousarray(hits, dtype=capi.HIT_DTYPE)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        fd = np.ascontiguousarray(first_draw, dtype=np.uint64) if first_draw is not None else None
        out = np.zeros(len(rays), dtype=capi.SCATTER_DTYPE)
        rc = self.lib.zro_kat_scatter(self._s, rays.ctypes.data, hits.ctypes.data, keys.ctypes.data, fd.ctypes.data if fd is not None else None,
                                      len(rays), out.ctypes.data)
        assert rc == 0
        return out

    def kat_texture(self, tex, uvp):
        uvp = np.ascontiguousarray(uvp, dtype=np.float64).reshape(-1, 5)
        out = np.zeros((len(uvp), 3))
        assert self.lib.zro_kat_texture(self._s, int(tex), uvp.ctypes.data, len(uvp), out.ctypes.data) == 0
        return out

    def kat_background(self, env, dirs):
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        out = np.zeros((len(dirs), 3))
        assert self.lib.zro_kat_background(self._s, C.byref(env), dirs.ctypes.data, len(dirs), out.ctypes.data) == 0
        return out

    def close(self):
        if self._s:
            self.lib.zro_scene_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kat_camera_rays(camera, seed, requests):
    """camera::initialize + get_ray of the CPU restatement: (n, 7) = origin, direction, draws"""
    req = np.ascontiguousarray(requests, dtype=np.int32).reshape(-1, 3)
    out = np.zeros((len(req), 7))
    assert load().zro_kat_camera_rays(C.byref(camera), C.c_uint64(seed), req.ctypes.data, len(req), out.ctypes.data) == 0
    return out


def post_process(params, frame, is_data_pass=False, apply_gamma=True):
    """CPU restatement of the post stack (zr_post_oracle.cpp)"""
    frame = np.ascontiguousarray(frame, dtype=np.float64)
    h, w = frame.shape[:2]
    out = np.zeros((h, w, 3), dtype=np.uint8)
    load().zro_post_process(C.byref(params), frame.ctypes.data, w, h, int(is_data_pass), int(apply_gamma), out.ctypes.data)
    return out


def analyze_frame(frame):
    frame = np.ascontiguousarray(frame, dtype=np.float64)
    st = capi.ImageStats()
    load().zro_analyze_frame(frame.ctypes.data, frame.size // 3, C.byref(st))
    return st


def auto_exposure(average_luminance, exposure, use_auto_exposure, target_luminance=0.12, compensation_stops=0.0):
    return load().zro_auto_exposure(average_luminance, exposure, int(use_auto_exposure), target_luminance, compensation_stops)


def ref_available():
    return os.path.exists(REF_BIN) and os.access(REF_BIN, os.X_OK)


def ref_run(*args, timeout=3600):
    """Runs the genuine-reference harness (prebuilt in this container from /root/reference) and parses its JSON line."""
    p = subprocess.run([REF_BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, check=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


MASK64 = (1 << 64) - 1


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def stream_key(seed, pixel, sample):
    g = 0x9E3779B97F4A7C15
    return mix64((mix64((seed + g * (pixel + 1)) & MASK64) + g * (sample + 1)) & MASK64)
