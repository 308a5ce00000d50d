"""ctypes view of the C ABI (include/zr_capi.h) — the Python host side of the drop-in.

The reference has no Python; this module exists because the measurement harness (bench.py), the parity
tests and the multi-GPU host (one process per GPU, torch.distributed over RCCL) are Python.  It binds
exactly the entry points include/zr_capi.h declares and adds no arithmetic of its own.

There is no CPU fallback: if libzr_hip.so is missing, `load()` raises; if no HIP device is present,
`Context()` raises with the library's own message.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZR_LIB: development override (scripts/ab_flags.sh, scripts/wave_profile.sh build experimental variants out of tree)
LIB_PATH = os.environ.get("ZR_LIB") or os.path.join(_HERE, "csrc", "libzr_hip.so")
SCENES_LIB_PATH = os.path.join(_HERE, "csrc", "libzr_scenes.so")

ZR_OK, ZR_E_INVALID, ZR_E_DEVICE, ZR_E_STATE, ZR_E_CANCELLED, ZR_E_NOMEM = 0, -1, -2, -3, -4, -5
NO_TEXTURE = 0xFFFFFFFF


class XformOp(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("mat", C.c_uint32), ("a", C.c_double * 3)]


class Object(C.Structure):
    _fields_ = [("type", C.c_uint32), ("index", C.c_uint32), ("chain_first", C.c_uint32), ("chain_count", C.c_uint32)]


class Medium(C.Structure):
    _fields_ = [("boundary_type", C.c_uint32), ("boundary_index", C.c_uint32), ("chain_first", C.c_uint32),
                ("chain_count", C.c_uint32), ("mat", C.c_uint32), ("pad_", C.c_uint32), ("neg_inv_density", C.c_double)]


class Material(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("tex", C.c_uint32), ("bump_tex", C.c_uint32), ("pad_", C.c_uint32),
                ("param", C.c_double), ("bump_strength", C.c_double), ("tint", C.c_double * 3)]


class Texture(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("odd", C.c_uint32), ("even", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("pad_", C.c_uint32), ("texel_offset", C.c_uint64), ("inv_scale", C.c_double),
                ("color", C.c_double * 3)]


class Env(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("hdr_texture", C.c_uint32), ("background_color", C.c_double * 3),
                ("intensity", C.c_double), ("hdri_rotation", C.c_double), ("hdri_tilt", C.c_double),
                ("hdri_roll", C.c_double), ("sun_direction", C.c_double * 3), ("sun_color", C.c_double * 3),
                ("sun_intensity", C.c_double), ("sun_size", C.c_double)]


class Camera(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("samples_per_pixel", C.c_int32),
                ("max_depth", C.c_int32), ("vfov", C.c_double), ("lookfrom", C.c_double * 3), ("lookat", C.c_double * 3),
                ("vup", C.c_double * 3), ("defocus_angle", C.c_double), ("focus_dist", C.c_double)]

    def copy(self):
        c = Camera()
        C.memmove(C.byref(c), C.byref(self), C.sizeof(Camera))
        return c


class Region(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("tile_size", C.c_int32),
                ("tile_mod", C.c_int32), ("tile_rem", C.c_int32), ("tile_skew", C.c_int32)]


class _Defaults:
    """defaults(**kw) of a parameter struct: the class's _defaults_ in field order, then the fields named in kw (an unknown name raises AttributeError)"""
    _defaults_ = ()

    @classmethod
    def defaults(cls, **kw):
        p = cls(*cls._defaults_)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(f"{cls.__name__} has no field {k!r}")
            setattr(p, k, v)
        return p


class PostParams(_Defaults, C.Structure):
    """zr_post_params: post_processor's fields (color_processing.hpp:46-75); defaults are the reference's"""
    _fields_ = [("exposure", C.c_float), ("saturation", C.c_float), ("contrast", C.c_float), ("hue_shift", C.c_float),
                ("vignette_intensity", C.c_float), ("bloom_threshold", C.c_float), ("bloom_intensity", C.c_float), ("bloom_radius", C.c_int32),
                ("color_balance", C.c_double * 3), ("sharpen_amount", C.c_double), ("use_aces_tone_mapping", C.c_int32),
                ("use_bloom", C.c_int32), ("use_sharpening", C.c_int32), ("debug_red", C.c_int32), ("debug_green", C.c_int32),
                ("debug_blue", C.c_int32), ("debug_luminance", C.c_int32), ("debug_bvh", C.c_int32)]

    _defaults_ = (0.5, 1.0, 1.0, 0.0, 1.0, 1.0, 0.3, 4, (1.0, 1.0, 1.0), 0.2, 0, 0, 0, 0, 0, 0, 0, 0)

    @classmethod
    def defaults(cls, **kw):
        """color_balance takes any three numbers; debug=(red, green, blue, luminance, bvh) sets the five debug flags"""
        debug = kw.pop("debug", None)
        if "color_balance" in kw:
            kw["color_balance"] = (C.c_double * 3)(*kw["color_balance"])
        p = super().defaults(**kw)
        if debug is not None:
            p.debug_red, p.debug_green, p.debug_blue, p.debug_luminance, p.debug_bvh = [int(x) for x in debug]
        return p


class DenoiseParams(_Defaults, C.Structure):
    """zr_denoise_params: the a-trous denoiser behind camera::use_denoiser (not OIDN; include/zr_capi.h)"""
    _fields_ = [("iterations", C.c_int32), ("demodulate_albedo", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float)]

    # defaults(): ZR_DENOISE_DEFAULT_* of include/zr_capi.h (what the drop-in's camera::render uses); depth guide off
    _defaults_ = (5, 0, 1.5, 64.0, 0.25, 0.0)


class DenoiseGuidedParams(_Defaults, C.Structure):
    """zr_denoise_guided_params: the variance-guided form of the a-trous denoiser (include/zr_capi.h)"""
    _fields_ = [("iterations", C.c_int32), ("demodulate_albedo", C.c_int32), ("sigma_variance", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float), ("epsilon", C.c_float)]

    # defaults(): ZR_DENOISE_GUIDED_DEFAULT_* of include/zr_capi.h (what the drop-in's camera::render uses with denoise_variance_guided); depth guide off
    _defaults_ = (4, 1, 3.0, 64.0, 0.25, 0.0, 1e-8)


class DenoiseNlmParams(_Defaults, C.Structure):
    """zr_denoise_nlm_params: the dual-buffer non-local-means denoiser (include/zr_capi.h)"""
    _fields_ = [("search_radius", C.c_int32), ("patch_radius", C.c_int32), ("demodulate_albedo", C.c_int32), ("pad_", C.c_int32), ("k", C.c_float),
                ("alpha", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float), ("epsilon", C.c_float)]

    # defaults(): ZR_DENOISE_NLM_DEFAULT_* of include/zr_capi.h (what the drop-in's camera::render uses with denoise_nlm)
    _defaults_ = (7, 1, 0, 0, 0.7, 1.0, 64.0, 0.25, 1e-10)


class TemporalParams(_Defaults, C.Structure):
    """zr_temporal_params: how a frame's history is reprojected and blended (include/zr_capi.h)"""
    _fields_ = [("alpha", C.c_double), ("max_history", C.c_int32), ("pad_", C.c_int32), ("plane_tolerance", C.c_double), ("normal_cos", C.c_double)]

    # defaults(): ZR_TEMPORAL_DEFAULT_* of include/zr_capi.h (what the drop-in's camera::render uses with temporal_accumulation)
    _defaults_ = (0.4, 32, 0, 0.03, 0.9)


ROBUST_GINI, ROBUST_FIXED = 0, 1
ROBUST_DEFAULT_STRENGTH = 1.0   # ZR_ROBUST_DEFAULT_STRENGTH of include/zr_capi.h


class RobustParams(_Defaults, C.Structure):
    """zr_robust_params: the firefly-robust resolve (include/zr_capi.h); mode ROBUST_GINI reads strength, ROBUST_FIXED reads trim"""
    _fields_ = [("mode", C.c_int32), ("trim", C.c_int32), ("strength", C.c_double)]

    # defaults(): Gini mode at ZR_ROBUST_DEFAULT_STRENGTH (what the drop-in's camera::render uses with robust_resolve)
    _defaults_ = (ROBUST_GINI, 0, ROBUST_DEFAULT_STRENGTH)


DIRECT_EMITTERS, DIRECT_SUN = 1, 2
DIRECT_MAX_SLOTS = 1 << 22
DIRECT_T_TOL = 1e-7
LIGHT_SPHERE, LIGHT_TRIANGLE, LIGHT_PARALLELOGRAM = 0, 1, 2


class DirectParams(_Defaults, C.Structure):
    """zr_direct_params: what the direct-light integrator samples (include/zr_capi.h): DIRECT_EMITTERS | DIRECT_SUN"""
    _fields_ = [("flags", C.c_uint32), ("pad_", C.c_uint32)]

    # defaults(): emitters and the sun
    _defaults_ = (DIRECT_EMITTERS | DIRECT_SUN, 0)


class DirectStats(C.Structure):
    """zr_direct_stats: the shadow queries of the last counted direct batch and the light table it used"""
    _fields_ = [("shadow_queries", C.c_uint64), ("shadow_visible", C.c_uint64), ("sun_queries", C.c_uint64), ("slots", C.c_uint64),
                ("sampled_objects", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


LIGHT_SLOT_DTYPE = np.dtype([("type", "<u4"), ("kind", "<u4"), ("index", "<u4"), ("face", "<u4"), ("o", "<f8", 3), ("e1", "<f8", 3), ("e2", "<f8", 3),
                             ("area", "<f8"), ("lum", "<f8"), ("weight", "<f8"), ("cdf", "<f8")])
LIGHT_SAMPLE_DTYPE = np.dtype([("choice", "<u4"), ("slot", "<u4"), ("kind", "<u4"), ("index", "<u4"), ("draws", "<u4"), ("pad_", "<u4"), ("y", "<f8", 3),
                               ("normal", "<f8", 3), ("w", "<f8", 3), ("dist", "<f8"), ("pdf", "<f8")])


DIRECT_ENV_MAX_TEXELS = 1 << 25


class EnvLightInfo(C.Structure):
    """zr_env_light_info: the environment table of a scene and an environment (include/zr_capi.h)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("sampled", C.c_uint32), ("pad_", C.c_uint32), ("total", C.c_double), ("weighted", C.c_uint64),
                ("build_ms", C.c_double)]


class BvhDebugParams(_Defaults, C.Structure):
    """zr_bvh_debug_params: global_settings::debug_bvh_level / bvh_thickness of the BVH debug view (include/zr_capi.h)"""
    _fields_ = [("level", C.c_int32), ("thickness", C.c_float)]

    # defaults(): ZR_BVH_DEBUG_DEFAULT_LEVEL / _THICKNESS (the reference's global_settings defaults: leaves, 0.01)
    _defaults_ = (-1, 0.01)


BVH_MISS, BVH_EDGE, BVH_VOLUME, BVH_SURFACE = 0, 1, 2, 3
BVH_ROOT_BOX, BVH_NO_BOX = 0x80000000, 0xFFFFFFFF


class ImageStats(C.Structure):
    _fields_ = [("average_luminance", C.c_float), ("max_luminance", C.c_float), ("histogram", C.c_int32 * 256)]


class Counters(C.Structure):
    _fields_ = [("primary_samples", C.c_uint64), ("segments", C.c_uint64), ("nodes_tested", C.c_uint64),
                ("spheres_tested", C.c_uint64), ("triangles_tested", C.c_uint64), ("cubes_tested", C.c_uint64),
                ("media_tested", C.c_uint64), ("hits", C.c_uint64), ("rng_draws", C.c_uint64),
                ("node_execs", C.c_uint64), ("node_lanes", C.c_uint64), ("leaf_execs", C.c_uint64), ("leaf_lanes", C.c_uint64),
                ("shade_execs", C.c_uint64), ("shade_lanes", C.c_uint64), ("rounds", C.c_uint64),
                ("extend_ms", C.c_double), ("shade_ms", C.c_double), ("kernel_ms", C.c_double), ("path", C.c_uint64),
                ("escaped", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}

    def algorithmic_bytes(self):
        """32 B per child box tested, 72 B per triangle (9 f64 vertices), 32 B per sphere,
        48 B per cube (6 f64: this layout keeps half extents + centre only), 76 B of shading data per hit."""
        return (32 * self.nodes_tested + 72 * self.triangles_tested + 32 * self.spheres_tested
                + 48 * self.cubes_tested + 76 * self.hits)


class AdaptiveParams(_Defaults, C.Structure):
    """zr_adaptive_params: the three counts are positive multiples of 64; a pixel goes on while err > threshold"""
    _fields_ = [("min_samples", C.c_int32), ("max_samples", C.c_int32), ("step_samples", C.c_int32), ("pad_", C.c_int32),
                ("threshold", C.c_double), ("dark_floor", C.c_double)]

    _defaults_ = (64, 512, 64, 0, 0.02, 0.01)


class AdaptiveStats(C.Structure):
    _fields_ = [("passes", C.c_uint64), ("samples", C.c_uint64), ("stopped_by_threshold", C.c_uint64), ("stopped_at_max", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class AovParams(C.Structure):
    _fields_ = [("z_depth_max_dist", C.c_double)]


class Hit(C.Structure):
    _fields_ = [("p", C.c_double * 3), ("normal", C.c_double * 3), ("tangent", C.c_double * 3),
                ("bitangent", C.c_double * 3), ("t", C.c_double), ("u", C.c_double), ("v", C.c_double),
                ("mat", C.c_uint32), ("front_face", C.c_uint32)]


HIT_DTYPE = np.dtype([("p", "<f8", 3), ("normal", "<f8", 3), ("tangent", "<f8", 3), ("bitangent", "<f8", 3),
                      ("t", "<f8"), ("u", "<f8"), ("v", "<f8"), ("mat", "<u4"), ("front_face", "<u4")])
assert HIT_DTYPE.itemsize == C.sizeof(Hit)


class ScatterOut(C.Structure):
    _fields_ = [("attenuation", C.c_double * 3), ("origin", C.c_double * 3), ("direction", C.c_double * 3), ("emitted", C.c_double * 3),
                ("scattered", C.c_uint32), ("draws", C.c_uint32)]


SCATTER_DTYPE = np.dtype([("attenuation", "<f8", 3), ("origin", "<f8", 3), ("direction", "<f8", 3), ("emitted", "<f8", 3),
                          ("scattered", "<u4"), ("draws", "<u4")])
assert SCATTER_DTYPE.itemsize == C.sizeof(ScatterOut)


BVH_DEBUG_HIT_DTYPE = np.dtype([("hit", HIT_DTYPE), ("color", "<f8", 3), ("cls", "<u4"), ("depth", "<i4"), ("tree", "<u4"), ("box", "<u4")])
TREE_BOX_DTYPE = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3), ("id", "<u4"), ("tree", "<u4"), ("parent", "<u4"), ("depth", "<i4"), ("slot", "<u4"),
                           ("leaf", "<u4"), ("kind", "<u4"), ("count", "<u4"), ("first", "<u4"), ("subtree", "<u4"), ("src", "<u4", 4)])


class RefitInfo(C.Structure):
    """zr_refit_info: what zr_scene_refit reports (include/zr_capi.h)"""
    _fields_ = [("epoch", C.c_uint64), ("dirty_entries", C.c_uint32), ("levels", C.c_uint32), ("area_ratio", C.c_double), ("host_ms", C.c_double),
                ("device_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SceneDesc(C.Structure):
    _fields_ = [("spheres", C.c_void_p), ("sphere_mat", C.c_void_p), ("n_spheres", C.c_uint64),
                ("tri_v", C.c_void_p), ("tri_n", C.c_void_p), ("tri_mat", C.c_void_p), ("n_tris", C.c_uint64),
                ("cubes", C.c_void_p), ("cube_mat", C.c_void_p), ("n_cubes", C.c_uint64),
                ("media", C.c_void_p), ("n_media", C.c_uint64),
                ("ops", C.c_void_p), ("n_ops", C.c_uint64),
                ("objects", C.c_void_p), ("n_objects", C.c_uint64),
                ("materials", C.c_void_p), ("n_materials", C.c_uint64),
                ("textures", C.c_void_p), ("n_textures", C.c_uint64),
                ("texels", C.c_void_p), ("texel_bytes", C.c_uint64),
                ("groups", C.c_void_p), ("n_groups", C.c_uint64)]


_lib = None
_scenes = None

# every symbol include/zr_capi.h declares (tests check that the library exports all of them)
CAPI_SYMBOLS = [
    "zr_abi_version", "zr_last_error", "zr_create", "zr_destroy", "zr_scene_create", "zr_scene_destroy",
    "zr_scene_set_spheres", "zr_scene_set_triangles", "zr_scene_set_triangle_uvs", "zr_scene_set_cubes", "zr_scene_set_media",
    "zr_scene_set_xform_ops", "zr_scene_set_objects", "zr_scene_set_groups", "zr_scene_set_materials", "zr_scene_set_textures",
    "zr_scene_set_all", "zr_scene_set_all_borrowed", "zr_scene_commit", "zr_scene_update_xform_ops", "zr_scene_update_spheres", "zr_scene_refit", "zr_scene_stats", "zr_scene_kernels", "zr_scene_traversal_stack", "zr_scene_builder", "zr_render", "zr_render_device",
    "zr_accum_create", "zr_accum_destroy", "zr_accum_reset", "zr_render_accumulate", "zr_accum_resolve", "zr_accum_resolve_device", "zr_accum_state",
    "zr_render_adaptive", "zr_accum_error", "zr_accum_sample_counts", "zr_accum_lane_sums",
    "zr_render_aov", "zr_render_passes", "zr_trace_paths", "zr_post_process", "zr_analyze_frame", "zr_denoise", "zr_sharpen_frame",
    "zr_accum_variance", "zr_denoise_guided", "zr_accum_denoise",
    "zr_accum_halves", "zr_denoise_nlm", "zr_accum_denoise_nlm",
    "zr_accum_resolve_robust", "zr_kat_resolve_robust",
    "zr_render_gbuffer", "zr_temporal_create", "zr_temporal_destroy", "zr_temporal_reset", "zr_temporal_state", "zr_temporal_accumulate", "zr_accum_temporal",
    "zr_temporal_view", "zr_temporal_track_motion", "zr_render_gbuffer_entries", "zr_scene_motion",
    "zr_render_bvh_debug", "zr_trace_bvh_debug", "zr_scene_tree_boxes", "zr_get_counters", "zr_last_presolved_pixels", "zr_last_round_loop", "zr_last_shade_builds", "zr_last_extend_fetches",
    "zr_get_kernel_times", "zr_trace", "zr_kat_scatter", "zr_kat_shade_lean", "zr_kat_texture", "zr_kat_background", "zr_kat_camera_rays", "zr_comm_unique_id", "zr_comm_create", "zr_comm_reduce_frame", "zr_comm_gather_frame", "zr_comm_destroy",
    "zr_accum_set_direct", "zr_accum_get_direct", "zr_render_direct", "zr_get_direct_stats", "zr_scene_lights", "zr_kat_light_sample", "zr_kat_light_pdf", "zr_kat_light_key",
    "zr_accum_set_direct_env", "zr_accum_get_direct_env", "zr_render_direct_env", "zr_scene_env_light", "zr_kat_env_light_sample", "zr_kat_env_light_pdf", "zr_get_direct_env_stats",
]


def load():
    """Loads libzr_hip.so (raises OSError with a build hint if it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    lib.zr_abi_version.restype = i32
    lib.zr_last_error.restype = C.c_char_p
    lib.zr_create.restype = vp; lib.zr_create.argtypes = [i32]
    lib.zr_destroy.argtypes = [vp]
    lib.zr_scene_create.restype = vp; lib.zr_scene_create.argtypes = [vp]
    lib.zr_scene_destroy.argtypes = [vp]
    lib.zr_scene_set_all.argtypes = [vp, C.POINTER(SceneDesc)]
    lib.zr_scene_set_all_borrowed.argtypes = [vp, C.POINTER(SceneDesc)]
    lib.zr_scene_set_spheres.argtypes = [vp, vp, vp, C.c_size_t]
    lib.zr_scene_set_triangles.argtypes = [vp, vp, vp, vp, C.c_size_t]
    if hasattr(lib, "zr_scene_set_triangle_uvs"):   # (a ZR_LIB built from older sources, loaded for an A/B, has none)
        lib.zr_scene_set_triangle_uvs.argtypes = [vp, vp, C.c_size_t]
    lib.zr_scene_set_cubes.argtypes = [vp, vp, vp, C.c_size_t]
    lib.zr_scene_set_media.argtypes = [vp, vp, C.c_size_t]
    lib.zr_scene_set_xform_ops.argtypes = [vp, vp, C.c_size_t]
    lib.zr_scene_set_objects.argtypes = [vp, vp, C.c_size_t]
    lib.zr_scene_set_materials.argtypes = [vp, vp, C.c_size_t]
    lib.zr_scene_set_textures.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
    lib.zr_scene_commit.argtypes = [vp]
    if hasattr(lib, "zr_scene_refit"):   # (a ZR_LIB built from older sources, loaded for an A/B, has none)
        lib.zr_scene_update_xform_ops.argtypes = [vp, C.c_size_t, vp, C.c_size_t]
        lib.zr_scene_update_spheres.argtypes = [vp, C.c_size_t, vp, C.c_size_t]
        lib.zr_scene_refit.argtypes = [vp, C.POINTER(RefitInfo)]
    lib.zr_scene_stats.argtypes = [vp, C.POINTER(u64 * 4)]
    lib.zr_scene_kernels.argtypes = [vp, C.POINTER(C.c_uint32 * 4)]
    lib.zr_scene_traversal_stack.argtypes = [vp]; lib.zr_scene_traversal_stack.restype = C.c_uint32
    lib.zr_scene_builder.argtypes = [vp]; lib.zr_scene_builder.restype = C.c_char_p
    lib.zr_render.argtypes = [vp, vp, C.POINTER(Camera), C.POINTER(Env), u64, C.POINTER(Region), i32, vp, vp, vp]
    lib.zr_render_device.argtypes = [vp, vp, C.POINTER(Camera), C.POINTER(Env), u64, C.POINTER(Region), i32, vp, vp]
    lib.zr_accum_create.restype = vp; lib.zr_accum_create.argtypes = [vp, i32, i32, C.POINTER(Region)]
    lib.zr_accum_destroy.argtypes = [vp]; lib.zr_accum_destroy.restype = None
    lib.zr_accum_reset.argtypes = [vp, i32]
    lib.zr_render_accumulate.argtypes = [vp, vp, C.POINTER(Camera), C.POINTER(Env), u64, vp, i32, i32, vp]
    lib.zr_accum_resolve.argtypes = [vp, vp]
    lib.zr_accum_resolve_device.argtypes = [vp, vp, vp]
    lib.zr_accum_state.argtypes = [vp, C.POINTER(C.c_int64 * 4)]
    lib.zr_render_adaptive.argtypes = [vp, vp, C.POINTER(Camera), C.POINTER(Env), u64, vp, C.POINTER(AdaptiveParams), i32, vp, C.POINTER(AdaptiveStats)]
    lib.zr_accum_error.argtypes = [vp, C.c_double, vp]
    lib.zr_accum_sample_counts.argtypes = [vp, vp]
    lib.zr_accum_lane_sums.restype = C.c_int64; lib.zr_accum_lane_sums.argtypes = [vp, vp, C.c_size_t]
    lib.zr_render_aov.argtypes = [vp, vp, C.POINTER(Camera), u64, C.POINTER(Region), C.POINTER(AovParams), vp, vp, vp]
    lib.zr_post_process.argtypes = [vp, C.POINTER(PostParams), vp, i32, i32, i32, i32, vp]
    lib.zr_analyze_frame.argtypes = [vp, vp, C.c_size_t, C.POINTER(ImageStats)]
    lib.zr_denoise.argtypes = [vp, C.POINTER(DenoiseParams), vp, vp, vp, vp, i32, i32, vp]
    lib.zr_sharpen_frame.argtypes = [vp, vp, i32, i32, C.c_double, vp]
    lib.zr_accum_variance.argtypes = [vp, vp]
    lib.zr_denoise_guided.argtypes = [vp, C.POINTER(DenoiseGuidedParams), vp, vp, vp, vp, vp, i32, i32, vp, vp]
    lib.zr_accum_denoise.argtypes = [vp, C.POINTER(DenoiseGuidedParams), vp, vp, vp, vp, vp]
    if hasattr(lib, "zr_denoise_nlm"):   # (a ZR_LIB built from older sources, loaded for an A/B, has none)
        lib.zr_accum_halves.argtypes = [vp, vp, vp]
        lib.zr_denoise_nlm.argtypes = [vp, C.POINTER(DenoiseNlmParams), vp, vp, vp, vp, vp, i32, i32, vp, vp]
        lib.zr_accum_denoise_nlm.argtypes = [vp, C.POINTER(DenoiseNlmParams), vp, vp, vp, vp]
    if hasattr(lib, "zr_accum_resolve_robust"):   # (a ZR_LIB built from older sources, loaded for an A/B, has none)
        lib.zr_accum_resolve_robust.argtypes = [vp, C.POINTER(RobustParams), vp, vp, vp]
        lib.zr_kat_resolve_robust.argtypes = [vp, C.POINTER(RobustParams), vp, vp, C.c_size_t, vp, vp, vp]
    if hasattr(lib, "zr_temporal_create"):   # (a ZR_LIB built from older sources, loaded for an A/B, has none)
        lib.zr_render_gbuffer.argtypes = [vp, vp, C.POINTER(Camera), u64, vp, vp, vp, vp]
        lib.zr_temporal_create.restype = vp; lib.zr_temporal_create.argtypes = [vp, i32, i32]
        lib.zr_temporal_destroy.argtypes = [vp]; lib.zr_temporal_destroy.restype = None
        lib.zr_temporal_reset.argtypes = [vp]
        lib.zr_temporal_state.argtypes = [vp, C.POINTER(C.c_int64 * 4)]
        lib.zr_temporal_accumulate.argtypes = [vp, C.POINTER(TemporalParams), vp, C.POINTER(Camera), u64, vp, vp, vp, vp, vp]
        lib.zr_accum_temporal.argtypes = [vp, vp, C.POINTER(TemporalParams), vp, C.POINTER(Camera), u64, vp, vp, vp]
        lib.zr_temporal_view.argtypes = [C.POINTER(Camera), C.POINTER(C.c_double * 16)]
    if hasattr(lib, "zr_scene_motion"):   # (likewise)
        lib.zr_temporal_track_motion.argtypes = [vp, i32]
        lib.zr_render_gbuffer_entries.argtypes = [vp, vp, C.POINTER(Camera), u64, vp]
        lib.zr_scene_motion.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.zr_render_bvh_debug.argtypes = [vp, vp, C.POINTER(Camera), C.POINTER(Env), u64, C.POINTER(Region), C.POINTER(BvhDebugParams), vp, vp, vp]
    lib.zr_trace_bvh_debug.argtypes = [vp, vp, C.POINTER(BvhDebugParams), vp, C.c_size_t, C.c_double, u64, u64, C.c_uint32, vp]
    lib.zr_scene_tree_boxes.argtypes = [vp, vp, C.c_size_t]
    lib.zr_trace_paths.argtypes = [vp, vp, C.POINTER(Camera), u64, vp, i32, i32, vp]
    lib.zr_render_passes.argtypes = [vp, vp, C.POINTER(Camera), C.POINTER(Env), u64, C.POINTER(Region), vp, vp, vp]
    lib.zr_get_counters.argtypes = [vp, C.POINTER(Counters)]
    if hasattr(lib, "zr_last_presolved_pixels"):   # (a ZR_LIB built from older sources, loaded for an A/B, has none)
        lib.zr_last_presolved_pixels.argtypes = [vp]; lib.zr_last_presolved_pixels.restype = u64
    if hasattr(lib, "zr_last_round_loop"):   # (likewise)
        lib.zr_last_round_loop.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(lib, "zr_last_extend_fetches"):   # (likewise)
        lib.zr_last_extend_fetches.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.zr_last_extend_fetches.restype = C.c_int
    if hasattr(lib, "zr_last_shade_builds"):   # (likewise)
        lib.zr_last_shade_builds.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.zr_get_kernel_times.argtypes = [vp, C.POINTER(C.c_float), i32]
    lib.zr_trace.argtypes = [vp, vp, vp, C.c_size_t, C.c_double, C.c_double, u64, u64, C.c_uint32, vp]
    lib.zr_kat_scatter.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    if hasattr(lib, "zr_kat_shade_lean"):   # (a ZR_LIB built from older sources, loaded for an A/B, has none)
        lib.zr_kat_shade_lean.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, vp, vp]
    lib.zr_kat_texture.argtypes = [vp, vp, C.c_uint32, vp, C.c_size_t, vp]
    lib.zr_kat_background.argtypes = [vp, vp, C.POINTER(Env), vp, C.c_size_t, vp]
    lib.zr_kat_camera_rays.argtypes = [vp, C.POINTER(Camera), u64, vp, C.c_size_t, vp]
    if hasattr(lib, "zr_render_direct"):
        lib.zr_accum_set_direct.argtypes = [vp, C.POINTER(DirectParams)]
        lib.zr_accum_get_direct.argtypes = [vp, C.POINTER(DirectParams)]
        lib.zr_render_direct.argtypes = [vp, vp, C.POINTER(Camera), C.POINTER(Env), u64, C.POINTER(Region), C.POINTER(DirectParams), i32, vp]
        lib.zr_get_direct_stats.argtypes = [vp, C.POINTER(DirectStats)]
        lib.zr_scene_lights.restype = C.c_int64; lib.zr_scene_lights.argtypes = [vp, vp, vp, C.c_size_t]
        lib.zr_kat_light_sample.argtypes = [vp, vp, C.POINTER(Env), C.POINTER(DirectParams), vp, vp, vp, vp, C.c_size_t, vp]
        lib.zr_kat_light_pdf.argtypes = [vp, vp, C.POINTER(Env), C.POINTER(DirectParams), vp, vp, C.c_size_t, vp, vp]
        lib.zr_kat_light_key.restype = u64; lib.zr_kat_light_key.argtypes = [u64, C.c_uint32]
    if hasattr(lib, "zr_render_direct_env"):
        lib.zr_accum_set_direct_env.argtypes = [vp, i32]
        lib.zr_accum_get_direct_env.argtypes = [vp, C.POINTER(i32)]
        lib.zr_render_direct_env.argtypes = [vp, vp, C.POINTER(Camera), C.POINTER(Env), u64, C.POINTER(Region), C.POINTER(DirectParams), i32, vp]
        lib.zr_scene_env_light.argtypes = [vp, vp, C.POINTER(Env), C.POINTER(EnvLightInfo), vp, vp]
        lib.zr_kat_env_light_sample.argtypes = [vp, vp, C.POINTER(Env), C.POINTER(DirectParams), vp, vp, vp, vp, C.c_size_t, vp]
        lib.zr_kat_env_light_pdf.argtypes = [vp, vp, C.POINTER(Env), C.POINTER(DirectParams), vp, C.c_size_t, vp]
        lib.zr_get_direct_env_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    lib.zr_comm_unique_id.argtypes = [vp]
    lib.zr_comm_create.restype = vp; lib.zr_comm_create.argtypes = [vp, i32, i32, vp]
    lib.zr_comm_reduce_frame.argtypes = [vp, vp, C.c_size_t, i32, vp]
    lib.zr_comm_gather_frame.argtypes = [vp, vp, i32, i32, C.POINTER(Region), i32, vp]
    lib.zr_comm_destroy.argtypes = [vp]
    _lib = lib
    return lib


def load_scenes():
    global _scenes
    if _scenes is not None:
        return _scenes
    load()
    if not os.path.exists(SCENES_LIB_PATH):
        raise OSError(f"{SCENES_LIB_PATH} not built: run __graft_entry__.build()")
    s = C.CDLL(SCENES_LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    s.zrs_build.restype = vp; s.zrs_build.argtypes = [C.c_char_p, i32, i32, i32, i32]
    s.zrs_free.argtypes = [vp]
    s.zrs_desc.restype = C.POINTER(SceneDesc); s.zrs_desc.argtypes = [vp]
    s.zrs_camera.restype = C.POINTER(Camera); s.zrs_camera.argtypes = [vp]
    s.zrs_env.restype = C.POINTER(Env); s.zrs_env.argtypes = [vp]
    s.zrs_seed.restype = C.c_uint64; s.zrs_seed.argtypes = [vp]
    s.zrs_warnings.restype = C.c_char_p; s.zrs_warnings.argtypes = [vp]
    s.zrs_kat_textures.argtypes = [vp, vp, i32]
    frame = [vp, i32, i32, i32, i32]   # every zrs_render_dropin* begins: handle, width, height, spp, device
    s.zrs_render_dropin.argtypes = frame + [vp, C.POINTER(Counters)]
    s.zrs_render_dropin_progressive.argtypes = frame + [i32, vp, vp, i32]
    s.zrs_render_dropin_adaptive.argtypes = frame + [C.c_double, i32, i32, vp, vp, vp, i32]
    s.zrs_render_dropin_robust.argtypes = frame + [C.c_double, C.c_double, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    if hasattr(s, "zrs_render_dropin_direct"):
        s.zrs_render_dropin_direct.argtypes = frame + [i32, i32, i32, vp, vp]
    if hasattr(s, "zrs_render_dropin_direct_env"):
        s.zrs_render_dropin_direct_env.argtypes = frame + [i32, i32, i32, vp, vp]
    s.zrs_render_dropin_threads.argtypes = frame + [i32, vp]
    s.zrs_render_dropin_denoise.argtypes = frame + [i32] + [vp] * 6
    s.zrs_render_dropin_denoise_guided.argtypes = frame + [C.c_double, i32, i32] + [vp] * 4
    s.zrs_render_dropin_denoise_nlm.argtypes = frame + [C.c_double, i32, i32] + [vp] * 5
    s.zrs_render_dropin_temporal.argtypes = frame + [i32, vp, i32, i32] + [vp] * 5
    s.zrs_render_dropin_bvh_debug.argtypes = frame + [i32, C.c_float, vp, vp]
    s.zrs_render_dropin_animated.argtypes = frame + [i32, i32, i32, vp, vp]
    if hasattr(s, "zrs_render_dropin_animated_temporal"):
        s.zrs_render_dropin_animated_temporal.argtypes = frame + [i32, i32, vp, vp, vp, vp]
    s.zrs_dropin_virtuals.argtypes = [vp, vp, i32, C.c_uint64, C.c_uint64, vp, vp]
    s.zrs_dropin_frame_to_rgb8.argtypes = [vp, i32, i32, vp, vp, C.POINTER(C.c_float)]
    _scenes = s
    return s


class ZrError(RuntimeError):
    pass


def _check(rc, allow_cancel=False):
    if rc == ZR_OK or (allow_cancel and rc == ZR_E_CANCELLED):
        return rc
    raise ZrError(f"zr error {rc}: {load().zr_last_error().decode()}")


def _like(shape, what, frames=(), outs=(), dtype=np.float64):
    """Frames like this one: `frames` as contiguous float64 arrays of `shape` (None stays None; another shape raises ValueError naming `what`), then one
    output per entry of `outs`, made (zeroed, of `dtype`) where it is None and otherwise asserted to be a contiguous `dtype` array of `shape`"""
    frames = [np.ascontiguousarray(f, dtype=np.float64) if f is not None else None for f in frames]
    for f in frames:
        if f is not None and f.shape != shape:
            raise ValueError(f"frame shape {f.shape} differs from {what} {shape}")
    outs = [np.zeros(shape, dtype=dtype) if o is None else o for o in outs]
    for o in outs:
        assert o.dtype == dtype and o.flags.c_contiguous and o.shape == shape
    return frames + outs


def _ptr(a):
    return a.ctypes.data if a is not None else None


_M64 = (1 << 64) - 1


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def light_key(key, bounce):
    """zr_light_key of include/zr_rng.h: the key of the light stream of the vertex that closest-hit query number `bounce` of the main stream `key` reached"""
    return _mix64((_mix64((int(key) ^ 0x4C494748545F5F5F) & _M64) + 0x9E3779B97F4A7C15 * (int(bounce) + 1)) & _M64)


class DemoScene:
    """One of the BASELINE.json scenes, built through the drop-in C++ scene API and flattened."""

    def __init__(self, name, *args):
        s = load_scenes()
        a = list(args) + [0] * (4 - len(args))
        self._h = s.zrs_build(name.encode(), *[int(x) for x in a[:4]])
        if not self._h:
            raise ValueError(f"unknown scene {name!r}")
        self.name = name
        self.desc = s.zrs_desc(self._h).contents
        self.camera = s.zrs_camera(self._h).contents.copy()
        self.env = s.zrs_env(self._h).contents
        self.seed = int(s.zrs_seed(self._h))
        self.warnings = s.zrs_warnings(self._h).decode()
        ids = (C.c_uint32 * 64)()
        self.kat_textures = [int(ids[k]) for k in range(min(64, s.zrs_kat_textures(self._h, ids, 64)))]

    def _size(self, width, height):
        """(H, W) of a drop-in render at width x height (0: the scene's own)"""
        return height or self.camera.image_height, width or self.camera.image_width

    def _frames(self, width, height, *names, n=0):
        """zeroed (H, W, 3) float64 outputs by name for a drop-in render at width x height; n > 0: (n, H, W, 3), a frame per render"""
        shape = ((n,) if n else ()) + self._size(width, height) + (3,)
        return {k: np.zeros(shape, dtype=np.float64) for k in names}

    @staticmethod
    def _rendered(ok):
        if not ok:
            raise ZrError(f"drop-in render failed: {load().zr_last_error().decode()}")

    def render_dropin(self, width=0, height=0, spp=0, device=0):
        """camera::render(world, env, post, flag) of include/zenith/zenith.hpp, end to end."""
        out = self._frames(width, height, "out")["out"]
        ctr = Counters()
        self._rendered(load_scenes().zrs_render_dropin(self._h, width, height, spp, device, out.ctypes.data, C.byref(ctr)) == 0)
        return out, ctr

    def render_dropin_progressive(self, samples_per_pass, width=0, height=0, spp=0, device=0, flag=True):
        """camera::render with camera::samples_per_pass set: (frame, current_samples_count afterwards, refreshes of render_accumulator).
        current_samples_count is -7 going in, so a render that does not touch it (samples_per_pass = 0) reports -7.
        flag: render_flag going in; with False an unfinished render is the expected outcome and is not raised."""
        out = self._frames(width, height, "out")["out"]
        info = (C.c_int * 2)()
        rc = load_scenes().zrs_render_dropin_progressive(self._h, width, height, spp, device, int(samples_per_pass), out.ctypes.data, info, int(bool(flag)))
        self._rendered(rc == 0 or (rc == -1 and not flag))
        return out, int(info[0]), int(info[1])

    def render_dropin_adaptive(self, threshold, min_samples=0, step=0, width=0, height=0, spp=0, device=0, flag=True):
        """camera::render with camera::adaptive_threshold set (min_samples / step 0: the camera's defaults of 64): (frame, camera::sample_counts as
        (H, W) int32 — all -1 when the render was not adaptive —, current_samples_count afterwards (-7 going in), passes).
        flag: render_flag going in; with False an unfinished render is the expected outcome and is not raised."""
        out = self._frames(width, height, "out")["out"]
        counts = np.full(out.shape[:2], -1, dtype=np.int32)
        info = (C.c_int * 2)()
        rc = load_scenes().zrs_render_dropin_adaptive(self._h, width, height, spp, device, float(threshold), int(min_samples), int(step), out.ctypes.data,
                                                      counts.ctypes.data, info, int(bool(flag)))
        self._rendered(rc == 0 or (rc == -1 and not flag))
        return out, counts, int(info[0]), int(info[1])

    def render_dropin_robust(self, robust=True, strength=None, threshold=0.0, min_samples=0, step=0, samples_per_pass=0, variance=False, temporal=False,
                             width=0, height=0, spp=0, device=0):
        """camera::render with camera::robust_resolve = robust and robust_strength = strength (None: the camera's default): adaptively when threshold > 0,
        progressively when samples_per_pass > 0, else as the flag decides (one pass through an accumulator at a multiple of 64 samples).  variance: also
        use_denoiser and denoise_variance_guided, which fill variance_buffer; temporal: temporal_accumulation (one frame of a fresh history).  Dict of
        render_accumulator, variance_buffer, temporal_buffer ((H, W, 3) float64; the last two all -1 when the render left them empty), sample_counts ((H, W) int32, all -1 likewise), robust (camera::resolve_used_robust), current_samples_count (-7 going in)
        and passes"""
        outs = self._frames(width, height, "render_accumulator", "variance_buffer", "temporal_buffer")
        counts = np.full(outs["render_accumulator"].shape[:2], -1, dtype=np.int32)
        info = (C.c_int * 3)()
        flags = (1 if robust else 0) | (2 if variance else 0) | (4 if temporal else 0)
        self._rendered(load_scenes().zrs_render_dropin_robust(self._h, width, height, spp, device, -1.0 if strength is None else float(strength), float(threshold),
                                                              int(min_samples), int(step), int(samples_per_pass), flags, outs["render_accumulator"].ctypes.data,
                                                              outs["variance_buffer"].ctypes.data, outs["temporal_buffer"].ctypes.data, counts.ctypes.data,
                                                              info) == 0)
        outs.update(sample_counts=counts, robust=bool(info[0]), current_samples_count=int(info[1]), passes=int(info[2]))
        return outs

    def render_dropin_direct(self, on=True, split=False, samples_per_pass=0, width=0, height=0, spp=0, device=0):
        """camera::render with camera::direct_lighting (split: use_reflection too, with which the flag is ignored) -> (frame, render_used_direct, passes)"""
        out = self._frames(width, height, "out")["out"]
        info = (C.c_int * 2)(0, 0)
        self._rendered(load_scenes().zrs_render_dropin_direct(self._h, width, height, spp, device, 1 if on else 0, 1 if split else 0, samples_per_pass, out.ctypes.data,
                                                              info) == 0)
        return out, bool(info[0]), int(info[1])

    def render_dropin_direct_env(self, on=True, env=True, samples_per_pass=0, width=0, height=0, spp=0, device=0):
        """camera::render with camera::direct_lighting = on and camera::direct_environment = env
        -> (frame, render_used_direct, render_used_direct_env, passes)"""
        out = self._frames(width, height, "out")["out"]
        info = (C.c_int * 3)(0, 0, 0)
        self._rendered(load_scenes().zrs_render_dropin_direct_env(self._h, width, height, spp, device, 1 if on else 0, 1 if env else 0, samples_per_pass,
                                                                  out.ctypes.data, info) == 0)
        return out, bool(info[0]), bool(info[2]), int(info[1])

    def render_dropin_threads(self, n, width=0, height=0, spp=0, device=0):
        """n drop-in renders, each on a fresh host thread, one after the other (the reference's render-restart pattern,
        main.cpp:1520-1531): (last frame, device contexts the process has created so far)"""
        out = self._frames(width, height, "out")["out"]
        rc = load_scenes().zrs_render_dropin_threads(self._h, width, height, spp, device, n, out.ctypes.data)
        self._rendered(rc >= 0)
        return out, rc

    def render_dropin_denoise(self, width=0, height=0, spp=0, device=0, passes=False, sharpening=False):
        """camera::render with use_denoiser (and optionally use_reflection / use_refraction, post.use_sharpening) through
        include/zenith/zenith.hpp: dict of render_accumulator, denoise_buffer, reflection_buffer, refraction_buffer,
        albedo_buffer, normal_buffer as (H, W, 3) float64"""
        outs = self._frames(width, height, "render_accumulator", "denoise_buffer", "reflection_buffer", "refraction_buffer", "albedo_buffer", "normal_buffer")
        flags = (1 if passes else 0) | (2 if sharpening else 0)
        self._rendered(load_scenes().zrs_render_dropin_denoise(self._h, width, height, spp, device, flags, *[o.ctypes.data for o in outs.values()]) == 0)
        return outs

    def render_dropin_denoise_guided(self, threshold, samples_per_pass=0, guided=True, width=0, height=0, spp=0, device=0):
        """camera::render with use_denoiser and (guided) denoise_variance_guided, adaptively when threshold > 0, progressively when
        samples_per_pass > 0, else in one shot: dict of render_accumulator, denoise_buffer, variance_buffer ((H, W, 3) float64; all -1 when the
        render left variance_buffer empty) and "guided" (whether the guided filter made denoise_buffer)"""
        outs = self._frames(width, height, "render_accumulator", "denoise_buffer", "variance_buffer")
        info = (C.c_int * 2)()
        self._rendered(load_scenes().zrs_render_dropin_denoise_guided(self._h, width, height, spp, device, float(threshold), int(samples_per_pass),
                                                                      1 if guided else 0, *[o.ctypes.data for o in outs.values()], info) == 0)
        outs["guided"] = bool(info[0])
        return outs

    def render_dropin_denoise_nlm(self, threshold, samples_per_pass=0, nlm=True, guided=False, temporal=False, width=0, height=0, spp=0, device=0):
        """camera::render with use_denoiser and (nlm) denoise_nlm, (guided) denoise_variance_guided, (temporal) temporal_accumulation; adaptively when
        threshold > 0, progressively when samples_per_pass > 0, else in one shot: dict of render_accumulator, denoise_buffer, variance_buffer,
        denoise_error_buffer ((H, W, 3) float64; all -1 when the render left the buffer empty), "nlm" (whether the non-local-means filter made
        denoise_buffer) and "guided" (whether the guided filter did)"""
        outs = self._frames(width, height, "render_accumulator", "denoise_buffer", "variance_buffer", "denoise_error_buffer")
        info = (C.c_int * 3)()
        flags = (1 if nlm else 0) | (2 if guided else 0) | (4 if temporal else 0)
        self._rendered(load_scenes().zrs_render_dropin_denoise_nlm(self._h, width, height, spp, device, float(threshold), int(samples_per_pass), flags,
                                                                   *[o.ctypes.data for o in outs.values()], info) == 0)
        outs["nlm"] = bool(info[0]); outs["guided"] = bool(info[1])
        return outs

    def render_dropin_temporal(self, cameras, temporal=True, guided=False, samples_per_pass=0, reset_before_last=False, width=0, height=0, spp=0, device=0):
        """a camera path through ONE drop-in camera object and one world object: a render per entry of `cameras` (capi.Camera: lookfrom / lookat are
        taken) with seed = the scene's + k, camera::temporal_accumulation = temporal, use_denoiser and denoise_variance_guided = guided, progressive when
        samples_per_pass > 0 else one-shot.  Dict of render_accumulator, temporal_buffer, variance_buffer, denoise_buffer ((n, H, W, 3) float64; a frame
        that left the buffer empty is all -1) and temporal_history_length ((n, H, W) int32, -1 likewise)"""
        n = len(cameras)
        cams = np.array([list(c.lookfrom) + list(c.lookat) for c in cameras], dtype=np.float64)
        outs = self._frames(width, height, "render_accumulator", "temporal_buffer", "variance_buffer", "denoise_buffer", n=n)
        outs["temporal_history_length"] = np.zeros((n, *self._size(width, height)), dtype=np.int32)
        flags = (1 if temporal else 0) | (2 if guided else 0) | (4 if reset_before_last else 0)
        self._rendered(load_scenes().zrs_render_dropin_temporal(self._h, width, height, spp, device, n, cams.ctypes.data, flags, int(samples_per_pass),
                                                                *[o.ctypes.data for o in outs.values()]) == 0)
        return outs

    def render_dropin_bvh_debug(self, level, thickness, width=0, height=0, spp=0, device=0):
        """camera::render with global_settings::bvh_debug_mode set through include/zenith/zenith.hpp: (render_accumulator,
        albedo_buffer) as (H, W, 3) float64 (the debug view leaves the AOV buffers as reset_accumulator made them)"""
        out, aux = self._frames(width, height, "out", "aux").values()
        aux.fill(-1.0)
        self._rendered(load_scenes().zrs_render_dropin_bvh_debug(self._h, width, height, spp, device, level, thickness, out.ctypes.data, aux.ctypes.data) == 0)
        return out, aux

    def render_dropin_animated(self, n_frames, reuse_scene, add_at=-1, width=0, height=0, spp=0, device=0):
        """n_frames renders of the shim's small moving world through ONE drop-in camera object with camera::reuse_scene = reuse_scene: one translate and
        one rotate_y re-created around a shared cube with new arguments for every frame, a sphere that rises, and from frame add_at on (-1: never) one
        object more.  Returns (frames (n, H, W, 3) float64, camera::last_scene_refit after each render as a list: 0 committed, 1 refitted)"""
        out = self._frames(width, height, "out", n=n_frames)["out"]
        refit = (C.c_int * n_frames)()
        self._rendered(load_scenes().zrs_render_dropin_animated(self._h, width, height, spp, device, int(n_frames), 1 if reuse_scene else 0, int(add_at),
                                                                out.ctypes.data, refit) == 0)
        return out, [int(x) for x in refit]

    def render_dropin_animated_temporal(self, n_frames, reuse_scene=True, temporal=True, track_motion=False, width=0, height=0, spp=0, device=0):
        """render_dropin_animated's world (nothing added) through ONE camera with camera::temporal_accumulation (progressive, 64 samples a pass) and
        camera::temporal_track_motion: dict of render_accumulator, temporal_buffer ((n, H, W, 3); all -1 where a frame left it empty),
        temporal_history_length ((n, H, W) int32, -1 likewise) and last_scene_refit (list)"""
        outs = self._frames(width, height, "render_accumulator", "temporal_buffer", n=n_frames)
        hist = np.zeros((n_frames, *self._size(width, height)), dtype=np.int32)
        refit = (C.c_int * n_frames)()
        flags = (1 if reuse_scene else 0) | (2 if temporal else 0) | (4 if track_motion else 0)
        self._rendered(load_scenes().zrs_render_dropin_animated_temporal(self._h, width, height, spp, device, int(n_frames), flags,
                                                                         outs["render_accumulator"].ctypes.data, outs["temporal_buffer"].ctypes.data,
                                                                         hist.ctypes.data, refit) == 0)
        outs["temporal_history_length"] = hist
        outs["last_scene_refit"] = [int(x) for x in refit]
        return outs

    def dropin_virtuals(self, rays8, seed, pixel=0x7ACE):
        """bvh_node(world).hit + rec.mat->emitted / scatter through the drop-in classes (one device launch per call):
        (recs[n,16], scat[n,14]) in the layout of `zenith_ref kat <scene> hits`"""
        rays8 = np.ascontiguousarray(rays8, dtype=np.float64).reshape(-1, 8)
        recs = np.zeros((len(rays8), 16)); scat = np.zeros((len(rays8), 14))
        if load_scenes().zrs_dropin_virtuals(self._h, rays8.ctypes.data, len(rays8), seed, pixel, recs.ctypes.data, scat.ctypes.data) != 0:
            raise ZrError("drop-in hit()/scatter() failed (see stderr)")
        return recs, scat

    def dropin_frame_to_rgb8(self, spp=0, device=0):
        """render (auto-exposure, reflection split) + post stack through include/zenith/zenith.hpp: (rgb8, reflection8, exposure)"""
        w, h = self.camera.image_width, self.camera.image_height
        a = np.zeros((h, w, 3), dtype=np.uint8); b = np.zeros((h, w, 3), dtype=np.uint8)
        ex = C.c_float(0)
        rc = load_scenes().zrs_dropin_frame_to_rgb8(self._h, spp, device, a.ctypes.data, b.ctypes.data, C.byref(ex))
        if rc != 0:
            raise ZrError(f"drop-in frame pipeline failed ({rc}): {load().zr_last_error().decode()}")
        return a, b, ex.value

    def close(self):
        if self._h:
            load_scenes().zrs_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    def __init__(self, device=0):
        self.lib = load()
        self._c = self.lib.zr_create(int(device))
        if not self._c:
            raise ZrError(self.lib.zr_last_error().decode())
        self.device = device

    def close(self):
        if self._c:
            self.lib.zr_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def post_process(self, params, frame, is_data_pass=False, apply_gamma=True):
        """camera::process_framebuffer_to_image up to the PNG encoder: (H, W, 3) float64 -> (H, W, 3) uint8"""
        frame = np.ascontiguousarray(frame, dtype=np.float64)
        h, w = frame.shape[:2]
        out = np.zeros((h, w, 3), dtype=np.uint8)
        _check(self.lib.zr_post_process(self._c, C.byref(params), frame.ctypes.data, w, h, int(is_data_pass), int(apply_gamma), out.ctypes.data))
        return out

    def analyze_frame(self, frame):
        frame = np.ascontiguousarray(frame, dtype=np.float64)
        st = ImageStats()
        _check(self.lib.zr_analyze_frame(self._c, frame.ctypes.data, frame.size // 3, C.byref(st)))
        return st

    def denoise(self, params, color, albedo, normal, zdepth=None, out=None):
        """zr_denoise (the a-trous filter of camera::use_denoiser): (H, W, 3) float64 frames -> (H, W, 3) float64.
        `out` may be `color` itself (in place)."""
        color = np.ascontiguousarray(color, dtype=np.float64)
        h, w = color.shape[:2]
        albedo, normal, zdepth, out = _like(color.shape, "the colour frame's", (albedo, normal, zdepth), (out,))
        _check(self.lib.zr_denoise(self._c, C.byref(params), color.ctypes.data, albedo.ctypes.data, normal.ctypes.data, _ptr(zdepth), w, h, out.ctypes.data))
        return out

    def denoise_guided(self, params, color, variance, albedo, normal, zdepth=None, out=None, out_variance=None):
        """zr_denoise_guided (the a-trous filter with variance-driven colour weights): (H, W, 3) float64 frames -> (frame, variance), both
        (H, W, 3) float64.  `out` may be `color` itself and `out_variance` may be `variance` itself (in place)."""
        color = np.ascontiguousarray(color, dtype=np.float64)
        h, w = color.shape[:2]
        variance, albedo, normal, zdepth, out, out_variance = _like(color.shape, "the colour frame's", (variance, albedo, normal, zdepth), (out, out_variance))
        _check(self.lib.zr_denoise_guided(self._c, C.byref(params), color.ctypes.data, variance.ctypes.data, albedo.ctypes.data, normal.ctypes.data,
                                          _ptr(zdepth), w, h, out.ctypes.data, out_variance.ctypes.data))
        return out, out_variance

    def denoise_nlm(self, params, half_a, half_b, variance, albedo, normal, out=None, out_error=None):
        """zr_denoise_nlm (dual-buffer non-local means: the weights of one half image filter the other): (H, W, 3) float64 frames -> (frame, error), both
        (H, W, 3) float64; `variance` is the variance of the full pixel mean.  `out` may be `half_a` itself (in place)."""
        half_a = np.ascontiguousarray(half_a, dtype=np.float64)
        h, w = half_a.shape[:2]
        *frames, out, out_error = _like(half_a.shape, "the first half's", (half_b, variance, albedo, normal), (out, out_error))
        _check(self.lib.zr_denoise_nlm(self._c, C.byref(params), half_a.ctypes.data, *[g.ctypes.data for g in frames], w, h, out.ctypes.data,
                                       out_error.ctypes.data))
        return out, out_error

    def sharpen(self, frame, amount, out=None):
        """post_processor::apply_sharpening on the device: (H, W, 3) float64 -> (H, W, 3) float64"""
        frame = np.ascontiguousarray(frame, dtype=np.float64)
        h, w = frame.shape[:2]
        out, = _like(frame.shape, "the frame's", outs=(out,))
        _check(self.lib.zr_sharpen_frame(self._c, frame.ctypes.data, w, h, C.c_double(amount), out.ctypes.data))
        return out

    def kat_camera_rays(self, camera, seed, requests):
        """camera::initialize + get_ray: (n, 7) = origin, direction, draws"""
        req = np.ascontiguousarray(requests, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((len(req), 7))
        _check(self.lib.zr_kat_camera_rays(self._c, C.byref(camera), C.c_uint64(seed), req.ctypes.data, len(req), out.ctypes.data))
        return out

    def kat_resolve_robust(self, lane_sums, counts, params=None):
        """zr_kat_resolve_robust: the robust resolve's kernel on caller-supplied lane sums (n, 3, 64) float64 with counts (n,) int32 -> (colour (n, 3),
        variance (n, 3), trim (n,) int32), in input order"""
        params = params if params is not None else RobustParams.defaults()
        lane_sums = np.ascontiguousarray(lane_sums, dtype=np.float64).reshape(-1, 3, 64)
        counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        n = len(lane_sums)
        if len(counts) != n:
            raise ValueError(f"{len(counts)} counts for {n} pixels of lane sums")
        out, var, trim = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=np.int32)
        _check(self.lib.zr_kat_resolve_robust(self._c, C.byref(params), lane_sums.ctypes.data, counts.ctypes.data, n, out.ctypes.data, var.ctypes.data,
                                              trim.ctypes.data))
        return out, var, trim

    def counters(self):
        c = Counters()
        _check(self.lib.zr_get_counters(self._c, C.byref(c)))
        return c

    # ---- direct light sampling ----
    def render_direct(self, scene, camera, env, seed, params=None, region=None, count=False, out=None):
        """zr_render_direct: the frame with next-event estimation and MIS — Accumulator + set_direct + accumulate(camera.samples_per_pixel) + resolve, bit for
        bit: (H, W, 3) float64; only the region's pixels of `out` are written"""
        params = params if params is not None else DirectParams.defaults()
        out, = _like((camera.image_height, camera.image_width, 3), "the camera's frame", outs=(out,))
        _check(self.lib.zr_render_direct(self._c, scene._s, C.byref(camera), C.byref(env), C.c_uint64(seed), C.byref(region) if region is not None else None,
                                         C.byref(params), 1 if count else 0, out.ctypes.data))
        return out

    def direct_stats(self):
        """zr_get_direct_stats -> dict: shadow queries of the last counted direct batch, slots and objects of the table it used"""
        st = DirectStats()
        _check(self.lib.zr_get_direct_stats(self._c, C.byref(st)))
        return st.as_dict()

    def kat_light_sample(self, scene, env, origins, keys, bounces, params=None, draws=None):
        """zr_kat_light_sample: one light sample per query from origins (n, 3) with the light stream of (keys[k], bounces[k]) -> array of LIGHT_SAMPLE_DTYPE.
        draws: (n, 8) numbers that replace the stream's first eight draws where they lie in [0, 1)"""
        params = params if params is not None else DirectParams.defaults()
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        b = np.ascontiguousarray(bounces, dtype=np.uint32).reshape(-1)
        d = np.ascontiguousarray(draws, dtype=np.float64).reshape(-1, 8) if draws is not None else None
        if len(k) != len(o) or len(b) != len(o) or (d is not None and len(d) != len(o)):
            raise ValueError("origins, keys, bounces and draws must have one row per query")
        out = np.zeros(len(o), dtype=LIGHT_SAMPLE_DTYPE)
        _check(self.lib.zr_kat_light_sample(self._c, scene._s, C.byref(env), C.byref(params), o.ctypes.data, k.ctypes.data, b.ctypes.data, _ptr(d), len(o),
                                            out.ctypes.data))
        return out

    def kat_light_pdf(self, scene, env, origins, dirs, params=None):
        """zr_kat_light_pdf: per ray the light density the MIS weight would use after the path's closest hit, and the hit's key (kind << 32 | index, all ones
        on a miss) -> ((n,) float64, (n,) uint64)"""
        params = params if params is not None else DirectParams.defaults()
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        if len(d) != len(o):
            raise ValueError("origins and dirs must have one row per ray")
        pdf, key = np.zeros(len(o)), np.zeros(len(o), dtype=np.uint64)
        _check(self.lib.zr_kat_light_pdf(self._c, scene._s, C.byref(env), C.byref(params), o.ctypes.data, d.ctypes.data, len(o), pdf.ctypes.data, key.ctypes.data))
        return pdf, key

    # ---- direct light sampling of the HDR environment map ----
    def render_direct_env(self, scene, camera, env, seed, params=None, region=None, count=False, out=None):
        """zr_render_direct_env: render_direct with the environment map sampled too — Accumulator + set_direct + set_direct_env + accumulate + resolve, bit for bit"""
        params = params if params is not None else DirectParams.defaults()
        out, = _like((camera.image_height, camera.image_width, 3), "the camera's frame", outs=(out,))
        _check(self.lib.zr_render_direct_env(self._c, scene._s, C.byref(camera), C.byref(env), C.c_uint64(seed), C.byref(region) if region is not None else None,
                                             C.byref(params), 1 if count else 0, out.ctypes.data))
        return out

    def direct_env_stats(self):
        """zr_get_direct_env_stats -> dict: shadow queries towards the environment map of the last counted direct batch, and those that saw it"""
        q, v = C.c_uint64(0), C.c_uint64(0)
        _check(self.lib.zr_get_direct_env_stats(self._c, C.byref(q), C.byref(v)))
        return {"env_queries": int(q.value), "env_visible": int(v.value)}

    def kat_env_light_sample(self, scene, env, origins, keys, bounces, params=None, draws=None):
        """zr_kat_env_light_sample: kat_light_sample with the environment on (choice 3: the map, slot = j W + i) -> array of LIGHT_SAMPLE_DTYPE"""
        params = params if params is not None else DirectParams.defaults()
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        b = np.ascontiguousarray(bounces, dtype=np.uint32).reshape(-1)
        d = np.ascontiguousarray(draws, dtype=np.float64).reshape(-1, 8) if draws is not None else None
        if len(k) != len(o) or len(b) != len(o) or (d is not None and len(d) != len(o)):
            raise ValueError("origins, keys, bounces and draws must have one row per query")
        out = np.zeros(len(o), dtype=LIGHT_SAMPLE_DTYPE)
        _check(self.lib.zr_kat_env_light_sample(self._c, scene._s, C.byref(env), C.byref(params), o.ctypes.data, k.ctypes.data, b.ctypes.data, _ptr(d), len(o),
                                                out.ctypes.data))
        return out

    def kat_env_light_pdf(self, scene, env, dirs, params=None):
        """zr_kat_env_light_pdf: the density a missed ray of each direction (any length) is weighted by -> (n,) float64"""
        params = params if params is not None else DirectParams.defaults()
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        pdf = np.zeros(len(d))
        _check(self.lib.zr_kat_env_light_pdf(self._c, scene._s, C.byref(env), C.byref(params), d.ctypes.data, len(d), pdf.ctypes.data))
        return pdf

    def presolved_pixels(self):
        """pixels the last render finished in the sky pre-pass (zr_last_presolved_pixels); 0 for every other path"""
        return int(self.lib.zr_last_presolved_pixels(self._c))

    def round_loop(self):
        """(drain_round, sub_pools) of the last pipeline render (zr_last_round_loop)"""
        d, k = C.c_int(0), C.c_int(0)
        _check(self.lib.zr_last_round_loop(self._c, C.byref(d), C.byref(k)))
        return d.value, k.value

    def shade_builds(self):
        """(in_place, sorted): SHADE launches of the last pipeline render by build (zr_last_shade_builds)"""
        a, b = C.c_int(0), C.c_int(0)
        _check(self.lib.zr_last_shade_builds(self._c, C.byref(a), C.byref(b)))
        return a.value, b.value

    def extend_fetches(self):
        """(checked, skipped): slots the lean EXTEND of the last counted render fetched with / without testing their meta word (zr_last_extend_fetches)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(self.lib.zr_last_extend_fetches(self._c, C.byref(a), C.byref(b)))
        return a.value, b.value

    def kernel_times_ms(self, cap=256):
        buf = (C.c_float * cap)()
        n = self.lib.zr_get_kernel_times(self._c, buf, cap)
        if n < 0:
            _check(n)
        return [buf[i] for i in range(min(n, cap))]


class Accumulator:
    """A frame rendered in batches of samples (zr_accum): device-resident lane sums for the pixels of `region` of a width x height frame.
    Any split of [0, N) into consecutive batches resolves to Scene.render's frame at N samples per pixel, bit for bit."""

    def __init__(self, ctx, width, height, region=None):
        self.ctx = ctx
        self.lib = ctx.lib
        self.width, self.height = int(width), int(height)
        self._a = self.lib.zr_accum_create(ctx._c, self.width, self.height, C.byref(region) if region is not None else None)
        if not self._a:
            raise ZrError(self.lib.zr_last_error().decode())

    def _like(self, frames=(), outs=()):
        return _like((self.height, self.width, 3), "the accumulator's frame", frames, outs)

    def accumulate(self, scene, camera, env, seed, n_samples, count=False, keep_going=None):
        """renders the next n_samples samples of every pixel and adds them (camera.samples_per_pixel is ignored); keep_going: a
        ctypes.c_uint8 polled like zr_render's — a cancelled batch raises nothing, returns ZR_E_CANCELLED and leaves the accumulator as it was"""
        kg = C.cast(C.byref(keep_going), C.c_void_p) if keep_going is not None else None
        return _check(self.lib.zr_render_accumulate(self.ctx._c, scene._s, C.byref(camera), C.byref(env), C.c_uint64(seed), self._a, int(n_samples),
                                                    1 if count else 0, kg), allow_cancel=True)

    def resolve(self, out=None):
        """the mean of the samples accumulated so far: (H, W, 3) float64; only the region's pixels of `out` are written"""
        out, = self._like(outs=(out,))
        _check(self.lib.zr_accum_resolve(self._a, out.ctypes.data))
        return out

    def reset(self, first_sample=0):
        _check(self.lib.zr_accum_reset(self._a, int(first_sample)))

    def set_direct(self, params=None, on=True):
        """zr_accum_set_direct: binds the direct-light integrator to this (empty) accumulator (params None: DirectParams.defaults()); on=False
        unbinds.  accumulate and render_adaptive then render with next-event estimation and MIS; every query of the accumulator works as before"""
        if on and params is None:
            params = DirectParams.defaults()
        _check(self.lib.zr_accum_set_direct(self._a, C.byref(params) if on else None))

    def get_direct(self):
        """zr_accum_get_direct -> the bound integrator's flags, or None"""
        p = DirectParams()
        _check(self.lib.zr_accum_get_direct(self._a, C.byref(p)))
        return int(p.flags) if p.pad_ else None

    def set_direct_env(self, on=True):
        """zr_accum_set_direct_env: the bound direct-light integrator also samples the HDR environment map; needs an empty accumulator with an
        integrator bound"""
        _check(self.lib.zr_accum_set_direct_env(self._a, 1 if on else 0))

    def get_direct_env(self):
        """zr_accum_get_direct_env -> bool"""
        on = C.c_int32(0)
        _check(self.lib.zr_accum_get_direct_env(self._a, C.byref(on)))
        return bool(on.value)

    def render_adaptive(self, scene, camera, env, seed, params, count=False, keep_going=None):
        """zr_render_adaptive: every pixel to params.min_samples, then params.step_samples more per pass for the pixels whose noise estimate is
        above params.threshold, up to params.max_samples.  Returns (rc, AdaptiveStats); a cancelled run raises nothing and returns
        ZR_E_CANCELLED with the statistics of the passes that completed."""
        kg = C.cast(C.byref(keep_going), C.c_void_p) if keep_going is not None else None
        stats = AdaptiveStats()
        rc = _check(self.lib.zr_render_adaptive(self.ctx._c, scene._s, C.byref(camera), C.byref(env), C.c_uint64(seed), self._a, C.byref(params),
                                                1 if count else 0, kg, C.byref(stats)), allow_cancel=True)
        return rc, stats

    def error(self, dark_floor=0.01, out=None):
        """the noise estimate of the sums held (relative standard error of the pixel mean): (H, W) float64; only the region's pixels are written"""
        out, = _like((self.height, self.width), "the accumulator's plane", outs=(out,))
        _check(self.lib.zr_accum_error(self._a, C.c_double(dark_floor), out.ctypes.data))
        return out

    def variance(self, out=None):
        """the variance of every pixel's mean per channel (zr_accum_variance): (H, W, 3) float64; only the region's pixels are written"""
        out, = self._like(outs=(out,))
        _check(self.lib.zr_accum_variance(self._a, out.ctypes.data))
        return out

    def resolve_robust(self, params=None, out=None, out_variance=None, out_trim=None):
        """zr_accum_resolve_robust: the Gini-trimmed mean of every pixel's lane sums, the variance of that mean and the trim: ((H, W, 3), (H, W, 3) float64,
        (H, W) int32); only the region's pixels are written"""
        params = params if params is not None else RobustParams.defaults()
        out, out_variance = self._like(outs=(out, out_variance))
        out_trim, = _like((self.height, self.width), "the accumulator's plane", outs=(out_trim,), dtype=np.int32)
        _check(self.lib.zr_accum_resolve_robust(self._a, C.byref(params), out.ctypes.data, out_variance.ctypes.data, out_trim.ctypes.data))
        return out, out_variance, out_trim

    def denoise(self, params, albedo, normal, zdepth=None):
        """zr_accum_denoise: Context.denoise_guided(params, resolve(), variance(), ...) bit for bit, with colour and variance resolved on the device;
        returns (frame, variance).  Whole-frame accumulators only."""
        albedo, normal, zdepth, out, out_variance = self._like((albedo, normal, zdepth), (None, None))
        _check(self.lib.zr_accum_denoise(self._a, C.byref(params), albedo.ctypes.data, normal.ctypes.data, _ptr(zdepth), out.ctypes.data, out_variance.ctypes.data))
        return out, out_variance

    def halves(self, out_a=None, out_b=None):
        """the two half images (zr_accum_halves: the means of the even and of the odd lanes' samples): two (H, W, 3) float64; only the region's pixels
        are written"""
        out_a, out_b = self._like(outs=(out_a, out_b))
        _check(self.lib.zr_accum_halves(self._a, out_a.ctypes.data, out_b.ctypes.data))
        return out_a, out_b

    def denoise_nlm(self, params, albedo, normal):
        """zr_accum_denoise_nlm: Context.denoise_nlm(params, *halves(), variance(), ...) bit for bit, with halves and variance resolved on the device;
        returns (frame, error).  Whole-frame accumulators only."""
        albedo, normal, out, out_error = self._like((albedo, normal), (None, None))
        _check(self.lib.zr_accum_denoise_nlm(self._a, C.byref(params), albedo.ctypes.data, normal.ctypes.data, out.ctypes.data, out_error.ctypes.data))
        return out, out_error

    def temporal(self, history, scene, camera, seed, params=None):
        """zr_accum_temporal: history.accumulate(scene, camera, seed, resolve(), variance(), params) bit for bit, with colour and variance resolved on
        the device; returns (colour, variance, history length).  Whole-frame accumulators only."""
        params = params if params is not None else TemporalParams.defaults()
        out, out_variance, length = history._outputs()
        _check(self.lib.zr_accum_temporal(self._a, history._t, C.byref(params), scene._s, C.byref(camera), C.c_uint64(seed), out.ctypes.data,
                                          out_variance.ctypes.data, length.ctypes.data))
        return out, out_variance, length

    def sample_counts(self, out=None):
        """samples per pixel: (H, W) int32; only the region's pixels are written"""
        if out is None:
            out = np.zeros((self.height, self.width), dtype=np.int32)
        assert out.dtype == np.int32 and out.flags.c_contiguous and out.shape == (self.height, self.width)
        _check(self.lib.zr_accum_sample_counts(self._a, out.ctypes.data))
        return out

    def lane_sums(self):
        """the raw lane sums, (pixels, 3, 64) float64 with the pixels in plan (tile) order"""
        n = int(self.lib.zr_accum_lane_sums(self._a, None, 0))
        if n < 0:
            _check(n)
        out = np.zeros((n // 192, 3, 64), dtype=np.float64)
        got = int(self.lib.zr_accum_lane_sums(self._a, out.ctypes.data, out.size))
        if got < 0:
            _check(got)
        return out

    def state(self):
        out = (C.c_int64 * 4)()
        _check(self.lib.zr_accum_state(self._a, C.byref(out)))
        return {"first": out[0], "done": out[1], "pixels": out[2], "device_bytes": out[3]}

    def close(self):
        if self._a:
            self.lib.zr_accum_destroy(self._a)
            self._a = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Temporal:
    """The history of a width x height frame across a moving camera (zr_temporal): blended colour, variance, history length and the
    previous frame's geometry buffer and camera, all on the device.  track_motion: follow a world that Scene.refit moves (zr_temporal_track_motion,
    DESIGN §18) — one refit between two frames is reprojected through its motion table, anything else restarts the frame."""

    def __init__(self, ctx, width, height, track_motion=False):
        self.ctx = ctx
        self.lib = ctx.lib
        self.width, self.height = int(width), int(height)
        self._t = self.lib.zr_temporal_create(ctx._c, self.width, self.height)
        if not self._t:
            raise ZrError(self.lib.zr_last_error().decode())
        if track_motion:
            self.track_motion(True)

    def track_motion(self, on):
        """zr_temporal_track_motion: off (the default) leaves resetting after a refit to the caller"""
        _check(self.lib.zr_temporal_track_motion(self._t, 1 if on else 0))

    def _outputs(self):
        shape = (self.height, self.width, 3)
        return np.zeros(shape, dtype=np.float64), np.zeros(shape, dtype=np.float64), np.zeros(shape[:2], dtype=np.int32)

    def accumulate(self, scene, camera, seed, color, variance, params=None):
        """zr_temporal_accumulate: takes the frame (color, variance of the pixel means: (H, W, 3) float64) rendered from `camera` into the history;
        returns (colour, variance, history length) of the blend"""
        params = params if params is not None else TemporalParams.defaults()
        shape = (self.height, self.width, 3)
        color = np.ascontiguousarray(color, dtype=np.float64); variance = np.ascontiguousarray(variance, dtype=np.float64)
        if color.shape != shape or variance.shape != shape:
            raise ValueError(f"frame shapes {color.shape}, {variance.shape} differ from the history's {shape}")
        out, out_variance, length = self._outputs()
        _check(self.lib.zr_temporal_accumulate(self._t, C.byref(params), scene._s, C.byref(camera), C.c_uint64(seed), color.ctypes.data,
                                               variance.ctypes.data, out.ctypes.data, out_variance.ctypes.data, length.ctypes.data))
        return out, out_variance, length

    def reset(self):
        """forgets the history (the caller's duty after a scene change): the next frame starts at length 1"""
        _check(self.lib.zr_temporal_reset(self._t))

    def state(self):
        out = (C.c_int64 * 4)()
        _check(self.lib.zr_temporal_state(self._t, C.byref(out)))
        return {"width": out[0], "height": out[1], "frames": out[2]}

    def tracks_motion(self):
        """the switch track_motion sets: zr_temporal_state's fourth value"""
        out = (C.c_int64 * 4)()
        _check(self.lib.zr_temporal_state(self._t, C.byref(out)))
        return bool(out[3])

    def close(self):
        if self._t:
            self.lib.zr_temporal_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MOTION_STATIC, MOTION_CUT = 0xFFFFFFFF, 0xFFFFFFFE   # ZR_MOTION_STATIC, ZR_MOTION_CUT


def temporal_view(camera):
    """zr_temporal_view: the camera as the reprojection sees it (no device): dict of center, pixel00, w, a, b (3 each) and f"""
    out = (C.c_double * 16)()
    _check(load().zr_temporal_view(C.byref(camera), C.byref(out)))
    v = np.array(out[:], dtype=np.float64)
    return {"center": v[0:3], "pixel00": v[3:6], "w": v[6:9], "a": v[9:12], "b": v[12:15], "f": float(v[15])}


class Scene:
    def __init__(self, ctx, desc, tri_uv=None, animated=False):
        """tri_uv: per-vertex texture coordinates of the description's triangles, (n_tris, 3, 2) or (n_tris, 6) float64 = u0 v0 u1 v1 u2 v2 per
        triangle (zr_scene_set_triangle_uvs); None: the triangles carry none (u = v = 0 on every triangle hit).
        animated: the library copies the description's arrays (zr_scene_set_all) instead of borrowing them, so that update_ops / update_spheres /
        refit can move the committed world"""
        self.ctx = ctx
        self.lib = ctx.lib
        self._s = self.lib.zr_scene_create(ctx._c)
        if not self._s:
            raise ZrError(self.lib.zr_last_error().decode())
        # the description's arrays outlive this call (the caller holds them): no need for the library to copy 200 MB of triangles
        _check((self.lib.zr_scene_set_all if animated else self.lib.zr_scene_set_all_borrowed)(self._s, C.byref(desc)))
        if tri_uv is not None:
            uv = np.ascontiguousarray(tri_uv, dtype=np.float64)
            if uv.ndim not in (2, 3) or uv.size != uv.shape[0] * 6:
                raise ValueError(f"tri_uv must be (n_tris, 3, 2) or (n_tris, 6), not {uv.shape}")
            _check(self.lib.zr_scene_set_triangle_uvs(self._s, uv.ctypes.data, uv.shape[0]))   # (the library copies it)
        _check(self.lib.zr_scene_commit(self._s))

    def update_ops(self, first, ops):
        """zr_scene_update_xform_ops: replaces wrapper ops [first, first + len(ops)) of the committed scene (only a[3] may differ).  ops: a NumPy array
        with XformOp's layout, or a sequence of XformOp.  The scene is stale until refit()."""
        if isinstance(ops, np.ndarray):
            arr = np.ascontiguousarray(ops)
            assert arr.dtype.itemsize == C.sizeof(XformOp), "ops must have zr_xform_op's layout"
            ptr, n = arr.ctypes.data, len(arr)
        else:
            arr = (XformOp * len(ops))(*ops)
            ptr, n = C.cast(arr, C.c_void_p), len(ops)
        _check(self.lib.zr_scene_update_xform_ops(self._s, int(first), ptr, n))

    def update_spheres(self, first, cxyz_r):
        """zr_scene_update_spheres: replaces the numbers (cx, cy, cz, radius) of spheres [first, first + len(cxyz_r)).  Stale until refit()."""
        q = np.ascontiguousarray(cxyz_r, dtype=np.float64).reshape(-1, 4)
        _check(self.lib.zr_scene_update_spheres(self._s, int(first), q.ctypes.data, len(q)))

    def refit(self):
        """zr_scene_refit: the device scene made to agree with the updates -> dict of zr_refit_info"""
        info = RefitInfo()
        _check(self.lib.zr_scene_refit(self._s, C.byref(info)))
        return info.as_dict()

    def stats(self):
        out = (C.c_uint64 * 4)()
        _check(self.lib.zr_scene_stats(self._s, C.byref(out)))
        return {"bvh_pairs": out[0], "bvh_depth": out[1], "objects": out[2], "device_bytes": out[3],
                "traversal_stack": int(self.lib.zr_scene_traversal_stack(self._s)), "builder": self.lib.zr_scene_builder(self._s).decode()}

    def lights(self):
        """zr_scene_lights: the light table direct light sampling draws from -> array of LIGHT_SLOT_DTYPE, in table order"""
        n = self.lib.zr_scene_lights(self.ctx._c, self._s, None, 0)
        if n < 0:
            _check(n)
        out = np.zeros(n, dtype=LIGHT_SLOT_DTYPE)
        m = self.lib.zr_scene_lights(self.ctx._c, self._s, out.ctypes.data if n else None, n)
        if m < 0:
            _check(m)
        return out

    def env_light(self, env, arrays=True):
        """zr_scene_env_light: the environment table direct light sampling draws from under `env` -> dict: width, height, sampled, total, weighted,
        build_ms and, where it is sampled and arrays is set, row_cdf (H,) and cdf (H, W)"""
        info = EnvLightInfo()
        _check(self.lib.zr_scene_env_light(self.ctx._c, self._s, C.byref(env), C.byref(info), None, None))
        out = {"width": int(info.width), "height": int(info.height), "sampled": bool(info.sampled), "total": float(info.total), "weighted": int(info.weighted),
               "build_ms": float(info.build_ms)}
        if info.sampled and arrays:
            row, cdf = np.zeros(info.height), np.zeros((info.height, info.width))
            _check(self.lib.zr_scene_env_light(self.ctx._c, self._s, C.byref(env), C.byref(info), row.ctypes.data, cdf.ctypes.data))
            out["row_cdf"], out["cdf"] = row, cdf
        return out

    def kernels(self):
        """the kernel builds the committed scene renders through (zr_scene_kernels)"""
        out = (C.c_uint32 * 4)()
        _check(self.lib.zr_scene_kernels(self._s, C.byref(out)))
        return {"extend_level": out[0], "shade_lean": out[1], "fused_ok": out[2], "leaf_objects": out[3]}

    def render(self, camera, env, seed, region=None, count=False, out=None):
        h, w = camera.image_height, camera.image_width
        if out is None:
            out = np.zeros((h, w, 3), dtype=np.float64)
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (h, w, 3)
        rp = C.byref(region) if region is not None else None
        _check(self.lib.zr_render(self.ctx._c, self._s, C.byref(camera), C.byref(env), C.c_uint64(seed), rp,
                                  1 if count else 0, out.ctypes.data, None, None))
        return out

    def render_aov(self, camera, seed, z_depth_max_dist, region=None):
        """first-hit albedo / normal / z-depth passes (camera.hpp:464-488): three (H, W, 3) float64 frames"""
        h, w = camera.image_height, camera.image_width
        outs = [np.zeros((h, w, 3), dtype=np.float64) for _ in range(3)]
        ap = AovParams(float(z_depth_max_dist))
        rp = C.byref(region) if region is not None else None
        _check(self.lib.zr_render_aov(self.ctx._c, self._s, C.byref(camera), C.c_uint64(seed), rp, C.byref(ap),
                                      outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data))
        return outs

    def render_gbuffer(self, camera, seed):
        """zr_render_gbuffer: the first hit of every pixel's centre ray: dict of position (H, W, 3), normal (H, W, 3, unit), t (H, W) float64 and
        mat (H, W) uint32 (0xFFFFFFFF on a miss, where position holds the ray direction)"""
        h, w = max(camera.image_height, 1), max(camera.image_width, 1)
        g = {"position": np.zeros((h, w, 3)), "normal": np.zeros((h, w, 3)), "t": np.zeros((h, w)), "mat": np.zeros((h, w), dtype=np.uint32)}
        _check(self.lib.zr_render_gbuffer(self.ctx._c, self._s, C.byref(camera), C.c_uint64(seed), *[a.ctypes.data for a in g.values()]))
        return g

    def render_gbuffer_entries(self, camera, seed):
        """zr_render_gbuffer_entries: the world-list entry under each pixel of render_gbuffer, (H, W) uint32, 0xFFFFFFFF on a miss (animated scenes only)"""
        h, w = max(camera.image_height, 1), max(camera.image_width, 1)
        out = np.zeros((h, w), dtype=np.uint32)
        _check(self.lib.zr_render_gbuffer_entries(self.ctx._c, self._s, C.byref(camera), C.c_uint64(seed), out.ctypes.data))
        return out

    def motion(self):
        """zr_scene_motion: the motion table of the last refit -> (slot per world-list entry, uint32: MOTION_STATIC, MOTION_CUT or a record's index;
        records (n, 21) float64: a[12] rows of (linear 3, translation), nm[9] by rows)"""
        n = C.c_size_t(0)
        _check(self.lib.zr_scene_motion(self._s, None, None, 0, C.byref(n)))
        slot = np.zeros(n.value, dtype=np.uint32); rec = np.zeros((max(n.value, 1), 21))
        _check(self.lib.zr_scene_motion(self._s, slot.ctypes.data, rec.ctypes.data, n.value, C.byref(n)))
        used = slot[slot < MOTION_CUT]
        return slot, rec[:int(used.max()) + 1 if len(used) else 0].copy()

    PATH_RECORD = 17

    def trace_paths(self, camera, seed, requests, max_segments):
        """per-segment records of the primary samples (px, py, sample): (n, max_segments, 17) float64, see zr_trace_paths"""
        req = np.ascontiguousarray(requests, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((req.shape[0], max_segments, self.PATH_RECORD), dtype=np.float64)
        _check(self.lib.zr_trace_paths(self.ctx._c, self._s, C.byref(camera), C.c_uint64(seed), req.ctypes.data, req.shape[0], max_segments,
                                       out.ctypes.data))
        return out

    def render_passes(self, camera, env, seed, region=None):
        """beauty / reflection / refraction frames with the split enabled (camera.hpp:490-517): three (H, W, 3) float64 frames"""
        h, w = camera.image_height, camera.image_width
        outs = [np.zeros((h, w, 3), dtype=np.float64) for _ in range(3)]
        rp = C.byref(region) if region is not None else None
        _check(self.lib.zr_render_passes(self.ctx._c, self._s, C.byref(camera), C.byref(env), C.c_uint64(seed), rp,
                                         outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data))
        return outs

    def render_bvh_debug(self, camera, env, seed, params=None, region=None, out=None, keep_going=None, rows_done=None):
        """the BVH debug view (global_settings::bvh_debug_mode): (H, W, 3) float64.  keep_going: a ctypes.c_uint8 polled between
        kernel batches (0 cancels: ZR_E_CANCELLED is raised); rows_done: a ctypes.c_int advanced like camera::lines_rendered"""
        h, w = camera.image_height, camera.image_width
        if out is None:
            out = np.zeros((h, w, 3), dtype=np.float64)
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (h, w, 3)
        params = params if params is not None else BvhDebugParams.defaults()
        rp = C.byref(region) if region is not None else None
        _check(self.lib.zr_render_bvh_debug(self.ctx._c, self._s, C.byref(camera), C.byref(env), C.c_uint64(seed), rp, C.byref(params),
                                            out.ctypes.data, C.byref(keep_going) if keep_going is not None else None,
                                            C.byref(rows_done) if rows_done is not None else None))
        return out

    def trace_bvh_debug(self, rays, params=None, tmin=0.001, seed=1, pixel=0x7ACE, bounce=0):
        """bvh_node::hit in debug mode for (n, 6) rays -> array of BVH_DEBUG_HIT_DTYPE"""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        out = np.zeros(len(rays), dtype=BVH_DEBUG_HIT_DTYPE)
        params = params if params is not None else BvhDebugParams.defaults()
        _check(self.lib.zr_trace_bvh_debug(self.ctx._c, self._s, C.byref(params), rays.ctypes.data, len(rays), tmin, C.c_uint64(seed),
                                           C.c_uint64(pixel), bounce, out.ctypes.data))
        return out

    def tree_boxes(self):
        """every box of the committed trees (zr_scene_tree_boxes) -> array of TREE_BOX_DTYPE"""
        n = self.lib.zr_scene_tree_boxes(self._s, None, 0)
        if n < 0:
            _check(n)
        out = np.zeros(n, dtype=TREE_BOX_DTYPE)
        m = self.lib.zr_scene_tree_boxes(self._s, out.ctypes.data if n else None, n)
        if m < 0:
            _check(m)
        return out

    def render_device(self, camera, env, seed, d_ptr, stream=0, region=None, count=False):
        rp = C.byref(region) if region is not None else None
        _check(self.lib.zr_render_device(self.ctx._c, self._s, C.byref(camera), C.byref(env), C.c_uint64(seed), rp,
                                         1 if count else 0, C.c_void_p(d_ptr), C.c_void_p(stream)))

    def trace(self, rays, tmin=0.001, tmax=float("inf"), seed=1, pixel=0x7ACE, bounce=0):
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        n = rays.shape[0]
        out = np.zeros(n, dtype=HIT_DTYPE)
        _check(self.lib.zr_trace(self.ctx._c, self._s, rays.ctypes.data, n, tmin, tmax, C.c_uint64(seed),
                                 C.c_uint64(pixel), bounce, out.ctypes.data))
        return out

    # ---- per-function known-answer entry points (zr_kat_*) ----
    def kat_scatter(self, rays, hits, keys, first_draw=None):
        """material::scatter + emitted for (ray, hit record) pairs -> array of SCATTER_DTYPE"""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        fd = np.ascontiguousarray(first_draw, dtype=np.uint64) if first_draw is not None else None
        out = np.zeros(len(rays), dtype=SCATTER_DTYPE)
        _check(self.lib.zr_kat_scatter(self.ctx._c, self._s, rays.ctypes.data, hits.ctypes.data, keys.ctypes.data,
                                       fd.ctypes.data if fd is not None else None, len(rays), out.ctypes.data))
        return out

    def kat_shade_lean(self, rays, keys, first_draw=None):
        """the lean pair per call: closest hit over (0.001, inf), then lean_rec + lean_shade -> (array of HIT_DTYPE, array of SCATTER_DTYPE)"""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        fd = np.ascontiguousarray(first_draw, dtype=np.uint64) if first_draw is not None else None
        hits = np.zeros(len(rays), dtype=HIT_DTYPE)
        out = np.zeros(len(rays), dtype=SCATTER_DTYPE)
        _check(self.lib.zr_kat_shade_lean(self.ctx._c, self._s, rays.ctypes.data, keys.ctypes.data, fd.ctypes.data if fd is not None else None,
                                          len(rays), hits.ctypes.data, out.ctypes.data))
        return hits, out

    def kat_texture(self, tex, uvp):
        uvp = np.ascontiguousarray(uvp, dtype=np.float64).reshape(-1, 5)
        out = np.zeros((len(uvp), 3))
        _check(self.lib.zr_kat_texture(self.ctx._c, self._s, int(tex), uvp.ctypes.data, len(uvp), out.ctypes.data))
        return out

    def kat_background(self, env, dirs):
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        out = np.zeros((len(dirs), 3))
        _check(self.lib.zr_kat_background(self.ctx._c, self._s, C.byref(env), dirs.ctypes.data, len(dirs), out.ctypes.data))
        return out

    def close(self):
        if self._s:
            self.lib.zr_scene_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
