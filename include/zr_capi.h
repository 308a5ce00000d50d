/* zr_capi.h — C ABI of the MI355X path-tracing integrator ("zr" = Zenith replacement).
 *
 * The reference (jarek1992/raytracer_project) has no FFI: its seam is the C++ virtual API
 *   hittable::hit / bounding_box          /root/reference/hittable.hpp:29-36
 *   material::scatter / emitted           /root/reference/material.hpp:7-31
 *   texture::value                        /root/reference/texture.hpp:6-10
 *   camera::render(world, env, post, flag) /root/reference/camera.hpp:236
 * and its objects keep all data private.  The drop-in therefore has two layers:
 *   (1) include/zenith/ — C++20 classes with the reference's names, constructors and signatures whose
 *       camera::render() flattens the world and calls
 *   (2) this C ABI — plain pointers and sizes, no C++ or torch types — implemented by
 *       raytracer_project_amd/csrc (libzr_hip.so).  It is what a cgo/JNI/ctypes binding would bind.
 *
 * Every entry point names the reference interface it replaces.  All arithmetic on the path is FP64,
 * as in the reference (vec3 is 3 x double, /root/reference/vec3.hpp:7-115).
 *
 * Ownership: every pointer is caller-owned; the library copies on set_*.  A zr_ctx is bound to one HIP
 * device and must be used from one host thread at a time.  Functions returning int return 0 on
 * success and a negative ZR_E_* code otherwise; zr_last_error() describes the last failure of the
 * calling thread.  Nothing throws across this boundary.
 */
#ifndef ZR_CAPI_H
#define ZR_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZR_ABI_VERSION 3

enum {
    ZR_OK = 0,
    ZR_E_INVALID = -1,  /* bad argument / inconsistent scene */
    ZR_E_DEVICE = -2,   /* HIP runtime error (no device, launch failure, out of memory) */
    ZR_E_STATE = -3,    /* call order violated (e.g. render before commit) */
    ZR_E_CANCELLED = -4, /* render_flag went false; partial results were written */
    ZR_E_NOMEM = -5      /* device memory exhausted where the library could not work around it (it first shrinks its own buffers) */
};

/* ---- primitive / object kinds ------------------------------------------------------------- */
enum {
    ZR_PRIM_SPHERE = 0,   /* sphere            /root/reference/sphere.hpp:5-89 */
    ZR_PRIM_TRIANGLE = 1, /* triangle          /root/reference/triangle.hpp:5-110 */
    ZR_PRIM_CUBE = 2,     /* cube              /root/reference/cube.hpp:7-143 */
    ZR_PRIM_MEDIUM = 3,   /* constant_medium   /root/reference/constant_medium.hpp:24-87 */
    ZR_PRIM_GROUP = 6     /* a run of triangles (zr_group) placed as ONE object: what a wrapper around a mesh is in the reference
                             (translate / rotate_* / scale / material_instance holding a model or a bvh_node, scene_management.hpp:
                             112-117): the run is stored and built once however many objects name it (two-level BVH) */
};

/* instance wrappers (applied outermost first to the ray, innermost first to the hit record) */
enum {
    ZR_OP_TRANSLATE = 0, /* translate          /root/reference/translate.hpp:6-41   a = offset */
    ZR_OP_ROTATE_X = 1,  /* rotate_x (degrees) /root/reference/rotate_x.hpp:7-80    a[0]=sin a[1]=cos */
    ZR_OP_ROTATE_Y = 2,  /* rotate_y (radians) /root/reference/rotate_y.hpp:7-83    a[0]=sin a[1]=cos */
    ZR_OP_ROTATE_Z = 3,  /* rotate_z (degrees) /root/reference/rotate_z.hpp:7-77    a[0]=sin a[1]=cos */
    ZR_OP_SCALE = 4,     /* scale              /root/reference/scale.hpp:5-45       a = factors */
    ZR_OP_MATERIAL = 5   /* material_instance  /root/reference/material_instance.hpp:5-41  mat = id */
};

typedef struct zr_xform_op {
    uint32_t kind; /* ZR_OP_* */
    uint32_t mat;  /* ZR_OP_MATERIAL: material id */
    double a[3];
} zr_xform_op;

/* one entry of the world list (what hittable_list::add received, hittable_list.hpp:24-27) */
typedef struct zr_object {
    uint32_t type;        /* ZR_PRIM_* */
    uint32_t index;       /* index into that type's array */
    uint32_t chain_first; /* first wrapper op (outermost) in the op array */
    uint32_t chain_count; /* number of wrapper ops, 0 = bare primitive */
} zr_object;

/* triangles [first_triangle, first_triangle + triangle_count) of the triangle arrays, in their own (object) space; they are not
 * world-list entries themselves.  A zr_object of type ZR_PRIM_GROUP with index = position in the group array places the run
 * under that object's wrapper chain; several objects may place the same group. */
typedef struct zr_group {
    uint32_t first_triangle;
    uint32_t triangle_count;
} zr_group;

/* constant_medium(boundary, density, tex|color): boundary is a sphere or cube entry that is not
 * itself part of the world list; `mat` is the id of a ZR_MAT_ISOTROPIC material. */
typedef struct zr_medium {
    uint32_t boundary_type;  /* ZR_PRIM_SPHERE or ZR_PRIM_CUBE */
    uint32_t boundary_index;
    uint32_t chain_first;    /* wrappers applied to the boundary (inside the medium) */
    uint32_t chain_count;
    uint32_t mat;
    uint32_t pad_;
    double neg_inv_density;  /* -1/density, constant_medium.hpp:30,37 */
} zr_medium;

/* ---- materials and textures --------------------------------------------------------------- */
enum {
    ZR_MAT_LAMBERTIAN = 0, /* material.hpp:58-108 */
    ZR_MAT_METAL = 1,      /* material.hpp:111-163   param = fuzz (already clamped to <= 1) */
    ZR_MAT_DIELECTRIC = 2, /* material.hpp:166-242   param = refraction index, tint = albedo colour */
    ZR_MAT_LIGHT = 3,      /* diffuse_light, material.hpp:245-279 */
    ZR_MAT_ISOTROPIC = 4   /* isovolumetric, constant_medium.hpp:9-22 */
};

#define ZR_NO_TEXTURE 0xFFFFFFFFu

typedef struct zr_material {
    uint32_t kind;          /* ZR_MAT_* */
    uint32_t tex;           /* albedo / emission texture id (unused by dielectric) */
    uint32_t bump_tex;      /* bump map texture id or ZR_NO_TEXTURE (material.hpp:35-54) */
    uint32_t pad_;
    double param;           /* fuzz or refraction index */
    double bump_strength;
    double tint[3];         /* dielectric albedo */
} zr_material;

enum {
    ZR_TEX_SOLID = 0,     /* solid_color     texture.hpp:86-102 */
    ZR_TEX_CHECKER = 1,   /* checker_texture texture.hpp:104-133 */
    ZR_TEX_IMAGE_U8 = 2,  /* image_texture, 8-bit RGB   texture.hpp:12-84 */
    ZR_TEX_IMAGE_F32 = 3  /* image_texture, float RGB (HDR) */
};

/* A texture tree has at most this many checkers above any leaf (solid or image) and no cycle: the device's texture::value walks
 * ZR_MAX_CHECKER_DEPTH + 1 textures at most.  zr_scene_commit refuses a scene that holds a deeper tree (ZR_E_INVALID). */
#define ZR_MAX_CHECKER_DEPTH 15

typedef struct zr_texture {
    uint32_t kind;      /* ZR_TEX_* */
    uint32_t odd, even; /* checker: child texture ids */
    uint32_t width, height; /* image, each at most INT_MAX; 0 x 0 = the reference's "missing image" cyan fallback */
    uint32_t pad_;
    uint64_t texel_offset;  /* byte offset of the first texel inside the texel blob */
    double inv_scale;       /* checker */
    double color[3];        /* solid */
} zr_texture;

/* ---- environment: EnvironmentSettings, /root/reference/environment.hpp:8-76 ---------------- */
enum { ZR_ENV_PHYSICAL_SUN = 0, ZR_ENV_HDR_MAP = 1, ZR_ENV_SOLID_COLOR = 2 };

typedef struct zr_env {
    uint32_t mode;        /* ZR_ENV_* (same order as EnvironmentSettings::Mode) */
    uint32_t hdr_texture; /* texture id of an IMAGE_F32 texture, or ZR_NO_TEXTURE */
    double background_color[3];
    double intensity;
    double hdri_rotation, hdri_tilt, hdri_roll; /* radians */
    double sun_direction[3];
    double sun_color[3];
    double sun_intensity;
    double sun_size;
} zr_env;

/* ---- camera: the public fields camera::render reads, /root/reference/camera.hpp:26-57 ------- */
typedef struct zr_camera {
    int32_t image_width, image_height;
    int32_t samples_per_pixel;
    int32_t max_depth;
    double vfov;
    double lookfrom[3], lookat[3], vup[3];
    double defocus_angle;
    double focus_dist;
} zr_camera;

/* which part of the frame one call renders.  Pixels are visited in 2-D tiles of tile_size x tile_size;
 * tile t (row-major tile index) is rendered iff t % tile_mod == tile_rem — the interleaved pixel-tile
 * sharding across GPUs.  The rectangle [x0,x0+w) x [y0,y0+h) further restricts the
 * pixels (used by parity tests); w = h = 0 means the full frame. */
typedef struct zr_region {
    int32_t x0, y0, w, h;
    int32_t tile_size; /* 0 = default (32) */
    int32_t tile_mod;  /* 0 or 1 = every tile */
    int32_t tile_rem;
    int32_t tile_skew; /* 0: tile t (row-major index) belongs to the part t % tile_mod; s > 0: tile (tx, ty) belongs to (tx + s * ty) % tile_mod — a lattice
                          instead of the near-vertical stripes t % tile_mod makes when the tiles per row are a multiple of tile_mod / 2 (1920 / 32 = 60 tiles per
                          row over 8 ranks: a rank then owns the same two tile columns in every row, and the ranks under the middle of the picture are 4 %
                          slower than the others; with skew 3: round 4, profiles/r4_shards.txt).  (This word was padding until round 4: 0 keeps the old map.) */
} zr_region;

/* counters of the last zr_render on a context (collected only when `collect_counters` was set:
 * the counting kernel variant is slower and is never the timed one) */
typedef struct zr_counters {
    uint64_t primary_samples;
    uint64_t segments;       /* closest-hit queries = "ray·bounces" */
    uint64_t nodes_tested;   /* BVH child boxes tested */
    uint64_t spheres_tested;
    uint64_t triangles_tested;
    uint64_t cubes_tested;
    uint64_t media_tested;
    uint64_t hits;           /* segments that found a surface / medium event */
    uint64_t rng_draws;      /* main-stream draws */
    /* wave-scheduler statistics of the EXTEND kernel (counting build): executions of the NODE / LEAF phase and the lanes that were
     * ready at each execution (lanes / (64 * execs) = SIMT utilisation of the phase); shade_execs is unused by the pipeline; shade_lanes:
     * the slots the lean SHADE kernel shaded, i.e. the segments EXTEND traced for it (= segments - escaped); zero on every other build */
    uint64_t node_execs, node_lanes, leaf_execs, leaf_lanes, shade_execs, shade_lanes;
    uint64_t rounds;         /* kernel variant 2: EXTEND/SHADE rounds of the last render */
    double extend_ms, shade_ms; /* kernel variant 2: device time of the EXTEND / SHADE launches of the last render */
    double kernel_ms;        /* device time of the render kernels of the last call (hipEvents) */
    uint64_t path;           /* which kernels rendered the last frame: 0 pixel-group megakernel (fallback), 2 streaming pipeline
                                (EXTEND / SHADE rounds), 3 fused small-scene kernel (worlds of at most ZR_FUSED_MAX objects) — ABI 3 */
    uint64_t escaped;        /* kernel variant 2: of `segments`, those the lean SHADE kernel finished itself because the scattered ray provably
                                leaves the world (never reached EXTEND); 0 with ZR_SHADE_ESCAPE=0 and on every other path */
} zr_counters;

/* hit record returned by zr_trace (debug / known-answer entry): hit_record, hittable.hpp:9-26 */
typedef struct zr_hit {
    double p[3], normal[3], tangent[3], bitangent[3];
    double t, u, v;
    uint32_t mat;       /* material id, 0xFFFFFFFF on a miss */
    uint32_t front_face;
} zr_hit;

/* a whole flattened world as borrowed arrays (layouts as in the zr_scene_set_* calls below) */
typedef struct zr_scene_desc {
    const double* spheres;      const uint32_t* sphere_mat;   uint64_t n_spheres;
    const double* tri_v;        const double* tri_n;          const uint32_t* tri_mat; uint64_t n_tris;
    const double* cubes;        const uint32_t* cube_mat;     uint64_t n_cubes;
    const zr_medium* media;     uint64_t n_media;
    const zr_xform_op* ops;     uint64_t n_ops;
    const zr_object* objects;   uint64_t n_objects; /* 0 = implicit world list */
    const zr_material* materials; uint64_t n_materials;
    const zr_texture* textures; uint64_t n_textures;
    const void* texels;         uint64_t texel_bytes;
    const zr_group* groups;     uint64_t n_groups;   /* ABI 2 */
} zr_scene_desc;

typedef struct zr_ctx zr_ctx;
typedef struct zr_scene zr_scene;

/* ---- lifetime ----------------------------------------------------------------------------- */
int zr_abi_version(void);
const char* zr_last_error(void);
zr_ctx* zr_create(int device_ordinal); /* NULL on failure (no HIP device => fails loudly) */
void zr_destroy(zr_ctx*);

/* ---- scene: replaces building a hittable_list / bvh_node of reference objects -------------- */
zr_scene* zr_scene_create(zr_ctx*);
void zr_scene_destroy(zr_scene*);
/* sphere(center, radius, mat): 4 doubles per sphere = cx, cy, cz, radius (raw ctor argument) */
int zr_scene_set_spheres(zr_scene*, const double* cxyz_r, const uint32_t* mat, size_t n);
/* triangle(a,b,c,n0,n1,n2,mat): 9 doubles of vertices, 9 doubles of vertex normals */
int zr_scene_set_triangles(zr_scene*, const double* v9, const double* n9, const uint32_t* mat, size_t n);
/* per-vertex texture coordinates of the triangles given by zr_scene_set_triangles / _set_all / _set_all_borrowed:
 * 6 doubles per triangle = u0, v0, u1, v1, u2, v2 (vertex order of v9).  The array is copied.  n must equal the current triangle count and every
 * value must be finite (ZR_E_INVALID otherwise, nothing changed); uv6 == NULL with n == 0 removes the coordinates, and so does every later call that
 * replaces the triangles.  A hit on a triangle then carries the interpolated (u, v) and a world-space tangent frame; without
 * coordinates u = v = 0 and the frame is zero, as the reference's triangle::hit leaves them. */
int zr_scene_set_triangle_uvs(zr_scene*, const double* uv6, size_t n);
/* cube: 12 doubles = half_extents, center, min_p, max_p exactly as the cube members (cube.hpp:92-97) */
int zr_scene_set_cubes(zr_scene*, const double* hcmm12, const uint32_t* mat, size_t n);
int zr_scene_set_media(zr_scene*, const zr_medium*, size_t n);
int zr_scene_set_xform_ops(zr_scene*, const zr_xform_op*, size_t n);
/* the world list.  If never called, every sphere/triangle/cube/medium that is not a medium boundary
 * is a bare top-level object. */
int zr_scene_set_objects(zr_scene*, const zr_object*, size_t n);
/* runs of triangles that ZR_PRIM_GROUP objects place (needs an explicit world list: the implicit one would also list the
 * runs' triangles as bare objects) */
int zr_scene_set_groups(zr_scene*, const zr_group*, size_t n);
int zr_scene_set_materials(zr_scene*, const zr_material*, size_t n);
int zr_scene_set_textures(zr_scene*, const zr_texture*, size_t n, const void* texel_blob, size_t texel_bytes);
/* all of the above in one call */
int zr_scene_set_all(zr_scene*, const zr_scene_desc*);
/* the same without the copies: the library keeps POINTERS to the geometry arrays of `desc` (spheres, triangles, cubes, media, ops,
 * objects, texels — 216 MB for a million triangles) and reads them during the next zr_scene_commit, after which it forgets them.
 * The caller keeps them valid and unchanged until that commit has returned.  The small tables (materials, textures) are copied. */
int zr_scene_set_all_borrowed(zr_scene*, const zr_scene_desc*);
/* builds the flattened BVH (replaces bvh_node's constructor, bvh.hpp:11-44) and uploads to HBM */
int zr_scene_commit(zr_scene*);
/* sizes of the committed scene: out[0]=bvh nodes (child-pair records), [1]=max depth, [2]=objects,
 * [3]=device bytes */
int zr_scene_stats(const zr_scene*, uint64_t out[4]);
/* which kernel builds the committed scene renders through: out[0] = the EXTEND build (0 bare triangles / spheres, 1 + cubes and
 * unwrapped media, 2 + wrapped objects and media, 3 + placed runs of triangles; ZR_EXTEND_LEVEL may only raise it), [1] = 1 for
 * SHADE's lean build, [2] = 1 when the world may take the fused small-scene kernel (zr_counters::path 3), [3] = leaf objects */
int zr_scene_kernels(const zr_scene*, uint32_t out[4]);
/* traversal-stack bound of the committed scene: the exact worst-case number of entries one ray's stack can hold while
 * walking the 4-wide tree (the recursion depth of bvh_node::hit, bvh.hpp:46-54, has no bound in the reference; here the
 * per-wave spill slabs are sized from this number, so no scene can overrun them); 0 = not committed */
uint32_t zr_scene_traversal_stack(const zr_scene*);
/* which builder made the committed tree: "host (binned SAH)" (zr_bvh.cpp) or "device (PLOC)" (zr_build.hip).  The tree is
 * built on the device for worlds of at least ZR_BVH_DEVICE_MIN world-list entries; ZR_BVH_BUILD=device|host forces one.  Replaces
 * bvh_node's constructor (/root/reference/bvh.hpp:11-44), which the reference runs on every render restart (main.cpp:1492-1500). */
const char* zr_scene_builder(const zr_scene*);

/* ---- moving worlds: update placements in place, refit the trees on the device ---------------- */
/* A committed scene whose arrays were COPIED (zr_scene_set_* / zr_scene_set_all; not zr_scene_set_all_borrowed, whose arrays the commit releases) can be
 * moved without a new commit.  What can move: the parameters a[3] of wrapper ops (a translate's offset, a rotation's sin / cos, a scale's factors) and the
 * four numbers of spheres that are leaf primitives of their own.  The tree keeps its topology: the moved entries' records and boxes are rewritten, and the
 * boxes of the world's trees are fitted anew on the device, level by level.  A refitted scene answers every ray as a fresh commit of the moved world would
 * (closest hit does not depend on the tree); how good the old topology still is for the new positions shows in zr_refit_info::area_ratio, and when to commit
 * anew is the caller's call.
 *   zr_scene_update_xform_ops  replaces ops [first, first + n) of the committed op array.  Only a[3] may differ from the committed op.
 *   zr_scene_update_spheres    replaces the numbers (cx, cy, cz, radius) of spheres [first, first + n).
 *     Both change the scene's host copy and mark the scene STALE; they do not touch the device and do not clear "committed".  ZR_E_STATE: the scene is not
 *     committed, or was committed from borrowed arrays.  ZR_E_INVALID, with NOTHING changed: NULL, a range that leaves the committed arrays, a value that is
 *     not finite, an op whose kind or mat differs from the committed one, a sphere that is a medium's boundary or sits inside a generic wrapper chain, or a
 *     change after which a world-list entry would be stored in another form than the commit chose (a uniform scale over a baked sphere made non-uniform, a
 *     scale factor of a placed cube set to 0): such a world needs a new commit.
 *     While a scene is stale every entry point that reads the device scene (zr_render*, zr_trace*, zr_kat_*, zr_render_gbuffer, zr_scene_tree_boxes, the
 *     accumulator and temporal entries) returns ZR_E_STATE, "scene updated but not refitted".
 *   zr_scene_refit             makes the device scene agree with the updates since the last refit: queued on the context's stream, so renders on that
 *     context follow it; one stream synchronisation (the new root box is a kernel argument).  With nothing stale it still runs (dirty_entries = 0): a
 *     legal way to ask for area_ratio.  ZR_E_STATE as for the updates.  On ANY failure the scene becomes uncommitted — a render then says "commit first";
 *     a moved box that no 4-wide node's grid can hold (not finite, beyond 1e30) is such a failure (ZR_E_INVALID, "commit anew").  The first refit after a
 *     commit builds its state (reverse indices, schedule, device buffers) and is slower; later ones allocate nothing.  (A world of at most ZR_FUSED_MAX
 *     objects also re-reads the fused kernel's argument copy.)
 * An accumulator binds (scene, epoch): a batch after a refit is refused like a batch with another scene (ZR_E_INVALID) until zr_accum_reset.  A zr_temporal
 * must be reset by the caller after a refit unless it tracks motion (zr_temporal_track_motion below): then it follows the refit's own motion table.
 *   zr_scene_motion            known-answer entry: the motion table of the LAST refit, i.e. of the one step epoch - 1 -> epoch.  Every refit
 *     replaces it, a refit with nothing dirty leaves it empty, a commit drops it.  Per world-list entry out_slot_per_entry holds ZR_MOTION_STATIC (the refit
 *     did not touch the entry), ZR_MOTION_CUT (it moved but cannot be followed: a radius or scale factor of 0 before or after, or a value that is not finite;
 *     its pixels get no history) or the index of its record.  A record is 21 doubles, FP64 in a fixed operation order: a[12], row k = a[4k .. 4k+2] linear and
 *     a[4k+3] translation, of A = M_prev M_now^-1, which takes a world point of the entry now to where that point of the entry was before the refit; then
 *     nm[9] by rows, (A_lin)^-T, for normals.  M is the entry's object-to-world map: its chain innermost first (translate p + a; rotate co a - sn b,
 *     sn a + co b; scale p a; a medium's inner chain inside the entry's own; a leaf sphere's own x -> c + max(0, r) x innermost).  *out_count = world-list
 *     entries; both arrays, when given, must have room for `capacity` >= that many entries (at most one record per entry); both may be NULL to ask for the
 *     count.  ZR_E_STATE: not committed, stale, or committed from borrowed arrays.
 * Out of scope, each needs a new commit: triangle vertices and cubes' own numbers; adding or removing entries; material or texture changes; the triangles
 * inside a group (a placement of the group may move; the group's own tree is never touched).  The motion table describes ONE refit: batch all updates of a
 * frame into one refit. */
#define ZR_MOTION_STATIC 0xFFFFFFFFu
#define ZR_MOTION_CUT 0xFFFFFFFEu
typedef struct zr_refit_info {
    uint64_t epoch;          /* refits applied to this commit (0 after zr_scene_commit) */
    uint32_t dirty_entries;  /* world-list entries whose record or box was recomputed (media reached through their inner chain included) */
    uint32_t levels;         /* launches of the 4-wide refit kernel = levels of the world's 4-wide tree below its root */
    double area_ratio;       /* sum of the half-areas of the world tree's pair boxes now / over the committed world, both as the refit computes them:
                                exactly 1.0 when everything is where the commit had it */
    double host_ms;          /* wall time of the call */
    double device_ms;        /* of it, device time from the first patch copy to the last tree kernel (HIP events) */
} zr_refit_info;
int zr_scene_update_xform_ops(zr_scene*, size_t first, const zr_xform_op* ops, size_t n);
int zr_scene_update_spheres(zr_scene*, size_t first, const double* cxyz_r, size_t n);
int zr_scene_refit(zr_scene*, zr_refit_info* out /* may be NULL */);
int zr_scene_motion(const zr_scene*, uint32_t* out_slot_per_entry, double* out_records21, size_t capacity, size_t* out_count);

/* ---- render: replaces camera::render's sample loop (camera.hpp:236-248, 404-579) ----------- */
/* Fills out_rgb[(j*W+i)*3 + c] (host memory, W*H*3 doubles, row 0 = top, mean over spp — the layout of
 * camera::render_accumulator) for the pixels of `region`; other pixels are left untouched.
 * `keep_going` (may be NULL) is polled between kernel batches and has render_flag's polarity
 * (camera.hpp:441): *keep_going == 0 stops the render (ZR_E_CANCELLED, finished batches are written).
 * `rows_done` (may be NULL) is advanced like camera::lines_rendered (camera.hpp:548-552): while the frame renders it holds
 * H x the finished fraction of the frame's samples (the pipeline finishes samples all over the frame, not row by row) and
 * it is set to H at the end (camera.hpp:576-578).  When rows_done is given, out_rgb is also refreshed a few times per
 * second (ZR_PREVIEW_PERIOD_S, default 0.2) with the mean of the samples finished so far — the live preview the
 * reference's GUI reads from render_accumulator mid-render (main.cpp:1576); the final image does not depend on it. */
int zr_render(zr_ctx*, const zr_scene*, const zr_camera*, const zr_env*, uint64_t seed,
              const zr_region* region, int collect_counters,
              double* out_rgb, volatile const uint8_t* keep_going, volatile int* rows_done);
/* Same, but the accumulator stays in HBM: d_out_rgb is a device pointer to W*H*3 doubles and the kernels run on
 * `hip_stream` (a hipStream_t, NULL = default stream), ordered after work already enqueued there.  The call BLOCKS until
 * the frame is complete: the streaming pipeline's round loop reads the active-path count back every few rounds, so the
 * stream is synchronised internally and is idle on return (no D2H copy of the frame takes place).  This is what the
 * multi-GPU host uses before the RCCL exchange. */
int zr_render_device(zr_ctx*, const zr_scene*, const zr_camera*, const zr_env*, uint64_t seed,
                     const zr_region* region, int collect_counters,
                     void* d_out_rgb, void* hip_stream);

/* ---- progressive accumulation: a frame rendered in batches of samples (camera::current_samples_count) --------------------
 * A zr_accum is device memory that carries a frame from one batch of samples to the next: for every pixel of the plan of
 * (width, height, region) — the region's pixels, not the frame's — 64 lane sums x 3 doubles (1536 bytes per pixel) and the
 * sample range [first, first + done) they hold.  Sample s of a pixel always belongs to lane s % 64 and a lane adds its samples
 * in increasing s: that is the order zr_render's reduce uses, so ANY split of [0, N) into consecutive batches resolves to the
 * image zr_render gives at samples_per_pixel = N, bit for bit, and every prefix [0, k) is the k-spp image.  (A sum of batch
 * means would differ in the last bits.)
 *   zr_accum_create       NULL (zr_last_error says why) for a bad size or region; the partials start at zero, first = 0
 *   zr_accum_reset        zeroes the partials; the next batch starts at first_sample >= 0; forgets the camera / seed / scene
 *   zr_render_accumulate  renders the samples [first + done, first + done + n_samples) of every pixel of the accumulator's plan
 *                         and adds them.  camera.samples_per_pixel is ignored.  Takes the route zr_render would (pipeline, fused
 *                         kernel, pixel-group kernel); a batch must fit its route in one run (ZR_E_NOMEM otherwise: ask for fewer
 *                         samples).  ZR_E_INVALID: n_samples < 1, a camera of another size, or — after the first batch since
 *                         create / reset — a camera, seed or scene that differs from that batch's.  A cancelled batch
 *                         (*keep_going == 0) is discarded whole: ZR_E_CANCELLED, accumulator unchanged.  zr_get_counters
 *                         afterwards reports this batch.
 *   zr_accum_resolve      out_rgb (host, W*H*3 doubles) / d_out_rgb (device, on `hip_stream`, complete on return) receive the mean
 *                         of the `done` samples in the plan's pixels; other pixels are untouched.  ZR_E_STATE while done == 0.
 *                         Leaves the partials alone: callable after every batch.
 *   zr_accum_state        out = first, done, pixels, device bytes held */
typedef struct zr_accum zr_accum;
zr_accum* zr_accum_create(zr_ctx*, int width, int height, const zr_region* region);
void zr_accum_destroy(zr_accum*);
int zr_accum_reset(zr_accum*, int first_sample);
int zr_render_accumulate(zr_ctx*, const zr_scene*, const zr_camera*, const zr_env*, uint64_t seed, zr_accum*, int n_samples,
                         int collect_counters, volatile const uint8_t* keep_going);
int zr_accum_resolve(zr_accum*, double* out_rgb);
int zr_accum_resolve_device(zr_accum*, void* d_out_rgb, void* hip_stream);
int zr_accum_state(const zr_accum*, int64_t out[4]);

/* ---- adaptive sampling: further samples only for the pixels that are still noisy -----------------------------
 * With k = 64 m samples in a pixel every lane holds exactly m of them, so the 64 lane sums S_l are 64 equally weighted,
 * independent estimates of the pixel.  Their spread gives the noise estimate (FP64, in this order, no contraction):
 *   v_l = S_l.r + S_l.g + S_l.b;  T = sum v_l (xor butterfly 32, 16, ... 1);  mu = T * (1.0 / 64);  d_l = v_l - mu;
 *   Q = sum d_l * d_l (same butterfly);  se = sqrt(Q * (1.0 / 63) * (1.0 / 64)) * (1.0 / m);  I = mu * (1.0 / m);
 *   err = se / (I + dark_floor)          0 exactly when Q == 0 (all lanes equal), +inf when T is not finite
 * i.e. the standard error of the mean of the channel sum, relative to the channel sum.  tests/adaptive_model.py restates it.
 *   zr_render_adaptive   pass 0 brings every pixel of the accumulator's plan to min_samples (the accumulator is fresh, or holds
 *                        uniform batches with done a multiple of 64 and <= min_samples: ZR_E_STATE otherwise); every later pass
 *                        gives step_samples more to the pixels still active.  After each pass a pixel stays active iff
 *                        err > threshold and its count + step_samples <= max_samples; a pixel that stopped never restarts, so
 *                        the active pixels share one count, counts lie in {min + j * step} and A PIXEL THAT STOPPED AT k SAMPLES IS
 *                        THAT PIXEL OF THE k-spp zr_render FRAME, BIT FOR BIT (first = 0).  The loop ends when no pixel is active.
 *                        Passes take zr_render_accumulate's route and must fit it in one run (ZR_E_NOMEM: lower step_samples;
 *                        the accumulator is as the last complete pass left it).  *keep_going is looked at between passes and
 *                        inside them; a cancelled or failed pass is discarded whole (ZR_E_CANCELLED or its error code).
 *                        The parameters are checked before anything else, device or other arguments: ZR_E_INVALID for a count
 *                        that is not a positive multiple of 64, max_samples < min_samples, a threshold or floor that is negative or
 *                        not finite; then for the camera, seed or scene mismatches zr_render_accumulate refuses.  Once a pass
 *                        has completed the accumulator is NON-UNIFORM: zr_render_accumulate and zr_render_adaptive return
 *                        ZR_E_STATE until zr_accum_reset; resolve (1.0 / the pixel's own count) and the queries below keep
 *                        working; zr_accum_state's `done` is the largest per-pixel count.  `out` (may be NULL) receives the
 *                        statistics of the passes that completed, on every return (zeros when the call was refused); zr_get_counters afterwards holds the totals over all passes.
 *   zr_accum_error       the estimate of the current sums with this dark_floor, W*H doubles; ZR_E_STATE on a uniform accumulator
 *                        whose done is not a multiple of 64
 *   zr_accum_sample_counts  the per-pixel sample counts, W*H int32
 *   zr_accum_lane_sums   a known-answer entry like zr_trace: the raw sums, [pixel][channel][lane] with the pixels in plan (tile)
 *                        order, 192 doubles each; returns their number (out may be NULL with cap_doubles = 0 to ask for it) or a
 *                        negative ZR_E_* (ZR_E_STATE, the size query included, while nothing has been rendered; then ZR_E_INVALID:
 *                        cap_doubles too small)
 * The three queries write only the plan's pixels of W*H arrays and return ZR_E_STATE while nothing has been rendered. */
typedef struct zr_adaptive_params {
    int32_t min_samples, max_samples, step_samples;   /* positive multiples of 64, min <= max */
    int32_t pad_;
    double threshold;                                  /* a pixel goes on while err > threshold; 0: every pixel with any spread */
    double dark_floor;                                 /* 0.01 keeps near-black pixels from demanding samples for invisible noise */
} zr_adaptive_params;
typedef struct zr_adaptive_stats {
    uint64_t passes;                 /* passes completed (pass 0 included) */
    uint64_t samples;                /* primary samples rendered */
    uint64_t stopped_by_threshold;   /* pixels that stopped with err <= threshold */
    uint64_t stopped_at_max;         /* pixels still above the threshold when max_samples stopped them */
} zr_adaptive_stats;
int zr_render_adaptive(zr_ctx*, const zr_scene*, const zr_camera*, const zr_env*, uint64_t seed, zr_accum*, const zr_adaptive_params*,
                       int collect_counters, volatile const uint8_t* keep_going, zr_adaptive_stats* out);
int zr_accum_error(zr_accum*, double dark_floor, double* out);
int zr_accum_sample_counts(zr_accum*, int32_t* out);
int64_t zr_accum_lane_sums(zr_accum*, double* out, size_t cap_doubles);

/* ---- first-hit AOV passes: the albedo / normal / z-depth part of render_rows (camera.hpp:433, 464-488, 521-541) ---- */
/* For the first min(clamp(spp / 8, 64, 1024), spp) samples of every pixel the primary hit contributes
 *   albedo  += rec.mat->get_albedo(rec)                       (material.hpp:29-31,99-102,154-156,226-229,266-275)
 *   normal  += (unit(rec.normal) . (u, v, w) + 1) / 2          camera space; a miss adds (0.5, 0.5, 1.0)
 *   z-depth += 1 - clamp(rec.t / z_depth_max_dist, 0, 1)       as a grey colour
 * and the sums are divided by the number of those samples.  Same seeds and the same primary rays as zr_render.
 * Output buffers are W*H*3 doubles in host memory, laid out like out_rgb; a NULL buffer skips that pass. */
typedef struct zr_aov_params {
    double z_depth_max_dist; /* post_processor::z_depth_max_dist */
} zr_aov_params;
int zr_render_aov(zr_ctx*, const zr_scene*, const zr_camera*, uint64_t seed, const zr_region* region, const zr_aov_params*,
                  double* out_albedo, double* out_normal, double* out_zdepth);

/* The render with the reflection / refraction split enabled (camera.hpp:490-517, use_reflection || use_refraction): per
 * primary sample, after the beauty path, the first hit is scattered a second time (fresh draws: the sample's stream just
 * continues) and a second path of max_depth - 1 bounces is traced; its radiance, luma-clamped to 2.0 (0.2126 |c|), times
 * the attenuation goes to the reflection frame when the scattered direction is within acos(0.9) of the mirror direction,
 * else to the refraction frame when it points below the surface.  Frames are W*H*3 doubles, means over spp (light_scale,
 * camera.hpp:531-533); a NULL buffer skips that frame.  out_beauty equals zr_render's image.  zr_get_counters afterwards
 * reports primary samples, segments (both paths), hits and RNG draws of the call. */
int zr_render_passes(zr_ctx*, const zr_scene*, const zr_camera*, const zr_env*, uint64_t seed, const zr_region* region,
                     double* out_beauty, double* out_reflection, double* out_refraction);

/* ---- after the sample loop -------------------------------------------------------------------
 * zr_post_process = camera::process_framebuffer_to_image up to the PNG encoder (camera.hpp:701-780): optional bloom
 * (bloom.hpp:18-68 on the 2^exposure-scaled frame), optional sharpening (color_processing.hpp:207-227), then per pixel
 * x 2^exposure, post_processor::process (color_processing.hpp:76-147: x exposure, colour balance, contrast about 0.18,
 * vignette, hue/saturation in HSV, ACES, debug views, clamp, gamma 1/2.2) and (unsigned char)(255.999 c).  A data pass
 * (albedo, normals, z-depth, reflection, refraction frames) is only clamped and, if apply_gamma, gamma-corrected.
 * frame_rgb: W*H*3 doubles (host); out_rgb8: W*H*3 bytes (host).  Byte-exact with the reference. */
typedef struct zr_post_params {      /* post_processor, color_processing.hpp:46-75 */
    float exposure, saturation, contrast, hue_shift, vignette_intensity;
    float bloom_threshold, bloom_intensity;
    int32_t bloom_radius;
    double color_balance[3];
    double sharpen_amount;
    int32_t use_aces_tone_mapping, use_bloom, use_sharpening;
    int32_t debug_red, debug_green, debug_blue, debug_luminance, debug_bvh;
} zr_post_params;
int zr_post_process(zr_ctx*, const zr_post_params*, const double* frame_rgb, int width, int height, int is_data_pass, int apply_gamma,
                    uint8_t* out_rgb8);
/* post_processor::analyze_framebuffer (color_processing.hpp:150-183): maximum luminance, log2-mean luminance and the
 * 256-bin log-luminance histogram that auto-exposure (apply_auto_exposure, 186-205) and the GUI plot read */
typedef struct zr_image_stats {
    float average_luminance, max_luminance;
    int32_t histogram[256];
} zr_image_stats;
int zr_analyze_frame(zr_ctx*, const double* frame_rgb, size_t n_pixels, zr_image_stats* out);

/* ---- denoising: step 4 of camera::render (camera.hpp:268-291) -------------------------------------------------------
 * zr_denoise fills the role of the reference's apply_denoising (camera.hpp:581-699), but it is NOT Intel OIDN and does not
 * reproduce OIDN's output (OIDN is a trained network whose weights the reference does not ship).  It is an edge-avoiding
 * a-trous wavelet filter (Dammertz et al., HPG 2010) in FP32, guided by the first-hit albedo and normal frames of
 * zr_render_aov and, optionally, its z-depth frame.  Per pixel every input is cleaned (NaN / Inf -> 0; the reference
 * cleans only the guides), the normal is decoded from the [0,1] camera-space encoding (n = normalize(2e - 1), "no
 * information" when |2e - 1| < 1e-6) and, with demodulate_albedo, the colour is divided by the albedo (channels <= 1e-3
 * count as 1).  `iterations` levels of the 5 x 5 B3-spline kernel at steps 1, 2, 4, ... then weight each tap by
 *   exp(-|t(d_p) - t(d_q)|^2 / (sigma_color^2 4^-level))   t(x) = x / (1 + luminance(x)): tone-compressed colour distance
 *   max(0, n_p . n_q)^sigma_normal                          1 when either normal carries no information
 *   exp(-|a_p - a_q|^2 / sigma_albedo^2)
 *   exp(-|z_p - z_q| / sigma_depth)                          only with a depth frame and sigma_depth > 0
 * taps outside the frame are skipped; the result is multiplied back by the albedo and widened to double.  Deterministic
 * (a fixed tap order, no atomics).  The exact arithmetic is restated in NumPy by tests/denoise_model.py; DESIGN §9.
 * All frames are W*H*3 doubles in host memory, row-major like out_rgb; zdepth may be NULL, out may equal color.
 * The defaults below are what camera::render uses with use_denoiser. */
typedef struct zr_denoise_params {
    int32_t iterations;                 /* levels, 0..8; 0 = demodulate / remodulate only (identity up to FP32 rounding) */
    int32_t demodulate_albedo;          /* filter c / albedo instead of c */
    float sigma_color, sigma_normal, sigma_albedo, sigma_depth;   /* > 0; sigma_depth <= 0: depth guide off */
} zr_denoise_params;
/* defaults: chosen on 8-spp renders of cfg5 and mix0 against 1024 spp.  Demodulation is off: the 8-spp albedo
 * pass is itself noisy on textures, and dividing by it cost more than it saved on the textured scene. */
#define ZR_DENOISE_DEFAULT_ITERATIONS 5
#define ZR_DENOISE_DEFAULT_DEMODULATE 0
#define ZR_DENOISE_DEFAULT_SIGMA_COLOR 1.5f
#define ZR_DENOISE_DEFAULT_SIGMA_NORMAL 64.0f
#define ZR_DENOISE_DEFAULT_SIGMA_ALBEDO 0.25f
int zr_denoise(zr_ctx*, const zr_denoise_params*, const double* color, const double* albedo, const double* normal,
               const double* zdepth, int width, int height, double* out);

/* ---- variance-guided denoising: the filter above with the colour weight driven by each pixel's own noise ----
 * zr_accum_variance   the variance of every pixel's mean per channel, W*H*3 doubles laid out like out_rgb; only the plan's pixels
 *                     are written.  With k = 64 m samples in a pixel and lane sums S_l, per channel (FP64, in this order, no contraction):
 *                       T = sum S_l (xor butterfly 32, 16, ... 1);  mu = T * (1.0 / 64);  d_l = S_l - mu;
 *                       Q = sum d_l * d_l (same butterfly);  var = Q * (1.0 / 63) * (1.0 / 64) * (1.0 / m) * (1.0 / m)
 *                     0 exactly when all lanes are equal, +inf when T is not finite.  zr_accum_error's state rules: ZR_E_INVALID for
 *                     NULL, ZR_E_STATE while nothing has been rendered or on a uniform accumulator whose done is not a multiple
 *                     of 64; a non-uniform accumulator (after zr_render_adaptive) uses each pixel's own count.
 * zr_denoise_guided   the spatial stage of SVGF (Schied et al., HPG 2017, section 4.4) laid over zr_denoise: cleaning, normal decoding,
 *                     demodulation, taps, w_n, w_a, w_z and t(x) are zr_denoise's.  The variance frame is cleaned like the colour
 *                     (NaN / Inf -> 0), negative values count as 0, and with demodulate_albedo it is divided by albedo^2.  At every
 *                     level, with r = 1 / (1 + max(luminance(d), 0)) and s_q = r_q^2 (V_q.r + V_q.g + V_q.b) — the expected squared length
 *                     of the noise of t(d_q) — and s^_p the 3 x 3 Gaussian ([1 2 1] x [1 2 1] / 16, unit spacing at every level, taps off
 *                     the frame skipped and the weights renormalised) of s around p, the colour term of a tap's weight is
 *                       exp(-|t(d_p) - t(d_q)|^2 / (sigma_variance^2 s^_p + epsilon))
 *                     in place of exp(-|..|^2 / (sigma_color^2 4^-level)): colour differences are measured in standard deviations of the
 *                     pixel's own noise.  Colour and variance are filtered together, d'_p = sum w d_q / sum w and
 *                     V'_p = sum w^2 V_q / (sum w)^2 per channel.  A pixel without variance (background, a converged flat wall) has the
 *                     denominator epsilon: it keeps its value unless its neighbours agree with it.  `variance` may come from
 *                     zr_accum_variance or from anywhere else.  All frames W*H*3 doubles in host memory; zdepth and out_variance
 *                     may be NULL, out may equal color and out_variance may equal variance.  ZR_E_INVALID, before any device call:
 *                     NULL, sizes as zr_denoise, iterations outside 0..8, a sigma or epsilon that is not positive and finite
 *                     (sigma_depth: >= 0, 0 = no depth guide).  FP32, deterministic; tests/denoise_guided_model.py restates it.
 * zr_accum_denoise    zr_denoise_guided(zr_accum_resolve(), zr_accum_variance(), ...) bit for bit, with colour and variance resolved
 *                     on the device straight into the filter: only the guides go up and only the result comes down.  Whole-frame
 *                     accumulators only (ZR_E_INVALID for one made with a rectangle or tile_mod > 1); then zr_accum_variance's state
 *                     rules.  out_variance may be NULL. */
typedef struct zr_denoise_guided_params {
    int32_t iterations;                 /* levels, 0..8 */
    int32_t demodulate_albedo;          /* filter c / albedo (and variance / albedo^2) */
    float sigma_variance;               /* > 0: colour differences are measured in standard deviations of the pixel's own noise */
    float sigma_normal, sigma_albedo, sigma_depth;   /* as zr_denoise */
    float epsilon;                      /* > 0, finite: added to the variance term's denominator */
} zr_denoise_guided_params;
/* defaults: the setting of scripts/dev/denoise_guided_sweep.py with the best worse-of-two-scenes factor on 64-spp accumulators of
 * cfg5 and mix0 against 4096 spp; what camera::render uses with denoise_variance_guided.  Demodulation is on here: the
 * albedo pass of a 64-spp frame is clean enough to divide by, and it won on cfg5 at every sigma_variance. */
#define ZR_DENOISE_GUIDED_DEFAULT_ITERATIONS 4
#define ZR_DENOISE_GUIDED_DEFAULT_DEMODULATE 1
#define ZR_DENOISE_GUIDED_DEFAULT_SIGMA_VARIANCE 3.0f
#define ZR_DENOISE_GUIDED_DEFAULT_SIGMA_NORMAL 64.0f
#define ZR_DENOISE_GUIDED_DEFAULT_SIGMA_ALBEDO 0.25f
#define ZR_DENOISE_GUIDED_DEFAULT_EPSILON 1e-8f
int zr_accum_variance(zr_accum*, double* out_var);
int zr_denoise_guided(zr_ctx*, const zr_denoise_guided_params*, const double* color, const double* variance, const double* albedo,
                      const double* normal, const double* zdepth, int width, int height, double* out, double* out_variance);
int zr_accum_denoise(zr_accum*, const zr_denoise_guided_params*, const double* albedo, const double* normal, const double* zdepth,
                     double* out, double* out_variance);
/* ---- dual-buffer non-local-means denoising: the two halves of an accumulator's samples filter each other ----
 * Rousselle, Knaus, Zwicker, "Adaptive rendering with non-local means filtering" (SIGGRAPH Asia 2012): patch distances normalised by the
 * per-pixel variance, a variance-cancellation term subtracted from every squared difference, and cross filtering — the weights computed
 * from one half of the samples average the other half, so they are independent of the noise they average.
 * zr_accum_halves     the two half images, W*H*3 doubles each, laid out like out_rgb; only the plan's pixels are written.  The resolve
 *                     butterfly stopped one step early: per pixel with k = 64 m samples, per channel (FP64, no contraction), the xor butterfly
 *                     32, 16, 8, 4, 2 over the lane sums leaves T_A (the even lanes) in lane 0 and T_B (the odd lanes) in lane 1;
 *                       A = T_A * (1.0 / (k / 2));  B = T_B * (1.0 / (k / 2))
 *                     For k a power of two (A + B) * 0.5 is the streaming resolve (T_A + T_B) * (1.0 / k) bit for bit.  zr_accum_variance's
 *                     state rules.
 * zr_denoise_nlm      half_a / half_b: the two half images; variance: of the FULL pixel mean (zr_accum_variance, or anything else).  Cleaning,
 *                     normal decoding and the albedo divisor a' are zr_denoise's.  uA = clean(A) / a', uB = clean(B) / a',
 *                     Vh = 2 max(clean(variance), 0) / (a' a') (a half has twice the variance of the whole), V^ = the 3 x 3 Gaussian of Vh per
 *                     channel by zr_denoise_guided's stencil rules.  With clamp() moving a coordinate to the nearest frame pixel, for a buffer u,
 *                     pixels s and t, channel c:
 *                       delta_c = ((u_s - u_t)^2 - alpha (V^_s + min(V^_t, V^_s))) / (epsilon + k^2 (V^_s + V^_t))
 *                       e(s, t) = ((delta_x + delta_y) + delta_z) * (1/3)
 *                       e_D(s) = e(s, clamp(s + D));   D_D(p) = the mean of e_D(clamp(p + tau)) over tau in [-f, f]^2 (tau_y outer, tau_x inner)
 *                       w_u(p, D) = exp(-max(D_D(p), 0)) w_a w_n for q = p + D inside the frame (no weight outside; w_a, w_n: zr_denoise's albedo
 *                       and normal weights between p and q); the centre tap has weight 1
 *                       fB_p = sum_D w_uA(p, D) uB_q / sum_D w_uA(p, D), fA_p likewise with the weights of uB on uA; D in [-r, r]^2, Dy outer, Dx inner
 *                       out = ((fA + fB) * 0.5) * a';   out_error = (((fA - fB) * 0.5) * a')^2 per channel
 *                     out_error is a one-degree-of-freedom estimate of the output's variance.  All frames W*H*3 doubles in host memory;
 *                     out_error may be NULL, out may equal half_a.  ZR_E_INVALID, before any device call: parameters first (search_radius
 *                     outside 0..10, patch_radius outside 0..3, k, a sigma or epsilon that is not positive and finite, alpha negative or not
 *                     finite), then NULL and sizes as zr_denoise.  FP32, deterministic, independent of the kernel's tiling;
 *                     tests/denoise_nlm_model.py restates it as evaluated (zr_nlm.hip's header).
 * zr_accum_denoise_nlm  zr_denoise_nlm(zr_accum_halves(), zr_accum_variance(), ...) bit for bit, resolved on the device straight into the filter.
 *                     Whole-frame accumulators only (ZR_E_INVALID otherwise); then zr_accum_variance's state rules.  out_error may be NULL. */
typedef struct zr_denoise_nlm_params {
    int32_t search_radius;              /* r: taps q = p + D, D in [-r, r]^2; 0..10 */
    int32_t patch_radius;               /* f: patches of (2f+1)^2 pixels; 0..3 */
    int32_t demodulate_albedo;          /* filter halves / albedo (and variance / albedo^2) */
    int32_t pad_;
    float k;                            /* > 0: distance scale (the paper's k) */
    float alpha;                        /* >= 0: strength of the variance cancellation */
    float sigma_normal, sigma_albedo;   /* as zr_denoise */
    float epsilon;                      /* > 0, finite: added to the distance's denominator */
} zr_denoise_nlm_params;
/* defaults: the cheapest setting of scripts/dev/denoise_nlm_sweep.py within 2 % of the best worse-of-two-scenes factor on 64-spp accumulators
 * of cfg5 and mix0 against 4096 spp; what camera::render uses with denoise_nlm.  The sweep began at r 5, f 1, k 0.45.  Demodulation is off
 * here: dividing by the albedo lost on the textured scene at every setting — the patches already tell texture from noise. */
#define ZR_DENOISE_NLM_DEFAULT_SEARCH_RADIUS 7
#define ZR_DENOISE_NLM_DEFAULT_PATCH_RADIUS 1
#define ZR_DENOISE_NLM_DEFAULT_DEMODULATE 0
#define ZR_DENOISE_NLM_DEFAULT_K 0.7f
#define ZR_DENOISE_NLM_DEFAULT_ALPHA 1.0f
#define ZR_DENOISE_NLM_DEFAULT_SIGMA_NORMAL 64.0f
#define ZR_DENOISE_NLM_DEFAULT_SIGMA_ALBEDO 0.25f
#define ZR_DENOISE_NLM_DEFAULT_EPSILON 1e-10f
int zr_accum_halves(zr_accum*, double* out_a, double* out_b);
int zr_denoise_nlm(zr_ctx*, const zr_denoise_nlm_params*, const double* half_a, const double* half_b, const double* variance,
                   const double* albedo, const double* normal, int width, int height, double* out, double* out_error);
int zr_accum_denoise_nlm(zr_accum*, const zr_denoise_nlm_params*, const double* albedo, const double* normal, double* out, double* out_error);
/* ---- firefly-robust resolve: a Gini-trimmed mean over the accumulator's lanes ------------------------------------
 * After Buisine et al., "Firefly removal in Monte Carlo rendering with adaptive Median of meaNs" (EGSR 2021).  With k = 64 m samples in a pixel the
 * 64 lane sums S_l = (x, y, z) are 64 equally weighted, independent estimates of it; the rule rates how unequal they are, trims whole lanes by rank
 * symmetrically — from no trim (zr_accum_resolve's mean) to the median pair — and averages the rest.  Per pixel (FP64, in this order, no contraction;
 * tests/robust_model.py restates it; `sum` is the xor butterfly 32, 16, ... 1 in lane order, as in zr_accum_variance):
 *   key     v_l = (S_l.x + S_l.y) + S_l.z.  A lane is BAD when v_l is not finite; n_bad counts them; k_l = v_l, or +inf for a bad lane.
 *   rank    r_l = #{ j : k_j < k_l, or k_j == k_l and j < l } with IEEE < and == (-0.0 ties with 0.0): a stable total order, defined by counting and
 *           so independent of how a kernel finds it.  The good lanes hold the ranks 0 .. 63 - n_bad.
 *   Gini    K = the key of the good lane of highest rank (the largest finite key), 0.0 if every lane is bad;  k^_l = k_l, or K for a bad lane;
 *           T = sum k^_l;  A = sum (double)(2 r_l - 63) * k^_l;
 *           g = 1.0 if T or A is not finite, else 0.0 if T <= 0.0, else q = A / (64.0 * T), q < 0.0 -> 0.0, q > 1.0 -> 1.0
 *   trim    ZR_ROBUST_GINI: x = strength * g, x > 1.0 -> 1.0, t = min((int)floor(x * 32.0), 31);  ZR_ROBUST_FIXED: t = trim;
 *           then t = max(t, min(n_bad, 31)).  Lane l is KEPT iff t <= r_l <= 63 - t: n_k = 64 - 2 t >= 2 lanes, none of them bad while n_bad <= 31.
 *   colour  per channel c: Tk = sum (kept ? S_l.c : 0.0);  out_c = Tk * (1.0 / (double)(m * n_k))
 *   variance of that mean, per channel: mu = Tk * (1.0 / n_k);  d_l = kept ? S_l.c - mu : 0.0;  Q = sum d_l * d_l;
 *           var = Q * (1.0 / (n_k - 1)) * (1.0 / n_k) * inv_m * inv_m with inv_m = 1.0 / m; +inf when Tk is not finite (zr_accum_variance's rule)
 *   n_bad >= 32: colour and variance are +inf in every channel and t = 31.
 * With t = 0 the colour is zr_accum_resolve of the streaming route and the variance is zr_accum_variance, both bit for bit.  Whole lanes are trimmed by ONE
 * key, so a kept lane keeps all three channels and no colour shift appears.  A trimmed mean of a skewed distribution is biased low: the feature is opt-in.
 * zr_accum_resolve_robust  out_rgb, out_variance (may be NULL): W*H*3 doubles laid out like zr_accum_resolve's; out_trim (may be NULL): W*H int32, the
 *                     pixel's t.  Only the plan's pixels are written (region and tiled accumulators included); the partials are left alone.
 *                     zr_accum_variance's state rules (a non-uniform accumulator uses each pixel's own count).
 * zr_kat_resolve_robust    a known-answer entry like zr_kat_scatter: the same kernel on n_pix pixels of caller-supplied lane sums ([n_pix][3][64]) with
 *                     counts[n_pix]; the outputs are n_pix-long (x 3 for the first two) in input order, out_variance and out_trim may be NULL.
 * ZR_E_INVALID before any device call: NULL (params, then the other arguments), mode outside {0, 1}, trim outside 0..31, strength negative or not finite;
 * for the known-answer entry also a count that is not a positive multiple of 64.  Both fields are checked in both modes. */
#define ZR_ROBUST_GINI 0
#define ZR_ROBUST_FIXED 1
typedef struct zr_robust_params {
    int32_t mode;        /* ZR_ROBUST_GINI 0, ZR_ROBUST_FIXED 1 */
    int32_t trim;        /* FIXED: lanes trimmed at each end, 0..31 */
    double strength;     /* GINI: >= 0, finite; 0 = the plain mean unless lanes are bad */
} zr_robust_params;
/* default: scripts/dev/robust_sweep.py on 64-, 128- and 256-spp accumulators of cfg5 and mix0 against 4096 spp */
#define ZR_ROBUST_DEFAULT_STRENGTH 1.0
int zr_accum_resolve_robust(zr_accum*, const zr_robust_params*, double* out_rgb, double* out_variance, int32_t* out_trim);
int zr_kat_resolve_robust(zr_ctx*, const zr_robust_params*, const double* lane_sums, const int32_t* counts, size_t n_pix,
                          double* out_rgb, double* out_variance, int32_t* out_trim);
/* ---- temporal accumulation: a frame's history reprojected across a moving camera ------------------------------
 * The temporal stage of SVGF (Schied et al., HPG 2017, section 4.1) for a camera path; through a world that zr_scene_refit moves when the history tracks motion
 * (zr_temporal_track_motion).  The reference has no counterpart.
 * zr_render_gbuffer    the first hit of the ray through the centre of every pixel (get_center_ray, camera.hpp:809-814: origin `center`, direction
 *                      (pixel00_loc + i pixel_delta_u + j pixel_delta_v) - center; no jitter, no defocus disk), W*H pixels row-major: by definition what
 *                      zr_trace(those rays, tmin 0.001, tmax inf, seed, pixel = ZR_GBUFFER_STREAM, bounce 0) returns — constant-medium hits included — as
 *                      position rec.p, unit normal, t and material id.  A miss holds the ray DIRECTION in the position plane, normal 0, t 0 and
 *                      mat 0xFFFFFFFF.  Host memory; any output may be NULL.  Argument checks and error codes as zr_render_aov.
 * zr_temporal          the history of a width x height frame on the device, double-buffered in FP64: blended colour and variance, history length, the
 *                      previous frame's geometry buffer and the previous camera.  zr_temporal_reset forgets it (the caller's duty after any change of the
 *                      scene — a zr_scene_refit included unless the history tracks motion); zr_temporal_state: out = width, height, frames accumulated since
 *                      create / reset, 1 when it tracks motion else 0.
 * zr_temporal_accumulate  takes one frame — `color` and `variance` (of the pixel means, e.g. zr_accum_resolve / zr_accum_variance), W*H*3 doubles in host
 *                      memory — makes the camera's geometry buffer and, per pixel p (FP64, no contraction; tests/temporal_model.py restates it):
 *                        c, V: the inputs with NaN / Inf -> 0 and V <= 0 -> 0 (zr_denoise_guided's rules);
 *                        the first hit X_p is projected into the previous camera (a miss: its direction, so the sky follows rotation only): a point that is
 *                        not in front of it has no history; coordinates within 2^-20 px of a whole pixel snap to it, so an unchanged camera and
 *                        whole-pixel shifts reproject exactly;
 *                        the four bilinear taps q count when their weight is > 0, they lie in the frame, hold history, mat_q == mat_p and, for hits,
 *                        |(X_q - X_p) . n_p| <= plane_tolerance depth_p and n_p . n_q >= normal_cos;
 *                        no counting tap: N = 1, out = c, V_out = V (also the whole first frame after create / reset).  Else, over the counting taps,
 *                        h = sum w h_q / sum w, Vh = sum w V_q / sum w, N = min(min N_q + 1, max_history), beta = max(1 / N, alpha),
 *                        out = h + beta (c - h), V_out = (1 - beta)^2 Vh + beta^2 V;
 *                      out, V_out, N and the geometry buffer become the history.  out_color / out_variance (W*H*3 doubles) and out_history (W*H int32) are
 *                      host memory and may each be NULL; the first two may be handed to zr_denoise_guided as they are.  ZR_E_INVALID before any device
 *                      work: parameters out of range or not finite (checked first), NULL, a camera of another size or without a finite view, a scene or
 *                      history of another context; ZR_E_STATE: scene not committed.  Limits: a moving world needs zr_temporal_track_motion; mirrors, glass and
 *                      media reproject by their first hit (reflections of moving objects are not followed); the filtered image is not fed back.
 * zr_accum_temporal    zr_temporal_accumulate(zr_accum_resolve(), zr_accum_variance(), ...) bit for bit, resolved on the device straight into the kernel.
 *                      Whole-frame accumulators only (ZR_E_INVALID otherwise); then zr_accum_variance's state rules.
 * zr_temporal_track_motion  on != 0: the history remembers (scene, commit, epoch) of the frame it holds, and zr_temporal_accumulate / zr_accum_temporal choose:
 *                        same scene, commit and epoch: the path above;
 *                        same scene and commit, epoch exactly one more: per pixel the world-list entry under it is looked up in the refit's motion table
 *                        (zr_scene_motion).  STATIC or a miss: the path above.  CUT: no history (N = 1).  A record: Xr = A X_p, nr = Nm n_p / |Nm n_p| (no
 *                        history unless that length is > 0); Xr is what is projected into the previous camera, the plane test is
 *                        |(X_q - Xr) . nr| <= plane_tolerance depth_p with depth_p still of X_p in the current camera, the normal test nr . n_q >= normal_cos
 *                        (tests/temporal_motion_model.py restates it);
 *                        anything else — another scene, a new commit, two or more refits since the held frame — restarts the frame (N = 1 everywhere, as
 *                        after zr_temporal_reset) instead of ghosting.  So batch ALL updates of a frame into ONE zr_scene_refit.
 *                      Default off: the behaviour above, the caller's duty to reset included.  Switching changes nothing the history holds.
 * zr_render_gbuffer_entries  known-answer entry: the world-list entry under each pixel of zr_render_gbuffer, 0xFFFFFFFF on a miss.  Builds the host half of the
 *                      scene's refit state if there is none; ZR_E_STATE for a scene committed from borrowed arrays, as the updates say.
 * zr_temporal_view     known-answer entry, no device: the camera as the reprojection sees it, out = center 3, pixel00 3, unit w 3, a = du / (du . du) 3,
 *                      b = dv / (dv . dv) 3, focus_dist — from the quantities zr_render derives (camera::initialize, camera.hpp:358-399). */
#define ZR_GBUFFER_STREAM 0xFFFFFFFEull   /* the `pixel` of the geometry buffer's RNG keys: ray k draws from zr_stream_key(seed, ZR_GBUFFER_STREAM, k) */
int zr_render_gbuffer(zr_ctx*, const zr_scene*, const zr_camera*, uint64_t seed, double* out_position, double* out_normal, double* out_t, uint32_t* out_mat);
typedef struct zr_temporal zr_temporal;
typedef struct zr_temporal_params {
    double alpha;            /* floor of the blend weight, in (0, 1]; 1 = no reuse */
    int32_t max_history;     /* 1..65535 */
    int32_t pad_;
    double plane_tolerance;  /* > 0: |(X_q - X_p) . n_p| <= plane_tolerance * depth_p */
    double normal_cos;       /* in [-1, 1]: n_p . n_q >= normal_cos */
} zr_temporal_params;
/* defaults: the setting of scripts/dev/temporal_sweep.py with the best worse-of-two-scenes factor of the guided filter on the temporal frame, on 8-frame paths of
 * 64-spp frames of cfg5 and mix0 against 4096 spp; what camera::render uses with temporal_accumulation.  The sweep began at alpha 0.2 and plane_tolerance
 * 0.01: on the textured scene the repeated bilinear resampling costs more than the longer memory of a smaller alpha gains. */
#define ZR_TEMPORAL_DEFAULT_ALPHA 0.4
#define ZR_TEMPORAL_DEFAULT_MAX_HISTORY 32
#define ZR_TEMPORAL_DEFAULT_PLANE_TOLERANCE 0.03
#define ZR_TEMPORAL_DEFAULT_NORMAL_COS 0.9
zr_temporal* zr_temporal_create(zr_ctx*, int width, int height);
void zr_temporal_destroy(zr_temporal*);
int zr_temporal_reset(zr_temporal*);
int zr_temporal_state(const zr_temporal*, int64_t out[4]);
int zr_temporal_accumulate(zr_temporal*, const zr_temporal_params*, const zr_scene*, const zr_camera*, uint64_t seed, const double* color,
                           const double* variance, double* out_color, double* out_variance, int32_t* out_history);
int zr_accum_temporal(zr_accum*, zr_temporal*, const zr_temporal_params*, const zr_scene*, const zr_camera*, uint64_t seed, double* out_color,
                      double* out_variance, int32_t* out_history);
int zr_temporal_view(const zr_camera*, double out[16]);
int zr_temporal_track_motion(zr_temporal*, int on);
int zr_render_gbuffer_entries(zr_ctx*, zr_scene*, const zr_camera*, uint64_t seed, uint32_t* out_entry);

/* post_processor::apply_sharpening (color_processing.hpp:207-227) on its own: interior pixels become
 * c (1 - amount) + (5 c - the four neighbours) amount, border pixels are copied.  Double in, double out, byte-exact with
 * the reference; amount <= 0 copies.  Host memory, W*H*3 doubles; out may equal in. */
int zr_sharpen_frame(zr_ctx*, const double* in, int width, int height, double amount, double* out);

/* ---- BVH debug view: global_settings::bvh_debug_mode (bvh.hpp:46-110, aabb.hpp:44-84, camera.hpp:455-461, 928-953, 989-1004) ----
 * The reference's wireframe rule applied to the device's own trees: the nodes are the binary sibling-pair records; depth 0
 * is a tree's root box (the union of its first record's two child boxes), the children of a box at depth d sit at depth d + 1, a leaf is
 * a child box that holds a primitive range, "left" is child slot 0, boxes are the stored FP32 planes widened to double.  The tree of a
 * placed run of triangles (ZR_PRIM_GROUP) restarts at depth 0 and is walked in the placement's space.  Per node: the box is entered with
 * aabb::hit's arithmetic on the interval narrowed by the best hit so far; a node of the current level (depth == level, or a leaf for
 * level -1) whose entry point r.at(t_in + 0.0001f) or exit point r.at(t_out - 0.0001f) lies within
 * float(thickness * (0.05f + t_in * 0.1f)) of the planes of at least two axes is an EDGE hit at t_in (entry on the edge) or t_out and
 * emits (0.4, g, 1 - g) * 4, g = min(depth * 0.15f, 1); otherwise the walk goes on, left child first, and a hit below a current-level
 * node is re-coloured (0.4, g, 1 - g) * 0.1f (VOLUME; the outermost tree's such node wins).  The frame (zr_render_bvh_debug) is the
 * mean over spp of: the background on a primary miss; the debug colour on an edge / volume hit; emitted + attenuation * c on a surface
 * hit whose material scatters, where c is the secondary ray's debug colour, its surface's emission if longer than 0.1 or (0.01, 0.01,
 * 0.01), and 0 on a miss or with max_depth < 2.  Primary rays, RNG streams and scattering are zr_render's. */
typedef struct zr_bvh_debug_params {
    int32_t level;    /* global_settings::debug_bvh_level: -1 = leaves, 0 = the root, ...; below -1 is refused */
    float thickness;  /* global_settings::bvh_thickness: > 0 and finite */
} zr_bvh_debug_params;
#define ZR_BVH_DEBUG_DEFAULT_LEVEL -1
#define ZR_BVH_DEBUG_DEFAULT_THICKNESS 0.01f
/* box ids: the child box in slot s of pair record r is 2 r + s; the root box of the tree whose first record is R is ZR_BVH_ROOT_BOX | R.
 * A tree is named by R (0 = the world's tree). */
#define ZR_BVH_ROOT_BOX 0x80000000u
#define ZR_BVH_NO_BOX 0xFFFFFFFFu
enum { ZR_BVH_MISS = 0, ZR_BVH_EDGE = 1, ZR_BVH_VOLUME = 2, ZR_BVH_SURFACE = 3 };
/* the debug view's answer for one ray */
typedef struct zr_bvh_debug_hit {
    zr_hit hit;          /* SURFACE: the record zr_trace gives for that hit; EDGE / VOLUME: t, p = r.at(t), normal (0, 0, 1) (the volume's t is that of
                            the hit beneath it); mat = 0xFFFFFFFF unless SURFACE */
    double color[3];     /* what the hit emits: the edge / volume colour, or the surface material's emitted(u, v, p) */
    uint32_t cls;        /* ZR_BVH_MISS / EDGE / VOLUME / SURFACE */
    int32_t depth;       /* the deciding box's depth (EDGE: the edge's node, VOLUME: the current-level ancestor, SURFACE: the leaf); -1 on a miss */
    uint32_t tree;       /* ... its tree (first pair record of the tree) */
    uint32_t box;        /* ... its box id */
} zr_bvh_debug_hit;
/* camera::render with global_settings::bvh_debug_mode set: fills out_rgb like zr_render (host memory, W*H*3 doubles, region, keep_going polled
 * and rows_done advanced between kernel batches).  ZR_E_INVALID for a level below -1 or a thickness that is not a positive finite number. */
int zr_render_bvh_debug(zr_ctx*, const zr_scene*, const zr_camera*, const zr_env*, uint64_t seed, const zr_region* region,
                        const zr_bvh_debug_params*, double* out_rgb, volatile const uint8_t* keep_going, volatile int* rows_done);
/* known-answer entry: bvh_node::hit in debug mode on the interval (tmin, inf) for n rays (6 doubles each); the medium draw of ray k is keyed
 * by zr_stream_key(seed, pixel, k) and `bounce`, as in zr_trace */
int zr_trace_bvh_debug(zr_ctx*, const zr_scene*, const zr_bvh_debug_params*, const double* rays6, size_t n, double tmin, uint64_t seed,
                       uint64_t pixel, uint32_t bounce, zr_bvh_debug_hit* out);
/* every box of the committed trees, as the debug view walks them */
typedef struct zr_tree_box {
    float lo[3], hi[3];   /* the stored FP32 planes (a root: the union of its record's non-empty children) */
    uint32_t id;          /* box id (above) */
    uint32_t tree;        /* first pair record of its tree (0 = the world's) */
    uint32_t parent;      /* parent's box id, ZR_BVH_NO_BOX for a root */
    int32_t depth;
    uint32_t slot;        /* child slot in the parent's record (0 = left); 0 for a root */
    uint32_t leaf;        /* 1: holds a primitive range */
    uint32_t kind;        /* leaf: the range's kind: ZR_PRIM_SPHERE / TRIANGLE / CUBE / MEDIUM, 4 wrapped object, 5 cube under translate /
                             rotate_y / scale, 6 placed run of triangles (ZR_PRIM_GROUP) */
    uint32_t count;       /* leaf: primitives in the range (1 .. 4) */
    uint32_t first;       /* leaf: first primitive in the kind's leaf order; inner: the pair record holding its children */
    uint32_t subtree;     /* leaf of kind 6: the placed run's tree (its first pair record); else ZR_BVH_NO_BOX */
    uint32_t src[4];      /* leaf: the primitives' indices in the caller's arrays — spheres, triangles, cubes (kinds 2 and 5), media — and, for
                             kinds 4 and 6, the world-list entry (zr_scene_set_objects, or the implicit list's position) */
} zr_tree_box;
/* copies min(cap, n) boxes, world tree first, each tree in pre-order (a box, its left subtree, its right subtree); returns n (or a negative
 * ZR_E_*).  out may be NULL with cap = 0 to ask for n. */
int zr_scene_tree_boxes(const zr_scene*, zr_tree_box* out, size_t cap);

/* Known answers for whole paths: walks the primary sample (px, py, sample) of each request on the device and records
 * every segment, ZR_PATH_RECORD doubles each: ray origin, direction | hit flag, t, material id | scattered flag,
 * attenuation rgb | emission rgb | main-stream RNG draws consumed so far.  requests = n * 3 ints; out = n * max_segments *
 * ZR_PATH_RECORD doubles (zero-filled past the path's end).  Same arithmetic as zr_render; the environment plays no role
 * (a miss ends the record list). */
#define ZR_PATH_RECORD 17
int zr_trace_paths(zr_ctx*, const zr_scene*, const zr_camera*, uint64_t seed, const int32_t* requests, int n, int max_segments, double* out);

/* counters + device time of the last render on this context (synchronises the context's stream) */
int zr_get_counters(zr_ctx*, zr_counters*);
/* pixels the last render on this context finished in the sky pre-pass (every camera ray of the pixel provably sees only the environment, so the pixel never
 * entered the streaming pipeline; ZR_SKY_PREPASS=0 switches the pre-pass off); 0 for a render that took any other path, the counting render among them */
uint64_t zr_last_presolved_pixels(zr_ctx*);
/* the round loop of the last render that went through the streaming pipeline: *drain_round = the loop round after which the paths still alive were moved to the
 * small drain pool (0: they never were), *sub_pools = the sub-pools the frame began with (0: the render took another path).  Either pointer may be null.  With
 * zr_counters::rounds = R and no drain, the launch log holds (sub_pools - 1) + sub_pools * (R - [sub_pools > 1]) EXTEND launches for the frame; rounds after
 * drain_round contribute one each.  ZR_STREAM_POLL_LAG (default 1; 0: the host drains the streams at every poll) says how many rounds old the host's knowledge is. */
int zr_last_round_loop(zr_ctx*, int* drain_round, int* sub_pools);
/* which SHADE build the launches of the last render through the streaming pipeline took: *in_place = launches of the lean render's in-place build (a world with
 * one material kind, while work units are left; ZR_SHADE_IN_PLACE=0, read per render, switches it off), *sorted = launches of the builds that sort a block's slots
 * by what they execute.  Launches enqueued are counted, the rounds queued behind the one that emptied the pools included; both 0 for a render that took another
 * path.  Either pointer may be null. */
int zr_last_shade_builds(zr_ctx*, int* in_place, int* sorted);
/* how the lean EXTEND kernel (worlds of bare triangles and spheres) fetched its slots in the last COUNTED render on this context: *checked = slots whose meta
 * word it read and tested before asking for the ray, *skipped = slots it asked for at once because every slot of their pool was active (finished paths regenerate
 * in place while work units are left; ZR_EXTEND_ALL_ACTIVE=0, read per render, switches the skip off).  Both 0 for an uncounted render and for a world that takes
 * another EXTEND build.  Either pointer may be null. */
int zr_last_extend_fetches(zr_ctx*, uint64_t* checked, uint64_t* skipped);
/* drains the log of render-kernel launch durations (ms, measured with HIP events on the launch stream) recorded
 * since the previous call: copies the newest min(cap, n) of them, oldest first, and returns n */
int zr_get_kernel_times(zr_ctx*, float* ms, int cap);

/* ---- multi-GPU: the one collective of a frame, for hosts that stay C++ (no torch) ---------------------------- */
/* One process per GPU.  Each rank renders its interleaved tiles with zr_render_device(region.tile_mod = nranks,
 * region.tile_rem = rank, region.tile_size) into a W*H*3 double frame in HBM.  zr_comm_gather_frame then packs the pixels of
 * the rank's own tiles (1/nranks of the frame) and sends them to `root`, which receives the other ranks' shares (one grouped
 * ncclSend / ncclRecv exchange: only the root needs the frame) and scatters them into its frame: each rank's share crosses one
 * xGMI link once instead of a whole frame of mostly zeros going through a ring reduce, and no arithmetic touches the pixels.
 * `region` is the zr_region the rank rendered with: the exchange moves tile t from rank t % nranks, so anything but the whole
 * frame with tile_mod = nranks and tile_rem = rank is refused (ZR_E_INVALID) rather than silently overwriting rendered pixels
 * (ABI 3; ABI 2 took the bare tile size).  zr_comm_reduce_frame is the round-1 form: the
 * zero-initialised frames summed onto `root` in place (ncclReduce, ncclDouble, ncclSum); tiles are disjoint, so it is exact too.
 * The reference has no counterpart: it shards rows over std::threads in one address space (camera.hpp:557-573).
 * librccl.so is loaded lazily (dlopen) by these entry points only. */
#define ZR_COMM_ID_BYTES 128
typedef struct zr_comm zr_comm;
int zr_comm_unique_id(unsigned char id[ZR_COMM_ID_BYTES]);  /* rank 0 creates it and ships it to the other ranks */
zr_comm* zr_comm_create(zr_ctx*, int nranks, int rank, const unsigned char id[ZR_COMM_ID_BYTES]);
int zr_comm_reduce_frame(zr_comm*, void* d_frame, size_t n_doubles, int root, void* hip_stream);
int zr_comm_gather_frame(zr_comm*, void* d_frame, int W, int H, const zr_region* region, int root, void* hip_stream);
void zr_comm_destroy(zr_comm*);

/* ---- known-answer entry: world.hit(r, interval(tmin,tmax), rec) for a batch of rays ---------- */
/* rays: 6 doubles each (origin, direction).  The medium draw of ray k (zr_rng.h) is keyed by
 * zr_stream_key(seed, pixel, k) and `bounce`. */
int zr_trace(zr_ctx*, const zr_scene*, const double* rays6, size_t n, double tmin, double tmax,
             uint64_t seed, uint64_t pixel, uint32_t bounce, zr_hit* out);

/* ---- per-function known-answer entry points -------------------------------------------------------------------------
 * The reference's seam is its virtual API (hittable::hit hittable.hpp:29-36, material::scatter / emitted material.hpp:7-31,
 * texture::value texture.hpp:6-10) plus camera::get_ray / get_background_color (camera.hpp:784-794, 828-925).  zr_trace above
 * answers hittable::hit; the four calls below answer the others, n calls per launch, with the device arithmetic of the
 * render kernels.  They serve the parity tests (hand-placed edge cases against the genuine reference) and the drop-in
 * classes' hit() / scatter() / emitted() in include/zenith/zenith.hpp, which stay callable without any CPU evaluation. */
typedef struct zr_scatter_out {
    double attenuation[3], origin[3], direction[3];  /* material::scatter's outputs (zero when it returned false) */
    double emitted[3];                                /* material::emitted(rec.u, rec.v, rec.p) */
    uint32_t scattered;                               /* scatter's return value */
    uint32_t draws;                                   /* random_double() calls it made */
} zr_scatter_out;
/* material::scatter(r_in, rec, attenuation, scattered) and emitted for n (ray, hit record) pairs; recs[k].mat indexes the
 * scene's materials; draws come from the contract stream keys[k] (include/zr_rng.h), starting at draw first_draw[k] (NULL = 0) */
int zr_kat_scatter(zr_ctx*, const zr_scene*, const double* rays6, const zr_hit* recs, const uint64_t* keys, const uint64_t* first_draw,
                   size_t n, zr_scatter_out* out);
/* The lean pair per call (additive, ABI 3): for n rays, the closest hit over (0.001, inf) as zr_trace finds it, then the record and emitted + scatter as
 * SHADE's lean build computes them (lean_rec / lean_shade), draws from keys[k] starting at first_draw[k] (NULL = 0).  out_hits holds p, normal, mat,
 * front_face and t (the other fields are zero; mat = 0xFFFFFFFF on a miss), out is filled as zr_kat_scatter fills it.  A scene that did not commit
 * with the lean build (zr_scene_kernels: shade_lean = 0) is refused with ZR_E_STATE. */
int zr_kat_shade_lean(zr_ctx*, const zr_scene*, const double* rays6, const uint64_t* keys, const uint64_t* first_draw, size_t n, zr_hit* out_hits,
                      zr_scatter_out* out);
/* texture::value(u, v, p) of the scene's texture `texture_id`; uvp5 = n x (u, v, px, py, pz); out = n x rgb */
int zr_kat_texture(zr_ctx*, const zr_scene*, uint32_t texture_id, const double* uvp5, size_t n, double* out_rgb);
/* camera::get_background_color(ray(., dir), env) for n directions (env.hdr_texture indexes the scene's textures) */
int zr_kat_background(zr_ctx*, const zr_scene*, const zr_env*, const double* dirs3, size_t n, double* out_rgb);
/* camera::get_ray(i, j) after camera::initialize() for n requests (i, j, sample); out = n x (origin, direction, draws used) */
int zr_kat_camera_rays(zr_ctx*, const zr_camera*, uint64_t seed, const int32_t* requests3, size_t n, double* out7);

/* ---- direct light sampling: next-event estimation with multiple importance sampling, opt-in ------------------------
 * An integrator bound to an accumulator.  It walks exactly the vertices of zr_render's path — same camera draws, same scatter() draws, same Russian
 * roulette, no extra draw from the main stream — so a sample's segments, hits and main-stream draws are the plain integrator's; only the radiance
 * bookkeeping differs:   L = sum_k beta_k (w_k Le(x_k) + D_k).
 *   Sampled lights   world-level leaf primitives whose stored material is ZR_MAT_LIGHT and whose stored form is world-space or affine: spheres and triangles
 *                    (bare or baked), bare cubes (six rectangles about the origin, as cube::hit tests them) and placed cubes (scale -> rotate_y -> translate:
 *                    six parallelograms).  Emitters under generic wrapper chains, inside groups and media are not sampled: they keep w = 1 when hit.
 *                    One slot per sphere / triangle / face, weight = area x lum (lum = 0.2126 r + 0.7152 g + 0.0722 b of a solid emission texture, 1.0 for
 *                    any other); slots whose weight is zero, negative or not finite are skipped.  Order: spheres, triangles, cubes, placed cubes by stored
 *                    index, a cube's faces -x +x -y +y -z +z.  cdf = the FP64 running sum of the weights in that order.  One draw u selects the first slot
 *                    with cdf > u * total, so every point of an object has the area density rho = lum / total.
 *   The sun          with ZR_ENV_PHYSICAL_SUN, the disc on and sun_size > 0: the cone cos(theta) in [sun_thr, 1] uniformly by solid angle,
 *                    pdf = 1 / (2 pi (1 - sun_thr)), in a fixed frame about the sun direction s: a = (0,1,0) if |s.x| > 0.9 else (1,0,0), t = unit(a x s),
 *                    b = s x t, direction = sin cos(phi) t + sin sin(phi) b + cos s with cos = 1 - u1 (1 - sun_thr), phi = 2 pi u2.  Its radiance is the
 *                    sun term of the background alone; the sky always comes from scattering with weight 1.
 *   Draws            zr_light_key (zr_rng.h), in this order: sun-or-emitter (only when both are sampled: u < 0.5 takes an emitter; each then has P = 1/2),
 *                    the slot, then the point: sphere c + r random_unit_vector (rejection, three draws a round), triangle u1, u2 folded to 1 - u1, 1 - u2
 *                    when u1 + u2 > 1, parallelogram o + u1 e1 + u2 e2.
 *   D_k              at Lambertian and isotropic vertices that have a next segment within max_depth: a shadow query from the scattered ray's origin —
 *                    the path's own closest hit over (0.001, dist + tol), tol = ZR_DIRECT_T_TOL max(1, dist), its medium draws keyed with
 *                    bounce | 0x80000000 — sees the sample iff it answers with the chosen object at |t - dist| <= tol (the sun: iff it misses).  Emission
 *                    comes from that hit's record.  pdf_w = P rho dist^2 / cos_l (cos_l = |n . w| with the slot's geometric normal; <= 1e-12: nothing);
 *                    Lambertian f cos = albedo max(0, wn . w) / pi and p_b = max(0, wn . w) / pi with scatter()'s shading normal wn, isotropic
 *                    f = albedo / 4 pi and p_b = 1 / 4 pi;  D = beta f cos Le / (pdf_w + p_b)   (balance heuristic).
 *   w_k              p_b / (p_b + pdf_w) where the vertex before took a D and x_k is a sampled light (the sun term of a miss likewise); 1 everywhere else.
 * zr_accum_set_direct  binds the integrator to an accumulator (params NULL: unbinds).  ZR_E_STATE unless the accumulator holds nothing (done == 0);
 *                      zr_accum_reset keeps the binding.  zr_render_accumulate and zr_render_adaptive then render through the direct kernel (one thread
 *                      per sample, the pixel-group route's pairing: zr_counters::path 0), and everything that reads an accumulator works unchanged.
 *                      The light table is built from the device's final primitive arrays at the first direct render of a (commit, refit epoch), and kept.
 * zr_accum_get_direct  *out = the binding: its flags, pad_ = 1 while an integrator is bound (0: none)
 * zr_render_direct     zr_accum_create -> zr_accum_set_direct -> zr_render_accumulate(camera.samples_per_pixel) -> zr_accum_resolve, bit for bit
 * zr_get_direct_stats  of the last direct batch on the context: shadow queries made / that saw their sample, sun queries among them (a counting
 *                      batch only, else 0), and the table's slots and objects.  zr_get_counters reports the path's own segments, hits and draws only.
 * Refusals come before any device call and zr_last_error names the argument: NULL, flags outside ZR_DIRECT_EMITTERS | ZR_DIRECT_SUN, more than
 * ZR_DIRECT_MAX_SLOTS slots (ZR_E_INVALID). */
#define ZR_DIRECT_EMITTERS 1u
#define ZR_DIRECT_SUN 2u
#define ZR_DIRECT_MAX_SLOTS (1u << 22)
#define ZR_DIRECT_T_TOL 1e-7
typedef struct zr_direct_params {
    uint32_t flags;   /* ZR_DIRECT_EMITTERS | ZR_DIRECT_SUN */
    uint32_t pad_;
} zr_direct_params;
typedef struct zr_direct_stats {
    uint64_t shadow_queries, shadow_visible, sun_queries, slots, sampled_objects;
} zr_direct_stats;
int zr_accum_set_direct(zr_accum*, const zr_direct_params* /* or NULL */);
int zr_accum_get_direct(const zr_accum*, zr_direct_params* out);
int zr_render_direct(zr_ctx*, const zr_scene*, const zr_camera*, const zr_env*, uint64_t seed, const zr_region* region, const zr_direct_params*,
                     int collect_counters, double* out_rgb);
int zr_get_direct_stats(zr_ctx*, zr_direct_stats* out);
/* known-answer entries.  zr_scene_lights: the light table of the committed scene; copies min(cap, n) slots, returns n (out NULL with cap 0 asks for n) or a
 * negative ZR_E_*.  zr_kat_light_sample: one light sample per query from origins3[k] with the light stream zr_light_key(keys[k], bounces[k]); draws8
 * (may be NULL) holds 8 numbers per query that replace the stream's draws 0..7 where they lie in [0, 1).  zr_kat_light_pdf: closest hit of the ray
 * (origins3[k], dirs3[k]) over (0.001, inf) as the path finds it, then the light density the MIS weight would use there (0: nothing sampled answers) and
 * the hit's key, kind << 32 | index as closest hit names it (all ones on a miss).  `params` selects what is sampled, `env` describes the sun. */
enum { ZR_LIGHT_SPHERE = 0, ZR_LIGHT_TRIANGLE = 1, ZR_LIGHT_PARALLELOGRAM = 2 };
typedef struct zr_light_slot {
    uint32_t type;            /* ZR_LIGHT_* */
    uint32_t kind, index;     /* the object as closest hit names it: ZR_PRIM_SPHERE / TRIANGLE / CUBE or 5 (placed cube), index in that kind's stored array */
    uint32_t face;            /* cube face 0..5 = -x +x -y +y -z +z, else 0 */
    double o[3], e1[3], e2[3]; /* triangle: v0, v1 - v0, v2 - v0; parallelogram: corner and edges; sphere: o = centre, e1[0] = radius */
    double area, lum, weight, cdf;
} zr_light_slot;
typedef struct zr_light_sample {
    uint32_t choice;          /* 0 nothing to sample, 1 an emitter, 2 the sun */
    uint32_t slot;            /* emitter: the slot chosen */
    uint32_t kind, index;     /* ... and its object */
    uint32_t draws, pad_;     /* light-stream draws used */
    double y[3], normal[3], w[3]; /* the point, the slot's geometric normal there, the unit direction from the origin (the sun: y and normal zero) */
    double dist;              /* +inf for the sun */
    double pdf;               /* pdf_w as if unoccluded; 0 where the sample contributes nothing */
} zr_light_sample;
int64_t zr_scene_lights(zr_ctx*, const zr_scene*, zr_light_slot* out, size_t cap);
int zr_kat_light_sample(zr_ctx*, const zr_scene*, const zr_env*, const zr_direct_params*, const double* origins3, const uint64_t* keys, const uint32_t* bounces,
                        const double* draws8, size_t n, zr_light_sample* out);
int zr_kat_light_pdf(zr_ctx*, const zr_scene*, const zr_env*, const zr_direct_params*, const double* origins3, const double* dirs3, size_t n, double* out_pdf,
                     uint64_t* out_key);
uint64_t zr_kat_light_key(uint64_t key, uint32_t bounce);   /* zr_light_key of zr_rng.h, for bindings */

/* ---- direct light sampling of the HDR environment map, opt-in on top of the above -----------------------------------
 * The third kind of light: with ZR_ENV_HDR_MAP the map itself is importance-sampled.  The lookup reads the nearest texel, so radiance is constant over
 * texel cells: row j covers theta in [j pi / H, (j + 1) pi / H), column i covers atan2(z, x) in -pi + 2 pi [i, i + 1) / W in map space (the direction after
 * the environment's yaw, tilt and roll), and a cell of row j has the solid angle omega_j = (2 pi / W)(cos(j pi / H) - cos((j + 1) pi / H)).
 *   Sampled when     env.mode == ZR_ENV_HDR_MAP, hdr_texture names a ZR_TEX_IMAGE_F32 or ZR_TEX_IMAGE_U8 texture of W x H > 0 texels, intensity is finite
 *                    and > 0, and T (below) is finite and > 0.  Otherwise nothing of the environment is sampled and every miss keeps weight 1; that is no
 *                    error, except that a map of more than ZR_DIRECT_ENV_MAX_TEXELS texels is refused (ZR_E_INVALID).
 *   The table        w_ji = lum(c_ji) omega_j with c_ji the texel's colour at intensity 1 and lum as above; a weight that is zero, negative or not finite
 *                    counts as 0.  cdf[j][i] = the FP64 running sum of row j's weights (from zero in every row), row_cdf[j] = the running sum of the rows'
 *                    totals, T = row_cdf[H - 1].  Summation order of a row: 256 chunks of c = ceil(W / 256) consecutive columns, each summed left to
 *                    right from zero; the chunk sums' running sum in index order gives each chunk's offset; an entry is offset + the chunk's running sum.
 *                    Built on the device at the first use and kept per (commit, texture): rotation, intensity and refits do not enter it.
 *   Draws            on the vertex's light stream: emitter-or-map first (only when both are sampled: u < 0.5 takes an emitter; each then has P = 1/2), then
 *                    u_r (the first row with row_cdf[j] > u_r T), u_c (the first column with cdf[j][i] > u_c cdf[j][W - 1]; either search takes the last
 *                    entry when none exceeds), u_a: cos theta = cos(j pi / H) - u_a (cos(j pi / H) - cos((j + 1) pi / H)), u_b: phi = -pi + 2 pi (i + u_b) / W.
 *                    Map-space direction (sin theta cos phi, cos theta, sin theta sin phi), taken to the world by the inverse roll, tilt, yaw.
 *   The sample       pdf_w = P lum(c_ji) / T (0 on a texel without weight), radiance c_ji x intensity (the chosen texel's, not a second lookup), dist = +inf;
 *                    the shadow query is the sun's: it sees the sample iff it misses.
 *   The miss         of a scattered ray whose vertex took a D: all of the background colour bg is weighted by p_b / (p_b + p_l),
 *                    p_l = P lum(bg) / (intensity T), 0 where that is not finite and positive.
 * zr_accum_set_direct_env   switches it on (on != 0) or off for an accumulator.  ZR_E_STATE unless the accumulator is empty and a direct integrator is bound;
 *                           zr_accum_reset keeps it, zr_accum_set_direct(NULL) clears it.  Where nothing of the environment is sampled the accumulator
 *                           renders exactly as without it.
 * zr_render_direct_env      zr_accum_create -> zr_accum_set_direct -> zr_accum_set_direct_env(1) -> zr_render_accumulate -> zr_accum_resolve, bit for bit
 * zr_scene_env_light        the table of (scene, env): *info; row_cdf (H doubles) and cdf (W x H doubles, row-major), each may be NULL, are written when
 *                           info->sampled
 * zr_kat_env_light_sample   zr_kat_light_sample with the environment on: choice 3 = the map, slot = j W + i, kind and index all ones, y and normal zero
 * zr_kat_env_light_pdf      the density a missed ray of direction dirs3[k] (any length) is weighted by
 * zr_get_direct_env_stats   of the last counted direct batch: shadow queries towards the map, and those that saw it
 * Refusals come before any device call and zr_last_error names the argument. */
#define ZR_DIRECT_ENV_MAX_TEXELS (1u << 25)
typedef struct zr_env_light_info {
    uint32_t width, height;   /* of the map (0 x 0: the environment has no image map) */
    uint32_t sampled, pad_;   /* 1: the map is sampled */
    double total;             /* T */
    uint64_t weighted;        /* texels with weight */
    double build_ms;          /* device time of the kernel that built the table, when it was built */
} zr_env_light_info;
int zr_accum_set_direct_env(zr_accum*, int on);
int zr_accum_get_direct_env(const zr_accum*, int* on);
int zr_render_direct_env(zr_ctx*, const zr_scene*, const zr_camera*, const zr_env*, uint64_t seed, const zr_region* region, const zr_direct_params*,
                         int collect_counters, double* out_rgb);
int zr_scene_env_light(zr_ctx*, const zr_scene*, const zr_env*, zr_env_light_info* info, double* row_cdf /* H or NULL */, double* cdf /* W x H or NULL */);
int zr_kat_env_light_sample(zr_ctx*, const zr_scene*, const zr_env*, const zr_direct_params*, const double* origins3, const uint64_t* keys,
                            const uint32_t* bounces, const double* draws8, size_t n, zr_light_sample* out);
int zr_kat_env_light_pdf(zr_ctx*, const zr_scene*, const zr_env*, const zr_direct_params*, const double* dirs3, size_t n, double* out_pdf);
int zr_get_direct_env_stats(zr_ctx*, uint64_t* env_queries, uint64_t* env_visible);

#ifdef __cplusplus
}
#endif
#endif /* ZR_CAPI_H */
