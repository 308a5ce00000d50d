// zr_entry.h — the entry rules both BVH builders share: how a world-list entry gets its bounding box (the reference's constructors) and what record it
// becomes in the primitive arrays (bare, baked, placed).  A frame must not depend on which builder made the tree, so these are written once: the host
// flattener (zr_flatten.h, g++) and the device builder (zr_build.hip, hipcc, -ffp-contract=off like the host) compile the same functions, over the same
// two views — the scene as given (BuildSceneIn) and the final primitive arrays (BuildPrimOut).  No HIP in here when g++ compiles it.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/zr_capi.h"
#include "zr_bvh.h"
#include "zr_device_types.h"

#ifdef __HIPCC__
#define ZR_HD __host__ __device__
#else
#define ZR_HD
#endif

namespace zr {

// the scene as the caller gave it: the host's own arrays, or their unchanged copies on the device
struct BuildSceneIn {
    const double* spheres = nullptr; const uint32_t* sphere_mat = nullptr;
    const double* tri_v = nullptr; const double* tri_n = nullptr; const uint32_t* tri_mat = nullptr;
    const double* tri_uv = nullptr;      // 6 per triangle, or null
    const double* cubes = nullptr; const uint32_t* cube_mat = nullptr;
    const zr_medium* media = nullptr; const zr_xform_op* ops = nullptr;
    const double* group_box = nullptr;   // per zr_group: lo[3], hi[3] of its triangles in their own space (the layout of BuildBox)
};
static_assert(sizeof(BuildBox) == 6 * sizeof(double), "an array of BuildBox is read as BuildSceneIn::group_box");

// where a tree's leaves put their primitive records: the scene's final arrays and the first index this tree may use per leaf kind
struct BuildPrimOut {
    double* spheres = nullptr; uint32_t* sphere_mat = nullptr;
    double* tri_v = nullptr; double* tri_s = nullptr;
    double* tri_uv = nullptr;            // null when the scene has no texture coordinates
    double* cubes = nullptr; uint32_t* cube_mat = nullptr;
    double* pcubes = nullptr; uint32_t* pcube_mat = nullptr;
    DInstance* insts = nullptr; uint32_t* inst_group = nullptr;
    uint32_t base[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t* src[8] = {};   // per leaf kind (may be null): each leaf primitive's index in the caller's arrays (note_src)
};

// ---- the box of an entry, following the reference's constructors ---------------------------------------------------------------------------
ZR_HD inline BuildBox apply_op_box(const zr_xform_op& op, const BuildBox& b) {
    BuildBox o;
    if (op.kind == ZR_OP_TRANSLATE) { for (int k = 0; k < 3; k++) { o.lo[k] = b.lo[k] + op.a[k]; o.hi[k] = b.hi[k] + op.a[k]; } return o; }   // translate.hpp:12
    if (op.kind == ZR_OP_SCALE) {   // scale.hpp:11-17
        for (int k = 0; k < 3; k++) { const double a0 = b.lo[k] * op.a[k], a1 = b.hi[k] * op.a[k]; o.lo[k] = fmin(a0, a1); o.hi[k] = fmax(a0, a1); }
        return o;
    }
    if (op.kind == ZR_OP_MATERIAL) return b;
    // rotate_*.hpp constructors: the box of the eight rotated corners.  rotate_y.hpp:26-27 builds its box with the INVERSE rotation (+sin) although
    // hit() maps object points with (cos x - sin z, sin x + cos z) (rotate_y.hpp:63-64): for children that are not symmetric about the y axis the
    // reference's box misses real geometry and what gets culled depends on its random tree.  Bound the true geometry.
    // A rotation about one axis turns the rectangle [a0, a1] x [b0, b1] of the other two; its four corners, with the constructors' arithmetic
    // (scalars only: no indexed local arrays — the first version indexed a local double[3] inside the corner loop and
    // came back from the gfx950 compiler with the unrotated coordinate overwritten, found by ZR_BUILD_CHECK)
    const double sn = op.a[0], co = op.a[1];
    const int ia = op.kind == ZR_OP_ROTATE_X ? 1 : 0, ib = op.kind == ZR_OP_ROTATE_Z ? 1 : 2, ic = 3 - ia - ib;   // (a, b) plane, c = the axis
    const double a0 = ia == 0 ? b.lo[0] : b.lo[1], a1 = ia == 0 ? b.hi[0] : b.hi[1];
    const double b0 = ib == 1 ? b.lo[1] : b.lo[2], b1 = ib == 1 ? b.hi[1] : b.hi[2];
    const double c0 = ic == 0 ? b.lo[0] : (ic == 1 ? b.lo[1] : b.lo[2]), c1 = ic == 0 ? b.hi[0] : (ic == 1 ? b.hi[1] : b.hi[2]);
    // rotate_y: x' = co x - sn z, z' = sn x + co z   (a = x, b = z)
    // rotate_x: y' = co y - sn z, z' = sn y + co z   (a = y, b = z)
    // rotate_z: x' = co x - sn y, y' = sn x + co y   (a = x, b = y)
    const double u00 = co * a0 - sn * b0, u10 = co * a1 - sn * b0, u01 = co * a0 - sn * b1, u11 = co * a1 - sn * b1;
    const double v00 = sn * a0 + co * b0, v10 = sn * a1 + co * b0, v01 = sn * a0 + co * b1, v11 = sn * a1 + co * b1;
    const double ulo = fmin(fmin(u00, u10), fmin(u01, u11)), uhi = fmax(fmax(u00, u10), fmax(u01, u11));
    const double vlo = fmin(fmin(v00, v10), fmin(v01, v11)), vhi = fmax(fmax(v00, v10), fmax(v01, v11));
    if (op.kind == ZR_OP_ROTATE_Y) { o.lo[0] = ulo; o.hi[0] = uhi; o.lo[1] = c0; o.hi[1] = c1; o.lo[2] = vlo; o.hi[2] = vhi; }
    else if (op.kind == ZR_OP_ROTATE_X) { o.lo[0] = c0; o.hi[0] = c1; o.lo[1] = ulo; o.hi[1] = uhi; o.lo[2] = vlo; o.hi[2] = vhi; }
    else { o.lo[0] = ulo; o.hi[0] = uhi; o.lo[1] = vlo; o.hi[1] = vhi; o.lo[2] = c0; o.hi[2] = c1; }
    return o;
}
// a box under wrappers ops[cf .. cf + cn), outermost first in the list: the innermost is applied first
ZR_HD inline BuildBox wrap_box(const BuildSceneIn& in, BuildBox b, uint32_t cf, uint32_t cn) {
    for (int k = (int)cn - 1; k >= 0; k--) b = apply_op_box(in.ops[cf + k], b);
    return b;
}
// a primitive that is no medium, in its own space (a group: the box of its triangles)
ZR_HD inline BuildBox bare_box(const BuildSceneIn& in, uint32_t type, uint32_t idx) {
    BuildBox b;
    if (type == ZR_PRIM_GROUP) { for (int k = 0; k < 3; k++) { b.lo[k] = in.group_box[(size_t)idx * 6 + k]; b.hi[k] = in.group_box[(size_t)idx * 6 + 3 + k]; } return b; }
    if (type == ZR_PRIM_SPHERE) {   // sphere.hpp:12-14 (raw radius argument)
        const double* q = in.spheres + (size_t)idx * 4;
        for (int k = 0; k < 3; k++) { b.lo[k] = fmin(q[k] - q[3], q[k] + q[3]); b.hi[k] = fmax(q[k] - q[3], q[k] + q[3]); }
    } else if (type == ZR_PRIM_TRIANGLE) {   // triangle.hpp:84-101
        const double* v = in.tri_v + (size_t)idx * 9;
        for (int k = 0; k < 3; k++) {
            b.lo[k] = fmin(v[k], fmin(v[3 + k], v[6 + k]));
            b.hi[k] = fmax(v[k], fmax(v[3 + k], v[6 + k]));
            if (b.hi[k] - b.lo[k] < 0.0001) { b.lo[k] -= 0.0001; b.hi[k] += 0.0001; }
        }
    } else {   // cube.hpp:34-41
        const double* q = in.cubes + (size_t)idx * 12;
        for (int k = 0; k < 3; k++) { b.lo[k] = q[6 + k] - 0.00005; b.hi[k] = q[9 + k] + 0.00005; }
    }
    return b;
}
ZR_HD inline BuildBox prim_box(const BuildSceneIn& in, uint32_t type, uint32_t idx) {
    if (type != ZR_PRIM_MEDIUM) return bare_box(in, type, idx);
    const zr_medium m = in.media[idx];   // constant_medium.hpp:79-81: the boundary's box (a sphere or a cube under the medium's own chain)
    return wrap_box(in, bare_box(in, m.boundary_type, m.boundary_index), m.chain_first, m.chain_count);
}
ZR_HD inline BuildBox chain_box(const BuildSceneIn& in, uint32_t type, uint32_t idx, uint32_t cf, uint32_t cn) { return wrap_box(in, prim_box(in, type, idx), cf, cn); }

// ---- the record of an entry: one primitive at index di of its kind's array ----------------------------------------------------------------------
constexpr uint32_t kKeepMaterial = 0xFFFFFFFEu;
// `mat` != kKeepMaterial: the primitive sits under material_instance wrappers only, which do nothing but replace rec.mat
// (material_instance.hpp:12-28) — it is stored bare with the outermost instance's material
ZR_HD inline void put_sphere(const BuildSceneIn& in, const BuildPrimOut& out, size_t di, uint32_t idx, uint32_t mat) {
    const double* q = in.spheres + (size_t)idx * 4;
    double* d = out.spheres + di * ZR_SPHERE_DOUBLES;
    d[0] = q[0]; d[1] = q[1]; d[2] = q[2]; d[3] = fmax(0.0, q[3]);   // sphere.hpp:9
    out.sphere_mat[di] = mat != kKeepMaterial ? mat : in.sphere_mat[idx];
}
ZR_HD inline void put_cube(const BuildSceneIn& in, const BuildPrimOut& out, size_t di, uint32_t idx, uint32_t mat) {
    const double* q = in.cubes + (size_t)idx * 12;
    for (int k = 0; k < ZR_CUBE_DOUBLES; k++) out.cubes[di * ZR_CUBE_DOUBLES + k] = q[k];
    out.cube_mat[di] = mat != kKeepMaterial ? mat : in.cube_mat[idx];
}
// a stored triangle: vertices for the intersection test, the shading record with its two words, and its texture coordinates, which travel with it
// unchanged (baked or not: they are no geometry)
ZR_HD inline void put_triangle_raw(const BuildSceneIn& in, const BuildPrimOut& out, size_t di, uint32_t idx, const double* v, const double* nn, uint32_t mat, uint32_t refaced) {
    double* tv = out.tri_v + di * ZR_TRI_STRIDE;
    double* t = out.tri_s + di * ZR_TRI_SHADE_DOUBLES;
    for (int k = 0; k < 9; k++) { tv[k] = v[k]; t[k] = v[k]; t[9 + k] = nn[k]; }
    const uint64_t mbits = mat, fbits = refaced ? (refaced % 2 ? 1u : 3u) : 0u;   // bit 0: under translate / rotate_y wrappers, bit 1: an even number of them
    __builtin_memcpy(t + 18, &mbits, 8); __builtin_memcpy(t + 19, &fbits, 8);
    if (out.tri_uv) for (int k = 0; k < 6; k++) out.tri_uv[di * 6 + k] = in.tri_uv[(size_t)idx * 6 + k];
}
// A triangle under a chain of translate / rotate_x,y,z / material_instance wrappers is stored in WORLD space as a bare
// triangle: vertices and (un-normalised) vertex normals mapped object -> world with the wrappers' own forward maps
// (translate.hpp:24-27, rotate_*.hpp hit(): the maps apply_op_rec uses for hit points), material = the outermost
// material_instance, plus how many translate / rotate_y wrappers the chain holds: each calls set_face_normal again on the
// normal the triangle has already turned against the ray, which answers front_face = true unless dot(d, normal) is exactly
// 0 (zr_device.h reface() restates both cases from the world-space dot product — the wrappers' maps are
// exact where sin and cos are 0 and 1, and elsewhere a dot product within rounding of 0 has no sign to agree on in either space).  t is the same in both spaces (the wrappers do not normalise the transformed direction), so
// only the last bits of the hit differ from transforming the ray — and every mesh the reference's scenes place in the
// world (model -> material_instance -> rotate -> translate) runs on the bare-triangle fast path instead of paying a
// chain transform per candidate.  scale is excluded: it would change which triangles count as degenerate.
// A bare triangle is the same with an empty chain.
ZR_HD inline void put_triangle(const BuildSceneIn& in, const BuildPrimOut& out, size_t di, uint32_t idx, uint32_t cf = 0, uint32_t cn = 0) {
    double v[9], nn[9];
    for (int k = 0; k < 9; k++) { v[k] = in.tri_v[(size_t)idx * 9 + k]; nn[k] = in.tri_n[(size_t)idx * 9 + k]; }
    uint32_t mat = in.tri_mat[idx];
    uint32_t refaced = 0;
    for (int k = (int)cn - 1; k >= 0; k--) {   // innermost wrapper first, as the hit record travels outwards
        const zr_xform_op op = in.ops[cf + k];
        const double sn = op.a[0], co = op.a[1];
        for (int c = 0; c < 3; c++) {
            double* p = v + 3 * c; double* q = nn + 3 * c;
            switch (op.kind) {
                case ZR_OP_TRANSLATE: p[0] += op.a[0]; p[1] += op.a[1]; p[2] += op.a[2]; break;
                case ZR_OP_ROTATE_Y: { double x = p[0], z = p[2]; p[0] = co * x - sn * z; p[2] = sn * x + co * z;
                                       x = q[0]; z = q[2]; q[0] = co * x - sn * z; q[2] = sn * x + co * z; } break;
                case ZR_OP_ROTATE_X: { double y = p[1], z = p[2]; p[1] = co * y - sn * z; p[2] = sn * y + co * z;
                                       y = q[1]; z = q[2]; q[1] = co * y - sn * z; q[2] = sn * y + co * z; } break;
                case ZR_OP_ROTATE_Z: { double x = p[0], y = p[1]; p[0] = co * x - sn * y; p[1] = sn * x + co * y;
                                       x = q[0]; y = q[1]; q[0] = co * x - sn * y; q[1] = sn * x + co * y; } break;
                default: break;
            }
        }
        if (op.kind == ZR_OP_TRANSLATE || op.kind == ZR_OP_ROTATE_Y) refaced++;
        if (op.kind == ZR_OP_MATERIAL) mat = op.mat;
    }
    put_triangle_raw(in, out, di, idx, v, nn, mat, refaced);
}
// A sphere under uniform scale / translate / material_instance wrappers (the demo scene's instanced spheres:
// scale -> material_instance -> translate) is the sphere (c s + offset, r s): same t, same unit normal, same u/v and
// tangent (no rotation involved); bit 31 of its material word records that a translate calls set_face_normal again on the turned
// normal (zr_device.h reface(); one bit: classify_object leaves a sphere under two or more translates to the interpreter).
ZR_HD inline void put_baked_sphere(const BuildSceneIn& in, const BuildPrimOut& out, size_t di, const zr_object& o) {
    const double* q = in.spheres + (size_t)o.index * 4;
    double c[3] = {q[0], q[1], q[2]}, r = fmax(0.0, q[3]);
    uint32_t mat = in.sphere_mat[o.index];
    bool refaced = false;
    for (int k = (int)o.chain_count - 1; k >= 0; k--) {
        const zr_xform_op op = in.ops[o.chain_first + k];
        if (op.kind == ZR_OP_SCALE) { c[0] *= op.a[0]; c[1] *= op.a[0]; c[2] *= op.a[0]; r *= op.a[0]; }
        else if (op.kind == ZR_OP_TRANSLATE) { c[0] += op.a[0]; c[1] += op.a[1]; c[2] += op.a[2]; refaced = true; }
        else if (op.kind == ZR_OP_MATERIAL) mat = op.mat;
    }
    double* d = out.spheres + di * ZR_SPHERE_DOUBLES;
    d[0] = c[0]; d[1] = c[1]; d[2] = c[2]; d[3] = r;
    out.sphere_mat[di] = refaced ? (mat | 0x80000000u) : mat;
}
// A cube under translate, or under rotate_y then translate, either with a scale as the innermost wrapper (material_instance wrappers
// anywhere) — how every cube of the reference's scenes is placed (scene_management.hpp:132-139 and the scaled, turned instances of its
// master cube, :178-201; cfg5's walls and boxes) — is stored as a PLACED CUBE: the cube's own numbers plus the wrappers' parameters in one
// 128-byte record.  The device applies the wrappers' ray and hit-record maps in the
// chain's order with the chain's arithmetic (zr_device.h pcube_ray / object_rec), so results are those of the wrapped object;
// what is saved is the op-list loop, its loads and the registers of the generic chain code in the traversal kernel.
ZR_HD inline void put_pcube(const BuildSceneIn& in, const BuildPrimOut& out, size_t di, const zr_object& o) {
    const double* q = in.cubes + (size_t)o.index * 12;
    double rec[ZR_PCUBE_STRIDE] = {q[0], q[1], q[2], q[3], q[4], q[5], 0, 0, 0, 0, 1, 0, 1, 1, 1, 0};
    uint32_t mat = in.cube_mat[o.index];
    for (int k = (int)o.chain_count - 1; k >= 0; k--) {   // inside-out: the outermost material_instance is applied last
        const zr_xform_op op = in.ops[o.chain_first + k];
        if (op.kind == ZR_OP_TRANSLATE) { rec[6] = op.a[0]; rec[7] = op.a[1]; rec[8] = op.a[2]; }
        else if (op.kind == ZR_OP_ROTATE_Y) { rec[9] = op.a[0]; rec[10] = op.a[1]; rec[11] = 1.0; }
        else if (op.kind == ZR_OP_SCALE) { rec[12] = op.a[0]; rec[13] = op.a[1]; rec[14] = op.a[2]; rec[15] = 1.0; }
        else if (op.kind == ZR_OP_MATERIAL) mat = op.mat;
    }
    for (int k = 0; k < ZR_PCUBE_STRIDE; k++) out.pcubes[di * ZR_PCUBE_STRIDE + k] = rec[k];
    out.pcube_mat[di] = mat;
}
// where leaf primitive `di` of kind `kind` came from: the world-list entry for wrapped objects and placed runs, else the primitive's own index
ZR_HD inline void note_src(const BuildPrimOut& out, uint32_t kind, size_t di, uint32_t oi, const zr_object& o) {
    if (out.src[kind & 7]) out.src[kind & 7][di] = (kind == ZR_KIND_WRAPPED || kind == ZR_KIND_INSTANCE) ? oi : o.index;
}
// World-list entry `o` as a leaf primitive of a plain kind (sphere / triangle / cube / placed cube / placed group) at index di of that kind's array.
// baked: the stored form the plan gave it (classify_object) — 0 as is, 1 baked triangle, 2 material-only chain, 3 baked sphere, 4 placed cube.
// A placed group's DInstance names its chain; its group's roots among the pair records and the 4-wide nodes follow once those are numbered.
ZR_HD inline void put_entry(const BuildSceneIn& in, const BuildPrimOut& out, const zr_object& o, uint32_t baked, size_t di) {
    if (o.type == ZR_PRIM_GROUP) {
        DInstance inst; inst.chain_first = o.chain_first; inst.chain_count = o.chain_count; inst.root = 0; inst.pad_ = 0;
        out.insts[di] = inst; out.inst_group[di] = o.index;
    }
    else if (baked == 1) put_triangle(in, out, di, o.index, o.chain_first, o.chain_count);
    else if (baked == 3) put_baked_sphere(in, out, di, o);
    else if (baked == 4) put_pcube(in, out, di, o);
    else {
        const uint32_t mat = baked == 2 ? in.ops[o.chain_first].mat : kKeepMaterial;   // material-only chain: the outermost wrapper is applied last
        if (o.type == ZR_PRIM_SPHERE) put_sphere(in, out, di, o.index, mat);
        else if (o.type == ZR_PRIM_TRIANGLE) put_triangle(in, out, di, o.index);
        else put_cube(in, out, di, o.index, mat);
    }
}

}  // namespace zr
