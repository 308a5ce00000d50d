// zr_refit.h — host-visible interface of the DEVICE side of a refit (zr_refit.hip): the committed trees keep their topology and their references, the moved
// primitives' boxes and records are scattered into the scene's arrays, and the boxes of the world's 4-wide tree and of its pair records are recomputed level by
// level, deepest first, one launch per level.  Nothing in here hands work from one workgroup to another inside a launch: a level reads what the launch before it
// wrote.  The patch formats are plain data; zr_update.h fills them without HIP (ZR_REFIT_TYPES_ONLY leaves the launch interface out).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "zr_device_types.h"

namespace zr {

// the new box of leaf primitive `di` of leaf kind `kind` (its place in the kind's array), rounded outwards to float like the device builder's (f_down / f_up)
struct RefitBoxPatch { uint32_t kind, di; float lo[3], hi[3]; };
static_assert(sizeof(RefitBoxPatch) == 32, "two 16-byte accesses");
// the new record of leaf primitive `di`: `doubles` values from payload[at ..) — a sphere's 4 (DScene::spheres), a triangle's 18 (vertices, vertex normals: words
// 0-17 of its shading record, the first 9 also its vertex record), a placed cube's 16
struct RefitRecPatch { uint32_t kind, di, at, doubles; };

#ifndef ZR_REFIT_TYPES_ONLY
}  // namespace zr
#include <hip/hip_runtime_api.h>
namespace zr {

// what the kernels work on: the scene's own arrays and the refit state's side arrays
struct RefitScene {
    NodeQ* quads; NodePair* pairs;
    float* prim_box[7];      // per leaf kind: 6 floats (lo, hi) per leaf primitive of the world's tree, in the kind's array order
    float* quad_box;         // 6 floats per 4-wide node: its TRUE box (the union of its children's true boxes), never a grid box
    float* pair_box;         // 6 floats per pair record: the union of its two children's true boxes
    double* spheres; double* tri_v; double* tri_s; double* pcubes;
};
// one level of a tree: order[first .. first + count) are the node indices of the level; block0: the level's first slot among the per-block partial sums
struct RefitLevel { uint32_t first, count, block0; };
// what a refit reads back, once: the root of the 4-wide tree, whether a box could not be put on a grid, then the pair kernels' partial sums
struct RefitResult { NodeF root; uint32_t quant_fail; uint32_t pad_[3]; };

hipError_t refit_patch(hipStream_t st, const RefitScene& sc, const RefitBoxPatch* d_box, uint32_t n_box, const RefitRecPatch* d_rec, uint32_t n_rec, const double* d_payload);
// the motion table's leaf words: d_pairs holds n pairs of 32-bit words (leaf address, new word), each address once; addresses >= n_leaves are ignored
hipError_t refit_motion(hipStream_t st, const void* d_pairs, uint32_t n, uint32_t* d_leaf_word, uint32_t n_leaves);
// the 4-wide tree: levels deepest first, then the FP32 root from `root` (its references; the boxes are rewritten) into result->root
hipError_t refit_quads(hipStream_t st, const RefitScene& sc, const uint32_t* d_order, const RefitLevel* levels, size_t n_levels, const NodeF& root, RefitResult* d_result);
// the pair records: levels deepest first; d_partial[level.block0 + block] = the sum of the half-areas of the child boxes the block wrote
hipError_t refit_pairs(hipStream_t st, const RefitScene& sc, const uint32_t* d_order, const RefitLevel* levels, size_t n_levels, double* d_partial);
#endif

}  // namespace zr
