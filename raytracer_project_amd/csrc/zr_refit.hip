// zr_refit.hip — the device side of zr_scene_refit (zr_refit.h): a moved world keeps its trees and gets their boxes anew.
//
//   k_refit_patch   one thread per patch: the moved leaf primitives' boxes into the per-kind box arrays, their records into the scene's primitive arrays
//   k_refit_motion  one thread per leaf word of the motion table that changes: a slot among the refit's motion records, STATIC or CUT (zr_motion.h)
//   k_refit_quads   one launch per level of the world's 4-wide tree, deepest first, one thread per node: every child's TRUE box — a leaf's is the union of its
//                   1-4 primitives' boxes, an inner child's was written to the side array by the launch before — goes onto a fresh 8-bit grid with the
//                   builder's own quant_axis (zr_quant.h), and the node's own true box goes to the side array for its parent.  References are not touched.
//                   True boxes travel upwards, never grid boxes: a grid box contains its true box with up to a grid step to spare, and a parent fitted around
//                   grid boxes would grow by such a step per level and again with every refit.
//   k_refit_root    the FP32 root (a kernel argument of every render) from its children's true boxes, widened by one float like the builder's (k_plan)
//   k_refit_pairs   the same schedule over the world's pair records (the pixel-group kernel, the BVH debug view and ZR_TRACE_ENGINE=pairs walk these): FP32
//                   planes widened by one float like the builder's (k_pairs), and per block the sum of the half-areas it wrote, reduced in a fixed order
//
// Levels are separated by kernel boundaries only: no counter a workgroup climbs on, no fence, no waiting on another workgroup.  A tree of a million leaves has
// ten to twenty levels, and a launch costs microseconds.  Group subtrees are in no level: a placement moves, its triangles stay where they are in their own space.
// Plain C++ and vector stores only; -ffp-contract=off like zr_build.hip, whose arithmetic this restates.
#include <hip/hip_runtime.h>

#include "zr_quant.h"
#include "zr_refit.h"

namespace zr {
namespace {

struct Box3 { float lo[3], hi[3]; };

__device__ __forceinline__ Box3 load_box(const float* __restrict__ p) {
    Box3 b;
    b.lo[0] = p[0]; b.lo[1] = p[1]; b.lo[2] = p[2]; b.hi[0] = p[3]; b.hi[1] = p[4]; b.hi[2] = p[5];
    return b;
}
__device__ __forceinline__ void store_box(float* __restrict__ p, const Box3& b) {
    p[0] = b.lo[0]; p[1] = b.lo[1]; p[2] = b.lo[2]; p[3] = b.hi[0]; p[4] = b.hi[1]; p[5] = b.hi[2];
}
__device__ __forceinline__ void grow(Box3& a, const Box3& b) {
    for (int k = 0; k < 3; k++) { a.lo[k] = fminf(a.lo[k], b.lo[k]); a.hi[k] = fmaxf(a.hi[k], b.hi[k]); }
}
__device__ __forceinline__ const float* kind_boxes(const RefitScene& sc, uint32_t kind) {
    switch (kind) {   // (a switch, not an index: the pointers stay in the kernel's scalar arguments)
        case 0: return sc.prim_box[0];
        case 1: return sc.prim_box[1];
        case 2: return sc.prim_box[2];
        case 3: return sc.prim_box[3];
        case 4: return sc.prim_box[4];
        case 5: return sc.prim_box[5];
        default: return sc.prim_box[6];
    }
}
// a leaf's box: the union of its primitives' (count >= 1)
__device__ __forceinline__ Box3 leaf_box(const RefitScene& sc, uint32_t kind, uint32_t first, uint32_t count) {
    const float* __restrict__ pb = kind_boxes(sc, kind) + (size_t)first * 6;
    Box3 b = load_box(pb);
    for (uint32_t k = 1; k < count; k++) grow(b, load_box(pb + (size_t)k * 6));
    return b;
}
__device__ __forceinline__ Box3 quad_child_box(const RefitScene& sc, uint32_t ref) {
    if (ref & ZR_REF_LEAF) return leaf_box(sc, (ref >> 28) & 7u, ref & 0xFFFFFFu, ((ref >> 24) & 15u) + 1u);
    return load_box(sc.quad_box + (size_t)ref * 6);
}

__global__ __launch_bounds__(256) void k_refit_patch(RefitScene sc, const RefitBoxPatch* __restrict__ box, uint32_t n_box, const RefitRecPatch* __restrict__ rec, uint32_t n_rec,
                                                     const double* __restrict__ payload) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_box) {
        const RefitBoxPatch p = box[i];
        float* __restrict__ d = const_cast<float*>(kind_boxes(sc, p.kind)) + (size_t)p.di * 6;
        d[0] = p.lo[0]; d[1] = p.lo[1]; d[2] = p.lo[2]; d[3] = p.hi[0]; d[4] = p.hi[1]; d[5] = p.hi[2];
    }
    if (i < n_rec) {
        const RefitRecPatch p = rec[i];
        const double* __restrict__ v = payload + p.at;
        if (p.kind == ZR_PRIM_SPHERE) {
            double* __restrict__ d = sc.spheres + (size_t)p.di * ZR_SPHERE_DOUBLES;
            for (int k = 0; k < ZR_SPHERE_DOUBLES; k++) d[k] = v[k];
        } else if (p.kind == ZR_PRIM_TRIANGLE) {   // the material and reface words (18, 19) stay as put_triangle_raw wrote them
            double* __restrict__ tv = sc.tri_v + (size_t)p.di * ZR_TRI_STRIDE;
            double* __restrict__ ts = sc.tri_s + (size_t)p.di * ZR_TRI_SHADE_DOUBLES;
            for (int k = 0; k < 9; k++) tv[k] = v[k];
            for (int k = 0; k < 18; k++) ts[k] = v[k];
        } else if (p.kind == ZR_KIND_PCUBE) {
            double* __restrict__ d = sc.pcubes + (size_t)p.di * ZR_PCUBE_STRIDE;
            for (int k = 0; k < ZR_PCUBE_STRIDE; k++) d[k] = v[k];
        }
    }
}

__global__ __launch_bounds__(256) void k_refit_quads(RefitScene sc, const uint32_t* __restrict__ order, uint32_t first, uint32_t count, RefitResult* __restrict__ result) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const uint32_t qi = order[first + t];
    NodeQ nq = sc.quads[qi];
    // the children in use: slots 0 .. nk - 1 (both builders fill a node's slots from the front; the host checked it when it made the schedule)
    int nk = 0;
    for (int c = 0; c < 4; c++) if (nq.ref[c] != ZR_REF_EMPTY) nk = c + 1;
    if (nk == 0) return;
    Box3 cb[4];
    for (int c = 0; c < 4; c++) cb[c] = quad_child_box(sc, c < nk ? nq.ref[c] : nq.ref[0]);   // (an unused slot repeats the first child: no runtime-indexed array)
    Box3 own = cb[0];
    for (int c = 1; c < 4; c++) grow(own, cb[c]);
    store_box(sc.quad_box + (size_t)qi * 6, own);
    for (int k = 0; k < 6; k++) nq.q[k] = 0;
    bool ok = true;
    for (int ax = 0; ax < 3; ax++) {
        float lo[4], hi[4]; uint32_t ql[4], qh[4];
        for (int k = 0; k < 4; k++) { lo[k] = cb[k].lo[ax]; hi[k] = cb[k].hi[ax]; }
        if (!quant_axis(lo, hi, nk, nq.origin[ax], nq.scale[ax], ql, qh)) { ok = false; break; }
        for (int k = 0; k < 4; k++) if (k < nk) { nq.q[ax] |= ql[k] << (8 * k); nq.q[3 + ax] |= qh[k] << (8 * k); }
    }
    if (!ok) { result->quant_fail = 1u; return; }   // (every writer writes the same word; the host reads it after the last launch)
    sc.quads[qi] = nq;
}

__global__ void k_refit_root(RefitScene sc, NodeF root, RefitResult* __restrict__ result) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int c = 0; c < 4; c++) {
        if (root.ref[c] == ZR_REF_EMPTY) continue;
        const Box3 b = quad_child_box(sc, root.ref[c]);
        root.lox[c] = nextafterf(b.lo[0], -__builtin_huge_valf()); root.loy[c] = nextafterf(b.lo[1], -__builtin_huge_valf()); root.loz[c] = nextafterf(b.lo[2], -__builtin_huge_valf());
        root.hix[c] = nextafterf(b.hi[0], __builtin_huge_valf()); root.hiy[c] = nextafterf(b.hi[1], __builtin_huge_valf()); root.hiz[c] = nextafterf(b.hi[2], __builtin_huge_valf());
    }
    result->root = root;
}

__global__ __launch_bounds__(256) void k_refit_pairs(RefitScene sc, const uint32_t* __restrict__ order, uint32_t first, uint32_t count, double* __restrict__ partial) {
    __shared__ double sum[256];
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    double area = 0.0;
    if (t < count) {
        const uint32_t pi = order[first + t];
        NodePair pr = sc.pairs[pi];
        Box3 own; bool any = false;
        for (int s = 0; s < 2; s++) {
            const uint32_t meta = pr.meta[s], n = meta & 0xFFFFu;
            if (meta != 0 && n == 0) continue;   // an empty child (a one-leaf world's second slot) keeps its record
            const Box3 b = meta == 0 ? load_box(sc.pair_box + (size_t)pr.child[s] * 6) : leaf_box(sc, ((meta >> 16) - 1u) & 7u, pr.child[s], n);
            if (any) grow(own, b); else { own = b; any = true; }
            for (int a = 0; a < 3; a++) { pr.lo[s][a] = nextafterf(b.lo[a], -__builtin_huge_valf()); pr.hi[s][a] = nextafterf(b.hi[a], __builtin_huge_valf()); }
            const double dx = (double)pr.hi[s][0] - (double)pr.lo[s][0], dy = (double)pr.hi[s][1] - (double)pr.lo[s][1], dz = (double)pr.hi[s][2] - (double)pr.lo[s][2];
            area += dx * dy + dy * dz + dz * dx;
        }
        if (any) { store_box(sc.pair_box + (size_t)pi * 6, own); sc.pairs[pi] = pr; }
    }
    // the block's sum in a fixed order (a tree over the thread index): the same bits whenever the same boxes are written
    sum[threadIdx.x] = area;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) sum[threadIdx.x] += sum[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sum[0];
}

inline dim3 grid_for(uint32_t n) { return dim3((n + 255u) / 256u); }

}  // namespace

// the motion table's leaf words: one thread per (leaf address, word) pair; an address names a leaf primitive of the world's tree once per call
__global__ __launch_bounds__(256) void k_refit_motion(const uint2* __restrict__ pairs, uint32_t n, uint32_t* __restrict__ leaf_word, uint32_t n_leaves) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint2 p = pairs[i];
    if (p.x < n_leaves) leaf_word[p.x] = p.y;
}

hipError_t refit_motion(hipStream_t st, const void* d_pairs, uint32_t n, uint32_t* d_leaf_word, uint32_t n_leaves) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_motion, grid_for(n), dim3(256), 0, st, (const uint2*)d_pairs, n, d_leaf_word, n_leaves);
    return hipGetLastError();
}

hipError_t refit_patch(hipStream_t st, const RefitScene& sc, const RefitBoxPatch* d_box, uint32_t n_box, const RefitRecPatch* d_rec, uint32_t n_rec, const double* d_payload) {
    const uint32_t n = n_box > n_rec ? n_box : n_rec;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_patch, grid_for(n), dim3(256), 0, st, sc, d_box, n_box, d_rec, n_rec, d_payload);
    return hipGetLastError();
}

hipError_t refit_quads(hipStream_t st, const RefitScene& sc, const uint32_t* d_order, const RefitLevel* levels, size_t n_levels, const NodeF& root, RefitResult* d_result) {
    for (size_t l = 0; l < n_levels; l++) {
        if (levels[l].count == 0) continue;
        hipLaunchKernelGGL(k_refit_quads, grid_for(levels[l].count), dim3(256), 0, st, sc, d_order, levels[l].first, levels[l].count, d_result);
    }
    hipLaunchKernelGGL(k_refit_root, dim3(1), dim3(64), 0, st, sc, root, d_result);
    return hipGetLastError();
}

hipError_t refit_pairs(hipStream_t st, const RefitScene& sc, const uint32_t* d_order, const RefitLevel* levels, size_t n_levels, double* d_partial) {
    for (size_t l = 0; l < n_levels; l++) {
        if (levels[l].count == 0) continue;
        hipLaunchKernelGGL(k_refit_pairs, grid_for(levels[l].count), dim3(256), 0, st, sc, d_order, levels[l].first, levels[l].count, d_partial + levels[l].block0);
    }
    return hipGetLastError();
}

}  // namespace zr
