// zr_temporal.hip — temporal accumulation: the geometry buffer of a camera and the reprojection of a frame's history into it.
// The reference has no counterpart (its roadmap lists camera paths); this is the temporal stage of SVGF (Schied et al., HPG 2017, section 4.1) with the
// variance propagated analytically from zr_accum_variance instead of estimated from temporal moments.  The contract of this file is its NumPy restatement,
// tests/temporal_model.py, which follows it operation for operation: FP64, compiled with -ffp-contract=off, no transcendental, no atomics.
//
//   gbuffer_rays        pixel (i, j) -> the ray through its centre (get_center_ray, camera.hpp:809-814): origin = center,
//                       direction_k = ((pixel00_k + i du_k) + j dv_k) - center_k.  No jitter, no defocus disk.
//   gbuffer_pack        zr_hit -> planes: position rec.p, normal rec.normal / sqrt((x x + y y) + z z) (0 when that length is 0), t, mat;
//                       a miss: position = the ray DIRECTION, normal 0, t 0, mat 0xFFFFFFFF
//   temporal_reproject  per pixel p, dots as (x x + y y) + z z, primed quantities are the previous view's:
//     1. c, V = colour and variance with NaN / Inf -> 0, V <= 0 -> 0
//     2. d = X_p - center' (hit) or X_p (miss: the stored direction);  zc = -(d . w'), no history unless zc > 0;  s = f' / zc;
//        q_k = (center'_k + d_k s) - pixel00'_k;  fx = q . a', fy = q . b';  depth_p = -((X_p - center) . w)
//     3. fx = rint(fx) when |fx - rint(fx)| <= 2^-20, likewise fy; no history unless -1 <= fx <= W and -1 <= fy <= H (outside that no tap lies in the frame)
//     4. x0 = floor(fx), wx = fx - x0, same in y; taps (x0 + dx, y0 + dy), dy outer / dx inner, weight (dx ? wx : 1 - wx) (dy ? wy : 1 - wy); a tap counts iff
//        weight > 0, inside the frame, N_q > 0, mat_q == mat_p and, for hits, |(X_q - X_p) . n_p| <= plane_tolerance depth_p and n_p . n_q >= normal_cos
//     5. no counting tap: N = 1, out = c, V_out = V.  Else sw = sum w, h = (sum w h_q) / sw, Vh = (sum w V_q) / sw, N = min(min N_q + 1, max_history),
//        beta = max(1.0 / N, alpha), out = h + beta (c - h), om = 1 - beta, V_out = (om om) Vh + (beta beta) V
//     6. out, V_out, N are written to the other half of the history; the caller swaps the halves and the views
//   temporal_reproject<true>  the motion build (its restatement: tests/temporal_motion_model.py), for a frame one refit after the history's.  A hit pixel's
//     (kind, index) names a leaf primitive of the world's tree (a placed group's triangle: the placement, kind >> 8) and so a word of the refit's motion table:
//       STATIC, or a miss: Xr = X_p, nr = n_p — the steps above exactly.   CUT: no history, N = 1.
//       a slot: with its record a[12], nm[9]:  Xr_k = ((a[4k] x + a[4k+1] y) + a[4k+2] z) + a[4k+3],  g_k = (nm[3k] nx + nm[3k+1] ny) + nm[3k+2] nz,
//       l = sqrt(g . g), nr = g / l; no history unless l > 0.
//     Step 2 projects Xr (d = Xr - center'); depth_p stays that of X_p in the current view.  Step 4 tests |(X_q - Xr) . nr| <= plane_tolerance depth_p and
//     nr . n_q >= normal_cos.  Everything else is unchanged.
//   gbuffer_entries     the (kind, index) plane -> the world-list entry under each pixel through the refit state's inverted slot array; 0xFFFFFFFF on a miss
#include <hip/hip_runtime.h>

#include <cstdint>

#include "zr_device_types.h"
#include "zr_launch.h"

namespace zr {

namespace {

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

__global__ __launch_bounds__(256) void gbuffer_rays(DCamera cam, double* __restrict__ rays) {
    const int i = blockIdx.x * 16 + threadIdx.x, j = blockIdx.y * 16 + threadIdx.y;
    if (i >= cam.W || j >= cam.H) return;
    double* r = rays + ((size_t)j * cam.W + i) * 6;
    const double fi = (double)i, fj = (double)j;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        r[k] = cam.center[k];
        r[3 + k] = ((cam.pixel00[k] + fi * cam.du[k]) + fj * cam.dv[k]) - cam.center[k];
    }
}

__global__ __launch_bounds__(256) void gbuffer_pack(const zr_hit* __restrict__ hits, const double* __restrict__ rays, size_t n, double* __restrict__ pos,
                                                    double* __restrict__ nrm, double* __restrict__ t, uint32_t* __restrict__ mat) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const zr_hit& h = hits[p];
    const uint32_t m = h.mat;
    double px, py, pz, nx = 0.0, ny = 0.0, nz = 0.0, tt = 0.0;
    if (m != 0xFFFFFFFFu) {
        px = h.p[0]; py = h.p[1]; pz = h.p[2]; tt = h.t;
        const double x = h.normal[0], y = h.normal[1], z = h.normal[2];
        const double l = sqrt(dot3(x, y, z, x, y, z));
        if (l > 0.0) { nx = x / l; ny = y / l; nz = z / l; }
    } else {
        px = rays[p * 6 + 3]; py = rays[p * 6 + 4]; pz = rays[p * 6 + 5];
    }
    if (pos) { pos[3 * p] = px; pos[3 * p + 1] = py; pos[3 * p + 2] = pz; }
    if (nrm) { nrm[3 * p] = nx; nrm[3 * p + 1] = ny; nrm[3 * p + 2] = nz; }
    if (t) t[p] = tt;
    if (mat) mat[p] = m;
}

__device__ __forceinline__ double clean(double v) { return isfinite(v) ? v : 0.0; }
__device__ __forceinline__ double clean_var(double v) { return isfinite(v) && v > 0.0 ? v : 0.0; }

// the leaf primitive (kind, index) names, as an address into the per-leaf arrays of the refit state; n_leaves (never an address) when it names none
__device__ __forceinline__ uint32_t leaf_address(const TemporalMotion& mv, uint2 ki) {
    const uint32_t k = ki.x & 0xFFu, idx = k == ZR_KIND_INSTANCE ? ki.x >> 8 : ki.y;
    if (ki.x == 0xFFFFFFFFu || k >= 7u) return mv.n_leaves;
    uint32_t base = 0, top = 0;   // (selects, not an indexed read of the kernel arguments)
#pragma unroll
    for (uint32_t kk = 0; kk < 7u; kk++) { base = k == kk ? mv.leaf_base[kk] : base; top = k == kk ? mv.leaf_base[kk + 1] : top; }
    return top <= mv.n_leaves && base <= top && idx < top - base ? base + idx : mv.n_leaves;
}

__global__ __launch_bounds__(256) void gbuffer_entries(TemporalMotion mv, const uint32_t* __restrict__ leaf_entry, size_t n, uint32_t* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t at = leaf_address(mv, mv.ki[p]);
    out[p] = at < mv.n_leaves ? leaf_entry[at] : 0xFFFFFFFFu;
}

template <bool MOTION>
__global__ __launch_bounds__(256) void temporal_reproject(int W, int H, TemporalView cur, TemporalView prev, int have_prev, zr_temporal_params tp,
                                                          const double* __restrict__ color, const double* __restrict__ variance, TemporalPlanes now,
                                                          TemporalPlanes before, TemporalMotion mv) {
    const int i = blockIdx.x * 16 + threadIdx.x, j = blockIdx.y * 16 + threadIdx.y;
    if (i >= W || j >= H) return;
    const size_t p = (size_t)j * W + i;
    const double c[3] = {clean(color[3 * p]), clean(color[3 * p + 1]), clean(color[3 * p + 2])};
    const double V[3] = {clean_var(variance[3 * p]), clean_var(variance[3 * p + 1]), clean_var(variance[3 * p + 2])};
    const double X[3] = {now.pos[3 * p], now.pos[3 * p + 1], now.pos[3 * p + 2]};
    const double n[3] = {now.nrm[3 * p], now.nrm[3 * p + 1], now.nrm[3 * p + 2]};
    const uint32_t m = now.mat[p];
    const bool hit = m != 0xFFFFFFFFu;

    double sw = 0.0, sh[3] = {0.0, 0.0, 0.0}, sv[3] = {0.0, 0.0, 0.0};
    int min_n = 0x7FFFFFFF;
    double Xr[3] = {X[0], X[1], X[2]}, nr[3] = {n[0], n[1], n[2]};   // where the pixel's point was in the history's frame, and its normal there
    bool followed = true;
    if constexpr (MOTION) {
        if (hit && have_prev) {
            const uint32_t at = leaf_address(mv, mv.ki[p]);
            const uint32_t word = at < mv.n_leaves ? mv.leaf_word[at] : ZR_MOTION_STATIC;
            if (word == ZR_MOTION_CUT) followed = false;
            else if (word < mv.n_slots) {
                const double* __restrict__ a = mv.records + (size_t)word * 21;
                const double* __restrict__ nm = a + 12;
                double g[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    Xr[k] = ((a[4 * k] * X[0] + a[4 * k + 1] * X[1]) + a[4 * k + 2] * X[2]) + a[4 * k + 3];
                    g[k] = (nm[3 * k] * n[0] + nm[3 * k + 1] * n[1]) + nm[3 * k + 2] * n[2];
                }
                const double l = sqrt(dot3(g[0], g[1], g[2], g[0], g[1], g[2]));
                if (l > 0.0) { nr[0] = g[0] / l; nr[1] = g[1] / l; nr[2] = g[2] / l; }
                else followed = false;
            }
        }
    }
    if (have_prev && followed) {
        double d[3];
#pragma unroll
        for (int k = 0; k < 3; k++) d[k] = hit ? Xr[k] - prev.center[k] : Xr[k];
        const double zc = -dot3(d[0], d[1], d[2], prev.w[0], prev.w[1], prev.w[2]);
        if (zc > 0.0) {
            const double s = prev.f / zc;
            double q[3];
#pragma unroll
            for (int k = 0; k < 3; k++) q[k] = (prev.center[k] + d[k] * s) - prev.pixel00[k];
            double fx = dot3(q[0], q[1], q[2], prev.a[0], prev.a[1], prev.a[2]);
            double fy = dot3(q[0], q[1], q[2], prev.b[0], prev.b[1], prev.b[2]);
            const double depth = -dot3(X[0] - cur.center[0], X[1] - cur.center[1], X[2] - cur.center[2], cur.w[0], cur.w[1], cur.w[2]);
            const double snap = 0x1p-20;
            const double rx = rint(fx), ry = rint(fy);
            if (fabs(fx - rx) <= snap) fx = rx;
            if (fabs(fy - ry) <= snap) fy = ry;
            if (fx >= -1.0 && fx <= (double)W && fy >= -1.0 && fy <= (double)H) {   // (false for NaN; the integer conversions below are then in range)
                const double flx = floor(fx), fly = floor(fy);
                const double wx = fx - flx, wy = fy - fly;
                const int x0 = (int)flx, y0 = (int)fly;
                const double bound = tp.plane_tolerance * depth;
#pragma unroll
                for (int dy = 0; dy < 2; dy++) {
#pragma unroll
                    for (int dx = 0; dx < 2; dx++) {
                        const double w = (dx ? wx : 1.0 - wx) * (dy ? wy : 1.0 - wy);
                        const int qx = x0 + dx, qy = y0 + dy;
                        if (!(w > 0.0) || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                        const size_t qi = (size_t)qy * W + qx;
                        const int nq = before.len[qi];
                        if (nq <= 0 || before.mat[qi] != m) continue;
                        if (hit) {
                            const double ex = before.pos[3 * qi] - Xr[0], ey = before.pos[3 * qi + 1] - Xr[1], ez = before.pos[3 * qi + 2] - Xr[2];
                            if (!(fabs(dot3(ex, ey, ez, nr[0], nr[1], nr[2])) <= bound)) continue;
                            if (!(dot3(nr[0], nr[1], nr[2], before.nrm[3 * qi], before.nrm[3 * qi + 1], before.nrm[3 * qi + 2]) >= tp.normal_cos)) continue;
                        }
                        sw = sw + w;
#pragma unroll
                        for (int k = 0; k < 3; k++) {
                            sh[k] = sh[k] + w * before.col[3 * qi + k];
                            sv[k] = sv[k] + w * before.var[3 * qi + k];
                        }
                        min_n = nq < min_n ? nq : min_n;
                    }
                }
            }
        }
    }
    int N = 1;
    double o[3] = {c[0], c[1], c[2]}, vo[3] = {V[0], V[1], V[2]};
    if (sw > 0.0) {
        N = min_n + 1 < tp.max_history ? min_n + 1 : tp.max_history;
        const double beta = fmax(1.0 / (double)N, tp.alpha);
        const double om = 1.0 - beta;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double h = sh[k] / sw, vh = sv[k] / sw;
            o[k] = h + beta * (c[k] - h);
            vo[k] = (om * om) * vh + (beta * beta) * V[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) { now.col[3 * p + k] = o[k]; now.var[3 * p + k] = vo[k]; }
    now.len[p] = N;
}

}  // namespace

// rays: W*H*6 doubles (origin, direction), row-major pixels
hipError_t launch_gbuffer_rays(const DCamera& cam, double* d_rays, hipStream_t stream) {
    const dim3 block(16, 16), grid((unsigned)((cam.W + 15) / 16), (unsigned)((cam.H + 15) / 16));
    hipLaunchKernelGGL(gbuffer_rays, grid, block, 0, stream, cam, d_rays);
    return hipGetLastError();
}

// any of the four planes may be null
hipError_t launch_gbuffer_pack(const zr_hit* d_hits, const double* d_rays, size_t n, double* d_pos, double* d_nrm, double* d_t, uint32_t* d_mat, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(gbuffer_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_hits, d_rays, n, d_pos, d_nrm, d_t, d_mat);
    return hipGetLastError();
}

// now: this frame's geometry planes (read) and the history half that receives out / V_out / N; before: the previous frame's planes and history (read; ignored
// without have_prev).  motion (may be null: the build without motion): this frame's (kind, index) plane and the table of the refit between `before` and `now`.
// The caller has validated the parameters.
hipError_t launch_temporal_reproject(int W, int H, const TemporalView& cur, const TemporalView& prev, bool have_prev, const zr_temporal_params& tp,
                                     const double* d_color, const double* d_variance, const TemporalPlanes& now, const TemporalPlanes& before,
                                     const TemporalMotion* motion, hipStream_t stream) {
    const dim3 block(16, 16), grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16));
    if (motion) hipLaunchKernelGGL(temporal_reproject<true>, grid, block, 0, stream, W, H, cur, prev, have_prev ? 1 : 0, tp, d_color, d_variance, now, before, *motion);
    else hipLaunchKernelGGL(temporal_reproject<false>, grid, block, 0, stream, W, H, cur, prev, have_prev ? 1 : 0, tp, d_color, d_variance, now, before, TemporalMotion{});
    return hipGetLastError();
}

// out[p] = the world-list entry of the leaf primitive mv.ki[p] names (d_leaf_entry: mv.n_leaves words), 0xFFFFFFFF on a miss
hipError_t launch_gbuffer_entries(const TemporalMotion& mv, const uint32_t* d_leaf_entry, size_t n, uint32_t* d_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(gbuffer_entries, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, mv, d_leaf_entry, n, d_out);
    return hipGetLastError();
}

}  // namespace zr
